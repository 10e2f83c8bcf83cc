"""One Engine.bench run of a synthetic Q4_K model (128-token prompts, 5 warm-up and 40 timed decode rounds):

    [MIPIPE_LIB=libmipipe_other.so] python tools/engine_ab.py TAG MB_SIZE [key=value ...]

Keys: row_sampling=true, row_masks=true (engine keys, as before); model=8b|70b (default 8b: synthetic
Llama-3-8B; 70b: Llama-3-70B widths), layers=N (fewer layers than the model's: per-layer figures scale),
ftype=Q4_K; lora_adapters=N (the engine key: N > 0 gives up the fused routes whatever is bound),
lora_rank=R (default 16, all seven targets of every layer, written by mipipe.lora.write_adapter_gguf),
lora_bind=none|one|mixed (none: no adapter loaded; one: every row on adapter 0; mixed: rows spread over
min(4, N) adapters plus unbound rows, round robin).

Prints one line `AB TAG LIBRARY MB_SIZE {json}`.  MIPIPE_LIB selects another build of the library in
lib/, so two builds (or two engine keys) can be alternated inside one job for an A/B comparison."""
import json, os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from mipipe.engine import Engine
tag, mb = sys.argv[1], int(sys.argv[2])
kw, opt = {}, dict(model="8b", layers="0", ftype="Q4_K", lora_adapters="0", lora_rank="16", lora_bind="none")
for a in sys.argv[3:]:
    k, v = a.split("=")
    if k in opt:
        opt[k] = v
    else:
        kw[k] = v == "true"
syn = {"8b": dict(name="Llama-3-8B", n_layer=32, d_model=4096, n_head=32, n_head_kv=8, d_ff=14336, vocab=128256, rope_base=500000.0),
       "70b": dict(name="Llama-3-70B", n_layer=80, d_model=8192, n_head=64, n_head_kv=8, d_ff=28672, vocab=128256,
                   rope_base=500000.0)}[opt["model"]]
if int(opt["layers"]) > 0:
    syn["n_layer"] = int(opt["layers"])
n_ad, rank, bind = int(opt["lora_adapters"]), int(opt["lora_rank"]), opt["lora_bind"]
if n_ad > 0:
    kw["lora_adapters"] = n_ad
    kw["lora_max_rank"] = max(rank, 16)


def write_adapter(path, seed):
    from mipipe import lora
    from mipipe.utils import quants as Q
    rng = np.random.default_rng(seed)
    d, qd, kvd, F = syn["d_model"], syn["d_model"], syn["d_model"] // syn["n_head"] * syn["n_head_kv"], syn["d_ff"]
    dims = dict(attn_q=(qd, d), attn_k=(kvd, d), attn_v=(kvd, d), attn_output=(d, qd), ffn_gate=(F, d), ffn_up=(F, d), ffn_down=(d, F))
    pairs = {}
    for li in range(syn["n_layer"]):
        for t, (n, k) in dims.items():
            pairs[f"blk.{li}.{t}.weight"] = ((rng.standard_normal((rank, k), dtype=np.float32) / np.sqrt(k)),
                                             rng.standard_normal((n, rank), dtype=np.float32) * 0.01)
    lora.write_adapter_gguf(path, "llama", float(rank), pairs, Q.F16)


with tempfile.TemporaryDirectory() as tmp, Engine(synthetic=syn, ftype=opt["ftype"], n_mb=1, mb_size=mb, max_ctx=512, **kw) as eng:
    if n_ad > 0 and bind != "none":
        use = 1 if bind == "one" else min(4, n_ad)
        for a in range(use):
            p = os.path.join(tmp, f"a{a}.gguf")
            write_adapter(p, a)
            assert eng.load_adapter(p) == a
        ids = [0] * mb if bind == "one" else [(m % (use + 1)) - 1 for m in range(mb)]
        eng.set_slot_adapters(list(range(mb)), ids, [1.0] * mb)   # set for the bench's own start()
    r = eng.bench(128, 5, 40)
    caps = [s["graph_captures"] for s in eng.health()["stages"]]
out = {k: r[k] for k in r if k in ("decode_tok_s", "p50_ms", "decode_ms")}
out.update(model=opt["model"], layers=syn["n_layer"], lora_adapters=n_ad, lora_bind=bind if n_ad else "off", graph_captures=caps)
print("AB", tag, os.environ.get("MIPIPE_LIB", "libmipipe.so"), mb, json.dumps(out))
