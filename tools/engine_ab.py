"""One Engine.bench run of synthetic Llama-3-8B Q4_K (128-token prompts, 5 warm-up and 40 timed decode rounds):

    [MIPIPE_LIB=libmipipe_other.so] python tools/engine_ab.py TAG MB_SIZE [row_sampling=true] [row_masks=true]

Prints one line `AB TAG LIBRARY MB_SIZE {json}`.  MIPIPE_LIB selects another build of the library in
lib/, so two builds (or two engine keys) can be alternated inside one job for an A/B comparison."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mipipe.engine import Engine
tag, mb = sys.argv[1], int(sys.argv[2])
kw = {}
for a in sys.argv[3:]:
    k, v = a.split("=")
    kw[k] = v == "true"
syn = dict(name="Llama-3-8B", n_layer=32, d_model=4096, n_head=32, n_head_kv=8, d_ff=14336, vocab=128256, rope_base=500000.0)
with Engine(synthetic=syn, ftype="Q4_K", n_mb=1, mb_size=mb, max_ctx=512, **kw) as eng:
    r = eng.bench(128, 5, 40)
print("AB", tag, os.environ.get("MIPIPE_LIB", "libmipipe.so"), mb, json.dumps({k: r[k] for k in r if k in ("decode_tok_s", "p50_ms", "decode_ms")}))
