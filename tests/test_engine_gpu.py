"""T2/T3 model-level tests on one MI355X: engine vs the pure-torch fp32 oracle, hipGraph vs eager,
pipeline emulation (PP=2/3 stages on one GPU with LocalLink) vs PP=1, micro-batch invariance."""
import numpy as np
import pytest
import torch

from conftest import make_model

pytestmark = pytest.mark.gpu


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


@pytest.mark.parametrize("name,ftype", [("stories15m", "F32"), ("tiny-gqa", "Q8_0"), ("tiny-gqa", "Q4_K_M"),
                                        ("tiny-l3", "Q6_K"), ("tiny-gqa", "Q5_K_M"), ("tiny-gqa", "BF16"),
                                        ("tiny-moe", "Q8_0"), ("tiny-moe", "Q4_K_M"), ("tiny-qwen2", "Q4_K_M"),
                                        ("tiny-qwen2", "Q8_0")])
def test_engine_matches_reference(cuda, native, model_dir, name, ftype):
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, name, ftype)
    ref = RefLlama.from_gguf(path)
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(3, cfg.vocab, 37)]
    with Engine(gguf=path, max_ctx=256, prefill_chunk=16, graphs=True) as eng:
        eng.start([prompt])
        lg = eng.logits()[0]
        ref.reset()
        rl = ref.forward(prompt, 0)[-1].numpy()
        assert nmse(lg, rl) < 2e-4, nmse(lg, rl)
        pos = len(prompt)
        for step in range(6):
            tok = eng.tokens()[0][-1]
            rtop = np.sort(rl)[-2:]
            if rl.argmax() != tok:   # allowed only on a near-tie
                assert rl.max() - rl[tok] < 1e-2 * (abs(rtop).max() + 1), (step, tok, rl.argmax())
            eng.decode(1)
            lg = eng.logits()[0]
            rl = ref.forward([tok], pos)[-1].numpy()
            pos += 1
            assert nmse(lg, rl) < 2e-4, (step, nmse(lg, rl))


def test_70b_width_mb256_matches_reference(cuda, native, model_dir):
    """The headline path at its real widths: a 2-layer Llama-3-70B-width Q4_K
    model (d 8192, 64 / 8 heads, d_ff 28672), 256 sequences in one micro-batch, so prompt chunks and
    every decode projection run on the MFMA GEMMs with K = 8192 / 28672 and split-K; logits of
    sampled rows against the fp32 oracle after the prompt and after two decode rounds."""
    import os
    from mipipe.engine import Engine
    from mipipe.models.config import CONFIGS
    from mipipe.models.reference import RefLlama
    from mipipe.models.synthetic import write_synthetic_gguf
    cfg = CONFIGS["llama3-70b"].scaled(n_layer=2, vocab=4096, name="l70w2")
    path = os.path.join(str(model_dir), "l70w2-Q4_K.gguf")
    if not os.path.exists(path):
        write_synthetic_gguf(path, cfg, "Q4_K", seed=3, fast_random_blocks=True)
    rng = np.random.default_rng(5)
    mb = 256
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(4, 24, mb)]
    with Engine(gguf=path, max_ctx=64, n_mb=1, mb_size=mb, prefill_chunk=512) as eng:
        eng.start(prompts)
        lg0 = eng.logits(rows=mb)
        eng.decode(2)
        lg2 = eng.logits(rows=mb)
        toks = eng.tokens()
    ref = RefLlama.from_gguf(path, device="cuda")
    for r in (0, 1, 63, 64, 77, 128, 200, 255):
        ref.reset()
        rl = ref.forward(prompts[r], 0)[-1].float().cpu().numpy()
        assert nmse(lg0[r], rl) < 2e-4, (r, nmse(lg0[r], rl))
        pos = len(prompts[r])
        for t in toks[r][:2]:   # the engine's own tokens (a near-tie flip would only change the path)
            rl = ref.forward([t], pos)[-1].float().cpu().numpy()
            pos += 1
        assert nmse(lg2[r], rl) < 2e-4, (r, nmse(lg2[r], rl))
    del ref
    torch.cuda.empty_cache()


def _fp8_round(t):
    return t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(t.dtype)


@pytest.mark.parametrize("name,ftype", [("tiny-gqa", "Q8_0"), ("tiny-l3", "Q6_K"), ("tiny-qwen2", "Q4_K_M")])
def test_fp8_kv_cache_matches_reference(cuda, native, model_dir, name, ftype):
    """kv_dtype="fp8" (OCP e4m3 KV pages: prefill flash attention + fused decode attention, paged)
    against the fp32 oracle whose cached K / V are rounded to e4m3 the same way, and close to the f16
    cache's logits."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, name, ftype)
    ref = RefLlama.from_gguf(path)
    ref.kv_round = _fp8_round
    prompt = [int(t) for t in np.random.default_rng(2).integers(3, cfg.vocab, 45)]
    with Engine(gguf=path, max_ctx=256, prefill_chunk=16, kv_dtype="fp8") as eng, \
            Engine(gguf=path, max_ctx=256, prefill_chunk=16) as e16:
        assert eng.info["kv_bytes_local"] * 2 == e16.info["kv_bytes_local"]
        eng.start([prompt])
        e16.start([prompt])
        ref.reset()
        rl = ref.forward(prompt, 0)[-1].numpy()
        assert nmse(eng.logits()[0], rl) < 5e-4, nmse(eng.logits()[0], rl)
        assert nmse(eng.logits()[0], e16.logits()[0]) < 2e-2
        pos = len(prompt)
        for step in range(6):
            tok = eng.tokens()[0][-1]
            eng.decode(1)
            rl = ref.forward([tok], pos)[-1].numpy()
            pos += 1
            assert nmse(eng.logits()[0], rl) < 5e-4, (step, nmse(eng.logits()[0], rl))


def test_fp8_kv_cache_checkpoint_and_batch(cuda, native, model_dir, tmp_path):
    """fp8 pages survive save_state / load_state byte for byte, and a micro-batch of 4 paged
    sequences gives each sequence's single-stream tokens."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    rng = np.random.default_rng(4)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (70, 5, 33, 130)]
    kw = dict(gguf=path, max_ctx=512, n_mb=1, mb_size=4, prefill_chunk=64, kv_dtype="fp8")
    with Engine(**kw) as eng:
        eng.start(prompts)
        eng.decode(4)
        eng.save_state(str(tmp_path / "st"))
        eng.decode(5)
        full = eng.tokens()
    with Engine(**kw) as eng:
        eng.load_state(str(tmp_path / "st"))
        eng.decode(5)
        assert eng.tokens() == full
    # an fp8 checkpoint is refused by an f16-KV engine (and vice versa): the fingerprint names the
    # KV dtype and the payload size is checked against the stage's own kv_state_bytes
    with Engine(**dict(kw, kv_dtype="f16")) as eng:
        with pytest.raises(RuntimeError, match="load_state"):
            eng.load_state(str(tmp_path / "st"))
    alone = []
    with Engine(gguf=path, max_ctx=512, prefill_chunk=64, kv_dtype="fp8") as eng:
        for p in prompts:
            alone.append(eng.generate([p], 10)[0][0])
    assert full == alone


@pytest.mark.parametrize("name,ftype", [("tiny-gqa", "Q4_K_M"), ("tiny-qwen2", "Q8_0"), ("tiny-moe", "Q8_0")])
def test_fused_norm_matches_reference(cuda, native, model_dir, name, ftype):
    """fused_norm=true (deferred RMSNorm in the qkv / gate-up GEMVs, applied by the decode attention
    incl. the Qwen2 q|k|v bias) against the fp32 oracle, single stream and mb 3 (prefill chunks of
    <= 4 tokens take the fused gate/up too)."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, name, ftype)
    ref = RefLlama.from_gguf(path)
    prompt = [int(t) for t in np.random.default_rng(1).integers(3, cfg.vocab, 23)]
    with Engine(gguf=path, max_ctx=256, prefill_chunk=4, graphs=True, fused_norm=True) as eng:
        eng.start([prompt])
        ref.reset()
        rl = ref.forward(prompt, 0)[-1].numpy()
        assert nmse(eng.logits()[0], rl) < 2e-4
        pos = len(prompt)
        for step in range(5):
            tok = eng.tokens()[0][-1]
            eng.decode(1)
            rl = ref.forward([tok], pos)[-1].numpy()
            pos += 1
            assert nmse(eng.logits()[0], rl) < 2e-4, (step, nmse(eng.logits()[0], rl))
    prompts = [[5, 6, 7, 8, 9], [100, 200, 300], [7] * 11]
    with Engine(gguf=path, max_ctx=256, n_mb=1, mb_size=3, prefill_chunk=4, fused_norm=True) as eng:
        eng.start(prompts)
        eng.decode(2)
        lg, toks = eng.logits(rows=3), eng.tokens()
    for i, pr in enumerate(prompts):
        ref.reset()
        seq = pr + toks[i][:2]
        rl = ref.forward(seq, 0)[-1].numpy()
        assert nmse(lg[i], rl) < 2e-4, (i, nmse(lg[i], rl))


def test_graph_equals_eager(cuda, native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    prompts = [[5, 6, 7, 8, 9], [100, 200, 300]]
    outs = []
    for graphs in (False, True):
        with Engine(gguf=path, max_ctx=256, n_mb=1, mb_size=2, graphs=graphs) as eng:
            out, _ = eng.generate(prompts, 12)
            outs.append(out)
    assert outs[0] == outs[1]


@pytest.mark.parametrize("stages", [2, 3])
def test_pipeline_emulation_matches_pp1(cuda, native, model_dir, stages):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    rng = np.random.default_rng(1)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (9, 40, 3, 17)]
    with Engine(gguf=path, max_ctx=256, n_mb=2, mb_size=2, prefill_chunk=16) as eng:
        ref_out, _ = eng.generate(prompts, 10)
    with Engine(gguf=path, max_ctx=256, n_mb=2, mb_size=2, prefill_chunk=16, stages=stages,
                devices=[0] * stages, link="local", split="even") as eng:
        assert len(eng.info["stages"]) == stages
        out, st = eng.generate(prompts, 10)
    assert out == ref_out


def test_microbatch_invariance(cuda, native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    prompts = [[11, 12, 13], [400, 5, 6, 7, 8, 9, 10], [42]]
    singles = []
    with Engine(gguf=path, max_ctx=128) as eng:
        for p in prompts:
            o, _ = eng.generate([p], 8)
            singles.append(o[0])
    with Engine(gguf=path, max_ctx=128, n_mb=2, mb_size=2) as eng:
        o, _ = eng.generate(prompts, 8)
    assert o == singles


@pytest.mark.parametrize("mb_size", [24, 40, 64, 96, 200])
def test_wide_microbatch_matches_single(cuda, native, model_dir, mb_size):
    """Decode micro-batches above 16 rows: the GEMV with 2-4 MFMA row groups per weight fragment;
    above 64 rows the decode projections and the LM head run on the GEMMs (gemm4).  Rows on
    both sides of every 64-row boundary and the last row are checked against the fp32 oracle: a
    single-block 64-thread position advance once froze rows >= 64 at their prompt position (found by
    the 70B-width test)."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    rng = np.random.default_rng(mb_size)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, size=int(rng.integers(1, 9)))] for _ in range(mb_size)]
    rows = sorted({0, 1, 2, mb_size - 1} | {r for b in range(64, mb_size, 64) for r in (b - 1, b)})
    with Engine(gguf=path, max_ctx=128, n_mb=1, mb_size=mb_size) as eng:
        o, _ = eng.generate(prompts, 6)
    # every generated token is the fp32 oracle's argmax at its position, teacher-forced on the row's own
    # tokens, up to near-ties (a random tiny model has top-2 logits within 1e-3 of each other: exact
    # token equality with the single-stream GEMV path flipped on such ties when only a summation
    # order changed)
    ref = RefLlama.from_gguf(path)
    for r in rows:
        seq = prompts[r] + o[r]
        ref.reset()
        lg = ref.forward(seq[:-1], 0).numpy()
        for i, tok in enumerate(o[r]):
            lo = lg[len(prompts[r]) - 1 + i]
            # within 5 % of the logit range of the oracle's max (f16 activations / KV move logits by
            # ~1 % of it; a token decoded from a wrong context lands near the mean, ~40 % below)
            span = lo.max() - lo.min()
            assert lo[tok] >= lo.max() - 0.05 * span, (r, i, float(lo.max() - lo[tok]))
            # and exactly the oracle's argmax wherever its top-2 margin is clear (> 2 % of the range):
            # only genuine near-ties may flip
            top2 = np.sort(lo)[-2:]
            if top2[1] - top2[0] > 0.02 * span:
                assert tok == int(lo.argmax()), (r, i, float(top2[1] - top2[0]), float(span))


def test_wide_microbatches_pipelined_match_single(cuda, native, model_dir):
    """The bench.py layout at PP > 1 (N + 1 micro-batches of > 64 rows circulating through the
    ring), emulated with two stages on one GPU: rows on both sides of the 64-row boundary of both
    micro-batches against one sequence at a time."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    rng = np.random.default_rng(144)
    mb = 72
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, size=int(rng.integers(1, 9)))] for _ in range(2 * mb)]
    rows = [0, 63, 64, mb - 1, mb, mb + 63, mb + 64, 2 * mb - 1]
    with Engine(gguf=path, max_ctx=64) as eng:
        singles = [eng.generate([prompts[r]], 5)[0][0] for r in rows]
    with Engine(gguf=path, max_ctx=64, n_mb=2, mb_size=mb, stages=2, devices=[0, 0], link="local",
                split="even") as eng:
        o, _ = eng.generate(prompts, 5)
    assert [o[r] for r in rows] == singles


def test_synthetic_engine_runs(cuda, native):
    from mipipe.engine import Engine
    syn = dict(n_layer=2, d_model=1024, n_head=8, n_head_kv=2, d_ff=2816, vocab=4096)
    with Engine(synthetic=syn, ftype="Q4_K_M", max_ctx=256, n_mb=2, mb_size=4) as eng:
        r = eng.bench(prompt_len=32, warmup=2, steps=8)
    assert r["decode_tok_s"] > 0 and r["p50_ms"] > 0


def test_moe_batched_matches_single(cuda, native, model_dir):
    """Routed experts see several tokens each (prefill chunks of 16+, 4 sequences per micro-batch):
    the grouped expert GEMV must give the same greedy stream as one sequence at a time."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-moe", "Q8_0")
    rng = np.random.default_rng(3)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (40, 7, 23, 2)]
    singles = []
    with Engine(gguf=path, max_ctx=128, prefill_chunk=32) as eng:
        for p in prompts:
            o, _ = eng.generate([p], 8)
            singles.append(o[0])
    with Engine(gguf=path, max_ctx=128, n_mb=1, mb_size=4, prefill_chunk=32) as eng:
        o, _ = eng.generate(prompts, 8)
    assert o == singles


def test_sampling_seeded(cuda, native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    prompts = [[5, 6, 7], [8, 9, 10, 11]]
    outs = []
    for _ in range(2):
        with Engine(gguf=path, max_ctx=128, mb_size=2, temp=1.5, top_k=50, top_p=0.95, seed=7) as eng:
            o, _ = eng.generate(prompts, 16)
            outs.append(o)
    assert outs[0] == outs[1]
    assert all(0 <= t < cfg.vocab for seq in outs[0] for t in seq)
    with Engine(gguf=path, max_ctx=128, mb_size=2) as eng:
        greedy, _ = eng.generate(prompts, 16)
    assert greedy != outs[0]


def test_synthetic_moe_engine_runs(cuda, native):
    from mipipe.engine import Engine
    syn = dict(n_layer=2, d_model=1024, n_head=8, n_head_kv=2, d_ff=1536, vocab=4096, n_expert=8, n_expert_used=2)
    with Engine(synthetic=syn, ftype="Q4_K_M", max_ctx=256, n_mb=1, mb_size=8) as eng:
        r = eng.bench(prompt_len=40, warmup=2, steps=8)
    assert r["decode_tok_s"] > 0


_MP_SCRIPT = r"""
import json, sys
sys.path.insert(0, {repo!r})
import torch
from mipipe.engine import Engine
cfg = json.loads(sys.argv[1])
with Engine(**cfg) as eng:
    out, _ = eng.generate({prompts!r}, 7)
    print("OUT " + json.dumps(out if cfg["rank"] == cfg["world"] - 1 else None), flush=True)
"""


def test_multiprocess_pipeline_one_gpu_tcp(cuda, native, model_dir):
    """mode="mp" (one process per stage, the torchrun layout of bench.py) with two ranks sharing
    the single GPU of the box; TCP links (RCCL refuses two ranks on one GPU)."""
    import json, socket, subprocess, sys
    from conftest import REPO
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    prompts = [[3, 4, 5, 6], [7, 8], [9, 10, 11], [12]]
    with Engine(gguf=path, max_ctx=64, n_mb=2, mb_size=2) as eng:
        ref_out, _ = eng.generate(prompts, 7)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = _MP_SCRIPT.format(repo=REPO, prompts=prompts)
    procs = []
    for r in range(2):
        c = dict(gguf=path, mode="mp", world=2, rank=r, device=0, link="tcp", base_port=port,
                 max_ctx=64, n_mb=2, mb_size=2, split="even")
        procs.append(subprocess.Popen([sys.executable, "-c", script, json.dumps(c)], stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True, cwd=REPO))
    outs = []
    for p in procs:
        o, _ = p.communicate(timeout=300)
        assert p.returncode == 0, o[-3000:]
        outs.append(o)
    last = [l for l in outs[-1].splitlines() if l.startswith("OUT ")]
    assert last and json.loads(last[0][4:]) == ref_out


_MP_SPEC_SCRIPT = r"""
import json, sys
sys.path.insert(0, {repo!r})
import torch
from mipipe.engine import Engine
cfg = json.loads(sys.argv[1])
with Engine(**cfg) as eng:
    out, st = eng.spec_generate({prompts!r}, 10, draft_max=4, ngram=2)
    print("OUT " + json.dumps(dict(out=out, stats=st)), flush=True)
"""


def test_spec_generate_multiprocess_hip_stages(cuda, native, model_dir):
    """Speculative decoding with one process per HIP stage (two ranks on the box's GPU, TCP links):
    the verify tokens cross the ring from device staging buffers; both ranks return single-process
    greedy output."""
    import json, socket, subprocess, sys
    from conftest import REPO
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    prompts = [[5, 6, 7, 8, 5, 6, 7, 8, 5, 6], [9, 10, 11, 9, 10, 11, 9], [20, 21, 22, 23, 20, 21], [40, 41, 40, 41]]
    with Engine(gguf=path, max_ctx=64, n_mb=2, mb_size=2, prefill_chunk=32) as eng:
        ref_out, _ = eng.generate(prompts, 10)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = _MP_SPEC_SCRIPT.format(repo=REPO, prompts=prompts)
    procs = []
    for r in range(2):
        c = dict(gguf=path, mode="mp", world=2, rank=r, device=0, link="tcp", base_port=port,
                 max_ctx=64, n_mb=2, mb_size=2, prefill_chunk=32, split="even")
        procs.append(subprocess.Popen([sys.executable, "-c", script, json.dumps(c)], stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True, cwd=REPO))
    for p in procs:
        o, _ = p.communicate(timeout=300)
        assert p.returncode == 0, o[-3000:]
        d = json.loads([l for l in o.splitlines() if l.startswith("OUT ")][-1][4:])
        assert d["out"] == ref_out and d["stats"]["verify_rounds"] >= 1


@pytest.mark.parametrize("name", ["tiny-gqa", "stories15m"])
def test_fused_decode_attention_matches_unfused(cuda, native, model_dir, name):
    """Fused RoPE + KV append + split-K attention + last-arriver merge == the three-kernel path,
    across several KV splits (split_len 128, contexts up to ~400)."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, name, "Q8_0")
    rng = np.random.default_rng(5)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (300, 5, 130, 255)]
    res = []
    for fused in (False, True):
        with Engine(gguf=path, max_ctx=512, n_mb=2, mb_size=2, prefill_chunk=64, fused_attn=fused) as eng:
            out, _ = eng.generate(prompts, 12)
            lg = eng.logits()
            res.append((out, lg))
    assert res[0][0] == res[1][0]
    assert nmse(res[1][1], res[0][1]) < 1e-6


@pytest.mark.parametrize("name,ftype,kv", [("tiny-gqa", "Q4_K_M", "f16"), ("tiny-qwen2", "Q8_0", "f16"),
                                            ("stories15m", "Q8_0", "f16"), ("tiny-gqa", "Q4_K_M", "fp8")])
@pytest.mark.parametrize("mb_size", [1, 3])
def test_qkv_append_epilogue_matches_attention_append(cuda, native, model_dir, name, ftype, kv, mb_size):
    """Knob ATTN_PRE: RoPE + the KV append in the qkv GEMV's epilogue (gemvs QkvAppend, also the
    mixed-type gemvs2 launch of Q4_K_M and the q/k/v biases of qwen2) == the decode attention doing
    them itself: same tokens, logits within rounding, f16 and fp8 KV, single stream and M = 3."""
    from mipipe import _native as N
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, name, ftype)
    rng = np.random.default_rng(11)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (37, 70, 5)][:mb_size]
    res = []
    try:
        for pre in (0, 1):
            N.check(N.lib().mp_set_knob(b"ATTN_PRE", pre), "knob")
            with Engine(gguf=path, max_ctx=256, mb_size=mb_size, prefill_chunk=16, kv_dtype=kv) as eng:
                out, _ = eng.generate(prompts, 70)   # crosses a 64-token page for every prompt
                res.append((out, eng.logits(rows=mb_size)))
    finally:
        N.lib().mp_reset_knob(b"ATTN_PRE")
    if kv == "f16":
        assert res[0][0] == res[1][0]
        assert nmse(res[1][1], res[0][1]) < 1e-6, nmse(res[1][1], res[0][1])
    else:   # e4m3 rounding of K amplifies f32 contraction-order differences into rare late near-tie flips
        assert all(a[:16] == b[:16] for a, b in zip(res[0][0], res[1][0]))
        if res[0][0] == res[1][0]:
            assert nmse(res[1][1], res[0][1]) < 1e-3, nmse(res[1][1], res[0][1])


def test_prefill_gemm_matches_gemv_path(cuda, native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    rng = np.random.default_rng(9)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (200, 33, 70)]
    res = []
    for pg in (False, True):
        with Engine(gguf=path, max_ctx=512, n_mb=1, mb_size=3, prefill_chunk=128, prefill_gemm=pg) as eng:
            out, _ = eng.generate(prompts, 8)
            res.append((out, eng.logits()))
    assert res[0][0] == res[1][0]
    assert nmse(res[1][1], res[0][1]) < 1e-5


def test_repetition_penalties_match_reference(cuda, native, model_dir):
    """On-GPU penalties (graph-captured penalize + history ring) against the oracle logits with
    the penalties applied in Python; the returned logits are the penalized ones."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    ref = RefLlama.from_gguf(path)
    prompt = [5, 9, 5, 17, 30, 9]
    rep, fq, pr, last_n = 1.8, 0.3, 0.4, 8

    def penalize(lg, window):
        lg = lg.copy()
        for t in set(window):
            c = window.count(t)
            lg[t] = (lg[t] / rep if lg[t] > 0 else lg[t] * rep) - c * fq - pr
        return lg

    with Engine(gguf=path, max_ctx=64, graphs=True, repeat_penalty=rep, frequency_penalty=fq,
                presence_penalty=pr, repeat_last_n=last_n) as eng:
        eng.start([prompt])
        ref.reset()
        seq = list(prompt)
        rl = penalize(ref.forward(prompt, 0)[-1].numpy(), seq[-last_n:])
        for step in range(8):
            lg = eng.logits()[0]
            assert nmse(lg, rl) < 2e-4, (step, nmse(lg, rl))
            tok = eng.tokens()[0][-1]
            if rl.argmax() != tok:   # allowed only on a near-tie
                assert rl.max() - rl[tok] < 1e-2 * (abs(rl).max() + 1), (step, tok, rl.argmax())
            seq.append(tok)
            eng.decode(1)
            rl = penalize(ref.forward([tok], len(seq) - 1)[-1].numpy(), seq[-last_n:])


@pytest.mark.parametrize("stages,n_mb,mb_size", [(1, 1, 1), (1, 2, 2), (2, 2, 2)])
def test_speculative_lookup_matches_greedy(cuda, native, model_dir, stages, n_mb, mb_size):
    """Prompt-lookup speculative decoding on the HIP path (verify chunks through the prefill GEMV/
    GEMM + per-row LM head and argmax) equals plain greedy decoding; PP=2 emulated on one GPU."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    rng = np.random.default_rng(3)
    motif = [int(t) for t in rng.integers(3, cfg.vocab, 6)]
    prompts = [motif * 4, [int(t) for t in rng.integers(3, cfg.vocab, 11)], motif * 2 + [7, 8], [42, 43, 44]]
    prompts = prompts[: n_mb * mb_size]
    kw = dict(gguf=path, max_ctx=128, n_mb=n_mb, mb_size=mb_size, prefill_chunk=32, stages=stages,
              devices=[0] * stages, link="local", split="even")
    with Engine(**kw) as eng:
        ref, _ = eng.generate(prompts, 24)
    with Engine(**kw) as eng:
        out, st = eng.spec_generate(prompts, 24, draft_max=5, ngram=3)
        again, _ = eng.generate(prompts[:1], 6)
    assert out == ref
    assert again[0] == ref[0][:6]
    assert st["drafted"] >= st["accepted"] >= 0


@pytest.mark.parametrize("stages,sampling", [(1, False), (2, True)])
def test_checkpoint_resume(cuda, native, model_dir, tmp_path, stages, sampling):
    """HIP stages: KV pages, ring tokens and sampler step survive save_state / load_state; the
    resumed engine (graphs re-captured) continues the generation token for token."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    rng = np.random.default_rng(4)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (9, 70, 3, 17)]
    kw = dict(gguf=path, max_ctx=256, n_mb=2, mb_size=2, prefill_chunk=16, stages=stages,
              devices=[0] * stages, link="local", split="even")
    if sampling:
        kw.update(temp=1.1, top_k=40, seed=5, repeat_penalty=1.2, repeat_last_n=16)
    with Engine(**kw) as eng:
        eng.start(prompts)
        eng.decode(5)
        eng.save_state(str(tmp_path / "st"))
        eng.decode(7)
        full = eng.tokens()
    with Engine(**kw) as eng:
        eng.load_state(str(tmp_path / "st"))
        eng.decode(7)
        resumed = eng.tokens()
    assert resumed == full


def test_prefix_cache_multiturn(cuda, native, model_dir):
    """HIP stages: a follow-up request that extends the previous prompt + reply prefills only its
    new tail and produces the same greedy tokens as an engine without the prefix cache."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    rng = np.random.default_rng(6)
    p1 = [int(t) for t in rng.integers(3, cfg.vocab, 50)]
    kw = dict(gguf=path, max_ctx=256, prefill_chunk=16, n_mb=2, mb_size=2, stages=2, devices=[0, 0],
              link="local", split="even")
    with Engine(**kw) as eng:
        o1, _ = eng.generate([p1, p1[:20]], 8)
        p2 = [p1 + o1[0] + [5, 6, 7], p1[:20] + [9]]
        o2, _ = eng.generate(p2, 8)
        assert eng.health()["prefix_reused_tokens"] == (len(p1) + 7) + 20
    with Engine(prefix_cache=False, **kw) as eng:
        c2, _ = eng.generate(p2, 8)
    assert o2 == c2


def test_long_context_matches_reference(cuda, native, model_dir):
    """~3000-token prompt: chunked prefill attention over a long cache and flash-decoding with many
    KV splits (auto split: 16 splits of 256 keys) against the fp32 torch oracle."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    ref = RefLlama.from_gguf(path)
    rng = np.random.default_rng(9)
    prompt = [int(t) for t in rng.integers(3, cfg.vocab, 3000)]
    with Engine(gguf=path, max_ctx=4096, prefill_chunk=256) as eng:
        eng.start([prompt])
        lg = eng.logits()[0]
        ref.reset()
        rl = ref.forward(prompt, 0)[-1].numpy()
        assert nmse(lg, rl) < 1e-4, nmse(lg, rl)
        pos = len(prompt)
        for step in range(3):
            tok = eng.tokens()[0][-1]
            eng.decode(1)
            lg = eng.logits()[0]
            rl = ref.forward([tok], pos)[-1].numpy()
            pos += 1
            assert nmse(lg, rl) < 1e-4, (step, nmse(lg, rl))


def test_max_ctx_auto_fills_hbm(cuda, native):
    """max_ctx "auto" sizes the per-stage KV cache from the card's HBM: Llama-3-8B geometry with a
    128K training context and 64 sequence slots gets tens of thousands of tokens per sequence."""
    from mipipe.engine import Engine
    syn = dict(n_layer=32, d_model=4096, n_head=32, n_head_kv=8, d_ff=14336, vocab=128256, rope_base=500000.0,
               n_ctx_train=131072)
    total = torch.cuda.get_device_properties(0).total_memory
    with Engine(synthetic=syn, ftype="Q4_K_M", max_ctx="auto", mb_size=64, graphs=False) as eng:
        ctx = eng.info["max_ctx"]
        kv = eng.info["kv_bytes_local"]
        assert 1024 <= ctx <= 131072 and ctx % 64 == 0
        assert kv < 0.9 * total
        if total > 200 * (1 << 30):   # MI355X: 288 GB
            assert kv > 0.5 * total, (ctx, kv, total)
        eng.start([[5, 6, 7]])
        eng.decode(2)


def test_bench_contract_line(cuda, native):
    """bench.py prints ONE JSON line with the driver's keys (small model, few steps)."""
    import json as _json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--model", "tinyllama", "--ftype", "Q4_K_M",
                        "--steps", "3", "--warmup", "1", "--mb-size", "4", "--prompt-len", "16", "--no-secondary"],
                       capture_output=True, text=True, timeout=240, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = _json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
    assert d["config"]["parallelism"] == "pp1" and d["config"]["global_batch"] == 4


def test_bench_dump_outputs(cuda, native, tmp_path):
    """bench.py --dump-outputs DIR: a plain run (no `secondary`) of exactly --steps timed rounds, then
    the generated tokens (float64) and the last round's logits (float32) as .npy; the logits' greedy
    argmax is every sequence's last token."""
    import json as _json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--model", "tinyllama",
                        "--ftype", "Q4_K_M", "--steps", "3", "--warmup", "1", "--mb-size", "4", "--prompt-len", "16",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=240, cwd=repo)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = _json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and "secondary" not in d
    assert sorted(os.listdir(out)) == ["logits.npy", "logits_rows.npy", "tokens.npy"]
    toks, logits, rows = (np.load(out / f) for f in ("tokens.npy", "logits.npy", "logits_rows.npy"))
    assert toks.dtype == np.float64 and toks.shape == (4, 1 + 1 + 3)   # prompt's token + warmup + steps
    assert logits.dtype == np.float32 and logits.shape == (4, 32000) and np.isfinite(logits).all()
    assert rows.tolist() == [0, 1, 2, 3]
    assert ((toks >= 0) & (toks < 32000) & (toks == np.round(toks))).all()
    assert logits.argmax(axis=1).tolist() == toks[:, -1].tolist()


def test_bench_two_ranks_torchrun(cuda, native):
    """The N > 1 bench path end to end on one GPU: torchrun with 2 ranks (both on GPU 0, gloo
    process group, TCP stage links -- RCCL refuses two ranks of one communicator on one GPU),
    init_from_torchrun, the MAX-over-ranks bracket and the JSON line with the data plane the
    engine reports (2 stages, 3 micro-batches, link kind, torch world size)."""
    import json as _json
    import os
    import socket
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(repo, "bench.py"),
           "--gpus", "2", "--same-device", "--model", "tinyllama", "--ftype", "Q4_K_M", "--steps", "3",
           "--warmup", "1", "--mb-size", "4", "--prompt-len", "16", "--set", f"base_port={port + 7}", "--no-secondary"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=repo)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = _json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0
    assert d["config"]["parallelism"] == "pp2" and d["config"]["micro_batches"] == 3
    assert d["config"]["global_batch"] == 12 and len(d["config"]["stages"]) == 2
    assert d["link"]["kind"] == ["tcp"] and d["link"]["torch_pg_world"] == 2 and d["link"]["links_per_rank"] == 2


@pytest.mark.parametrize("gpus,link", [(2, "auto"), (3, "rccl")])
def test_bench_inprocess_same_device(cuda, native, gpus, link):
    """`python bench.py --gpus N` WITHOUT a launcher runs PP=N in one process (engine mode "local",
    one host thread per stage).  --same-device puts every stage on GPU 0: link auto picks the
    peer-copy LocalLink; link rccl asks ncclCommInitAll for the pairs, RCCL refuses a duplicate GPU,
    and the engine falls back to LocalLinks and says so in link.fallback."""
    import json as _json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(repo, "bench.py"), "--gpus", str(gpus), "--same-device", "--link", link,
           "--model", "tinyllama", "--ftype", "Q4_K_M", "--steps", "3", "--warmup", "1", "--mb-size", "4",
           "--prompt-len", "16", "--no-secondary"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=repo, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = _json.loads(lines[0])
    assert d["n_gpus"] == gpus and d["value"] > 0 and "secondary" not in d
    assert d["config"]["parallelism"] == f"pp{gpus}" and d["config"]["micro_batches"] == gpus + 1
    assert len(d["config"]["stages"]) == gpus
    L = d["link"]
    assert L["launcher"] == "in-process" and L["engine_mode"] == "local" and L["devices"] == [0]
    assert L["kind"] == ["local"] and L["comm_nranks"] == [0] and L["links_per_rank"] == 2 * gpus
    assert L["act_dtype"] == "f32" and L["wire_bytes_per_token"] == 2048 * 4   # same GPU: f32 boundary
    assert ("fallback" in L) == (link == "rccl")


def test_local_link_single_copy_cross_stage(cuda, native, model_dir):
    """The posted-queue LocalLink (one device copy per message, receiver reads the sender's buffer):
    PP=3 on one GPU with 3 micro-batches and ring tokens generates what PP=1 generates."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    rng = np.random.default_rng(21)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (9, 3, 17, 5, 11, 2)]
    with Engine(gguf=path, max_ctx=128, n_mb=3, mb_size=2, prefill_chunk=16) as eng:
        ref, _ = eng.generate(prompts, 9)
    with Engine(gguf=path, max_ctx=128, n_mb=3, mb_size=2, prefill_chunk=16, stages=3, devices=[0, 0, 0],
                link="local", split="even") as eng:
        out, _ = eng.generate(prompts, 9)
        h = eng.health()
    assert out == ref
    assert all(s["link"] == "local" and s["msgs_sent"] > 0 for s in h["stages"])


@pytest.mark.parametrize("n_msgs,n_bufs,delay_us", [(200, 2, 300), (300, 100, 50), (40, 1, 2000)])
def test_local_link_posted_queue_delayed_receiver(cuda, native, n_msgs, n_bufs, delay_us):
    """LocalLink's posted queue under a slow receiver: messages arrive in order with their own
    bytes, senders cycling 1-100 buffers never overwrite one before its message has been copied
    (wait_consumed), and more messages than the queue depth (64) push back instead of failing."""
    assert native.mp_local_link_selftest(0, n_msgs, 1 << 16, n_bufs, delay_us) == 0


@pytest.mark.parametrize("stages", [1, 2])
def test_continuous_batching(cuda, native, model_dir, stages):
    """HIP stages: sequences admitted between decode rounds (row-selective head, ring tokens,
    per-slot positions) and a recycled slot generate what each generates alone."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    rng = np.random.default_rng(12)
    P = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (9, 30, 5, 17, 12)]
    alone = []
    with Engine(gguf=path, max_ctx=128, prefill_chunk=16) as eng:
        for p in P:
            o, _ = eng.generate([p], 10)
            alone.append(o[0])
    kw = dict(gguf=path, max_ctx=128, n_mb=2, mb_size=2, prefill_chunk=16, stages=stages,
              devices=[0] * stages, link="local", split="even")
    with Engine(**kw) as eng:
        eng.start([P[0], P[1]])
        eng.decode(3)
        eng.admit([2, 3], [P[2], P[3]])
        eng.decode(5)
        eng.release(0)
        eng.admit([0], [P[4]])
        eng.decode(4)
        t = eng.tokens()
    assert t[1][:10] == alone[1][:10] and t[2][:10] == alone[2][:10] and t[3][:10] == alone[3][:10]
    assert t[0][:5] == alone[4][:5]


def test_gpu_device_probe(cuda, native):
    """Halda device profile of the MI355X: HBM streaming read and the Q4_K decode GEMV rate."""
    from mipipe.engine import device_probe
    d = device_probe(0)
    print(d)
    assert 2000 < d["hbm_read_gbps"] < 9000
    assert 1000 < d["gemv_gbps"] < 9000
    assert d["speed"] == d["gemv_gbps"]


@pytest.mark.parametrize("ftype,mb", [("Q4_K_M", 1), ("Q8_0", 3), ("Q6_K", 1), ("Q4_K_M", 4)])
def test_fused_attention_o_matches_two_kernels(cuda, native, model_dir, ftype, mb):
    """Single-stream decode with attention + o-projection in ONE launch (attention.hip
    attn_o_kernel: W_o slice copied to LDS by DMA during the attention, split-K by kv head with
    atomics into the residual) against the two-kernel path (attn_o_max_ctx=0) and the fp32 oracle.
    tiny-l3: head dim 128, 4 query heads per kv head, the Llama-3-8B attention shape."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-l3", ftype)
    rng = np.random.default_rng(mb)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(5, 90, mb)]
    res = []
    for amc in (0, 512):
        with Engine(gguf=path, max_ctx=256, n_mb=1, mb_size=mb, attn_o_max_ctx=amc) as eng:
            out, _ = eng.generate(prompts, 10)
            res.append((out, eng.logits(rows=mb)))
    assert res[0][0] == res[1][0]
    for r in range(mb):
        assert nmse(res[1][1][r], res[0][1][r]) < 1e-5
    ref = RefLlama.from_gguf(path, device="cuda")
    for r in range(mb):
        toks = [t for t in res[1][0][r] if t >= 0]
        if len(toks) < 10:   # stopped early (end-of-generation token): its logits are not the last step's
            continue
        ref.reset()
        ref.forward(prompts[r], 0)
        pos = len(prompts[r])
        for t in toks[:-1]:
            rl = ref.forward([t], pos)[-1].float().cpu().numpy()
            pos += 1
        assert nmse(res[1][1][r], rl) < 2e-4, (r, nmse(res[1][1][r], rl))


def test_int8_gemm_mode_70b_width(cuda, native, model_dir):
    """int8_gemm=true (opt-in): the M > 64 projections run gemm3<P_I8> on per-row int8
    activations x per-row int8 re-quantized weights (requant_i8_kernel at load).  70B-width 2-layer
    Q4_K model at mb 256: logits within int8 precision of the fp32 oracle (each GEMM ~1.4e-4 NMSE)
    and of the exact f16 engine; tokens of the exact and int8 engines agree on most rows."""
    import os
    from mipipe.engine import Engine
    from mipipe.models.config import CONFIGS
    from mipipe.models.reference import RefLlama
    from mipipe.models.synthetic import write_synthetic_gguf
    cfg = CONFIGS["llama3-70b"].scaled(n_layer=2, vocab=4096, name="l70w2")
    path = os.path.join(str(model_dir), "l70w2-Q4_K.gguf")
    if not os.path.exists(path):
        write_synthetic_gguf(path, cfg, "Q4_K", seed=3, fast_random_blocks=True)
    rng = np.random.default_rng(5)
    mb = 256
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(4, 24, mb)]
    res = {}
    for i8 in (False, True):
        with Engine(gguf=path, max_ctx=64, n_mb=1, mb_size=mb, prefill_chunk=512, int8_gemm=i8) as eng:
            eng.start(prompts)
            lg0 = eng.logits(rows=mb)
            eng.decode(2)
            res[i8] = (lg0, eng.logits(rows=mb), eng.tokens())
    ref = RefLlama.from_gguf(path, device="cuda")
    errs = []
    for r in (0, 63, 64, 130, 255):
        ref.reset()
        rl = ref.forward(prompts[r], 0)[-1].float().cpu().numpy()
        e0 = nmse(res[True][0][r], rl)
        pos = len(prompts[r])
        for t in res[True][2][r][:2]:
            rl = ref.forward([t], pos)[-1].float().cpu().numpy()
            pos += 1
        errs.append((r, e0, nmse(res[True][1][r], rl)))
    print("int8_gemm NMSE vs fp32 (row, prompt, decode):", errs)
    assert all(e0 < 3e-3 and e2 < 3e-3 for _, e0, e2 in errs), errs
    same = sum(res[True][2][r][:3] == res[False][2][r][:3] for r in range(mb))
    assert same >= 0.8 * mb, same
    del ref
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ftype", ["Q4_K", "Q4_K_M"])
def test_moe_grouped_gemm_matches_slices_and_reference(cuda, native, model_dir, ftype):
    """K13: a MoE FFN call of more than 64 tokens (prompt chunks, wide decode micro-batches) runs ONE
    grouped expert GEMM per projection (gemm4.hip MoE mode: rows gathered per routed expert, SwiGLU
    scattered by slot, the down projection weighted into the token).  80 sequences in one
    micro-batch: prefill chunks of 256 rows and decode rounds of 80 rows take it; logits agree with
    the 64-row GEMV slices (moe_gemm=False) and with the fp32 oracle."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-moe", ftype)
    rng = np.random.default_rng(5)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(3, 12, 80)]
    outs, logits = {}, {}
    for grouped in (True, False):
        with Engine(gguf=path, max_ctx=64, mb_size=80, prefill_chunk=256, moe_gemm=grouped) as eng:
            eng.start(prompts)
            logits[grouped] = eng.logits(rows=80).copy()
            eng.decode(3)
            outs[grouped] = eng.tokens()
    assert nmse(logits[True], logits[False]) < 1e-6
    same = sum(a == b for a, b in zip(outs[True], outs[False]))
    assert same >= 76, same   # greedy near-ties may flip a few sequences
    ref = RefLlama.from_gguf(path)
    for i in (0, 37, 79):
        ref.reset()
        rl = ref.forward(prompts[i], 0)[-1].numpy()
        assert nmse(logits[True][i], rl) < 2e-4, i
