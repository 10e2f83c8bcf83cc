"""Qwen3-MoE family on one MI355X: tiny-qwen3moe (128 experts, 8 per token, expert width 256; the
fused router kernel, the grouped expert GEMV / GEMM) against the pure-torch fp32 oracle, with the
criterion of test_engine_gpu.py: NMSE < 2e-4 on the logits, a token mismatch only on a near-tie.

Routing near-ties.  The engine's hidden state legitimately differs from the fp32 oracle's, so a
k-th / (k+1)-th router logit pair closer than that difference may select another expert, and with
128 experts such pairs are common.  A compared row is EXCUSED when, for that token in any layer, the
oracle's margin l_(k) - l_(k+1) is below w = 8 sqrt(N0) rms(logit row).  N0 is the largest logits
NMSE dense tiny-qwen3 of the same file type reaches against the oracle over the prompt and the 6
decode steps of test_engine_matches_reference_qwen3, measured on an MI355X (docs/PERFORMANCE.md);
the factor 8 is headroom for the MoE layers' own rounding.  At most one of a test's compared rows may
be excused; the prompt seeds below were chosen, by running the oracle alone with greedy tokens, so
that none is."""
import numpy as np
import pytest
import torch

from conftest import make_model

pytestmark = pytest.mark.gpu

# measured (MI355X, dense tiny-qwen3, prompt of 37 + 6 decode steps):
#   Q8_0   1.27e-06  (rows: 1.27e-6 8.9e-7 8.8e-7 9.1e-7 1.06e-6 1.12e-6 1.09e-6)
#   Q4_K_M 5.40e-06  (rows: 5.40e-6 5.36e-6 5.38e-6 4.62e-6 4.18e-6 3.92e-6 3.58e-6)
N0 = {"Q8_0": 1.27e-6, "Q4_K_M": 5.40e-6}


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


def _excused(ref, ftype):
    """The last token of the oracle's latest forward() has a routing near-tie in some layer."""
    w = 8.0 * np.sqrt(N0[ftype])
    return any(m[-1] < w * r[-1] for _, _, m, r in ref.router_margins[-ref.L:])


# prompt seed per file type, and the smallest margin / w over the 7 compared rows x 2 layers of the
# oracle's own greedy run
MAIN_SEED = {"Q8_0": (13, 2.03), "Q4_K_M": (291, 2.11)}


@pytest.mark.parametrize("ftype", ["Q8_0", "Q4_K_M"])
def test_engine_matches_reference_qwen3moe(cuda, native, model_dir, ftype):
    """Prefill of 37 tokens in chunks of 16 (fused router at M = 16 and 5, grouped GEMV) and 6
    single-stream decode steps, graphs on."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-qwen3moe", ftype)
    ref = RefLlama.from_gguf(path)
    rng = np.random.default_rng(MAIN_SEED[ftype][0])
    prompt = [int(t) for t in rng.integers(3, cfg.vocab, 37)]
    excused = 0
    with Engine(gguf=path, max_ctx=256, prefill_chunk=16, graphs=True) as eng:
        m = eng.info["model"]
        assert m["arch"] == "qwen3moe" and m["n_expert"] == 128 and m["n_expert_used"] == 8 and m["qk_norm"]
        eng.start([prompt])
        lg = eng.logits()[0]
        ref.reset()
        rl = ref.forward(prompt, 0)[-1].numpy()
        ex = _excused(ref, ftype)
        excused += ex
        print("prompt nmse", nmse(lg, rl), "excused" if ex else "")
        if not ex:
            assert nmse(lg, rl) < 2e-4, nmse(lg, rl)
        pos = len(prompt)
        for step in range(6):
            tok = eng.tokens()[0][-1]
            rtop = np.sort(rl)[-2:]
            if rl.argmax() != tok and not ex:   # allowed only on a near-tie
                assert rl.max() - rl[tok] < 1e-2 * (abs(rtop).max() + 1), (step, tok, rl.argmax())
            eng.decode(1)
            lg = eng.logits()[0]
            rl = ref.forward([tok], pos)[-1].numpy()
            ex = _excused(ref, ftype)
            excused += ex
            pos += 1
            print("step", step, "nmse", nmse(lg, rl), "excused" if ex else "")
            if not ex:
                assert nmse(lg, rl) < 2e-4, (step, nmse(lg, rl))
    assert excused <= 1, excused


# prompt-set seed per width (Q4_K_M) and the smallest margin / w over the 4 compared rows
MB_SEED = {3: (1, 1.70), 6: (2, 1.50), 80: (21, 1.23)}


def _mb_against_oracle(path, cfg, ftype, mb, seed, **kw):
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    rng = np.random.default_rng(seed)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(2, 25, mb)]
    with Engine(gguf=path, max_ctx=64, n_mb=1, mb_size=mb, prefill_chunk=max(16, 2 * mb), **kw) as eng:
        eng.start(prompts)
        lg0 = eng.logits(rows=mb)
        eng.decode(2)
        lg2 = eng.logits(rows=mb)
        toks = eng.tokens()
    ref = RefLlama.from_gguf(path)
    excused = 0
    for r in (0, mb - 1):
        ref.reset()
        rl = ref.forward(prompts[r], 0)[-1].numpy()
        ex = _excused(ref, ftype)
        excused += ex
        print("row", r, "prompt nmse", nmse(lg0[r], rl), "excused" if ex else "")
        if not ex:
            assert nmse(lg0[r], rl) < 2e-4, (r, nmse(lg0[r], rl))
        pos = len(prompts[r])
        for t in toks[r][:2]:   # the engine's own tokens (a near-tie flip would only change the path)
            rl = ref.forward([t], pos)[-1].numpy()
            pos += 1
        ex = _excused(ref, ftype)
        excused += ex
        print("row", r, "decode nmse", nmse(lg2[r], rl), "excused" if ex else "")
        if not ex:
            assert nmse(lg2[r], rl) < 2e-4, (r, nmse(lg2[r], rl))
    assert excused <= 1, excused


@pytest.mark.parametrize("mb", [3, 6, 80])
def test_microbatch_widths_match_reference_qwen3moe(cuda, native, model_dir, mb):
    """Ragged prompts of 2-24 tokens, two decode rounds; logits of the first and last row against the
    oracle.  Widths 3 / 6 / 80: the M <= 4 gemvs and the 5-64 gemv2 attention projections with the
    grouped expert GEMV, and the > 64 GEMM route with the grouped expert gemm4."""
    path, cfg = make_model(model_dir, "tiny-qwen3moe", "Q4_K_M")
    _mb_against_oracle(path, cfg, "Q4_K_M", mb, MB_SEED[mb][0])


def test_graph_equals_eager_qwen3moe(cuda, native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-qwen3moe", "Q4_K_M")
    prompts = [[5, 6, 7, 8, 9], [100, 200, 300]]
    outs = []
    for graphs in (False, True):
        with Engine(gguf=path, max_ctx=256, n_mb=1, mb_size=2, graphs=graphs) as eng:
            out, _ = eng.generate(prompts, 8)
            outs.append(out)
    assert outs[0] == outs[1]


def test_deterministic_bitwise_qwen3moe(cuda, native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-qwen3moe", "Q4_K_M")
    rng = np.random.default_rng(3)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(5, 40, 3)]
    runs = []
    for _ in range(2):
        with Engine(gguf=path, max_ctx=128, n_mb=1, mb_size=3, prefill_chunk=64, seed=7, deterministic=True) as eng:
            eng.start(prompts)
            eng.decode(3)
            runs.append((eng.logits(rows=3), eng.tokens()))
    assert np.array_equal(runs[0][0], runs[1][0]), float(np.abs(runs[0][0] - runs[1][0]).max())
    assert runs[0][1] == runs[1][1]
    assert np.isfinite(runs[0][0]).all()


def _fp8_round(t):
    return t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(t.dtype)


# The fp8 cache's own noise: the largest logits NMSE of dense tiny-qwen3 Q4_K_M with kv_dtype fp8
# against the oracle with the e4m3-rounded cache, over the prompt and the 6 decode steps of
# test_fp8_kv_cache_matches_reference_qwen3 (measured on an MI355X; rows 1.95e-4 2.47e-4 2.51e-4
# 2.26e-4 2.44e-4 2.61e-4 2.27e-4).  It is 50 times the f16-cache N0: engine and oracle round
# slightly different K / V to e4m3, and a value near a rounding boundary lands a whole fp8 step apart.
N0_FP8 = 2.61e-4
# prompt seed: by the oracle's own greedy run the prompt row and decode steps 0 and 3 are free of
# near-ties (margin / w 1.18, 1.25, 1.05); no seed of 600 scanned has more than 3 such rows
FP8_SEED = 362


def test_fp8_kv_cache_matches_reference_qwen3moe(cuda, native, model_dir):
    """Body and bounds of test_fp8_kv_cache_matches_reference_qwen3 (NMSE < 5e-4 against the oracle
    with the rounded cache, < 2e-2 against the f16-cache engine on the prompt).

    The excusal rule of this file with the hidden-state noise of THIS configuration, N0_FP8: w = 8
    sqrt(N0_FP8) rms = 0.13 rms, which most rows of a 128-expert router fall under (the mean k-th /
    (k+1)-th gap is about 0.06 rms), so the at-most-one-excused condition cannot hold here.  Instead
    the prompt row must be compared and at least 2 of the 7 rows in all.  With the f16-cache N0 (w =
    0.019 rms) a row that rule does not excuse did select another expert: step 5 of seed 11, NMSE
    4.7e-3, after six rows at 0.95e-4 .. 1.8e-4."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    ftype = "Q4_K_M"
    path, cfg = make_model(model_dir, "tiny-qwen3moe", ftype)
    ref = RefLlama.from_gguf(path)
    ref.kv_round = _fp8_round
    prompt = [int(t) for t in np.random.default_rng(FP8_SEED).integers(3, cfg.vocab, 45)]
    w = 8.0 * np.sqrt(N0_FP8)

    def excused():
        return any(m[-1] < w * r[-1] for _, _, m, r in ref.router_margins[-ref.L:])

    compared = 0
    with Engine(gguf=path, max_ctx=256, prefill_chunk=16, kv_dtype="fp8") as eng, \
            Engine(gguf=path, max_ctx=256, prefill_chunk=16) as e16:
        assert eng.info["kv_bytes_local"] * 2 == e16.info["kv_bytes_local"]
        eng.start([prompt])
        e16.start([prompt])
        ref.reset()
        rl = ref.forward(prompt, 0)[-1].numpy()
        assert not excused()
        print("prompt nmse", nmse(eng.logits()[0], rl), "vs f16 cache", nmse(eng.logits()[0], e16.logits()[0]))
        assert nmse(eng.logits()[0], rl) < 5e-4, nmse(eng.logits()[0], rl)
        assert nmse(eng.logits()[0], e16.logits()[0]) < 2e-2
        compared += 1
        pos = len(prompt)
        for step in range(6):
            tok = eng.tokens()[0][-1]
            eng.decode(1)
            rl = ref.forward([tok], pos)[-1].numpy()
            ex = excused()
            pos += 1
            print("step", step, "nmse", nmse(eng.logits()[0], rl), "excused" if ex else "")
            assert np.isfinite(eng.logits()[0]).all()
            if not ex:
                assert nmse(eng.logits()[0], rl) < 5e-4, (step, nmse(eng.logits()[0], rl))
                compared += 1
    assert compared >= 2, compared


def test_pipeline_emulation_matches_pp1_qwen3moe(cuda, native, model_dir):
    """Two stages on one GPU over LocalLink give the tokens of one stage."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-qwen3moe", "Q8_0")
    rng = np.random.default_rng(1)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (9, 40, 3, 17)]
    with Engine(gguf=path, max_ctx=256, n_mb=2, mb_size=2, prefill_chunk=16) as eng:
        ref_out, _ = eng.generate(prompts, 10)
    with Engine(gguf=path, max_ctx=256, n_mb=2, mb_size=2, prefill_chunk=16, stages=2, devices=[0, 0],
                link="local", split="even") as eng:
        assert len(eng.info["stages"]) == 2
        out, st = eng.generate(prompts, 10)
    assert out == ref_out


def test_synthetic_qwen3moe_engine_runs(cuda, native):
    """A synthetic config with 128 experts, 8 per token, and qk_norm generates tokens in range."""
    from mipipe.engine import Engine
    syn = dict(n_layer=2, d_model=1024, n_head=16, n_head_kv=8, head_dim=128, d_ff=768, vocab=4096,
               rope_base=1e6, eps=1e-6, qk_norm=True, n_expert=128, n_expert_used=8)
    with Engine(synthetic=syn, ftype="Q4_K", n_mb=1, mb_size=2, max_ctx=128, prefill_chunk=16) as eng:
        m = eng.info["model"]
        assert m["qk_norm"] and m["head_dim"] == 128 and m["n_expert"] == 128 and m["n_expert_used"] == 8
        out, _ = eng.generate([[1, 2, 3, 4, 5], [6, 7]], 4)
    assert all(len(o) == 4 and all(0 <= t < 4096 for t in o) for o in out)
