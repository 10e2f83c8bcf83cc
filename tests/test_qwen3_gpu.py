"""Qwen3 family on one MI355X: the engine (per-head Q/K RMSNorm kernel before RoPE, head_dim
decoupled from d_model / n_head) against the pure-torch fp32 oracle on every projection route, with
the criterion of test_engine_gpu.py: NMSE < 2e-4 on the logits, a token mismatch only on a near-tie."""
import numpy as np
import pytest
import torch

from conftest import make_model

pytestmark = pytest.mark.gpu


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


@pytest.mark.parametrize("name,ftype", [("tiny-qwen3", "Q4_K_M"), ("tiny-qwen3", "Q8_0"), ("tiny-qwen3-hd64", "Q4_K_M")])
def test_engine_matches_reference_qwen3(cuda, native, model_dir, name, ftype):
    """Prefill (rope_kv + flash attention) and the single-stream gemvs decode path, graphs on."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, name, ftype)
    ref = RefLlama.from_gguf(path)
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(3, cfg.vocab, 37)]
    with Engine(gguf=path, max_ctx=256, prefill_chunk=16, graphs=True) as eng:
        assert eng.info["model"]["qk_norm"] and eng.info["model"]["head_dim"] == cfg.hd
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


def _mb_against_oracle(path, cfg, mb, **kw):
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    rng = np.random.default_rng(5)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(2, 25, mb)]
    with Engine(gguf=path, max_ctx=64, n_mb=1, mb_size=mb, prefill_chunk=max(16, 2 * mb), **kw) as eng:
        eng.start(prompts)
        lg0 = eng.logits(rows=mb)
        eng.decode(2)
        lg2 = eng.logits(rows=mb)
        toks = eng.tokens()
    ref = RefLlama.from_gguf(path)
    for r in (0, mb - 1):
        ref.reset()
        rl = ref.forward(prompts[r], 0)[-1].numpy()
        assert nmse(lg0[r], rl) < 2e-4, (r, nmse(lg0[r], rl))
        pos = len(prompts[r])
        for t in toks[r][:2]:   # the engine's own tokens (a near-tie flip would only change the path)
            rl = ref.forward([t], pos)[-1].numpy()
            pos += 1
        assert nmse(lg2[r], rl) < 2e-4, (r, nmse(lg2[r], rl))


@pytest.mark.parametrize("mb", [3, 6, 80])
def test_microbatch_widths_match_reference_qwen3(cuda, native, model_dir, mb):
    """Ragged prompts of 2-24 tokens, two decode rounds; logits of the first and last row against the
    oracle.  Widths 3 / 6 / 80: the M <= 4 gemvs, the 5-64 gemv2 and the > 64 GEMM routes."""
    path, cfg = make_model(model_dir, "tiny-qwen3", "Q4_K_M")
    _mb_against_oracle(path, cfg, mb)


@pytest.mark.parametrize("mb", [1, 3])
def test_fused_norm_option_matches_reference_qwen3(cuda, native, model_dir, mb):
    """fused_norm=True: a q/k-normed layer cannot defer the attn_norm into the decode attention (the
    head norm needs final q|k|v), so it takes the standalone norm; the split-K accumulator is still
    cleared for the next layer."""
    path, cfg = make_model(model_dir, "tiny-qwen3", "Q4_K_M")
    _mb_against_oracle(path, cfg, mb, fused_norm=True, graphs=True)
    _mb_against_oracle(path, cfg, mb, fused_norm=True, small_gemv=False)


def test_graph_equals_eager_qwen3(cuda, native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-qwen3", "Q4_K_M")
    prompts = [[5, 6, 7, 8, 9], [100, 200, 300]]
    outs = []
    for graphs in (False, True):
        with Engine(gguf=path, max_ctx=256, n_mb=1, mb_size=2, graphs=graphs) as eng:
            out, _ = eng.generate(prompts, 8)
            outs.append(out)
    assert outs[0] == outs[1]


def test_deterministic_bitwise_qwen3(cuda, native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-qwen3", "Q4_K_M")
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


def test_fp8_kv_cache_matches_reference_qwen3(cuda, native, model_dir):
    """Body and bounds of test_fp8_kv_cache_matches_reference: the oracle's cached K (after the head
    norm and RoPE) and V are rounded to e4m3 the same way."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-qwen3", "Q4_K_M")
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


def test_pipeline_emulation_matches_pp1_qwen3(cuda, native, model_dir):
    """Two stages on one GPU over LocalLink give the tokens of one stage."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-qwen3", "Q8_0")
    rng = np.random.default_rng(1)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (9, 40, 3, 17)]
    with Engine(gguf=path, max_ctx=256, n_mb=2, mb_size=2, prefill_chunk=16) as eng:
        ref_out, _ = eng.generate(prompts, 10)
    with Engine(gguf=path, max_ctx=256, n_mb=2, mb_size=2, prefill_chunk=16, stages=2, devices=[0, 0],
                link="local", split="even") as eng:
        assert len(eng.info["stages"]) == 2
        out, st = eng.generate(prompts, 10)
    assert out == ref_out


def test_synthetic_qwen3_engine_runs(cuda, native):
    """A synthetic config with qk_norm (all-ones norm weights, head_dim != d_model / n_head) runs."""
    from mipipe.engine import Engine
    syn = dict(n_layer=2, d_model=1024, n_head=16, n_head_kv=8, head_dim=128, d_ff=3072, vocab=4096,
               rope_base=1e6, eps=1e-6, qk_norm=True)
    with Engine(synthetic=syn, ftype="Q4_K", n_mb=1, mb_size=2, max_ctx=128, prefill_chunk=16) as eng:
        assert eng.info["model"]["qk_norm"] and eng.info["model"]["head_dim"] == 128
        out, _ = eng.generate([[1, 2, 3, 4, 5], [6, 7]], 4)
    assert all(len(o) == 4 and all(0 <= t < 4096 for t in o) for o in out)
