"""The qkv split-K reduction in its init form (csrc/runtime/hip_stage.cpp, layer_forward): when every
qkv segment stores split-K partials, the attention norm launch no longer fills q|k|v with the bias and
the reductions write q|k|v = bias + partials.

Model: a 3-layer Qwen2-style synthetic (a qkv bias) of width 2048, the narrowest whose qkv GEMMs split
at all (32 stages of K); the Q4_K_M mix gives qkv one Q4_K segment in layers 0-1 and two segments of
different types in layer 2, each reducing its own columns.  65 and 129 rows per micro-batch.

The comparison the engine can express: `gemm_splitk_store` false runs the same GEMMs whole-K onto the
bias fill, so its sums have another order than the split ones and the two settings are not bitwise
comparable, with or without `deterministic`.  Both settings are therefore held against the fp32
reference model at the engine tests' NMSE bound, and the init form against itself run to run,
bitwise, under `deterministic`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


def _run(path, prompts, mb, **kw):
    from mipipe.engine import Engine
    with Engine(gguf=path, max_ctx=64, n_mb=1, mb_size=mb, prefill_chunk=256, deterministic=True, **kw) as eng:
        eng.start(prompts)
        lg0 = eng.logits(rows=mb)
        eng.decode(2)
        return lg0, eng.logits(rows=mb), eng.tokens()


@pytest.fixture(scope="module")
def qwen2(model_dir):
    import os
    from mipipe.models.config import CONFIGS
    from mipipe.models.synthetic import write_synthetic_gguf
    cfg = CONFIGS["tiny-qwen2"].scaled(n_layer=3, d_model=2048, n_head=16, n_head_kv=4, d_ff=2048, name="qwen2-w2048")
    path = os.path.join(str(model_dir), "qwen2-w2048-Q4_K_M.gguf")
    if not os.path.exists(path):
        write_synthetic_gguf(path, cfg, "Q4_K_M", seed=4, fast_random_blocks=True)
    return path, cfg


@pytest.mark.parametrize("mb", [65, 129])
def test_qkv_reduce_init_engine(cuda, native, qwen2, mb):
    from mipipe.models.reference import RefLlama
    from mipipe.ops.kernels import gemm4_plan, pack_type, EPI_ATOMIC
    from mipipe.utils import quants as Q
    path, cfg = qwen2
    assert cfg.qkv_bias
    # the route under test exists at this shape: the decode qkv GEMMs (K = d_model) split
    # (q|k|v in one Q4_K segment, or q|k Q4_K and v Q6_K in the layers the mix promotes)
    q_dim, kv_dim = cfg.n_head * cfg.hd, cfg.n_head_kv * cfg.hd
    for qt, n in ((Q.Q4_K, q_dim + 2 * kv_dim), (Q.Q4_K, q_dim + kv_dim), (Q.Q6_K, kv_dim)):
        pl = gemm4_plan(pack_type(qt), EPI_ATOMIC, mb, n // 16, cfg.d_model // 256, True, True)
        assert pl["ok"] and pl["nsplit"] >= 2, pl
    rng = np.random.default_rng(9)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(3, 9, mb)]
    a0, a2, ta = _run(path, prompts, mb, gemm_splitk_store=True)
    b0, b2, tb = _run(path, prompts, mb, gemm_splitk_store=True)
    assert np.array_equal(a0, b0) and np.array_equal(a2, b2) and ta == tb
    c0, c2, tc = _run(path, prompts, mb, gemm_splitk_store=False)
    ref = RefLlama.from_gguf(path, device="cuda")
    for r in (0, 1, 63, 64, mb - 1):
        for lg0, lg2, toks in ((a0, a2, ta), (c0, c2, tc)):
            ref.reset()
            rl = ref.forward(prompts[r], 0)[-1].float().cpu().numpy()
            assert nmse(lg0[r], rl) < 2e-4, (r, nmse(lg0[r], rl))
            pos = len(prompts[r])
            for t in toks[r][:2]:   # the engine's own tokens (a near-tie flip would only change the path)
                rl = ref.forward([t], pos)[-1].float().cpu().numpy()
                pos += 1
            assert nmse(lg2[r], rl) < 2e-4, (r, nmse(lg2[r], rl))
