"""mx8_gemm=true (opt-in): the M > 64 projections run gemm_mx_kernel on MX-FP8 activations and weights."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# Per-GEMM NMSE of the format change, as tests/test_gemm_mx8_gpu.py prints it on an MI355X ("vs fp32",
# Q4_K, the largest of M = 65 / 256 / 300).  Nine sequential GEMM stages (2 layers x qkv, o, gate/up,
# down, and the head's input) add up to 9x that if nothing dilutes them; the bound allows 1.5x.
PER_GEMM_NMSE = 1.42e-3
BOUND = 1.5 * 9 * PER_GEMM_NMSE


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


def test_mx8_gemm_mode_70b_width(cuda, native, model_dir):
    """70B-width 2-layer Q4_K model at mb 256: the mode is engaged, stays within the format's error of the
    fp32 oracle, and cannot be combined with int8_gemm.  Token agreement is printed."""
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
    for mx in (False, True):
        with Engine(gguf=path, max_ctx=64, n_mb=1, mb_size=mb, prefill_chunk=512, mx8_gemm=mx) as eng:
            eng.start(prompts)
            lg0 = eng.logits(rows=mb)
            eng.decode(2)
            res[mx] = (lg0, eng.logits(rows=mb), eng.tokens())
    engaged = nmse(res[True][0], res[False][0])
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
    same = sum(res[True][2][r][:3] == res[False][2][r][:3] for r in range(mb))
    print(f"mx8_gemm vs exact engine NMSE {engaged:.2e}; rows with the same 3 tokens: {same} / {mb}")
    print("mx8_gemm NMSE vs fp32 (row, prompt, decode):", errs, "bound", BOUND)
    del ref
    torch.cuda.empty_cache()
    assert engaged > 1e-6
    assert all(e0 < BOUND and e2 < BOUND for _, e0, e2 in errs), errs
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        Engine(gguf=path, max_ctx=64, mb_size=mb, int8_gemm=True, mx8_gemm=True)
