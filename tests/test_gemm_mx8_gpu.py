"""MX-FP8 GEMM mode (csrc/kernels/gemm_mx.hip): the quantizer equals a torch reference of the format bit
for bit (scaling f16 by a power of two is exact, both round to nearest even); the GEMM is checked against
the f64 product of the decoded operands, the format change against the fp32 product of the K-quant weights."""
import math

import numpy as np
import pytest
import torch

from mipipe.utils import quants as Q

pytestmark = pytest.mark.gpu


def nmse(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


def mx8_ref(x):
    """The format on the CPU: (scale bytes [M][K / 32], e4m3 elements [M][K]) of x [M][K]."""
    M, K = x.shape
    xb = x.float().view(M, K // 32, 32)
    amax = xb.abs().amax(2)
    m, ex = torch.frexp(amax)                                  # amax = m 2^ex, m in [0.5, 1)
    e = ex - 9 + (m > 0.875).int()                             # smallest s = 2^e with amax / s <= 448 = 0.875 * 2^9
    E = torch.where(amax == 0, torch.full_like(e, 127), (e + 127).clamp(0, 254))
    q = (xb / torch.exp2(E.float() - 127)[..., None]).to(torch.float8_e4m3fn)
    return E.to(torch.uint8), q.view(M, K)


def mx8_decode(q, s):
    """f64 values of e4m3 bytes q [M][K] (uint8) and scale bytes s [M][K / 32]."""
    return q.cpu().view(torch.float8_e4m3fn).double() * torch.exp2(s.cpu().double() - 127).repeat_interleave(32, dim=1)


def _setup(qt, n, k, M, seed):
    from mipipe.ops.kernels import PackedWeight, Mx8Weight
    rng = np.random.default_rng(seed)
    wf = (rng.standard_normal((n, k)) / math.sqrt(k)).astype(np.float32)
    raw = Q.quantize(wf, qt)
    deq = torch.from_numpy(Q.dequantize(raw, qt).reshape(n, k))
    w = PackedWeight(raw, qt, n, k)
    g = torch.Generator().manual_seed(seed)
    xh = torch.zeros(M, w.k_pad, dtype=torch.float16)
    xh[:, :k] = torch.randn(M, k, generator=g).half()
    return Mx8Weight(w), deq, xh


def test_quant_rows_mx8_matches_format(cuda, native):
    from mipipe.ops.kernels import quant_rows_mx8
    x = torch.randn(37, 768, generator=torch.Generator().manual_seed(1)) * torch.linspace(0.1, 10, 37)[:, None]
    x[5, 64:96] = 0                      # an all-zero block: E = 127
    x[9, 130] = 1000 * x[9, 130].sign() * x[9].abs().max()   # a single 1000x outlier in its block
    x = x.half()
    q, s = quant_rows_mx8(x.cuda())
    E, ref = mx8_ref(x)
    assert int(s[5, 2]) == 127 and torch.equal(s.cpu(), E)
    assert torch.equal(q.cpu().view(torch.float8_e4m3fn).float(), ref.float())


@pytest.mark.parametrize("qt", [Q.Q4_K, Q.Q6_K])
@pytest.mark.parametrize("M", [65, 256, 300])
def test_gemm_mx8_exact_block_scaled_math(cuda, native, qt, M):
    from mipipe.ops.kernels import gemm_mx8, quant_rows_mx8, EPI_STORE, EPI_ATOMIC, EPI_SWIGLU
    n, k = 512, 2048
    w8, deq, xh = _setup(qt, n, k, M, 31 + M + qt)
    # every block of every row gets its own power of two (and so its own scale byte)
    p = (3 * torch.arange(M)[:, None] + 5 * torch.arange(k // 32)[None, :]) % 13 - 6
    xh = (xh.float() * torch.exp2(p.float()).repeat_interleave(32, dim=1)).half()
    q, s = quant_rows_mx8(xh.cuda())
    ref = mx8_decode(q, s) @ w8.dense().double().cpu().T
    y = gemm_mx8(w8, xq=(q, s), epi=EPI_STORE).cpu()
    base = torch.randn(M, n)
    y2 = gemm_mx8(w8, xq=(q, s), epi=EPI_ATOMIC, y=base.clone().cuda()).cpu()
    h = gemm_mx8(w8, xq=(q, s), epi=EPI_SWIGLU).cpu()
    gi = torch.tensor([16 * (o // 8) + (o % 8) for o in range(n // 2)])
    href = torch.nn.functional.silu(ref[:, gi]) * ref[:, gi + 8]
    # the format change itself: MX-FP8 x and w against the fp32 product of the K-quant weights
    full = xh[:, :k].float() @ deq.T
    errs = nmse(y, ref), nmse(y2 - base, ref), nmse(h.float(), href), nmse(y, full)
    print(f"mx8 ({Q.TYPE_NAMES[qt]}, M={M}): store {errs[0]:.2e} atomic {errs[1]:.2e} swiglu {errs[2]:.2e} "
          f"vs fp32 {errs[3]:.2e}")
    assert errs[0] < 1e-9      # f32 accumulation of K = 2048 exact products: ~K 2^-48 = 7e-12
    assert errs[1] < 1e-8      # + the f32 add onto the base
    assert errs[2] < 1e-5      # f16 output rounding
    assert errs[3] < 3e-3      # 2x the 1.40e-3 of the format on Gaussian data (CPU simulation)


def test_gemm_mx8_outlier_channels_stay_local(cuda, native):
    """Two x channels at 300x and 1000x: the other channels keep their precision (per-row int8 cannot)."""
    from mipipe.ops.kernels import gemm_mx8, quant_rows_mx8, EPI_STORE
    n, k, M = 512, 2048, 256
    w8, deq, xh = _setup(Q.Q4_K, n, k, M, 77)
    out = [301, 1500]
    xh[:, out[0]] *= 300
    xh[:, out[1]] *= 1000
    q, s = quant_rows_mx8(xh.cuda())
    y = gemm_mx8(w8, xq=(q, s), epi=EPI_STORE).cpu().double()
    xd, wd = mx8_decode(q, s), w8.dense().double().cpu()
    rest = xh[:, :k].double()
    rest[:, out] = 0
    err = nmse(y - xd[:, out] @ wd[:, out].T, rest @ deq.double().T)
    print(f"mx8 outlier channels: NMSE of the other channels' contribution {err:.2e}")
    assert err < 3e-3
