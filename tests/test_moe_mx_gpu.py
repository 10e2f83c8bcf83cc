"""mipipe.ops.kernels.moe_gemm_mx (moe_mx.hip) against the exact block-scaled product in f64: the test's own
quant_rows_mx8 bytes and scale bytes, decoded, times the values the B image encodes, gathered by the lists.  The
reference never sees the f16 input: the bounds are tests/test_mxfp4_gpu.py's, for the arithmetic alone."""
import functools

import numpy as np
import pytest
import torch

from mipipe.utils import quants as Q
from test_mxfp4_gpu import _weights, _x, nmse

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _experts(fmt, n, k, E):
    """(images, estride_w, scales, estride_s, fp4, ntiles, nsb, [values the image of expert e encodes, f64 [n][k]]),
    shared.  fp8: the MX-FP8 image of Q4_K experts; fp4: MXFP4 "blocks" experts (a scale byte per block)."""
    from mipipe.ops import kernels as KN
    ws, vals = [], []
    for e in range(E):
        if fmt == "fp4":
            raw, deq = _weights(n, k, "blocks", seed=e)
            ws.append(KN.Mx4Weight(KN.PackedWeight(raw, Q.MXFP4, n, k)))
            vals.append(deq)
        else:
            w = np.random.default_rng(n + k + e).standard_normal((n, k)).astype(np.float32) / k ** 0.5
            ws.append(KN.Mx8Weight(KN.PackedWeight(Q.quantize(w, Q.Q4_K), Q.Q4_K, n, k)))
            vals.append(ws[-1].dense()[:, :k].double().cpu())
    return (*KN.stack_mx_experts(ws), fmt == "fp4", ws[0].ntiles, ws[0].nsb, vals)


def _decode(q, s):
    return q.cpu().view(torch.float8_e4m3fn).double() * torch.exp2(s.cpu().double() - 127).repeat_interleave(32, dim=1)


def _block_scaled(M, k, seed):   # x rows with a power of two per block, as test_gemm_fp4_exact_block_scaled_math
    p = (3 * torch.arange(M)[:, None] + 5 * torch.arange(k // 32)[None, :]) % 13 - 10
    return (_x(M, k, seed).float() * torch.exp2(p.float()).repeat_interleave(32, dim=1)).half()


@pytest.mark.parametrize("M", [65, 129, 200])      # expert 0's rows cross the 64-row tile, the 128-row tile twice
@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_gateup_then_down(cuda, native, fmt, M):
    """tiny-moe widths, top-2 of 4 experts, expert 0 favoured, expert 3 empty; expert 1's count is cut in
    half, so the tail of its list must not be read and those slots' H rows keep their fill."""
    from mipipe.ops import kernels as KN
    D, F, E, K = 512, 768, 4, 2
    gw, gs, gws, gss, fp4, g_nt, g_nsb, gv = _experts(fmt, 2 * F, D, E)
    dw, ds, dws, dss, _, d_nt, d_nsb, dv = _experts(fmt, D, F, E)
    g = torch.Generator().manual_seed(M)
    logits = torch.randn(M, E, generator=g) + torch.tensor([2.5, 0.0, 0.0, -30.0])
    counts, lists, weights = KN.moe_route(logits.cuda(), K)
    cnt = counts.cpu().tolist()
    assert cnt[3] == 0 and sum(cnt) == M * K
    cnt[1] //= 2
    counts = torch.tensor(cnt, dtype=torch.int32, device="cuda")
    xq = KN.quant_rows_mx8(_block_scaled(M, D, 31 + M).cuda())
    h = torch.full((M * K, F), 3.0, dtype=torch.float16, device="cuda")
    KN.moe_gemm_mx(gw, gs, gws, gss, fp4, g_nt, g_nsb, F, KN.EPI_SWIGLU, xq, M, E, K, counts, lists, h=h)
    base = torch.randn(M, D, generator=g)
    y = base.clone().cuda()
    hq = KN.quant_rows_mx8(h)
    KN.moe_gemm_mx(dw, ds, dws, dss, fp4, d_nt, d_nsb, D, KN.EPI_ATOMIC, hq, M, E, K, counts, lists, weights,
                   x_per_slot=True, y=y)
    xd, hd, hc, wts = _decode(*xq), _decode(*hq), h.float().cpu(), weights.cpu().double()
    gi = torch.tensor([16 * (o // 8) + (o % 8) for o in range(F)])   # tile rows 0-7 gate, 8-15 up
    listed, href, y_ref = [], [], torch.zeros(M, D, dtype=torch.float64)
    for e in range(E):
        sl = lists[e, : cnt[e]].long().cpu()
        G = xd[sl // K] @ gv[e].T
        href.append((torch.nn.functional.silu(G[:, gi]) * G[:, gi + 8]).clamp(-65504, 65504))
        listed.append(sl)
        y_ref.index_add_(0, sl // K, wts[sl][:, None] * (hd[sl] @ dv[e].T))
    listed, rest = torch.cat(listed), torch.ones(M * K, dtype=torch.bool)
    rest[listed] = False
    e_h, e_y = nmse(hc[listed], torch.cat(href)), nmse(y.cpu() - base, y_ref)
    print(f"moe_gemm_mx {fmt} M={M} counts {cnt}: NMSE gate/up {e_h:.2e}, down {e_y:.2e}")
    assert rest.sum() > 0 and bool((hc[rest] == 3.0).all())
    assert e_h < 1e-5 and e_y < 1e-8


@pytest.mark.parametrize("fmt,one_hot", [("fp8", False), ("fp4", False), ("fp4", True)])
def test_down_alone(cuda, native, fmt, one_hot):
    """n = 208: 13 tiles, the last 32-column group half empty.  one_hot: each slot's row has one 1.5 at a column
    of its own, so every output is a sum of k exact products and a row gathered from another slot shows."""
    from mipipe.ops import kernels as KN
    n, k, E, K, M = 208, 768, 3, 2, 70
    dw, ds, dws, dss, fp4, nt, nsb, dv = _experts(fmt, n, k, E)
    counts, lists, weights = KN.moe_route(torch.randn(M, E, generator=torch.Generator().manual_seed(9)).cuda(), K)
    xh = torch.zeros(M * K, k, dtype=torch.float16) if one_hot else _block_scaled(M * K, k, 77)
    if one_hot:
        xh[torch.arange(M * K), (37 * torch.arange(M * K) + 5) % k] = 1.5
    xq = KN.quant_rows_mx8(xh.cuda())
    base = torch.zeros(M, n) if one_hot else torch.randn(M, n, generator=torch.Generator().manual_seed(3))
    y = base.clone().cuda()
    KN.moe_gemm_mx(dw, ds, dws, dss, fp4, nt, nsb, n, KN.EPI_ATOMIC, xq, M, E, K, counts, lists, weights, x_per_slot=True, y=y)
    xd, wts = _decode(*xq), weights.cpu()
    ref = torch.zeros(M, n, dtype=torch.float32 if one_hot else torch.float64)
    for e in range(E):
        sl = lists[e, : int(counts[e])].long().cpu()
        prod = xd[sl] @ dv[e].T
        # one_hot: the kernel's own f32 steps (an exact product, times the router weight, two addends per token)
        ref.index_add_(0, sl // K, wts[sl][:, None] * prod.float() if one_hot else wts[sl].double()[:, None] * prod)
    assert torch.equal(y.cpu(), ref) if one_hot else nmse(y.cpu() - base, ref) < 1e-8


def test_launcher_checks(cuda, native):
    """Host-side only: nothing is launched."""
    from mipipe.ops import kernels as KN
    n, k, E, K, M = 208, 768, 3, 2, 70
    dw, ds, dws, dss, fp4, nt, nsb, _ = _experts("fp4", n, k, E)
    counts, lists, weights = KN.moe_route(torch.randn(M, E).cuda(), K)
    xq, y = KN.quant_rows_mx8(torch.zeros(M * K, k, dtype=torch.float16, device="cuda")), torch.zeros(M, n, device="cuda")
    args = (dw, ds, dws, dss, fp4, nt, nsb, n, KN.EPI_ATOMIC, xq, M, E, K, counts, lists, weights)
    with pytest.raises(RuntimeError, match="list_cap"):
        KN.moe_gemm_mx(*args, x_per_slot=True, y=y, list_cap=M - 1)
    with pytest.raises(RuntimeError, match="bfmt"):
        KN.moe_gemm_mx(*args, x_per_slot=True, y=y, bfmt=2)
