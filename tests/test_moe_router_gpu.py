"""The fused router for 64 < E <= 128 experts (csrc/kernels/moe.hip: moe_router_kernel +
moe_bucket_kernel) against fp64 torch, and the grouped expert kernels at the many-experts /
few-rows-per-expert shapes of Qwen3-MoE (128 experts, 8 per token, expert widths 256 and 768)
routed by it.

Logits are compared with x . R^T in fp64 on the same f16-rounded operands, within the f32
accumulation bound K 2^-23 sum |x_i r_i| per element.  Selection, lists and weights are compared with
an fp64 evaluation of the kernel's OWN stored f32 logits, so the expected expert set and order are
exact (ties to the lower index); the weights to 1e-6 relative, plus 2^-126 absolute: a weight below
f32's smallest normal number (a logit 160 under the maximum gives e^-160) is not representable."""
import functools

import numpy as np
import pytest
import torch

from mipipe.utils import quants as Q

pytestmark = pytest.mark.gpu

SENT = -7   # pre-fill of the list buffers: the tails must keep it


def _route_ref(L, k):
    """fp64 routing of f32 logits L [M][E] (cpu): experts [M][k] in descending-logit order, ties to
    the lower index; renormalised softmax weights [M][k]."""
    srt, order = torch.sort(L, dim=-1, descending=True, stable=True)
    idx = order[:, :k]
    p = torch.softmax(L.double(), -1)
    w = torch.gather(p, -1, idx)
    return idx, w / w.sum(-1, keepdim=True)


def _run(x, r, k, pad=3, extra_cap=5):
    from mipipe.ops.kernels import moe_router
    M, E = x.shape[0], r.shape[0]
    buf = torch.full((M, E + pad), float("nan"), dtype=torch.float32, device="cuda")
    lists = torch.full((E, M * k + extra_cap), SENT, dtype=torch.int32, device="cuda")
    logits, counts, lists, weights = moe_router(x, r, k, logits=buf, lists=lists)
    torch.cuda.synchronize()
    return buf, counts, lists, weights


def _check(x, r, k, res=None):
    """Every property of one router call; returns (experts [M][k], weights [M][k]) as the kernel chose."""
    M, K = x.shape
    E = r.shape[0]
    buf, counts, lists, weights = res if res is not None else _run(x, r, k)
    L = buf[:, :E].cpu()
    assert torch.isnan(buf[:, E:]).all(), "padding columns written"
    assert torch.isfinite(L).all()
    ref = x.double() @ r.double().T
    bound = K * 2.0 ** -23 * (x.double().abs() @ r.double().abs().T)
    excess = ((L.double() - ref.cpu()).abs() - bound.cpu()).max()
    assert excess <= 0, float(excess)

    idx, wref = _route_ref(L, k)
    cnt = counts.cpu().long()
    cap = lists.shape[1]
    assert int(cnt.sum()) == M * k
    assert torch.equal(cnt, torch.bincount(idx.reshape(-1), minlength=E))
    lc = lists.cpu()
    live = torch.arange(cap)[None, :] < cnt[:, None]
    assert (lc[~live] == SENT).all(), "list tail written"
    slots = lc[live].long()                                           # expert-major
    owner = torch.arange(E)[:, None].expand(E, cap)[live]
    assert torch.equal(torch.sort(slots).values, torch.arange(M * k))   # every slot listed exactly once
    sel = torch.empty(M * k, dtype=torch.long)
    sel[slots] = owner
    # per token the expert of slot t k + j is the j-th largest logit; hence per expert the set of slots
    assert torch.equal(sel.view(M, k), idx), (sel.view(M, k) != idx).nonzero()[:4]
    w = weights.cpu().double().view(M, k)
    err = (w - wref).abs() - (1e-6 * wref + 2.0 ** -126)
    assert err.max() <= 0, (float(err.max()), float(((w - wref).abs() / wref.clamp_min(1e-300)).max()))
    return sel.view(M, k), w


def _operands(M, E, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).half().cuda()
    r = (torch.randn(E, K, generator=g) / K ** 0.5).half().cuda()   # logits of about unit standard deviation
    return x, r


@pytest.mark.parametrize("K", [256, 2048])
@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("E", [65, 96, 128])
@pytest.mark.parametrize("M", [1, 5, 16, 64, 257])
def test_moe_router_against_fp64(cuda, native, M, E, k, K):
    x, r = _operands(M, E, K, 1000 * M + 10 * E + k + K)
    _check(x, r, k)


@pytest.mark.parametrize("E", [66, 128])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_moe_router_adversarial_rows(cuda, native, E, k):
    """Rows with exactly known logits: x row i is the i-th unit vector, so its logits are column i of
    the router (f16-exact values)."""
    K = 256
    r = torch.zeros(E, K)
    r[:, 0] = 1.0                                           # row 0: all logits equal -> experts 0 .. k-1
    r[:, 1] = -torch.arange(E) / 64.0                       # row 1: strictly descending -> 0 .. k-1
    r[:, 2] = torch.arange(E) / 64.0                        # row 2: ascending -> E-1, E-2, ..
    r[:, 3] = torch.arange(E) / 256.0; r[63, 3] = r[64, 3] = 5.0     # maxima straddling lanes 63 | 0 of the two halves
    r[:, 4] = torch.arange(E) / 256.0; r[64, 4] = r[65, 4] = 5.0     # ... and indices 64 / 65 (lanes 0 / 1, upper half)
    r[:, 5] = -80.0; r[[3, 63, 64, E - 1], 5] = 80.0        # +-80: softmax must not overflow or lose the top
    r[:, 6] = 2.0; r[0, 6] = r[64, 6] = 1.0                 # ties everywhere but two holes
    r[:, 7] = -torch.arange(E) / 64.0; r[10, 7] = r[E - 1, 7] = r[64, 7] = 3.0
    n = 8
    x = torch.zeros(n + 1, K)
    x[torch.arange(n), torch.arange(n)] = 1.0               # (row 8 = 0: all logits 0 -> experts 0 .. k-1)
    sel, w = _check(x.half().cuda(), r.half().cuda(), k)
    first = list(range(k))
    assert sel[0].tolist() == first and sel[1].tolist() == first and sel[8].tolist() == first
    assert sel[2].tolist() == [E - 1 - j for j in range(k)]
    assert sel[3].tolist()[:2] == [63, 64][:k] and sel[4].tolist()[:2] == [64, 65][:k]
    assert sel[5].tolist() == ([3, 63, 64, E - 1] + [0, 1, 2, 4])[:k]
    assert sel[6].tolist() == [1, 2, 3, 4, 5, 6, 7, 8][:k]
    assert sel[7].tolist()[:3] == [10, 64, E - 1][:k]
    np.testing.assert_allclose(w[0].numpy(), 1.0 / k, rtol=1e-6)
    top = min(k, 4)
    np.testing.assert_allclose(w[5, :top].numpy(), 1.0 / top, rtol=1e-6)
    assert (w[5, top:] < 1e-30).all()


@pytest.mark.parametrize("M,E,k,K", [(257, 128, 8, 2048), (33, 65, 4, 256)])
def test_moe_router_bitwise_repeatable(cuda, native, M, E, k, K):
    x, r = _operands(M, E, K, 7)
    a, b = _run(x, r, k), _run(x, r, k)
    assert torch.equal(a[0][:, :E], b[0][:, :E]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    big = torch.iinfo(torch.int32).max   # order inside a list is free: compare the lists sorted
    sa, sb = (torch.sort(torch.where(t[2] == SENT, big, t[2]), dim=1).values for t in (a, b))
    assert torch.equal(sa, sb)


def test_moe_router_prefill_chunk(cuda, native):
    """M k = 2048 * 8 slots through the single-workgroup bucketing, with a skewed router: a shared
    component of x lifts expert 5's logit by 4, so nearly every token lists it."""
    M, E, k, K = 2048, 128, 8, 256
    x, r = _operands(M, E, K, 11)
    x[:, 0] = 4.0
    r[:, 0] = 0.0
    r[5, 0] = 1.0
    sel, _ = _check(x, r, k)
    assert torch.bincount(sel.reshape(-1), minlength=E)[5] > M // 2


# ---------------------------------------------------------------- grouped expert kernels, E = 128

D, E_N, K_TOP = 512, 128, 8


def nmse(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


@functools.lru_cache(maxsize=None)
def _experts(qt, F):
    """E_N experts' gate/up [2 F][D] and down [D][F] as two packed matrices of random blocks (the
    experts back to back: whole 16-row tiles each), and their dense f16 images per expert."""
    from mipipe.ops.kernels import PackedWeight
    gu = PackedWeight.random(qt, E_N * 2 * F, D, seed=3)
    dn = PackedWeight.random(qt, E_N * D, F, seed=4)
    torch.cuda.synchronize()
    return gu, dn, gu.unpack().view(E_N, 2 * F, D), dn.unpack().view(E_N, D, F)


@functools.lru_cache(maxsize=None)
def _routed(M):
    """x [M][D] and its routing by the fused router (shared by the cases of one M, left unchanged)."""
    from mipipe.ops.kernels import moe_router
    x, r = _operands(M, E_N, D, 40 + M)
    logits, counts, lists, weights = moe_router(x, r, K_TOP)
    torch.cuda.synchronize()
    return x, counts, lists, weights


@pytest.mark.parametrize("qt", [Q.Q4_K, Q.Q6_K], ids=["Q4_K", "Q6_K"])
@pytest.mark.parametrize("F", [256, 768])
@pytest.mark.parametrize("M", [3, 64, 80, 256])
def test_moe_expert_kernels_128_experts(cuda, native, M, F, qt):
    """M <= 64: the workgroup-shared grouped GEMV (the decode route, down unsplit and split over K);
    M > 64: the grouped gemm4 (96-row tiles, 2.5 / 16 routed rows per expert on average).  Expert
    widths of 1 and 3 super-blocks: shorter than the kernels' load pipelines.  Bounds of
    test_moe_gemm_gpu.py: NMSE 1e-4 on the SwiGLU output, 1e-5 on the down output given the kernel's
    own h."""
    from mipipe.ops.kernels import moe_gemm, moe_gemv, EPI_SWIGLU, EPI_ATOMIC
    gu, dn, gu_d, dn_d = _experts(qt, F)
    x, counts, lists, weights = _routed(M)
    cnt = counts.cpu().tolist()
    assert sum(cnt) == M * K_TOP
    if M == 3:
        assert sum(c == 0 for c in cnt) >= E_N // 4   # idle experts: their workgroups exit early
    gbytes, dbytes = gu.dev.numel() // E_N, dn.dev.numel() // E_N
    g_nt, d_nt = gu.ntiles // E_N, dn.ntiles // E_N
    base = torch.randn(M, D, generator=torch.Generator().manual_seed(M)).cuda()
    gi = torch.tensor([16 * (o // 8) + (o % 8) for o in range(F)], device="cuda")
    for nsplit in ((1, dn.nsb) if M <= 64 and dn.nsb > 1 else (1,)):
        h = torch.zeros(M * K_TOP, dn.k_pad, dtype=torch.float16, device="cuda")
        y = base.clone()
        if M <= 64:
            moe_gemv(gu.dev, gbytes, gu.ptype, g_nt, gu.nsb, F, EPI_SWIGLU, x, M, E_N, K_TOP, counts, lists, weights, h=h)
            moe_gemv(dn.dev, dbytes, dn.ptype, d_nt, dn.nsb, D, EPI_ATOMIC, h, M, E_N, K_TOP, counts, lists, weights,
                     x_per_slot=True, y=y, nsplit=nsplit)
        else:
            moe_gemm(gu.dev, gbytes, gu.ptype, g_nt, gu.nsb, F, EPI_SWIGLU, x, M, E_N, K_TOP, counts, lists, weights, h=h)
            moe_gemm(dn.dev, dbytes, dn.ptype, d_nt, dn.nsb, D, EPI_ATOMIC, h, M, E_N, K_TOP, counts, lists, weights,
                     x_per_slot=True, y=y)
        torch.cuda.synchronize()
        y_ref = torch.zeros(M, D, dtype=torch.float64, device="cuda")
        h_err = h_sq = 0.0
        for e in range(E_N):
            if cnt[e] == 0:
                continue
            sl = lists[e, : cnt[e]].long()
            tok = sl // K_TOP
            G = x[tok].float() @ gu_d[e].float().T
            href = torch.nn.functional.silu(G[:, gi]) * G[:, gi + 8]
            hk = h[sl, :F].float()
            h_err += float(((hk - href) ** 2).sum())
            h_sq += float((href ** 2).sum())
            y_ref.index_add_(0, tok, (weights[sl][:, None] * (hk @ dn_d[e].float().T)).double())
        assert h_err / h_sq < 1e-4, (nsplit, h_err / h_sq)
        assert nmse((y - base).cpu(), y_ref.cpu()) < 1e-5, (nsplit, nmse((y - base).cpu(), y_ref.cpu()))
