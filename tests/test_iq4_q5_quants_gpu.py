"""IQ4_XS / IQ4_NL / Q5_0 / Q5_1 on the GPU: the unpack kernel and the embedding gather against the
numpy dequantizer, every GEMV / GEMM route (gemvs M <= 4, gemv2 5..64, the 64 x 64 GEMM, gemm3, gemm4
with its row tiles and split-K partial stores, the MoE GEMV / grouped GEMM) against the fp32 product
with the dequantized weights, a ragged K (57 blocks of 32) on every route for the 32-weight-block
types, and the engine on the IQ4_XS / Q5_0 / Q5_1 file types against the torch fp32 oracle.

Every GEMV / GEMM case runs on quantized gaussian weights and on random block bytes (every quant,
high-bit and scale field live).  Bounds are the existing kernel tests': NMSE < 1e-5 (1e-4 for the f16
SwiGLU output of the GEMMs), 2e-4 for engine logits."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import make_model
from mipipe.utils import quants as Q

pytestmark = pytest.mark.gpu

NEW = [Q.IQ4_XS, Q.IQ4_NL, Q.Q5_0, Q.Q5_1]
BLOCK32 = [Q.IQ4_NL, Q.Q5_0, Q.Q5_1]
KINDS = ["quantized", "random_blocks"]


def nmse(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


@functools.lru_cache(maxsize=None)
def _weights(qt, kind, n, k, seed=0):
    """(raw GGUF bytes, dequantized [n][k] f32): computed once per shape, shared, never modified."""
    rng = np.random.default_rng(1000 * seed + 10 * qt + (kind == "quantized"))
    if kind == "quantized":
        raw = Q.quantize((rng.standard_normal((n, k)) / math.sqrt(k)).astype(np.float32), qt)
    else:
        raw = Q.random_blocks(rng, qt, n, k, 1.0 / math.sqrt(k))
    return raw, torch.from_numpy(Q.dequantize(raw, qt).reshape(n, k))


def _x(M, k, k_pad, seed):
    g = torch.Generator().manual_seed(seed)
    xh = torch.zeros(M, k_pad, dtype=torch.float16)
    xh[:, :k] = torch.randn(M, k, generator=g).half()
    return xh


def _xn(xf, gamma, eps):
    rs = torch.rsqrt((xf * xf).mean(-1, keepdim=True) + eps)
    return (xf * rs * gamma).half().float()


@pytest.fixture
def tuning(native):
    from mipipe.ops.kernels import set_gemm3_tuning
    yield set_gemm3_tuning
    set_gemm3_tuning(0, 0, 0, 0)


# ------------------------------------------------------------------------------- dequant kernels
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qt", NEW)
def test_unpack_matches_dequant(cuda, native, qt, kind):
    from mipipe.ops.kernels import PackedWeight
    n, k = 48, 768
    raw, deq = _weights(qt, kind, n, k)
    got = PackedWeight(raw, qt, n, k).unpack().float().cpu()
    torch.testing.assert_close(got, deq, rtol=2e-3, atol=2e-3 * deq.abs().max().item())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qt", NEW)
def test_embed(cuda, native, qt, kind):
    from mipipe.ops.kernels import embed
    V, d = 50, 512
    raw, deq = _weights(qt, kind, V, d)
    tok = torch.tensor([3, 0, 49, 17], dtype=torch.int32)
    x = embed(torch.from_numpy(raw).cuda(), qt, d, tok.cuda()).cpu()
    torch.testing.assert_close(x, deq[tok.long()], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------- gemvs (M <= 4)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qt", NEW)
@pytest.mark.parametrize("M", [1, 4])
def test_gemvs(cuda, native, qt, kind, M):
    """13 tiles (ragged last), 7 super-blocks: STORE with the fused norm and bias, ATOMIC over a
    residual at 1 and 3 k-splits."""
    from mipipe.ops.kernels import PackedWeight, gemv_small, EPI_STORE, EPI_ATOMIC
    n, k = 200, 1792
    raw, deq = _weights(qt, kind, n, k)
    w = PackedWeight(raw, qt, n, k)
    g = torch.Generator().manual_seed(M)
    xf = torch.randn(M, k, generator=g) * 3
    gamma = torch.rand(k, generator=g) + 0.5
    bias = torch.randn(n, generator=g)
    y = gemv_small(w, EPI_STORE, xf=xf.cuda(), gamma=gamma.cuda(), eps=1e-5, bias=bias.cuda())
    assert nmse(y.cpu(), _xn(xf, gamma, 1e-5) @ deq.T + bias) < 1e-5
    xh = _x(M, k, w.k_pad, 8 + M)
    base = torch.randn(M, n, generator=g)
    for nsplit in (1, 3):
        y = gemv_small(w, EPI_ATOMIC, x=xh.cuda(), y=base.clone().cuda(), nsplit=nsplit)
        assert nmse(y.cpu(), base + xh[:, :k].float() @ deq.T) < 1e-5, nsplit


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qt", NEW)
@pytest.mark.parametrize("M", [1, 4])
def test_gemvs_swiglu(cuda, native, qt, kind, M):
    from mipipe.ops.kernels import PackedWeight, gemv_small, EPI_SWIGLU
    F, k = 72, 1024
    raw, deq = _weights(qt, kind, 2 * F, k)
    w = PackedWeight(raw, qt, 2 * F, k, gateup=True)
    g = torch.Generator().manual_seed(20 + M)
    xf = torch.randn(M, k, generator=g)
    gamma = torch.rand(k, generator=g) + 0.5
    h = gemv_small(w, EPI_SWIGLU, xf=xf.cuda(), gamma=gamma.cuda(), eps=1e-5)
    xn = _xn(xf, gamma, 1e-5)
    ref = torch.nn.functional.silu(xn @ deq[:F].T) * (xn @ deq[F:].T)
    assert nmse(h.float().cpu(), ref) < 1e-5


# ------------------------------------------------------------------------------- gemv2 (5..64)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qt", NEW)
@pytest.mark.parametrize("M", [5, 17, 33, 64])
def test_gemv(cuda, native, qt, kind, M):
    from mipipe.ops.kernels import PackedWeight, gemv, EPI_STORE, EPI_ATOMIC
    n, k = 200, 1792
    raw, deq = _weights(qt, kind, n, k)
    w = PackedWeight(raw, qt, n, k)
    xh = _x(M, k, w.k_pad, 30 + M)
    ref = xh[:, :k].float() @ deq.T
    assert nmse(gemv(w, xh.cuda(), EPI_STORE).cpu(), ref) < 1e-5
    base = torch.randn(M, n, generator=torch.Generator().manual_seed(M))
    y = gemv(w, xh.cuda(), EPI_ATOMIC, y=base.clone().cuda(), nsplit=3)
    assert nmse(y.cpu(), base + ref) < 1e-5


# ------------------------------------------------------------------------------- GEMMs (M > 64)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qt", NEW)
def test_gemm1(cuda, native, qt, kind):
    from mipipe.ops.kernels import PackedWeight, gemm, EPI_STORE
    n, k, M = 200, 1792, 100
    raw, deq = _weights(qt, kind, n, k)
    w = PackedWeight(raw, qt, n, k)
    xh = _x(M, k, w.k_pad, 41)
    assert nmse(gemm(w, xh.cuda(), EPI_STORE, v=1).cpu(), xh[:, :k].float() @ deq.T) < 1e-5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qt", NEW)
@pytest.mark.parametrize("M", [100, 300])
def test_gemm3(cuda, tuning, qt, kind, M):
    """The 16x16x32 LDS-DMA GEMM (prefill_gemm_v=3) reads the same stage images in its own lane map."""
    from mipipe.ops.kernels import PackedWeight, gemm, EPI_STORE
    n, k = 208, 1280
    raw, deq = _weights(qt, kind, n, k)
    w = PackedWeight(raw, qt, n, k)
    xh = _x(M, k, w.k_pad, M + 2)
    assert nmse(gemm(w, xh.cuda(), EPI_STORE, v=3).cpu(), xh[:, :k].float() @ deq.T) < 1e-5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qt", NEW)
@pytest.mark.parametrize("bm", [0, 96, 256])
@pytest.mark.parametrize("M", [65, 200, 300])
def test_gemm4_tiles(cuda, tuning, qt, kind, bm, M):
    """13 tiles (a partial 256-column group), 5 super-blocks (20 stages), partial row blocks."""
    from mipipe.ops.kernels import PackedWeight, gemm, EPI_STORE, EPI_ATOMIC, EPI_SWIGLU
    tuning(bm, 0, 0, 0)
    n, k = 208, 1280
    raw, deq = _weights(qt, kind, n, k)
    w = PackedWeight(raw, qt, n, k)
    xh = _x(M, k, w.k_pad, M + 1)
    ref = xh[:, :k].float() @ deq.T
    y = gemm(w, xh.cuda(), EPI_STORE, v=4)
    assert nmse(y.cpu(), ref) < 1e-5
    base = torch.randn(M, n, generator=torch.Generator().manual_seed(M))
    y2 = gemm(w, xh.cuda(), EPI_ATOMIC, y=base.clone().cuda(), v=4)
    assert nmse(y2.cpu(), ref + base) < 1e-5
    h = gemm(w, xh.cuda(), EPI_SWIGLU, v=4)
    gi = torch.tensor([16 * (o // 8) + (o % 8) for o in range(n // 2)])
    href = torch.nn.functional.silu(ref[:, gi]) * ref[:, gi + 8]
    assert nmse(h.float().cpu(), href) < 1e-4


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("qt", NEW)
def test_gemm4_splitk_partial_stores(cuda, tuning, qt, kind):
    """Per-split partial stores + the fixed-order reduction: bitwise reproducible run to run."""
    from mipipe.ops.kernels import PackedWeight, gemm_splitk
    n, k, M = 256, 2048, 128
    raw, deq = _weights(qt, kind, n, k)
    w = PackedWeight(raw, qt, n, k)
    xh = _x(M, k, w.k_pad, 3 + M)
    ref = xh[:, :k].float() @ deq.T
    base = torch.randn(M, n, generator=torch.Generator().manual_seed(2))
    outs = []
    for _ in range(2):
        y = base.clone().cuda()
        assert gemm_splitk(w, xh.cuda(), y) >= 2
        outs.append(y.cpu())
    assert nmse(outs[0] - base, ref) < 1e-5
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------- ragged K
@pytest.mark.parametrize("route", ["unpack", "gemvs", "gemv2", "gemm1", "gemm3", "gemm4"])
@pytest.mark.parametrize("qt", BLOCK32)
def test_ragged_k(cuda, tuning, qt, route):
    """K = 1824 = 57 blocks of 32: the last chunk is an eighth full, its other seven blocks are the
    packer's zero fill (d = 0, m = 0) and x is zero-padded to k_pad.  Random block bytes."""
    from mipipe.ops.kernels import PackedWeight, gemv_small, gemv, gemm, EPI_STORE, EPI_ATOMIC
    n, k = 200, 1824
    raw, deq = _weights(qt, "random_blocks", n, k)
    w = PackedWeight(raw, qt, n, k)
    assert w.k_pad == 2048
    if route == "unpack":
        got = w.unpack().float().cpu()
        torch.testing.assert_close(got, deq, rtol=2e-3, atol=2e-3 * deq.abs().max().item())
        return
    M = {"gemvs": 4, "gemv2": 33, "gemm1": 100, "gemm3": 100, "gemm4": 200}[route]
    xh = _x(M, k, w.k_pad, 50 + M)
    ref = xh[:, :k].float() @ deq.T
    if route == "gemvs":
        base = torch.randn(M, n, generator=torch.Generator().manual_seed(M))
        y = gemv_small(w, EPI_ATOMIC, x=xh.cuda(), y=base.clone().cuda(), nsplit=1)
        assert nmse(y.cpu() - base, ref) < 1e-5
    elif route == "gemv2":
        assert nmse(gemv(w, xh.cuda(), EPI_STORE).cpu(), ref) < 1e-5
    else:
        assert nmse(gemm(w, xh.cuda(), EPI_STORE, v={"gemm1": 1, "gemm3": 3, "gemm4": 4}[route]).cpu(), ref) < 1e-5


# ------------------------------------------------------------------------------- MoE
MOE_D, MOE_F, MOE_E, MOE_K = 512, 768, 4, 2   # the tiny-moe widths


def _moe_case(kind, M):
    """IQ4_XS gate/up and Q5_0 down experts, skewed routing (expert 0 favoured, expert 3 empty)."""
    from mipipe.ops.kernels import PackedWeight, moe_route
    gu, dn = [], []
    for e in range(MOE_E):
        raw, deq = _weights(Q.IQ4_XS, kind, 2 * MOE_F, MOE_D, seed=1 + e)
        gu.append((PackedWeight(raw, Q.IQ4_XS, 2 * MOE_F, MOE_D, gateup=True), deq))
        raw, deq = _weights(Q.Q5_0, kind, MOE_D, MOE_F, seed=1 + e)
        dn.append((PackedWeight(raw, Q.Q5_0, MOE_D, MOE_F), deq))
    g = torch.Generator().manual_seed(M)
    logits = torch.randn(M, MOE_E, generator=g)
    logits[:, 0] += 2.5
    logits[:, 3] -= 30.0
    counts, lists, weights = moe_route(logits.cuda(), MOE_K)
    assert counts.cpu().tolist()[3] == 0 and int(counts.sum()) == M * MOE_K
    x = torch.randn(M, gu[0][0].k_pad, generator=g).half()
    base = torch.randn(M, MOE_D, generator=g)
    return gu, dn, counts, lists, weights, x, base


def _moe_check(run, kind, M):
    from mipipe.ops.kernels import EPI_SWIGLU, EPI_ATOMIC
    gu, dn, counts, lists, weights, x, base = _moe_case(kind, M)
    gu_all = torch.cat([w.dev for w, _ in gu])
    dn_all = torch.cat([w.dev for w, _ in dn])
    g0, d0 = gu[0][0], dn[0][0]
    h = torch.zeros(M * MOE_K, d0.k_pad, dtype=torch.float16, device="cuda")
    run(gu_all, g0.dev.numel(), g0.ptype, g0.ntiles, g0.nsb, MOE_F, EPI_SWIGLU, x.cuda(), M, MOE_E, MOE_K,
        counts, lists, weights, h=h)
    y = base.clone().cuda()
    run(dn_all, d0.dev.numel(), d0.ptype, d0.ntiles, d0.nsb, MOE_D, EPI_ATOMIC, h, M, MOE_E, MOE_K,
        counts, lists, weights, x_per_slot=True, y=y)
    torch.cuda.synchronize()
    cnt = counts.cpu().tolist()
    hc, wts = h.float().cpu(), weights.cpu()
    y_ref = torch.zeros(M, MOE_D, dtype=torch.float64)
    h_err = h_sq = 0.0
    for e in range(MOE_E):
        sl = lists[e, : cnt[e]].long().cpu()
        if sl.numel() == 0:
            continue
        tok = sl // MOE_K
        G = x[tok, :MOE_D].float() @ gu[e][1].T   # gate rows [0, F), up rows [F, 2F) of the GGUF matrix
        href = torch.nn.functional.silu(G[:, :MOE_F]) * G[:, MOE_F:]
        hk = hc[sl, :MOE_F]
        h_err += float(((hk - href) ** 2).sum())
        h_sq += float((href ** 2).sum())
        yd = hk @ dn[e][1].T   # the kernel's own h as the down input: isolates the down GEMM's error
        y_ref.index_add_(0, tok, (wts[sl][:, None] * yd).double())
    assert h_err / h_sq < 1e-4, h_err / h_sq
    assert nmse(y.cpu() - base, y_ref) < 1e-5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [3, 33])
def test_moe_gemv(cuda, native, kind, M):
    from mipipe.ops.kernels import moe_gemv
    _moe_check(moe_gemv, kind, M)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M", [65, 200])
def test_moe_gemm(cuda, native, kind, M):
    from mipipe.ops.kernels import moe_gemm
    _moe_check(moe_gemm, kind, M)


# ------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("name,ftype", [("tiny-gqa", "IQ4_XS"), ("tiny-l3", "Q5_1"), ("tiny-moe", "IQ4_XS"),
                                        ("tiny-qwen2", "Q5_0"), ("tiny-k384", "IQ4_XS"), ("tiny-k384", "Q5_0")])
def test_engine_matches_reference(cuda, native, model_dir, name, ftype):
    """Single stream: the fused single-stream extras (the v_dot2 GEMV form, the gemvs2 pair, attn_o
    with its o-projection) take none of the new types, so the stage falls to the plain routes.
    tiny-k384 has K = 384 on every projection but ffn_down: IQ4_XS becomes IQ4_NL / Q5_1 / Q8_0."""
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


def test_engine_mb96_gemm4(cuda, native, model_dir):
    """96 sequences in one micro-batch of tiny-gqa IQ4_XS (IQ4_XS beside Q5_K / Q6_K): the prompt
    chunks and every decode projection have more than 64 rows, so they run on gemm4."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-gqa", "IQ4_XS")
    rng = np.random.default_rng(5)
    mb = 96
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(4, 16, mb)]
    with Engine(gguf=path, max_ctx=64, n_mb=1, mb_size=mb, prefill_chunk=512) as eng:
        eng.start(prompts)
        lg0 = eng.logits(rows=mb)
        eng.decode(2)
        lg2 = eng.logits(rows=mb)
        toks = eng.tokens()
    ref = RefLlama.from_gguf(path)
    for r in (0, 63, 64, 95):
        ref.reset()
        rl = ref.forward(prompts[r], 0)[-1].numpy()
        assert nmse(lg0[r], rl) < 2e-4, (r, nmse(lg0[r], rl))
        pos = len(prompts[r])
        for t in toks[r][:2]:   # the engine's own tokens (a near-tie flip would only change the path)
            rl = ref.forward([t], pos)[-1].numpy()
            pos += 1
        assert nmse(lg2[r], rl) < 2e-4, (r, nmse(lg2[r], rl))


def test_synthetic_iq4_xs_engine(cuda, native):
    """Device-side random init of IQ4_XS / Q5_K / Q6_K weights (init.hip): finite logits whose spread
    is that of the same config at Q4_K to within 2x."""
    from mipipe.engine import Engine
    syn = dict(n_layer=2, d_model=512, n_head=8, n_head_kv=2, d_ff=1024, vocab=2048, rope_base=10000.0)
    prompts = [[1, 2, 3, 4, 5, 6, 7], [8, 9, 10]]
    std = {}
    for ftype in ("IQ4_XS", "Q4_K"):
        with Engine(synthetic=syn, ftype=ftype, max_ctx=128, n_mb=1, mb_size=2, prefill_chunk=16) as eng:
            eng.start(prompts)
            eng.decode(2)
            lg = np.asarray(eng.logits(rows=2), np.float64)
        assert np.isfinite(lg).all() and lg.shape[-1] == syn["vocab"]
        std[ftype] = float(lg.std())
    print("logit std", std)
    assert 0.5 < std["IQ4_XS"] / std["Q4_K"] < 2.0, std
