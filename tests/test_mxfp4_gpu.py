"""MXFP4 on the GPU: unpack and embedding gather exactly, the dequantising routes against the fp32 product
(bounds of tests/test_iq4_q5_quants_gpu.py), the fp4 B image read back, the native fp4-B GEMM against the
f64 product of its own MX-FP8 rows and the dequantized weights (bounds of tests/test_gemm_mx8_gpu.py),
and the engine in both modes."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import make_model
from mipipe.utils import quants as Q

pytestmark = pytest.mark.gpu
MX = Q.MXFP4


def nmse(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


@functools.lru_cache(maxsize=None)
def _weights(n, k, kind="quantized", seed=0):
    """(raw bytes, dequantized [n][k] f64), shared.  "blocks": random codes, every block of a row with
    its own scale byte, e - 127 in [-14, 0]."""
    rng = np.random.default_rng(n + k + 7919 * seed)
    if kind == "quantized":
        raw = Q.quantize((rng.standard_normal((n, k)) / math.sqrt(k)).astype(np.float32), MX)
    else:
        raw = rng.integers(0, 256, size=(n, k // 32, 17), dtype=np.uint8)
        raw[:, :, 0] = 113 + (3 * np.arange(n)[:, None] + np.arange(k // 32)[None, :]) % 15
        raw = raw.reshape(-1)
    return raw, torch.from_numpy(Q.dequantize(raw, MX).reshape(n, k)).double()


def _x(M, k, seed):
    return torch.randn(M, k, generator=torch.Generator().manual_seed(seed)).half()


@pytest.mark.parametrize("k", [256, 768])
def test_unpack_and_embed_exact(cuda, native, k):
    from mipipe.ops.kernels import PackedWeight, embed
    raw, deq = _weights(32, k, "blocks")
    assert torch.equal(PackedWeight(raw, MX, 32, k).unpack().double().cpu(), deq)
    tok = torch.tensor([3, 0, 31, 17], dtype=torch.int32)
    assert torch.equal(embed(torch.from_numpy(raw).cuda(), MX, k, tok.cuda()).double().cpu(), deq[tok.long()])


@pytest.mark.parametrize("k", [256, 1024])
@pytest.mark.parametrize("M", [1, 5, 33, 65, 129])
def test_exact_routes(cuda, native, M, k):
    """N = 200 (12.5 tiles).  M = 1: gemvs; 5, 33: gemv2; 65, 129: the 64 x 64 GEMM, gemm3, gemm4."""
    from mipipe.ops.kernels import PackedWeight, gemv_small, gemv, gemm, EPI_STORE, EPI_ATOMIC, EPI_SWIGLU
    raw, deq = _weights(200, k)
    w, xh = PackedWeight(raw, MX, 200, k), _x(M, k, 30 + M)
    ref = xh.float() @ deq.float().T
    base = torch.randn(M, 200, generator=torch.Generator().manual_seed(M))
    if M <= 64:
        run = (lambda **kw: gemv_small(w, EPI_ATOMIC, x=xh.cuda(), **kw)) if M == 1 else (lambda **kw: gemv(w, xh.cuda(), EPI_ATOMIC, **kw))
        for nsplit in (1, 3):
            assert nmse(run(y=base.clone().cuda(), nsplit=nsplit).cpu(), base + ref) < 1e-5, nsplit
        return
    for v in (1, 3, 4):
        assert nmse(gemm(w, xh.cuda(), EPI_STORE, v=v).cpu(), ref) < 1e-5, v
    assert nmse(gemm(w, xh.cuda(), EPI_ATOMIC, y=base.clone().cuda(), v=4).cpu(), ref + base) < 1e-5
    h = gemm(PackedWeight(raw[: 192 * (k // 32) * 17], MX, 192, k), xh.cuda(), EPI_SWIGLU, v=4)   # whole tiles
    gi = torch.tensor([16 * (o // 8) + (o % 8) for o in range(96)])
    assert nmse(h.float().cpu(), torch.nn.functional.silu(ref[:, gi]) * ref[:, gi + 8]) < 1e-4


@pytest.mark.parametrize("n,k", [(32, 256), (200, 1280)])
def test_relayout_is_a_permutation(cuda, native, n, k):
    """The B image through the inverse permutation, in numpy, is the file's nibbles and scale bytes."""
    from mipipe.ops.kernels import PackedWeight, Mx4Weight
    raw, _ = _weights(n, k, "blocks")
    blk, w4 = raw.reshape(n, k // 32, 17), Mx4Weight(PackedWeight(raw, MX, n, k))
    g, nsb = w4.ng, w4.nsb
    img = w4.dev.cpu().numpy().reshape(g, 4 * nsb, 2, 32, 16).transpose(0, 3, 1, 2, 4).reshape(g * 32, k // 2)
    codes = np.stack([img & 15, img >> 4], axis=-1).reshape(g * 32, k)      # (kb, l / 32, byte, nibble) = k order
    sc = w4.scales.cpu().numpy().reshape(g, nsb, 2, 32, 4).transpose(0, 3, 1, 4, 2).reshape(g * 32, k // 32)
    want = np.concatenate([blk[:, :, 1:] & 15, blk[:, :, 1:] >> 4], axis=-1).reshape(n, k)
    assert np.array_equal(codes[:n], want) and np.array_equal(sc[:n], blk[:, :, 0]) and not codes[n:].any()


@pytest.mark.parametrize("n", [32, 200, 416])            # 200: n_valid below the image's columns
@pytest.mark.parametrize("k", [256, 512, 1280])          # 1, 2, 5 super-blocks
@pytest.mark.parametrize("M", [65, 128, 129, 257])       # around both row tiles
def test_gemm_fp4_exact_block_scaled_math(cuda, native, M, k, n):
    from mipipe.ops.kernels import PackedWeight, Mx4Weight, gemm_mx8, quant_rows_mx8, EPI_STORE, EPI_ATOMIC, EPI_SWIGLU
    raw, deq = _weights(n, k, "blocks")
    w4 = Mx4Weight(PackedWeight(raw, MX, n, k))
    p = (3 * torch.arange(M)[:, None] + 5 * torch.arange(k // 32)[None, :]) % 13 - 10     # a scale byte per x block
    q, s = quant_rows_mx8((_x(M, k, 31 + M).float() * torch.exp2(p.float()).repeat_interleave(32, dim=1)).half().cuda())
    xd = q.cpu().view(torch.float8_e4m3fn).double() * torch.exp2(s.cpu().double() - 127).repeat_interleave(32, dim=1)
    ref, base = xd @ deq.T, torch.randn(M, n)
    assert nmse(gemm_mx8(w4, xq=(q, s), epi=EPI_STORE).cpu(), ref) < 1e-9
    assert nmse(gemm_mx8(w4, xq=(q, s), epi=EPI_ATOMIC, y=base.clone().cuda()).cpu() - base, ref) < 1e-8
    if n % 16 == 0:
        gi = torch.tensor([16 * (o // 8) + (o % 8) for o in range(n // 2)])
        h = gemm_mx8(w4, xq=(q, s), epi=EPI_SWIGLU).cpu()
        assert nmse(h.float(), torch.nn.functional.silu(ref[:, gi]) * ref[:, gi + 8]) < 1e-5


def test_gemm_fp4_one_hot_rows(cuda, native):
    """One-hot x rows, every weight block with its own scale: each output is one exact product, so a
    wrong op_sel, lane half or nibble order cannot cancel out."""
    from mipipe.ops.kernels import PackedWeight, Mx4Weight, gemm_mx8
    n, k, M = 96, 768, 130
    raw, deq = _weights(n, k, "blocks")
    xh, hot = torch.zeros(M, k, dtype=torch.float16), (37 * torch.arange(M) + 5) % k
    xh[torch.arange(M), hot] = 1.5
    y = gemm_mx8(Mx4Weight(PackedWeight(raw, MX, n, k)), x=xh.cuda()).double().cpu()
    assert torch.equal(y, 1.5 * deq[:, hot].T)


def test_gemm4_splitk_partial_stores(cuda, native):
    from mipipe.ops.kernels import PackedWeight, gemm_splitk
    raw, deq = _weights(256, 2048)
    xh, base = _x(128, 2048, 3), torch.randn(128, 256, generator=torch.Generator().manual_seed(2))
    y = base.clone().cuda()
    assert gemm_splitk(PackedWeight(raw, MX, 256, 2048), xh.cuda(), y) >= 2
    assert nmse(y.cpu() - base, xh.float() @ deq.float().T) < 1e-5


@pytest.mark.parametrize("M,route", [(3, "moe_gemv"), (33, "moe_gemv"), (65, "moe_gemm"), (200, "moe_gemm")])
def test_moe(cuda, native, M, route):
    """tiny-moe widths, 4 MXFP4 experts, top-2 routing with expert 0 favoured and expert 3 empty: the MoE GEMV
    and the grouped gemm4, with the bounds of tests/test_iq4_q5_quants_gpu.py's _moe_check."""
    from mipipe.ops import kernels as KN
    D, F, E, K = 512, 768, 4, 2
    gu, dn = [_weights(2 * F, D, seed=e) for e in range(E)], [_weights(D, F, seed=e) for e in range(E)]
    gw = [KN.PackedWeight(r, MX, 2 * F, D, gateup=True) for r, _ in gu]
    dw = [KN.PackedWeight(r, MX, D, F) for r, _ in dn]
    g = torch.Generator().manual_seed(M)
    logits = torch.randn(M, E, generator=g)
    logits[:, 0] += 2.5
    logits[:, 3] -= 30.0
    counts, lists, weights = KN.moe_route(logits.cuda(), K)
    cnt = counts.cpu().tolist()
    assert cnt[3] == 0 and sum(cnt) == M * K
    x, base = torch.randn(M, D, generator=g).half(), torch.randn(M, D, generator=g)
    run, h, y = getattr(KN, route), torch.zeros(M * K, F, dtype=torch.float16, device="cuda"), base.clone().cuda()
    run(torch.cat([w.dev for w in gw]), gw[0].dev.numel(), gw[0].ptype, gw[0].ntiles, gw[0].nsb, F, KN.EPI_SWIGLU,
        x.cuda(), M, E, K, counts, lists, weights, h=h)
    run(torch.cat([w.dev for w in dw]), dw[0].dev.numel(), dw[0].ptype, dw[0].ntiles, dw[0].nsb, D, KN.EPI_ATOMIC,
        h, M, E, K, counts, lists, weights, x_per_slot=True, y=y)
    hc, wts, y_ref, hk, href = h.float().cpu(), weights.cpu(), torch.zeros(M, D, dtype=torch.float64), [], []
    for e in range(E - 1):
        sl = lists[e, : cnt[e]].long().cpu()
        G = x[sl // K].float() @ gu[e][1].float().T          # gate rows [0, F), up rows [F, 2F) of the GGUF matrix
        href.append(torch.nn.functional.silu(G[:, :F]) * G[:, F:])
        hk.append(hc[sl])
        y_ref.index_add_(0, sl // K, (wts[sl][:, None] * (hk[-1] @ dn[e][1].float().T)).double())
    assert nmse(torch.cat(hk), torch.cat(href)) < 1e-4 and nmse(y.cpu() - base, y_ref) < 1e-5


@pytest.mark.parametrize("name,ftype,mb", [("tiny-gqa", "MXFP4", 1), ("tiny-moe", "MXFP4_MOE", 1), ("tiny-moe", "MXFP4", 8),
                                           ("tiny-gqa", "MXFP4", 96), ("tiny-moe", "MXFP4", 96)])
def test_engine(cuda, native, model_dir, capfd, name, ftype, mb):
    """Default mode, prompt and 4 decode steps against the torch oracle (logit bound and near-tie token
    allowance of tests/test_iq4_q5_quants_gpu.py): mb 1 takes the single-stream routes (gemvs with its
    qkv append, the MoE GEMV), 8 gemv2, 96 the wide GEMMs.  tiny-gqa at mb 96 also with mx8_gemm: the
    fp4 images are built, no fp8 copy, the logits move (x is MX-FP8 now: not a fall-back to gemm4) and stay
    within tests/test_mx8_engine_gpu.py's bound."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, name, ftype)
    rng = np.random.default_rng(5)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(4, 16, mb)]
    res = {}
    modes = (False, True) if (name, mb) == ("tiny-gqa", 96) else (False,)   # a MoE layer gets no image, attention included
    for mx in modes:
        with Engine(gguf=path, max_ctx=64, n_mb=1, mb_size=mb, prefill_chunk=512, mx8_gemm=mx) as eng:
            eng.start(prompts)
            lg0 = eng.logits(rows=mb)
            eng.decode(4)
            res[mx] = (lg0, eng.logits(rows=mb), eng.tokens())
        err = capfd.readouterr().err
        assert ("MXFP4 fp4 operand images" in err) == mx and "MX-FP8 weight copies" not in err
    ref = RefLlama.from_gguf(path)
    for mx, (lg0, lg4, toks) in res.items():
        bound = 1.5 * 9 * 1.42e-3 if mx else 2e-4
        for r in sorted({0, mb // 2, mb - 1}):
            ref.reset()
            rl, pos = ref.forward(prompts[r], 0)[-1].numpy(), len(prompts[r])
            assert nmse(lg0[r], rl) < bound, (mx, r)
            for t in toks[r][-5:-1]:          # the engine's own tokens: a near-tie flip only changes the path
                if not mx and rl.argmax() != t:
                    assert rl.max() - rl[t] < 1e-2 * (np.abs(np.sort(rl)[-2:]).max() + 1), (r, t)
                rl, pos = ref.forward([t], pos)[-1].numpy(), pos + 1
            assert nmse(lg4[r], rl) < bound, (mx, r)
    if True in res:
        assert nmse(res[True][0], res[False][0]) > 1e-7
