"""Blocked V pages ([page][Hkv][8][Dp][8], kernels_api.h) against the V^T layout ([page][Hkv][Dp][64]):
every op that reads or appends V pages runs once per layout on the same logical inputs.  The
blocked pages are the V^T pages permuted, Vp.view(P, H, Dp, 8, 8).permute(0, 1, 3, 2, 4); the two runs
must give bitwise-equal outputs, bitwise-equal K caches, and V caches that are bitwise equal after
the inverse permutation -- so the append landed in the right place and no other byte changed.  What
the V^T runs compute is the business of the existing oracle tests (test_attn_decode_gpu.py,
test_kernels_gpu.py); only the layout is under test here.

Positions {0, 7, 8, 63, 64, 65, 130}: both sides of an 8-key block edge and of a 64-key page edge,
and a third page.  The decode ops take one row per position (7 rows, one launch); the ops that take
several tokens of a sequence (rope_kv, attention with tq > 1, attn_prefill) take 5 consecutive
tokens starting at each position (7 sequences); the q|k|v GEMV's append epilogue takes at most 4
rows, so the positions go in two launches.  Shapes: G in {1, 8} x Dp in {64, 128} from the decode
test's list plus (128, 4, 4); attn_o only exists for hd 128 and G 4, and many splits reuse the
decode test's 66- and 128-split case.
"""
import functools

import numpy as np
import pytest
import torch

from mipipe.utils import quants as Q
from test_attn_decode_gpu import (NP, PF4, PF8, WAVE, Dev, _same_bytes, _store, attn_o_case, build_case,  # noqa: F401
                                  force_form, many_case)

gpu = pytest.mark.gpu

POS = (0, 7, 8, 63, 64, 65, 130)
T_SEQ = 5
SHAPES = [(128, 64, 8), (64, 32, 4), (48, 6, 6), (128, 4, 4)]   # (hd, Hq, Hkv): G 8 / 8 / 1 / 1, Dp 128 / 64 / 64 / 128
shape_param = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
kv_param = pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])


def to_blocked(v):
    P, H, Dp, _ = v.shape
    return v.view(P, H, Dp, 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(P, H, Dp, 64)


def from_blocked(v):
    P, H, Dp, _ = v.shape
    return v.view(P, H, 8, Dp, 8).permute(0, 1, 3, 2, 4).contiguous().view(P, H, Dp, 64)


def test_permutation_is_the_documented_offset():
    """Element (key, d) of a blocked page sits at (key >> 3) * Dp * 8 + d * 8 + (key & 7)."""
    Dp = 64
    v = torch.arange(Dp * 64, dtype=torch.int16).view(1, 1, Dp, 64)   # value = d * 64 + key
    b = to_blocked(v).reshape(-1)
    for key, d in ((0, 0), (7, 1), (8, 0), (63, 63), (13, 40)):
        assert int(b[(key >> 3) * Dp * 8 + d * 8 + (key & 7)]) == d * 64 + key
    assert torch.equal(from_blocked(to_blocked(v)), v)


def _bits(t):
    return t if t.dtype in (torch.uint8, torch.int32) else t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _assert_layouts_agree(legacy, blocked, vc_before, appends=True):
    """legacy / blocked: (outputs..., kc, vc) of the two runs, on the CPU."""
    *out_l, kc_l, vc_l = legacy
    *out_b, kc_b, vc_b = blocked
    for i, (a, b) in enumerate(zip(out_l, out_b)):
        assert torch.equal(_bits(a), _bits(b)), f"output {i} differs between the layouts"
        assert not torch.isnan(a.float()).any()
    assert _same_bytes(kc_l, kc_b), "K cache differs between the layouts"
    assert _same_bytes(vc_l, from_blocked(vc_b)), "V cache differs after the inverse permutation"
    assert _same_bytes(vc_l, vc_before) != appends, "the V append did not land" if appends else "V pages written"


def _both(run, vc):
    """run(blocked, vc_dev) -> tuple of CPU tensors; once per layout on the same logical V pages."""
    from mipipe.ops.kernels import v_layout
    res = []
    for blocked in (False, True):
        with v_layout(blocked):
            res.append(run(blocked, (to_blocked(vc) if blocked else vc).cuda()))
    torch.cuda.synchronize()
    return res


# ---------------------------------------------------------------- decode forms
@functools.lru_cache(maxsize=None)
def decode_case(shape, fp8, pre=False):
    hd, Hq, Hkv = shape
    return build_case(hd, Hq, Hkv, POS, fp8, "perm" if not pre else "slot0", seed=4000 + hd + Hq + 7 * fp8 + 3 * pre,
                      pre=pre)


def _run_decode(c, form, n_split):
    def run(blocked, vc):
        d = Dev(c, n_split)
        d.vc = vc
        out = d.run(form)
        return out, d.kc.cpu(), d.vc.cpu()
    return _both(run, c.vc)


@gpu
@shape_param
@kv_param
@pytest.mark.parametrize("form,n_split", [(WAVE, 1), (WAVE, 4), (PF4, 1), (PF8, 1), (NP, 1), (NP, 4)],
                         ids=["wave-s1", "wave-s4", "pf4-s1", "pf8-s1", "np-s1", "np-s4"])
def test_decode_forms(cuda, force_form, form, n_split, fp8, shape):
    c = decode_case(shape, fp8)
    force_form(form)
    legacy, blocked = _run_decode(c, form, n_split)
    _assert_layouts_agree(legacy, blocked, c.vc)


@gpu
@kv_param
@pytest.mark.parametrize("form", [NP, WAVE], ids=["np", "wave"])
def test_decode_many_splits(cuda, force_form, form, fp8):
    c = many_case(fp8)
    force_form(form)
    legacy, blocked = _run_decode(c, form, 128)
    _assert_layouts_agree(legacy, blocked, c.vc)


@gpu
@shape_param
@kv_param
@pytest.mark.parametrize("form", [PF4, PF8], ids=["pf4", "pf8"])
def test_decode_pre(cuda, force_form, form, fp8, shape):
    """q rotated and K / V already appended: the kernel only reads the pages."""
    c = decode_case(shape, fp8, True)
    force_form(form)
    legacy, blocked = _run_decode(c, form, 1)
    _assert_layouts_agree(legacy, blocked, c.vc, appends=False)


@gpu
@pytest.mark.parametrize("pre", [False, True], ids=["rot", "pre"])
@kv_param
def test_attn_o(cuda, native, fp8, pre):
    """attn_o_kernel (hd 128, G 4, M 4).  Y starts at zero and Hkv is 2, so each output is the sum of
    two atomically added partials: a + b whatever the order, bitwise."""
    from mipipe.ops.kernels import PackedWeight, attn_o
    c = attn_o_case(4, fp8, pre)
    n, k = 256, 1024
    rng = np.random.default_rng(9)
    w = PackedWeight(Q.quantize((rng.standard_normal((n, k)) / 32).astype(np.float32), Q.Q8_0), Q.Q8_0, n, k)

    def run(blocked, vc):
        d = Dev(c, 1)
        d.vc = vc
        a = d.args(c.qkv, c.pos)
        y = attn_o(w, torch.zeros(c.M, n, device="cuda"), *a[:-2], a[-1], slot=None, slot0=c.slot0, kv_fp8=fp8, pre=pre)
        return y.cpu(), d.kc.cpu(), d.vc.cpu()
    legacy, blocked = _both(run, c.vc)
    _assert_layouts_agree(legacy, blocked, c.vc, appends=not pre)
    assert float(legacy[0].abs().max()) > 0


# ---------------------------------------------------------------- several tokens per sequence
class SeqCase:
    pass


@functools.lru_cache(maxsize=None)
def seq_case(shape, fp8):
    """7 sequences, tokens [p, p + 5) of each (p in POS) in one chunk; every page holds finite data."""
    from mipipe.ops.kernels import rope_cs_table
    hd, Hq, Hkv = shape
    g = torch.Generator().manual_seed(5000 + hd + Hq + fp8)
    c = SeqCase()
    c.hd, c.Hq, c.Hkv, c.Dp, c.fp8 = hd, Hq, Hkv, 64 if hd <= 64 else 128, fp8
    c.max_pages = 4
    n_seq = len(POS)
    n_pages = n_seq * c.max_pages + 1
    perm = torch.randperm(n_pages, generator=g).to(torch.int32)
    slots = torch.randperm(n_seq + 2, generator=g)[:n_seq]
    c.bt = torch.full((n_seq + 2, c.max_pages), int(perm[-1]), dtype=torch.int32)
    for i in range(n_seq):
        c.bt[slots[i]] = perm[i * c.max_pages:(i + 1) * c.max_pages]
    c.pos = torch.tensor([p + j for p in POS for j in range(T_SEQ)], dtype=torch.int32)
    c.slot = slots.to(torch.int32).repeat_interleave(T_SEQ)
    c.segs = [(i * T_SEQ, T_SEQ) for i in range(n_seq)]
    c.M = len(c.pos)
    c.cs = rope_cs_table(c.max_pages * 64, hd, 10000.0)
    c.qkv = torch.randn(c.M, (Hq + 2 * Hkv) * hd, generator=g)
    c.kc = _store(torch.randn(n_pages, Hkv, 64, c.Dp, generator=g, dtype=torch.float64), fp8)
    c.vc = _store(torch.randn(n_pages, Hkv, c.Dp, 64, generator=g, dtype=torch.float64), fp8)
    c.q_scale = hd ** -0.5
    return c


def _rope_kv(c, kc, vc):
    from mipipe.ops.kernels import rope_kv
    return rope_kv(c.qkv.cuda(), c.pos.cuda(), c.slot.cuda(), c.bt.cuda(), c.cs.cuda(), c.Hq, c.Hkv, c.hd, c.Dp, c.q_scale,
                   kc, vc, kv_fp8=c.fp8)


@gpu
@shape_param
@kv_param
def test_rope_kv(cuda, native, fp8, shape):
    c = seq_case(shape, fp8)

    def run(blocked, vc):
        kc = c.kc.cuda()
        q = _rope_kv(c, kc, vc)
        return q.cpu(), kc.cpu(), vc.cpu()
    legacy, blocked = _both(run, c.vc)
    _assert_layouts_agree(legacy, blocked, c.vc)


@gpu
@shape_param
@kv_param
@pytest.mark.parametrize("n_split", [1, 2])
def test_attn_prefill(cuda, native, n_split, fp8, shape):
    """The page staging into LDS; n_split 2 with one page per split also runs the LSE merge."""
    from mipipe.ops.kernels import attn_prefill
    c = seq_case(shape, fp8)

    def run(blocked, vc):
        kc = c.kc.cuda()
        q = _rope_kv(c, kc, vc)
        out = attn_prefill(q, c.pos.cuda(), c.slot.cuda(), c.bt.cuda(), kc, vc, c.Hkv, c.hd, segs=c.segs, n_split=n_split,
                           split_pages=2 if n_split > 1 else 1, kv_fp8=fp8)
        return out.cpu(), kc.cpu(), vc.cpu()
    legacy, blocked = _both(run, c.vc)
    _assert_layouts_agree(legacy, blocked, c.vc)
    assert float(legacy[0].float().abs().max()) > 0


@gpu
@shape_param
@pytest.mark.parametrize("n_split", [1, 2])
def test_attention_tq(cuda, native, n_split, shape):
    """attn_kernel with several query tokens per row group (f16 pages only): 16 MFMA rows hold
    tq = min(5, 16 // G) tokens of one sequence."""
    from mipipe.ops.kernels import attention
    c = seq_case(shape, False)
    tq = min(T_SEQ, 16 // (c.Hq // c.Hkv))

    def run(blocked, vc):
        kc = c.kc.cuda()
        q = _rope_kv(c, kc, vc)
        outs = []
        for row0, T in c.segs:   # one launch per sequence: a row group never spans two
            s = slice(row0, row0 + T)
            outs.append(attention(q[s].contiguous(), (c.pos[s] + 1).cuda(), c.slot[s].cuda(), c.bt.cuda(), kc, vc, c.Hkv,
                                  c.hd, tq=tq, split_len=256 // n_split, n_split=n_split))
        return torch.cat(outs).cpu(), kc.cpu(), vc.cpu()
    legacy, blocked = _both(run, c.vc)
    _assert_layouts_agree(legacy, blocked, c.vc)
    assert float(legacy[0].float().abs().max()) > 0


# ---------------------------------------------------------------- the q|k|v GEMV's append epilogue
@gpu
@shape_param
@kv_param
def test_gemvs_qkv_append(cuda, native, fp8, shape):
    from mipipe.ops.kernels import PackedWeight, gemv_small_qkv
    hd, Hq, Hkv = shape
    c = seq_case(shape, fp8)
    d = 512
    w = PackedWeight.random(Q.Q4_K, (Hq + 2 * Hkv) * hd, d, seed=3)
    g = torch.Generator().manual_seed(11)
    gamma = (1.0 + 0.1 * torch.randn(d, generator=g)).cuda()
    groups = [POS[:4], POS[4:]]   # the epilogue takes M <= 4 rows; row m lives in slot slot0 + m
    bt = c.bt.clone()
    bt[:4] = c.bt[c.slot[::T_SEQ][:4].long()]   # four distinct, fully paged rows at slots 0..3

    def run(blocked, vc):
        kc = c.kc.cuda()
        ys = []
        for grp in groups:
            xf = torch.randn(len(grp), d, generator=torch.Generator().manual_seed(len(grp))).cuda()
            ys.append(gemv_small_qkv(w, xf, gamma, 1e-5, torch.tensor(grp, dtype=torch.int32).cuda(), 0, bt.cuda(),
                                     c.cs.cuda(), kc, vc, Hq, Hkv, hd, c.Dp, kv_fp8=fp8))
        return torch.cat(ys).cpu(), kc.cpu(), vc.cpu()
    legacy, blocked = _both(run, c.vc)
    _assert_layouts_agree(legacy, blocked, c.vc)
    assert float(legacy[0][:, :Hq * hd].abs().max()) > 0
