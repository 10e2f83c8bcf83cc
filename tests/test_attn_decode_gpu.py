"""The fused decode attention step (attention.hip: attn_decode_kernel, attn_decode_kernel8,
attn_decode_kernel_np, attn_decode_wave_kernel, attn_o_kernel) at op level against a float64 oracle.

The oracle is the operation's definition in plain torch float64 on the CPU: deferred norm / bias,
RoPE of q and the new k from the table the kernel gets, the scaled q (q_scale * log2 e) rounded to
f16 (the kernel's MFMA operand), the new K / V rounded to the cache type (f16, or e4m3 with the
+-448 clamp), keys [0, pos] of the row's slot through the block table exactly as stored, softmax and
P.V in float64.

The inputs make ONE wrong key visible in EVERY query head (random q / k / v cannot: the softmax is
flat and a key moves the output by ~1/L).  Per kv head there is a direction u (|u| = sqrt(hd)); the
rotated q of its G query heads is u + 0.5 noise; the keys at the boundary positions (chunk, page and
split edges, pos - 1 and the new token at pos) are 3 u / sqrt(hd) + 0.3 noise with v = +-32; every
position past the sequence (rest of the last page, spare pages, the trash page, and the slot at pos
that the kernel must overwrite) holds finite stale keys 6 u / sqrt(hd) + 0.3 noise with v = +-32
(the slot at pos: minus the new v) that would dominate if read, and non-zero values in the padded
dims d >= hd.  test_inputs_expose_one_wrong_key (CPU) proves the property on the oracle alone: one
extra key, any one boundary key dropped, or two block-table entries swapped moves every head by at
least 10x the output tolerance.

Tolerance: rtol = atol = 5e-3, the project's number for this arithmetic (f16 operands, f32
accumulate, f16 output; test_rope_kv_attention).  Largest |err| / (atol + rtol |ref|) per form and
KV type, first GPU run (test_forms_match_oracle, all shapes / splits / slot modes):
    prefetch 4 waves   f16 0.59   fp8 0.65
    prefetch 8 waves   f16 0.59   fp8 0.65
    no prefetch        f16 0.59   fp8 0.65
    wave               f16 0.86   fp8 0.76
(the other tests: second step 0.68, many splits 0.15, deferred norm 0.75, pre 0.36, lazy rescale
0.75, attn_o 0.55).  No form stays below 0.2, so the tolerance is not tightened.  The error is the
kernel's f16 rounding of the probabilities before the P.V MFMA: up to 2^-11 of each +-32 value
spike's weighted contribution, which the oracle (float64 P) does not have.

The many-splits case has rows at 65 * 128 + 5 and 128 * 128 - 1 with split_len 128 (66 and
128 = ATTN_MAX_SPLITS active splits); position 16383 needs 256 block-table entries per row, so
max_pages is 256 there.  One split always runs with split_len = the whole
context (the launch contract: n_split * split_len covers max_pages * 64), several with 128.
"""
import functools
import math

import numpy as np
import pytest
import torch

from mipipe.utils import quants as Q

gpu = pytest.mark.gpu

RTOL = ATOL = 5e-3
LOG2E = 1.4426950408889634
MAX_CTX, SPLIT_LEN = 512, 128
SHAPES = [(128, 32, 8), (128, 64, 8), (64, 32, 4), (48, 6, 6), (128, 16, 1)]
POSITIONS = (0, 1, 30, 31, 32, 63, 64, 95, 127, 128, 129, 255, 256, 383, 511)
BOUNDARY = (0, 31, 32, 63, 64, 127, 128, 255, 256)
PF4, PF8, NP, WAVE = 0, 1, 2, 3
FORM_NAMES = {PF4: "pf4", PF8: "pf8", NP: "np", WAVE: "wave"}
# (form, n_split): the prefetch forms take one split only, as in the launcher
FORM_SPLITS = [(PF4, 1), (PF8, 1), (NP, 1), (NP, 4), (WAVE, 1), (WAVE, 4)]
FORM_IDS = [f"{FORM_NAMES[f]}-s{s}" for f, s in FORM_SPLITS]
MANY_POS = (65 * 128 + 5, 128 * 128 - 1)
MANY_EXTRA = (8191, 8192, 8319, 8320, 16255, 16256)   # split edges round the 64-lane merge loops' wrap


# ---------------------------------------------------------------- cache number formats
def _round_cache(x, fp8):
    """float64 -> the nearest value of the cache type, as float64."""
    if fp8:
        return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float().double()
    return x.to(torch.float16).double()


def _store(x, fp8):
    """float64 values (already representable) -> the stored tensor (f16, or e4m3 bytes)."""
    if fp8:
        return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return x.to(torch.float16)


def _decode(t):
    """stored tensor -> float64 values, exactly."""
    if t.dtype == torch.uint8:
        return t.view(torch.float8_e4m3fn).float().double()
    return t.double()


def _codes(t):
    """stored tensor -> integers monotonic in the value (neighbouring codes differ by 1)."""
    if t.dtype == torch.uint8:
        c = t.to(torch.int32)
        return torch.where(c >= 128, -(c - 128), c)
    c = t.view(torch.int16).to(torch.int32)
    return torch.where(c < 0, -(c & 0x7FFF), c)


def _same_bytes(a, b):
    bits = lambda t: t if t.dtype == torch.uint8 else t.view(torch.int16)
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _rot(x, cs_row, inverse=False):
    """RoPE of x [..., hd] (interleaved pairs) with one table row cs_row [hd/2][2] (cos, sin)."""
    c, s = cs_row[:, 0].double(), cs_row[:, 1].double()
    if inverse:
        s = -s
    x0, x1 = x[..., 0::2], x[..., 1::2]
    o = torch.empty_like(x)
    o[..., 0::2] = x0 * c - x1 * s
    o[..., 1::2] = x0 * s + x1 * c
    return o


# ---------------------------------------------------------------- inputs
class Case:
    pass


def _default_gain(k_gain, extra=()):
    bset = set(BOUNDARY) | set(extra)
    return lambda j, pos: k_gain if (j in bset or j >= pos - 1) else None


def _make_qkv(c, poss, g, gain):
    """One decode step's f32 projections for rows at positions poss: q (rotated) = u + 0.5 noise, the
    new k (rotated) a boundary key, v = +-32; all supplied pre-RoPE (and before the deferred norm)."""
    hd, Hq, Hkv, G = c.hd, c.Hq, c.Hkv, c.G
    n = (Hq + 2 * Hkv) * hd
    qkv = torch.zeros(len(poss), n + 8, dtype=torch.float64)
    vnew = []
    for t, pos in enumerate(poss):
        q = c.u.repeat_interleave(G, 0) + 0.5 * torch.randn(Hq, hd, generator=g, dtype=torch.float64)
        kg = gain(pos, pos)
        k = kg * c.u / math.sqrt(hd) + c.k_noise * torch.randn(Hkv, hd, generator=g, dtype=torch.float64)
        v = 32.0 * (torch.randint(0, 2, (Hkv, hd), generator=g) * 2 - 1).double()
        vnew.append(v)
        if not c.pre:
            q, k = _rot(q, c.cs[pos], inverse=True), _rot(k, c.cs[pos], inverse=True)
        else:   # q arrives rotated; the k | v columns are unused (finite garbage)
            k = 5.0 * torch.randn(Hkv, hd, generator=g, dtype=torch.float64)
            v = 5.0 * torch.randn(Hkv, hd, generator=g, dtype=torch.float64)
        qkv[t, :n] = torch.cat([q.reshape(-1), k.reshape(-1), v.reshape(-1)])
    if c.ssq is not None:   # value = rsqrt(ssq / d + eps) * row + bias
        nrs = torch.rsqrt(c.ssq.double() / c.d_model + c.eps)
        b = c.bias.double() if c.bias is not None else torch.zeros(n, dtype=torch.float64)
        qkv[:, :n] = (qkv[:, :n] - b) / nrs[:len(poss), None]
    return qkv.float(), vnew


def build_case(hd, Hq, Hkv, poss, fp8, slot_mode, seed, *, max_pages=MAX_CTX // 64, k_gain=3.0, stale_gain=6.0,
               k_ord=1.0, k_noise=0.3, extra=(), gain=None, norm=None, pre=False, steps=1):
    from mipipe.ops.kernels import rope_cs_table
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sign = lambda *s: (torch.randint(0, 2, s, generator=g) * 2 - 1).double()
    c = Case()
    c.hd, c.Hq, c.Hkv, c.G, c.Dp, c.fp8, c.pre = hd, Hq, Hkv, Hq // Hkv, 64 if hd <= 64 else 128, fp8, pre
    c.M, c.pos, c.max_pages, c.k_noise = len(poss), list(poss), max_pages, k_noise
    c.q_scale = 1.0 / math.sqrt(hd)
    c.gain = gain or _default_gain(k_gain, extra)
    M, Dp = c.M, c.Dp
    n_slots = M + 3
    if slot_mode == "slot0":
        c.slot0, c.slots = 2, [2 + t for t in range(M)]
    else:
        c.slot0, c.slots = None, [int(s) for s in torch.randperm(n_slots, generator=g)[:M]]
    need = [(p + steps - 1) // 64 + 1 for p in poss]
    assert max(need) <= max_pages
    n_pages = sum(need) + 4
    perm = [int(p) for p in torch.randperm(n_pages, generator=g)]
    c.trash, c.n_pages = perm[0], n_pages
    c.bt = torch.full((n_slots, max_pages), c.trash, dtype=torch.int32)   # unused entries: the trash page
    nxt = 1
    for t in range(M):
        for i in range(need[t]):
            c.bt[c.slots[t], i] = perm[nxt]
            nxt += 1
    c.cs = rope_cs_table(max_pages * 64, hd, 10000.0)
    u = rnd(Hkv, hd)
    c.u = u * math.sqrt(hd) / u.norm(dim=1, keepdim=True)
    c.ssq = c.bias = None
    c.eps, c.d_model = 0.0, 0
    if norm:
        c.eps, c.d_model = 1e-5, 4096
        c.ssq = (c.d_model * (0.5 + 3.5 * torch.rand(M, generator=g))).float()
        if norm == "bias":
            c.bias = (0.5 * torch.randn((Hq + 2 * Hkv) * hd, generator=g)).float()
    # stale data everywhere first (what a kernel reading past the sequence would see)
    Kp = torch.zeros(n_pages, Hkv, 64, Dp, dtype=torch.float64)
    Vp = torch.zeros(n_pages, Hkv, Dp, 64, dtype=torch.float64)
    Kp[..., :hd] = stale_gain * c.u[None, :, None, :] / math.sqrt(hd) + 0.3 * rnd(n_pages, Hkv, 64, hd)
    Vp[:, :, :hd, :] = 32.0 * sign(n_pages, Hkv, hd, 64)
    if Dp > hd:
        Kp[..., hd:] = (0.5 + torch.rand(n_pages, Hkv, 64, Dp - hd, generator=g, dtype=torch.float64)) * sign(
            n_pages, Hkv, 64, Dp - hd)
        Vp[:, :, hd:, :] = (0.5 + torch.rand(n_pages, Hkv, Dp - hd, 64, generator=g, dtype=torch.float64)) * sign(
            n_pages, Hkv, Dp - hd, 64)
    # the sequences' history [0, pos): ordinary keys, boundary keys; zero padded dims
    for t, pos in enumerate(poss):
        Kr = k_ord * rnd(pos, Hkv, hd)
        Vr = rnd(pos, Hkv, hd)
        for j in range(pos):
            kg = c.gain(j, pos)
            if kg is not None:
                Kr[j] = kg * c.u / math.sqrt(hd) + k_noise * rnd(Hkv, hd)
                Vr[j] = 32.0 * sign(Hkv, hd)
        for i in range((pos + 63) // 64):
            lo, hi = 64 * i, min(64 * i + 64, pos)
            page = int(c.bt[c.slots[t], i])
            Kp[page, :, :hi - lo, :hd] = Kr[lo:hi].transpose(0, 1)
            Kp[page, :, :hi - lo, hd:] = 0.0
            Vp[page, :, :hd, :hi - lo] = Vr[lo:hi].permute(1, 2, 0)
            Vp[page, :, hd:, :hi - lo] = 0.0
    c.qkv, vnew = _make_qkv(c, poss, g, c.gain)
    for t, pos in enumerate(poss):   # the stale slot at pos: the opposite of the new v
        Vp[int(c.bt[c.slots[t], pos // 64]), :, :hd, pos % 64] = -vnew[t]
    c.qkv2 = _make_qkv(c, [p + 1 for p in poss], g, c.gain)[0] if steps > 1 else None
    c.kc, c.vc = _store(_round_cache(Kp, fp8), fp8), _store(_round_cache(Vp, fp8), fp8)
    if pre:   # the new K / V (boundary keys) are already in the cache, rounded to its type
        kn = [_round_cache(c.gain(p, p) * c.u / math.sqrt(hd) + k_noise * rnd(Hkv, hd), fp8) for p in poss]
        _append(c.kc, c.vc, c, poss, kn, [_round_cache(v, fp8) for v in vnew])
    return c


def _append(kc, vc, c, poss, knew, vnew):
    """Write rows' new K / V (float64, representable) into stored caches at (page, :, pos % 64); zero pads."""
    for t, pos in enumerate(poss):
        page = int(c.bt[c.slots[t], pos // 64])
        kc[page, :, pos % 64, :] = 0
        vc[page, :, :, pos % 64] = 0
        kc[page, :, pos % 64, :c.hd] = _store(knew[t], c.fp8)
        vc[page, :, :c.hd, pos % 64] = _store(vnew[t], c.fp8)


# ---------------------------------------------------------------- the oracle
def oracle(c, kc, vc, qkv, poss, *, drop=None, extra=False, bt=None):
    """out [M][Hq][hd], new K, new V [M][Hkv][hd] (float64; K / V as the cache type rounds them).
    Mutants (the input self-check only): drop = a key position left out, extra = key pos + 1 read
    too, bt = another block table."""
    hd, Hq, Hkv, G = c.hd, c.Hq, c.Hkv, c.G
    bt = c.bt if bt is None else bt
    Kl, Vl = _decode(kc), _decode(vc)
    n = (Hq + 2 * Hkv) * hd
    out = torch.zeros(len(poss), Hq, hd, dtype=torch.float64)
    knew, vnew = [], []
    for t, pos in enumerate(poss):
        x = qkv[t, :n].double()
        if c.ssq is not None:
            x = x * torch.rsqrt(c.ssq[t].double() / c.d_model + c.eps)
            if c.bias is not None:
                x = x + c.bias.double()
        q = x[:Hq * hd].view(Hq, hd)
        k = x[Hq * hd:(Hq + Hkv) * hd].view(Hkv, hd)
        v = x[(Hq + Hkv) * hd:].view(Hkv, hd)
        if not c.pre:
            q = _rot(q, c.cs[pos])
            knew.append(_round_cache(_rot(k, c.cs[pos]), c.fp8))
            vnew.append(_round_cache(v, c.fp8))
        qs = (q * (c.q_scale * LOG2E)).to(torch.float16).double()
        L = pos + 1 + (1 if extra else 0)
        j = torch.arange(L)
        inside = j < c.max_pages * 64   # an extra key past the row's table: the trash page
        pages = torch.where(inside, bt[c.slots[t], (j // 64).clamp(max=c.max_pages - 1)].long(),
                            torch.tensor(c.trash))
        K = Kl[pages, :, j % 64, :][:, :, :hd].clone()   # [L][Hkv][hd]
        V = Vl[pages, :, :, j % 64][:, :, :hd].clone()
        if not c.pre:
            K[pos], V[pos] = knew[-1], vnew[-1]
        keep = torch.ones(L, dtype=torch.bool)
        if drop is not None and drop < L:
            keep[drop] = False
        K, V = K[keep], V[keep]
        if K.shape[0] == 0:
            continue
        s2 = torch.einsum("hd,jhd->hj", qs, K.repeat_interleave(G, 1))   # exp2-domain scores
        p = torch.exp2(s2 - s2.max(dim=1, keepdim=True).values)
        out[t] = torch.einsum("hj,jhd->hd", p, V.repeat_interleave(G, 1)) / p.sum(1, keepdim=True)
    return out, knew, vnew


def _ratio(got, ref):
    return float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max())


def _head_ratio(a, ref):
    """[M][Hq]: per head, the largest |a - ref| in units of the output tolerance."""
    return ((a - ref).abs() / (ATOL + RTOL * ref.abs())).amax(dim=-1)


@functools.lru_cache(maxsize=None)
def matrix_case(shape, fp8, slot_mode):
    hd, Hq, Hkv = shape
    c = build_case(hd, Hq, Hkv, POSITIONS, fp8, slot_mode, seed=1000 + hd + Hq + Hkv + 7 * fp8 + 13 * (slot_mode == "perm"))
    c.ref = oracle(c, c.kc, c.vc, c.qkv, c.pos)
    return c


@functools.lru_cache(maxsize=None)
def many_case(fp8):
    c = build_case(128, 8, 2, MANY_POS, fp8, "slot0", seed=77 + fp8, max_pages=256, k_gain=5.0, stale_gain=8.0,
                   k_ord=0.3, extra=MANY_EXTRA)
    c.ref = oracle(c, c.kc, c.vc, c.qkv, c.pos)
    return c


# ---------------------------------------------------------------- input self-check (CPU)
def _check_mutants(c, boundary):
    ref = c.ref[0]
    bset = set(boundary)
    worst = float("inf")
    mut = oracle(c, c.kc, c.vc, c.qkv, c.pos, extra=True)[0]
    r = _head_ratio(mut, ref)
    assert (r >= 10).all(), ("extra key", float(r.min()))
    worst = min(worst, float(r.min()))
    for b in sorted(bset | set(p - 1 for p in c.pos if p > 0) | set(c.pos)):
        # the rows for which key b is inside the sequence and one of its boundary keys
        rows = torch.tensor([b <= p and (b in bset or b >= p - 1) for p in c.pos])
        if not rows.any():
            continue
        mut = oracle(c, c.kc, c.vc, c.qkv, c.pos, drop=b)[0]
        r = _head_ratio(mut, ref)[rows]
        assert (r >= 10).all(), ("dropped key", b, float(r.min()))
        worst = min(worst, float(r.min()))
    # two block-table entries swapped: the page of the row's last cached key (pos - 1) with the first
    # unused entry.  (Two pages
    # that both lie wholly inside the sequence may be swapped freely: the softmax does not depend
    # on the order of the keys.  So a row whose entries are all in use and full, and the row at
    # pos 0, whose only key comes from qkv, have no swap that could matter.)
    bt = c.bt.clone()
    rows = torch.tensor([0 < p and p // 64 + 1 < c.max_pages for p in c.pos])
    for t, p in enumerate(c.pos):
        if rows[t]:
            i, k = (p - 1) // 64, p // 64 + 1
            bt[c.slots[t], [i, k]] = bt[c.slots[t], [k, i]]
    r = _head_ratio(oracle(c, c.kc, c.vc, c.qkv, c.pos, bt=bt)[0], ref)[rows]
    assert (r >= 10).all(), ("swapped pages", float(r.min()))
    return min(worst, float(r.min()))


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_inputs_expose_one_wrong_key(shape, fp8):
    """On the oracle alone: for every shape and every position of the matrix, one extra key, any
    one boundary key dropped, or two block-table entries swapped moves EVERY query head by at
    least 10x the output tolerance on some element -- so a GPU result within tolerance has read
    exactly the keys [0, pos] through the right pages."""
    c = matrix_case(shape, fp8, "slot0")
    assert torch.isfinite(_decode(c.kc)).all() and torch.isfinite(_decode(c.vc)).all()
    worst = _check_mutants(c, BOUNDARY)
    print(f"least margin {shape} {'fp8' if fp8 else 'f16'}: {worst:.1f}x the tolerance")


@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
def test_inputs_expose_one_wrong_key_many_splits(fp8):
    c = many_case(fp8)
    worst = _check_mutants(c, BOUNDARY + MANY_EXTRA)
    print(f"least margin many splits {'fp8' if fp8 else 'f16'}: {worst:.1f}x the tolerance")


# ---------------------------------------------------------------- GPU harness
@pytest.fixture
def force_form(native):
    """Select a device form with the launcher's own knobs; every knob touched is reset."""
    from mipipe import _native as N
    names = (b"ATTN_WAVE", b"ATTN_PF_MAXWG", b"ATTN_NW8_MAXWG")

    def force(form):
        vals = {PF4: (0, 1 << 20, 0), PF8: (0, 1 << 20, 1 << 20), NP: (0, 0, 0), WAVE: (1, 1 << 20, 0)}[form]
        for name, v in zip(names, vals):
            N.check(N.lib().mp_set_knob(name, v), "set_knob")
    yield force
    for name in names:
        N.check(N.lib().mp_reset_knob(name), "reset_knob")


class Dev:
    """A case's buffers on the GPU (fresh copies: the launch appends into the caches)."""

    def __init__(self, c, n_split):
        from mipipe.ops.kernels import DecodeAttnScratch
        self.c, self.n_split = c, n_split
        self.split_len = SPLIT_LEN if n_split > 1 else c.max_pages * 64
        self.kc, self.vc = c.kc.cuda(), c.vc.cuda()
        self.bt, self.cs = c.bt.cuda(), c.cs.cuda()
        self.slot = None if c.slot0 is not None else torch.tensor(c.slots, dtype=torch.int32).cuda()
        self.ssq = None if c.ssq is None else c.ssq.cuda()
        self.bias = None if c.bias is None else c.bias.cuda()
        self.scratch = DecodeAttnScratch(c.M, c.Hq, c.Hkv, c.Dp, n_split)

    def args(self, qkv, poss):
        c = self.c
        return (qkv.cuda(), torch.tensor(poss, dtype=torch.int32).cuda(), self.bt, self.cs, self.kc, self.vc, c.Hq,
                c.Hkv, c.hd, c.Dp, c.q_scale, self.split_len, self.n_split, self.scratch)

    def kw(self):
        c = self.c
        return dict(slot=self.slot, slot0=c.slot0, ssq=self.ssq, eps=c.eps, d_model=c.d_model, kv_fp8=c.fp8,
                    pre=c.pre)

    def run(self, form, qkv=None, poss=None):
        from mipipe.ops.kernels import attn_decode, attn_decode_form
        c = self.c
        qkv = c.qkv if qkv is None else qkv
        poss = c.pos if poss is None else poss
        got = attn_decode_form(c.M, c.Hkv, self.n_split)
        assert got == form, f"meant to run {FORM_NAMES[form]}, the launcher selects {FORM_NAMES[got]}"
        out = attn_decode(*self.args(qkv, poss), bias=self.bias, **self.kw())
        torch.cuda.synchronize()
        assert int(self.scratch.counters.abs().sum()) == 0, "arrival counters did not return to zero"
        return out.cpu().double().view(c.M, c.Hq, c.hd)


def _assert_out(got, ref, what):
    r = _ratio(got, ref)
    print(f"error ratio {what}: {r:.3f}")
    bad = (got - ref).abs() > ATOL + RTOL * ref.abs()
    assert not bad.any(), (what, f"worst ratio {r:.2f}", "first (row, head, d):", bad.nonzero()[0].tolist(),
                           f"{int(bad.sum())} elements")


def _assert_appended(c, kc_after, vc_after, poss, knew, vnew, kc_before, vc_before):
    """The entries at (page, kv head, pos % 64) hold the oracle's rounded K / V (one code off on at
    most 1 % of the elements: the kernel rotates in f32, so a value within ~1e-7 of a rounding
    boundary may land on the neighbouring code), their padded dims are zero, every other byte of
    both caches (the trash page included) is what it was."""
    hd = c.hd
    ek, ev = kc_before.clone(), vc_before.clone()
    off, total = 0, 0
    for t, pos in enumerate(poss):
        page, idx = int(c.bt[c.slots[t], pos // 64]), pos % 64
        gk, gv = kc_after[page, :, idx, :], vc_after[page, :, :, idx]
        assert (_codes(gk[:, hd:]) == 0).all() and (_codes(gv[:, hd:]) == 0).all(), ("padded dims not zero", t, pos)
        dk = (_codes(gk[:, :hd]) - _codes(_store(knew[t], c.fp8))).abs()
        dv = (_codes(gv[:, :hd]) - _codes(_store(vnew[t], c.fp8))).abs()
        assert int(dk.max()) <= 1 and int(dv.max()) <= 1, ("appended K / V off by more than one code", t, pos,
                                                           int(dk.max()), int(dv.max()))
        off += int(dk.sum()) + int(dv.sum())
        total += dk.numel() + dv.numel()
        ek[page, :, idx, :], ev[page, :, :, idx] = gk, gv
    assert off <= 0.01 * total, (off, total)
    assert _same_bytes(kc_after, ek), "stray write into the K cache"
    assert _same_bytes(vc_after, ev), "stray write into the V cache"


kv_param = pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
shape_param = pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))


# ---------------------------------------------------------------- 1. forms against the oracle
@gpu
@pytest.mark.parametrize("slot_mode", ["slot0", "perm"])
@shape_param
@kv_param
@pytest.mark.parametrize("form,n_split", FORM_SPLITS, ids=FORM_IDS)
def test_forms_match_oracle(cuda, force_form, form, n_split, fp8, shape, slot_mode):
    """Every device form, f16 and e4m3 pages, one split and four, all 15 positions in one launch
    (each row in its own slot; (48, 6, 6) gives the wave form 90 items, not a multiple of 4)."""
    c = matrix_case(shape, fp8, slot_mode)
    force_form(form)
    out = Dev(c, n_split).run(form)
    _assert_out(out, c.ref[0], f"{FORM_IDS[FORM_SPLITS.index((form, n_split))]} {'fp8' if fp8 else 'f16'} {shape}")


# ---------------------------------------------------------------- 2. append, no stray writes
@gpu
@shape_param
@kv_param
@pytest.mark.parametrize("form,n_split", [(PF4, 1), (PF8, 1), (NP, 4), (WAVE, 4), (WAVE, 1)],
                         ids=["pf4-s1", "pf8-s1", "np-s4", "wave-s4", "wave-s1"])
def test_append_and_no_stray_writes(cuda, force_form, form, n_split, fp8, shape):
    c = matrix_case(shape, fp8, "perm")
    force_form(form)
    d = Dev(c, n_split)
    d.run(form)
    _assert_appended(c, d.kc.cpu(), d.vc.cpu(), c.pos, c.ref[1], c.ref[2], c.kc, c.vc)


# ---------------------------------------------------------------- 3. second step on the same buffers
STEP_POS = (0, 31, 63, 127, 255, 300)   # the second step crosses a chunk, a page, a split


@functools.lru_cache(maxsize=None)
def step_case(shape, fp8):
    hd, Hq, Hkv = shape
    c = build_case(hd, Hq, Hkv, STEP_POS, fp8, "perm", seed=300 + hd + Hq + fp8, steps=2)
    c.ref = oracle(c, c.kc, c.vc, c.qkv, c.pos)
    kc2, vc2 = c.kc.clone(), c.vc.clone()
    _append(kc2, vc2, c, c.pos, c.ref[1], c.ref[2])   # the oracle's own cache after step one
    c.pos2 = [p + 1 for p in c.pos]
    c.ref2 = oracle(c, kc2, vc2, c.qkv2, c.pos2)
    c.kc2, c.vc2 = kc2, vc2
    return c


@gpu
@pytest.mark.parametrize("shape", [(128, 32, 8), (48, 6, 6)], ids=lambda s: "x".join(map(str, s)))
@kv_param
@pytest.mark.parametrize("form,n_split", [(PF4, 1), (PF8, 1), (NP, 4), (WAVE, 4)],
                         ids=["pf4-s1", "pf8-s1", "np-s4", "wave-s4"])
def test_second_step_reads_the_append(cuda, force_form, form, n_split, fp8, shape):
    """pos + 1 with a new qkv on the same caches, counters and partials: the first append landed
    where the next step reads it (not only in the LDS patch), and the counters are back at zero."""
    c = step_case(shape, fp8)
    force_form(form)
    d = Dev(c, n_split)
    _assert_out(d.run(form), c.ref[0], "step 1")
    _assert_out(d.run(form, c.qkv2, c.pos2), c.ref2[0], "step 2")
    _assert_appended(c, d.kc.cpu(), d.vc.cpu(), c.pos2, c.ref2[1], c.ref2[2], *_after_first(c, d))


def _after_first(c, d):
    """The caches step two started from: the GPU's own first append is not known bit for bit (one
    code of slack), so take the entries of step one from the GPU's final cache."""
    kc, vc = c.kc.clone(), c.vc.clone()
    ka, va = d.kc.cpu(), d.vc.cpu()
    for t, pos in enumerate(c.pos):
        page, idx = int(c.bt[c.slots[t], pos // 64]), pos % 64
        kc[page, :, idx, :], vc[page, :, :, idx] = ka[page, :, idx, :], va[page, :, :, idx]
    return kc, vc


# ---------------------------------------------------------------- 4. many splits
@gpu
@kv_param
@pytest.mark.parametrize("form", [NP, WAVE], ids=["np", "wave"])
def test_many_splits(cuda, force_form, form, fp8):
    """n_act 66 (the merge's 64-lane loops go round twice; splits 66.. take no part) and
    n_act 128 = ATTN_MAX_SPLITS in one launch."""
    c = many_case(fp8)
    force_form(form)
    d = Dev(c, 128)
    _assert_out(d.run(form), c.ref[0], f"many splits {FORM_NAMES[form]}")
    _assert_appended(c, d.kc.cpu(), d.vc.cpu(), c.pos, c.ref[1], c.ref[2], c.kc, c.vc)


# ---------------------------------------------------------------- 5. deferred norm and bias
NORM_POS = (0, 31, 64, 129, 300, 511)


@functools.lru_cache(maxsize=None)
def norm_case(shape, fp8, norm):
    hd, Hq, Hkv = shape
    c = build_case(hd, Hq, Hkv, NORM_POS, fp8, "slot0", seed=500 + hd + fp8 + len(norm), norm=norm)
    c.ref = oracle(c, c.kc, c.vc, c.qkv, c.pos)
    return c


@gpu
@pytest.mark.parametrize("norm", ["ssq", "bias"])
@pytest.mark.parametrize("shape", [(128, 32, 8), (64, 32, 4)], ids=lambda s: "x".join(map(str, s)))
@kv_param
@pytest.mark.parametrize("form,n_split", [(NP, 4), (NP, 1), (WAVE, 1), (WAVE, 4)],
                         ids=["np-s4", "np-s1", "wave-s1", "wave-s4"])
def test_deferred_norm_and_bias(cuda, force_form, form, n_split, fp8, shape, norm):
    c = norm_case(shape, fp8, norm)
    force_form(form)
    d = Dev(c, n_split)
    _assert_out(d.run(form), c.ref[0], f"norm {norm} {FORM_NAMES[form]}")
    _assert_appended(c, d.kc.cpu(), d.vc.cpu(), c.pos, c.ref[1], c.ref[2], c.kc, c.vc)


@gpu
def test_pre_and_attn_o_refuse_the_deferred_norm(cuda, force_form):
    """attn_decode_pre_ok and attn_o_supported exclude ssq: both entry points fail cleanly."""
    from mipipe.ops.kernels import attn_decode, attn_o, PackedWeight
    c = norm_case((128, 32, 8), False, "ssq")
    force_form(PF4)
    d = Dev(c, 1)
    kw = d.kw()
    kw["pre"] = True
    with pytest.raises(RuntimeError, match="pre-appended"):
        attn_decode(*d.args(c.qkv, c.pos), **kw)
    c4 = attn_o_case(4, False, False)
    d4 = Dev(c4, 1)
    w = PackedWeight(Q.quantize(np.zeros((256, 1024), np.float32), Q.Q8_0), Q.Q8_0, 256, 1024)
    y = torch.zeros(4, 256, device="cuda")
    a = d4.args(c4.qkv, c4.pos)
    with pytest.raises(RuntimeError, match="unsupported"):
        attn_o(w, y, *a[:-2], a[-1], slot0=c4.slot0, ssq=torch.ones(4, device="cuda"), eps=1e-5, d_model=4096)
    torch.cuda.synchronize()
    assert _same_bytes(d.kc.cpu(), c.kc) and _same_bytes(d4.kc.cpu(), c4.kc) and float(y.abs().sum()) == 0


# ---------------------------------------------------------------- 6. pre inputs
@functools.lru_cache(maxsize=None)
def pre_case(shape, fp8):
    hd, Hq, Hkv = shape
    c = build_case(hd, Hq, Hkv, NORM_POS, fp8, "slot0", seed=600 + hd + fp8, pre=True)
    c.ref = oracle(c, c.kc, c.vc, c.qkv, c.pos)
    return c


@gpu
@pytest.mark.parametrize("shape", [(128, 32, 8), (48, 6, 6)], ids=lambda s: "x".join(map(str, s)))
@kv_param
@pytest.mark.parametrize("form", [PF4, PF8], ids=["pf4", "pf8"])
def test_pre_inputs(cuda, force_form, form, fp8, shape):
    """q already rotated, the new K / V already in the cache: no RoPE, no append, no write at all."""
    from mipipe.ops.kernels import attn_decode
    c = pre_case(shape, fp8)
    force_form(form)
    d = Dev(c, 1)
    _assert_out(d.run(form), c.ref[0], f"pre {FORM_NAMES[form]}")
    assert _same_bytes(d.kc.cpu(), c.kc) and _same_bytes(d.vc.cpu(), c.vc)
    d4 = Dev(c, 4)
    with pytest.raises(RuntimeError, match="pre-appended"):
        attn_decode(*d4.args(c.qkv, c.pos), **d4.kw())
    torch.cuda.synchronize()
    assert _same_bytes(d4.kc.cpu(), c.kc) and _same_bytes(d4.vc.cpu(), c.vc)


# ---------------------------------------------------------------- 7. lazy rescale
def _levels_gain(stride, levels):
    """One spike key per 32-key chunk; the chunks c with the same c // stride share an exp2-domain
    score level, so the wave that takes chunks c, c + stride, ... (and the wave kernel, every 4th or
    8th chunk) sees its running maximum rise by the level steps."""
    def gain(j, pos):
        ch = j // 32
        if j == pos or j == 32 * ch + (7 * ch + 3) % 32:
            return levels[min(ch // stride, len(levels) - 1)] / LOG2E
        return None
    return gain


def _lastmax_gain(j, pos):
    """The largest score (12 above the rest, exp2 domain) sits in the masked last chunk."""
    if j >= pos - 1:
        return 16.0 / LOG2E
    return 4.0 / LOG2E if j % 32 == 5 else None


RESCALE = {"rise7+9+7": _levels_gain(4, [0.0, 7.0, 16.0, 23.0]), "rise7+0+0": _levels_gain(4, [0.0, 7.0, 7.0, 7.0]),
           "rise7x8": _levels_gain(8, [0.0, 7.0]), "rise9x8": _levels_gain(8, [0.0, 9.0]), "lastmax": _lastmax_gain}


@functools.lru_cache(maxsize=None)
def rescale_case(name, fp8):
    poss = (300, 289) if name == "lastmax" else (511, 500)
    c = build_case(128, 32, 8, poss, fp8, "slot0", seed=700 + len(name) + fp8, k_ord=0.1, k_noise=0.1,
                   stale_gain=30.0 / LOG2E, gain=RESCALE[name])
    c.ref = oracle(c, c.kc, c.vc, c.qkv, c.pos)
    return c


@gpu
@pytest.mark.parametrize("name", list(RESCALE))
@kv_param
@pytest.mark.parametrize("form", [PF4, PF8, NP, WAVE], ids=["pf4", "pf8", "np", "wave"])
def test_lazy_rescale(cuda, force_form, form, fp8, name):
    """Running maxima that rise by about 7 (no rescale: p up to 2^7 against the old reference) and
    by about 9 (rescale) from chunk to chunk of one wave, both sides of the +8 threshold; and the
    largest score in the chunk that the key mask cuts."""
    c = rescale_case(name, fp8)
    force_form(form)
    _assert_out(Dev(c, 1).run(form), c.ref[0], f"rescale {name} {FORM_NAMES[form]}")


# ---------------------------------------------------------------- 8. attention + o-projection
ATTN_O_POS = {1: (129,), 4: (31, 64, 129, 300)}


@functools.lru_cache(maxsize=None)
def attn_o_case(M, fp8, pre):
    c = build_case(128, 8, 2, ATTN_O_POS[M], fp8, "slot0", seed=800 + M + fp8 + 2 * pre, pre=pre)
    c.ref = oracle(c, c.kc, c.vc, c.qkv, c.pos)
    return c


def _run_attn_o(c, w, y0):
    from mipipe.ops.kernels import attn_o
    d = Dev(c, 1)
    a = d.args(c.qkv, c.pos)
    kw = d.kw()
    y = attn_o(w, y0.clone().cuda(), *a[:-2], a[-1], slot=kw["slot"], slot0=kw["slot0"], kv_fp8=c.fp8, pre=c.pre)
    torch.cuda.synchronize()
    return y.cpu().double(), d


@gpu
@pytest.mark.parametrize("pre", [False, True], ids=["rot", "pre"])
@kv_param
@pytest.mark.parametrize("M", [1, 4])
def test_attn_o_identity(cuda, native, M, fp8, pre):
    """W_o picks attention element 4 i + s for output i with the exactly representable Q8_0 weight
    127 / 128 (after test_gemv_asymmetric_identity): Y - Y0 is the attention output itself."""
    from mipipe.ops.kernels import PackedWeight
    c = attn_o_case(M, fp8, pre)
    n, k, wv = 256, 1024, 127.0 / 128.0
    y0 = torch.randn(M, n, generator=torch.Generator().manual_seed(M))
    got = torch.zeros(M, k, dtype=torch.float64)
    for s in range(4):
        wmat = np.zeros((n, k), np.float32)
        wmat[np.arange(n), 4 * np.arange(n) + s] = wv
        raw = Q.quantize(wmat, Q.Q8_0)
        assert (Q.dequantize(raw, Q.Q8_0).reshape(n, k) == wmat).all()
        y, d = _run_attn_o(c, PackedWeight(raw, Q.Q8_0, n, k), y0)
        got[:, s::4] = (y - y0.double()) / wv
        if pre:
            assert _same_bytes(d.kc.cpu(), c.kc) and _same_bytes(d.vc.cpu(), c.vc)
        else:
            _assert_appended(c, d.kc.cpu(), d.vc.cpu(), c.pos, c.ref[1], c.ref[2], c.kc, c.vc)
    _assert_out(got.view(M, c.Hq, c.hd), c.ref[0], f"attn_o identity M{M}")


@gpu
@pytest.mark.parametrize("pre", [False, True], ids=["rot", "pre"])
@kv_param
@pytest.mark.parametrize("qt", [Q.Q4_K, Q.Q6_K, Q.Q8_0])
def test_attn_o_random_weights(cuda, force_form, qt, fp8, pre):
    """Y = Y0 + a . deq(W_o)^T in float64, a = the f16 output of the stand-alone decode launch on
    the same inputs (checked against the oracle here too); NMSE < 1e-5, the gemvs residual tests'
    bound."""
    from mipipe.ops.kernels import PackedWeight
    n, k = 256, 1024
    rng = np.random.default_rng(40 + qt)
    raw = Q.quantize((rng.standard_normal((n, k)) / math.sqrt(k)).astype(np.float32), qt)
    deq = torch.from_numpy(Q.dequantize(raw, qt).reshape(n, k)).double()
    w = PackedWeight(raw, qt, n, k)
    force_form(PF4)
    for M in (1, 4):
        c = attn_o_case(M, fp8, pre)
        a = Dev(c, 1).run(PF4)
        _assert_out(a, c.ref[0], f"attn_o stand-alone M{M}")
        y0 = torch.randn(M, n, generator=torch.Generator().manual_seed(M + qt))
        y, _ = _run_attn_o(c, w, y0)
        ref = y0.double() + a.view(M, k) @ deq.T
        nm = float(((y - ref) ** 2).sum() / (ref ** 2).sum())
        assert nm < 1e-5, (M, nm)
