"""Decode attention over shared prompt prefixes at op level: attn_shared (attn_shared.hip, the prefix
phase) followed by attn_decode over the private suffixes with the prefix partials in its merge
(attention.hip, attn_decode_body<SP>), together against a float64 oracle.

The oracle is the operation's definition and knows nothing about groups: deferred norm / bias, RoPE,
the scaled q (q_scale * log2 e) rounded to f16, the new K / V rounded to the cache type, keys
[0, pos] of each row through ITS OWN block-table row exactly as stored, softmax and P.V in float64.

Inputs follow test_attn_decode_gpu.py: per kv head a direction u; q = u + 0.5 noise; marked keys
5 u / sqrt(hd) + 0.3 noise with v = +-32 at the first and last key of every shared page, the first
private key (kv_begin), pos - 1 and pos; ordinary keys 0.3 noise; finite stale keys 8 u / sqrt(hd)
with v = +-32 (and non-zero padded dims) at every position past a row's pos, in the trash page and
behind the unshared spare table entries.  Checked once on the CPU while writing the test, on the
oracle alone, for every case below: leaving out any one shared page, or counting the last shared
page twice (in both phases), moves every head of every member row by at least 10x the tolerance
(least margin 77x).

Tolerance: rtol = atol = 5e-3, the project's number for this arithmetic (f16 operands, f32
accumulate, f16 output; test_attn_decode_gpu.py).  Largest |err| / (atol + rtol |ref|), first GPU
run, over all cases: f16 0.77, fp8 0.90 (the f16 rounding of the probabilities before the P.V MFMA, as in
test_attn_decode_gpu.py), so the tolerance is not tightened.
"""
import functools
import math

import pytest
import torch

from test_attn_decode_gpu import (NP, PF4, PF8, Case, _decode, _make_qkv, _rot, _round_cache, _same_bytes,  # noqa: F401
                                  _store, force_form)
from test_v_blocked_gpu import to_blocked

gpu = pytest.mark.gpu
RTOL = ATOL = 5e-3
LOG2E = 1.4426950408889634
M, MAX_PAGES = 24, 8
SUFFIX = (1, 64, 65, 130)   # pos - kv_begin + 1; 130 spans two suffix splits at split_len 128
# membership: [(member rows, index of the leader in them)]; every other row is ungrouped
MEMBERS = {"g2": [((5, 9), 0)], "g17": [(tuple(range(3, 20)), 0)], "two": [((1, 4, 7, 10), 2), ((2, 5, 20), 2)]}
UNGROUPED_POS = (0, 63, 64, 200, 17, 130, 449)   # the first ungrouped row sits at pos 0
# (hd, Hq, Hkv), fp8, blocked V, membership, shared pages, page splits, decode form, decode splits, norm
CASES = [((128, 32, 8), False, False, "two", 5, 2, NP, 4, None), ((128, 32, 8), True, True, "g17", 5, 1, NP, 4, None),
         ((64, 8, 2), False, True, "g2", 1, 1, PF4, 1, "bias"), ((64, 8, 2), True, False, "g17", 5, 2, PF8, 1, None),
         ((96, 6, 6), False, False, "g17", 1, 1, NP, 4, None), ((96, 6, 6), True, True, "two", 5, 2, NP, 4, "bias"),
         ((128, 16, 1), False, True, "g17", 5, 2, NP, 4, None), ((128, 16, 1), True, False, "two", 1, 1, PF4, 1, None)]


@functools.lru_cache(maxsize=None)
def build(shape, fp8, members, n_sh, norm):
    from mipipe.ops.kernels import rope_cs_table
    hd, Hq, Hkv = shape
    g = torch.Generator().manual_seed(hd + Hq + 7 * fp8 + 31 * n_sh + len(members))
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sign = lambda *s: (torch.randint(0, 2, s, generator=g) * 2 - 1).double()
    c = Case()
    c.hd, c.Hq, c.Hkv, c.G, c.Dp, c.fp8, c.pre = hd, Hq, Hkv, Hq // Hkv, 64 if hd <= 64 else 128, fp8, False
    # "two": row t sits in slot M - 1 - t, so a slot taken for a row index (or the reverse) is visible
    c.q_scale, c.k_noise, c.slots, Dp = 1.0 / math.sqrt(hd), 0.3, [M - 1 - t if members == "two" else t for t in range(M)], c.Dp
    c.kv_begin, c.pos, c.groups = [0] * M, [None] * M, []
    for rows, li in MEMBERS[members]:
        c.groups.append((c.slots[rows[li]], n_sh, list(rows)))
        for i, t in enumerate(rows):
            c.kv_begin[t], c.pos[t] = 64 * n_sh, 64 * n_sh + SUFFIX[i % 4] - 1
    free = [t for t in range(M) if c.pos[t] is None]
    for i, t in enumerate(free):
        c.pos[t] = UNGROUPED_POS[i % len(UNGROUPED_POS)]
    n_pages = sum(p // 64 + 1 for p in c.pos) + 2
    perm = [int(p) for p in torch.randperm(n_pages, generator=g)]
    c.trash = perm.pop()
    c.bt = torch.full((M, MAX_PAGES), c.trash, dtype=torch.int32)   # spare entries: the stale trash page
    for leader, _, rows in c.groups:
        shared = [perm.pop() for _ in range(n_sh)]
        for t in rows:
            c.bt[c.slots[t], :n_sh] = torch.tensor(shared, dtype=torch.int32)
    for t in range(M):
        for i in range(c.kv_begin[t] // 64, c.pos[t] // 64 + 1):
            c.bt[c.slots[t], i] = perm.pop()
    c.cs = rope_cs_table(MAX_PAGES * 64, hd, 10000.0)
    u = rnd(Hkv, hd)
    c.u = u * math.sqrt(hd) / u.norm(dim=1, keepdim=True)
    c.ssq, c.bias, c.eps, c.d_model = None, None, 0.0, 0
    if norm:
        c.eps, c.d_model = 1e-5, 4096
        c.ssq = (c.d_model * (0.5 + 3.5 * torch.rand(M, generator=g))).float()
        c.bias = (0.5 * torch.randn((Hq + 2 * Hkv) * hd, generator=g)).float()
    Kp, Vp = torch.zeros(n_pages, Hkv, 64, Dp, dtype=torch.float64), torch.zeros(n_pages, Hkv, Dp, 64, dtype=torch.float64)
    Kp[..., :hd] = 8.0 * c.u[None, :, None, :] / math.sqrt(hd) + 0.3 * rnd(n_pages, Hkv, 64, hd)   # stale everywhere
    Vp[:, :, :hd, :] = 32.0 * sign(n_pages, Hkv, hd, 64)
    Kp[..., hd:], Vp[:, :, hd:, :] = 0.5 + rnd(n_pages, Hkv, 64, Dp - hd).abs(), 0.5 + rnd(n_pages, Hkv, Dp - hd, 64).abs()

    def fill(page, lo, n, marked):   # n live keys from key `lo` of a page: ordinary, the marked ones aligned with u
        K, V = 0.3 * rnd(Hkv, n, hd), rnd(Hkv, hd, n)
        for j in marked:
            K[:, j - lo] = 5.0 * c.u / math.sqrt(hd) + 0.3 * rnd(Hkv, hd)
            V[:, :, j - lo] = 32.0 * sign(Hkv, hd)
        Kp[page, :, lo:lo + n, :hd], Kp[page, :, lo:lo + n, hd:] = K, 0.0
        Vp[page, :, :hd, lo:lo + n], Vp[page, :, hd:, lo:lo + n] = V, 0.0
    for leader, _, rows in c.groups:
        for i in range(n_sh):
            fill(int(c.bt[leader, i]), 0, 64, (0, 63))
    for t in range(M):
        for i in range(c.kv_begin[t] // 64, c.pos[t] // 64 + 1):
            n = min(64, c.pos[t] - 64 * i)   # keys [64 i, pos) of the page are history
            mark = {c.kv_begin[t] - 64 * i, c.pos[t] - 1 - 64 * i} & set(range(n))
            if n > 0:
                fill(int(c.bt[c.slots[t], i]), 0, n, mark)
    c.qkv = _make_qkv(c, c.pos, g, lambda j, pos: 5.0)[0]
    c.kc, c.vc = _store(_round_cache(Kp, fp8), fp8), _store(_round_cache(Vp, fp8), fp8)
    c.ref = oracle(c)
    return c


def oracle(c):
    hd, Hq, Hkv, G = c.hd, c.Hq, c.Hkv, c.G
    Kl, Vl, out = _decode(c.kc), _decode(c.vc), torch.zeros(M, Hq, hd, dtype=torch.float64)
    for t, pos in enumerate(c.pos):
        x = c.qkv[t, :(Hq + 2 * Hkv) * hd].double()
        if c.ssq is not None:
            x = x * torch.rsqrt(c.ssq[t].double() / c.d_model + c.eps) + c.bias.double()
        q, k, v = x[:Hq * hd].view(Hq, hd), x[Hq * hd:(Hq + Hkv) * hd].view(Hkv, hd), x[(Hq + Hkv) * hd:].view(Hkv, hd)
        qs = (_rot(q, c.cs[pos]) * (c.q_scale * LOG2E)).to(torch.float16).double()
        j = torch.arange(pos + 1)
        pages = c.bt[c.slots[t], j // 64].long()
        K, V = Kl[pages, :, j % 64, :hd].clone(), Vl[pages, :, :hd, j % 64].clone()   # [L][Hkv][hd]
        K[pos], V[pos] = _round_cache(_rot(k, c.cs[pos]), c.fp8), _round_cache(v, c.fp8)
        s2 = torch.einsum("hd,jhd->hj", qs, K.repeat_interleave(G, 1))
        p = torch.exp2(s2 - s2.max(dim=1, keepdim=True).values)
        out[t] = torch.einsum("hj,jhd->hd", p, V.repeat_interleave(G, 1)) / p.sum(1, keepdim=True)
    return out


@gpu
@pytest.mark.parametrize("shape,fp8,blocked,members,n_sh,n_psplit,form,n_split,norm", CASES,
                         ids=[f"{'x'.join(map(str, k[0]))}-{'fp8' if k[1] else 'f16'}-{'blk' if k[2] else 'vt'}-{k[3]}-"
                              f"p{k[4]}s{k[5]}-f{k[6]}s{k[7]}" for k in CASES])
def test_prefix_and_suffix_match_oracle(cuda, force_form, shape, fp8, blocked, members, n_sh, n_psplit, form, n_split,
                                        norm):
    from mipipe.ops.kernels import (DecodeAttnScratch, SharedAttnTable, attn_decode_form, attn_decode_shared,
                                    attn_shared, v_layout)
    c = build(shape, fp8, members, n_sh, norm)
    force_form(form)
    assert attn_decode_form(M, c.Hkv, n_split) == form
    kc, vc = c.kc.cuda(), (to_blocked(c.vc) if blocked else c.vc).cuda()
    bt, cs, qkv, pos = c.bt.cuda(), c.cs.cuda(), c.qkv.cuda(), torch.tensor(c.pos, dtype=torch.int32).cuda()
    table = SharedAttnTable(M, c.Hq, c.Dp, n_psplit, c.groups, c.slots, c.bt)
    scratch = DecodeAttnScratch(M, c.Hq, c.Hkv, c.Dp, n_split)
    kw = dict(ssq=None if c.ssq is None else c.ssq.cuda(), eps=c.eps, d_model=c.d_model,
              bias=None if c.bias is None else c.bias.cuda(), kv_fp8=fp8)
    with v_layout(blocked):
        attn_shared(qkv, pos, bt, cs, kc, vc, c.Hq, c.Hkv, c.hd, c.Dp, c.q_scale, table, **kw)
        out = attn_decode_shared(qkv, pos, bt, cs, kc, vc, c.Hq, c.Hkv, c.hd, c.Dp, c.q_scale,
                                 MAX_PAGES * 64 if n_split == 1 else 128, n_split, scratch, table, **kw,
                                 **(dict(slot=torch.tensor(c.slots, dtype=torch.int32).cuda()) if members == "two"
                                    else dict(slot0=0)))
    torch.cuda.synchronize()
    got = out.cpu().double().view(M, c.Hq, c.hd)
    ratio = ((got - c.ref).abs() / (ATOL + RTOL * c.ref.abs())).amax(dim=(1, 2))
    print(f"error ratio {'fp8' if fp8 else 'f16'} {shape} {members}: {float(ratio.max()):.3f}")
    assert (ratio <= 1).all(), ("rows off", (ratio > 1).nonzero().flatten().tolist(), float(ratio.max()))
    assert int(scratch.counters.abs().sum()) == 0, "arrival counters did not return to zero"
    shared = sorted({int(p) for leader, n, _ in c.groups for p in c.bt[leader, :n]})
    assert _same_bytes(kc.cpu()[shared], c.kc[shared]), "a shared K page was written"
    assert _same_bytes(vc.cpu()[shared], (to_blocked(c.vc) if blocked else c.vc)[shared]), "a shared V page was written"

