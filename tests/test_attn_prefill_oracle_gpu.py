"""The prefill path of the attention layer at op level against a float64 oracle: rope_kv
(elementwise.hip), attn_prefill with its LSE merge (attn_prefill.hip, attn_combine) and the row-group
fallback attention kernel (attention.hip: attn_kernel).

The oracle is the operations' definition in plain torch float64 on the CPU.  rope_kv: q and k rotated
by the (cos, sin) row the kernel is given, q scaled by q_scale and rounded to f16 with zeros in the
padded dims, k and v rounded to the cache type (f16, or e4m3 with the +-448 clamp) and stored at
(block_table[slot][pos / 64], head, pos % 64), V in the V^T or the blocked layout of kernels_api.h.
Attention: q is the f16 input times log2(e) in f32, rounded to f16 again (the MFMA operand of
attn_prefill_kernel); keys [0, pos[row]] of the row's slot through the block table from the stored
bytes exactly as decoded; softmax and P.V in float64.

The inputs make ONE wrong key visible in every query head of the rows it concerns (randn q / K / V
over zero pages cannot: the softmax is flat, and at a few hundred keys a stray slot moves the output
by ~1/L).  Per kv head there are five orthogonal directions u, e1 .. e4 of length sqrt(hd).  A row's
rotated q is u + c(p) + 0.1 noise with the positional code
c(p) = cos(t1 p) e1 + sin(t1 p) e2 + cos(t2 p) e3 + sin(t2 p) e4, t1 = 2 pi / 64, t2 = 2 pi / 40.  The
keys of the chunk are 1.5 c(j) / sqrt(hd) + 0.1 noise, so score(row p, key j) is about
1.5 (cos(t1 (j - p)) + cos(t2 (j - p))): 3 at j = p, a row weighs its ~6 nearest keys alike, and the
second frequency keeps the keys 64, 128, ... earlier well below them.  The boundary keys (0, 31, 32,
every page edge 64 k - 1 and 64 k, p0 - 1: the chunk, page and split edges) are 3 u / sqrt(hd) + 0.1
noise (score 3 for every row); the other keys of the prior context are -2 u / sqrt(hd) + 0.1 noise
with unit v.  Chunk and boundary keys have v = +-16.  Before any of that is written, EVERY page -- the
rest of the last pages, the pages of slots no row uses, spare pages no block table names, the trash
page behind the unused table entries -- holds finite stale keys 6 u / sqrt(hd) + 0.3 noise with
v = +-16 and non-zero padded dims, which would dominate if read.  Keys of the sequence above a tile's
last row are valid later tokens.  test_inputs_expose_one_wrong_key (CPU) proves on the oracle alone
that each of eight mutations (key p + 1 seen, key p dropped, every loaded page taken as `full`, the
tile's last page dropped, the stale slot past the segment read, two block-table entries swapped, the
neighbouring slot's table, one boundary key dropped) moves every head of every row whose set of cache
cells it changes by at least 10x the output tolerance; the least margin over all cases is 37x.

Two choices differ from the decode module's inputs, both measured:
  * |v| is 16, not 32.  A prefill row near the start of a sequence has 2 .. 8 keys, and the kernel
    rounds each probability to f16 (2^-12 relative) before the P.V MFMA; with +-32 values that is up
    to 32 * 2^-12 = 0.0078 on an element where the reference cancels to ~0, above atol.  The first GPU
    run with +-32 gave ratios up to 1.25 on 40 of 800 000 elements, and a CPU emulation of exactly
    that rounding reproduced the GPU's values bit for bit there.  +-16 bounds the effect by 0.0039.
  * the noise on valid keys and on q is 0.1, not 0.3 (the stale keys keep 0.3).  The property is a
    minimum over ~10^5 (row, head, key) triples, and at 0.3 (0.5 in the score) the -3.5 sigma key
    weighs a fifth of its neighbours: the least margin was 9x.

Tolerance: rtol = atol = 5e-3, the project's number for this arithmetic (f16 operands, f32
accumulate, f16 output; test_attn_decode_gpu.py, test_rope_kv_attention).  Largest
|err| / (atol + rtol |ref|) per kernel and KV type, first GPU run with these inputs (every row and
head of every case):
    attn_prefill, one split (shapes, segment sets, 300 tiles)   f16 0.74   fp8 0.62
    attn_prefill, splits + attn_combine                         f16 0.64   fp8 0.62
    rope_kv then attn_prefill (second chunk)                    f16 0.53   fp8 0.59
    lazy rescale (worst: rise7 f16, rise8 fp8)                  f16 0.58   fp8 0.83
    fallback attn_kernel: prefill, decode 1 split, 3 splits     f16 0.85 / 0.85 / 0.85
No entry stays below 0.2, so the tolerance is not tightened.  (The fallback kernel multiplies the f16 q
itself and exponentiates in base e; against an oracle with that operand it measures 0.60.  It is
compared with the same oracle as attn_prefill all the same: the difference is one f16 rounding of q.)
rope_kv: V cells equal the oracle's bytes; K cells are one code off on 3 of 61 440 elements in the
worst f16 case, on none with e4m3 pages.
"""
import functools
import math

import pytest
import torch

from test_attn_decode_gpu import _codes, _decode, _rot, _round_cache, _same_bytes, _store

gpu = pytest.mark.gpu

RTOL = ATOL = 5e-3
Q_RTOL = Q_ATOL = 2e-3          # q_out of rope_kv (test_rope_kv_attention)
LOG2E = 1.4426950408889634
MAX_PAGES = 8                   # block-table width: contexts of at most 448 leave one unused entry
THETA, THETA2 = 2 * math.pi / 64, 2 * math.pi / 40
A_CODE, SPIKE, ORDINARY, STALE = 3.0, 3.0, -2.0, 6.0
NOISE, STALE_NOISE = 0.1, 0.3
V_MAG = 16.0                    # |v| of every chunk, boundary and stale key (module docstring)

# (hd, Hq, Hkv)
SHAPES = [(128, 32, 8), (64, 32, 4), (48, 6, 6), (96, 8, 2), (128, 28, 4), (64, 6, 2), (64, 10, 2), (128, 12, 1),
          (128, 16, 1), (64, 32, 1)]
SEGS = {   # (slot, p0, T): rows at positions p0 .. p0 + T - 1 of `slot`
    "one": [(0, 0, 1)],
    "t65": [(0, 0, 65)],
    "straddle": [(1, 63, 2)],
    "mid": [(0, 200, 130)],
    "packed": [(2, 0, 20), (0, 100, 45), (1, 5, 3), (3, 0, 128)],
}
SEG_SHAPES = [(128, 32, 8), (64, 32, 4), (48, 6, 6)]   # G 4 / 8 / 1: 32, 16 and 128 tokens per tile
BIG_SHAPE, BIG_SEGS = (64, 128, 1), [(0, 0, 300)]       # one token per tile: 300 tiles, two launches
FALLBACK_SHAPES = [(128, 32, 8), (64, 32, 4), (48, 6, 6), (128, 28, 4), (128, 16, 1)]
ROPE_SHAPES = [(128, 32, 8), (64, 32, 4), (48, 6, 6), (96, 8, 2)]
CHAIN_SHAPES = [(128, 32, 8), (48, 6, 6)]
CHAIN_SEGS = [(1, 100, 60)]     # chunks [0, 100) and [100, 160): the boundary is inside page 1

sid = lambda s: "x".join(map(str, s))
kv_param = pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
layout_param = pytest.mark.parametrize("blocked", [False, True], ids=["vt", "vblk"])


class Case:
    pass


# ---------------------------------------------------------------- inputs
def _boundary(p0, S):
    b = {0, 31, 32, 63, 64, 127, 128, p0 - 1} | {64 * k - 1 for k in range(1, MAX_PAGES)} | {
        64 * k for k in range(1, MAX_PAGES)}
    return sorted(x for x in b if 0 <= x < S)


def _tiles(rows, bt_rows):
    """(first row, rows) of every tile, cut as mp_op_attn_prefill and HipStage::attention cut them."""
    return [(row0 + r, min(bt_rows, T - r)) for row0, T in rows for r in range(0, T, bt_rows)]


def build_case(shape, fp8, segs, seed, *, levels=None, stale=STALE, rope=False):
    """levels: the lazy-rescale inputs (every key of 32-key chunk c scores levels[c], base 2, for every
    row).  rope: the caches start as poison only; the sequence gets there through the rope_kv oracle
    in two chunks ([0, p0) and [p0, p0 + T)) from c.qkv, as the engine prefills it."""
    from mipipe.ops.kernels import rope_cs_table
    hd, Hq, Hkv = shape
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sign = lambda *s: (torch.randint(0, 2, s, generator=g) * 2 - 1).double()
    c = Case()
    c.hd, c.Hq, c.Hkv, c.G, c.Dp, c.fp8 = hd, Hq, Hkv, Hq // Hkv, 64 if hd <= 64 else 128, fp8
    c.segs, c.q_scale, c.max_pages = list(segs), 1.0 / math.sqrt(hd), MAX_PAGES
    G, Dp, rt = c.G, c.Dp, math.sqrt(hd)
    c.M = sum(T for _, _, T in segs)
    c.pos = torch.cat([torch.arange(p0, p0 + T, dtype=torch.int32) for _, p0, T in segs])
    c.slot = torch.cat([torch.full((T,), s, dtype=torch.int32) for s, _, T in segs])
    c.rows, row = [], 0
    for _, _, T in segs:
        c.rows.append((row, T))
        row += T
    c.tiles = _tiles(c.rows, 128 // G)
    # slots and pages: the segments' slots in any order, one more slot than the largest; the slots no
    # segment uses own two stale pages each; spare pages; unused table entries name the trash page
    used = [s for s, _, _ in segs]
    assert len(set(used)) == len(used)
    n_slots = max(used) + 2
    c.need = {s: (p0 + T - 1) // 64 + 1 for s, p0, T in segs}
    assert max(c.need.values()) < MAX_PAGES
    for s in range(n_slots):
        c.need.setdefault(s, 2)
    c.n_pages = sum(c.need.values()) + 4
    perm = [int(p) for p in torch.randperm(c.n_pages, generator=g)]
    c.trash = perm[0]
    c.bt = torch.full((n_slots, MAX_PAGES), c.trash, dtype=torch.int32)
    nxt = 1
    for s in sorted(c.need):
        for i in range(c.need[s]):
            c.bt[s, i] = perm[nxt]
            nxt += 1
    # the slot whose table a row would take by mistake: the next segment's, or an unused slot's
    c.neighbour = [used[(i + 1) % len(used)] if len(used) > 1 else (used[0] + 1) % n_slots for i in range(len(used))]
    c.cs = rope_cs_table(MAX_PAGES * 64, hd, 10000.0)
    basis = torch.linalg.qr(rnd(Hkv, hd, 5)).Q * rt           # orthogonal columns of length sqrt(hd)
    c.u, e = basis[:, :, 0], [basis[:, :, i] for i in range(1, 5)]
    # stale data everywhere first (what a kernel reading past the sequence would see)
    Kp = torch.zeros(c.n_pages, Hkv, 64, Dp, dtype=torch.float64)
    Vp = torch.zeros(c.n_pages, Hkv, Dp, 64, dtype=torch.float64)
    Kp[..., :hd] = stale * c.u[None, :, None, :] / rt + STALE_NOISE * rnd(c.n_pages, Hkv, 64, hd)
    Vp[:, :, :hd, :] = V_MAG * sign(c.n_pages, Hkv, hd, 64)
    if Dp > hd:
        pad = lambda *s: (0.5 + torch.rand(*s, generator=g, dtype=torch.float64)) * sign(*s)
        Kp[..., hd:] = pad(c.n_pages, Hkv, 64, Dp - hd)
        Vp[:, :, hd:, :] = pad(c.n_pages, Hkv, Dp - hd, 64)
    c.kc0, c.vc0 = _store(_round_cache(Kp, fp8), fp8), _store(_round_cache(Vp, fp8), fp8)
    # the sequences: rotated q, k and v of every position [0, p0 + T)
    c.bset, seqs = [], []
    for s, p0, T in segs:
        S = p0 + T
        j = torch.arange(S, dtype=torch.float64)
        code = sum(f(th * j)[:, None, None] * e[i] for i, (f, th) in enumerate(
            [(torch.cos, THETA), (torch.sin, THETA), (torch.cos, THETA2), (torch.sin, THETA2)]))      # [S][Hkv][hd]
        if levels is None:
            q = (c.u + code).repeat_interleave(G, 1) + NOISE * rnd(S, Hq, hd)
            K = ORDINARY * c.u / rt + NOISE * rnd(S, Hkv, hd)
            V = rnd(S, Hkv, hd)
            K[p0:] = 0.5 * A_CODE * code[p0:] / rt + NOISE * rnd(T, Hkv, hd)
            V[p0:] = V_MAG * sign(T, Hkv, hd)
            bset = _boundary(p0, S)
            for b in bset:
                K[b] = SPIKE * c.u / rt + NOISE * rnd(Hkv, hd)
                V[b] = V_MAG * sign(Hkv, hd)
        else:
            q = c.u.repeat_interleave(G, 0) + NOISE * rnd(S, Hq, hd)
            lev = torch.tensor([levels[min(int(x) // 32, len(levels) - 1)] for x in j], dtype=torch.float64) / LOG2E
            K = lev[:, None, None] * c.u / rt + NOISE * rnd(S, Hkv, hd)
            V = V_MAG * sign(S, Hkv, hd)
            bset = []
        c.bset.append(bset)
        seqs.append((q, K, V))
    c.vis = torch.arange(MAX_PAGES * 64)[None, :] <= c.pos[:, None].long()
    if rope:
        assert len(segs) == 1
        (s, p0, T), (q, K, V) = segs[0], seqs[0]
        S, n = p0 + T, (Hq + 2 * Hkv) * hd
        c.qkv = torch.full((S, n + 8), 1000.0, dtype=torch.float32)   # ldqkv > the row: poisoned padding
        for p in range(S):
            c.qkv[p, :n] = torch.cat([_rot(q[p], c.cs[p], inverse=True).reshape(-1),
                                      _rot(K[p], c.cs[p], inverse=True).reshape(-1), V[p].reshape(-1)]).float()
        c.pos_all = torch.arange(S, dtype=torch.int32)
        c.slot_all = torch.full((S,), s, dtype=torch.int32)
        c.p0 = p0
        q1, kc1, vc1 = oracle_rope(c, c.qkv[:p0], c.pos_all[:p0], c.slot_all[:p0], c.kc0, c.vc0)
        c.q, c.kc, c.vc = oracle_rope(c, c.qkv[p0:], c.pos_all[p0:], c.slot_all[p0:], kc1, vc1)
        c.q_first, c.kc_first, c.vc_first = q1, kc1, vc1
    else:
        c.q = torch.zeros(c.M, Hq, Dp, dtype=torch.float16)
        Kp, Vp = _decode(c.kc0), _decode(c.vc0)
        for (s, p0, T), (row0, _), (q, K, V) in zip(segs, c.rows, seqs):
            c.q[row0:row0 + T, :, :hd] = (q[p0:] * c.q_scale).to(torch.float16)
            for i in range(c.need[s]):
                lo, hi = 64 * i, min(64 * i + 64, p0 + T)
                page = int(c.bt[s, i])
                Kp[page, :, :hi - lo, :hd] = K[lo:hi].transpose(0, 1)
                Kp[page, :, :hi - lo, hd:] = 0.0
                Vp[page, :, :hd, :hi - lo] = V[lo:hi].permute(1, 2, 0)
                Vp[page, :, hd:, :hi - lo] = 0.0
        c.kc, c.vc = _store(_round_cache(Kp, fp8), fp8), _store(_round_cache(Vp, fp8), fp8)
    return c


# ---------------------------------------------------------------- the oracle
def oracle_rope(c, qkv, pos, slot, kc, vc):
    """rope_kv on f32 rows qkv: (q_out f16 [M][Hq][Dp], K cache, V cache) -- new tensors, the caches as
    stored (V in the V^T layout)."""
    hd, Hq, Hkv = c.hd, c.Hq, c.Hkv
    kc, vc = kc.clone(), vc.clone()
    q_out = torch.zeros(len(pos), Hq, c.Dp, dtype=torch.float16)
    for m in range(len(pos)):
        p, x = int(pos[m]), qkv[m].double()
        q = _rot(x[:Hq * hd].view(Hq, hd), c.cs[p])
        k = _rot(x[Hq * hd:(Hq + Hkv) * hd].view(Hkv, hd), c.cs[p])
        v = x[(Hq + Hkv) * hd:(Hq + 2 * Hkv) * hd].view(Hkv, hd)
        q_out[m, :, :hd] = (q * c.q_scale).to(torch.float16)
        page, idx = int(c.bt[int(slot[m]), p // 64]), p % 64
        kc[page, :, idx, :] = 0
        vc[page, :, :, idx] = 0
        kc[page, :, idx, :hd] = _store(_round_cache(k, c.fp8), c.fp8)
        vc[page, :, :hd, idx] = _store(_round_cache(v, c.fp8), c.fp8)
    return q_out, kc, vc


def oracle_attn(c, q=None, kc=None, vc=None, *, vis=None, bt=None, slot=None):
    """out [M][Hq][hd] float64.  vis [M][max_pages * 64]: the keys a row reads (default: j <= pos);
    vis, bt and slot are replaced only by the mutants of the input self-check."""
    hd, Hq, Hkv, G = c.hd, c.Hq, c.Hkv, c.G
    q = c.q if q is None else q
    Kl, Vl = _decode(c.kc if kc is None else kc), _decode(c.vc if vc is None else vc)
    vis = c.vis if vis is None else vis
    bt = c.bt if bt is None else bt
    slot = c.slot if slot is None else slot
    qs = (q[:, :, :hd].float() * torch.tensor(LOG2E, dtype=torch.float32)).to(torch.float16).double()
    out = torch.zeros(c.M, Hq, hd, dtype=torch.float64)
    for row0, T in c.rows:
        pages = bt[int(slot[row0])].long()
        K = Kl[pages][..., :hd].permute(0, 2, 1, 3).reshape(-1, Hkv, hd)       # [max_pages * 64][Hkv][hd]
        V = Vl[pages][:, :, :hd, :].permute(0, 3, 1, 2).reshape(-1, Hkv, hd)
        for r0 in range(row0, row0 + T, 64):
            r1 = min(r0 + 64, row0 + T)
            v = vis[r0:r1]
            cols = v.any(0).nonzero()
            if cols.numel() == 0:
                continue
            L = int(cols.max()) + 1
            s2 = torch.einsum("rkgd,jkd->rkgj", qs[r0:r1].view(-1, Hkv, G, hd), K[:L])   # exp2-domain scores
            s2 = s2.masked_fill(~v[:, None, None, :L], float("-inf"))
            mx = s2.amax(-1, keepdim=True)
            p = torch.exp2(s2 - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx))
            l = p.sum(-1, keepdim=True)
            o = torch.einsum("rkgj,jkd->rkgd", p, V[:L]) / torch.where(l > 0, l, torch.ones_like(l))
            out[r0:r1] = o.reshape(-1, Hq, hd)
    return out


def _ratio(got, ref):
    return float(((got - ref).abs() / (ATOL + RTOL * ref.abs())).max())


def _head_ratio(a, ref):
    """[M][Hq]: per head, the largest |a - ref| in units of the output tolerance."""
    return ((a - ref).abs() / (ATOL + RTOL * ref.abs())).amax(dim=-1)


@functools.lru_cache(maxsize=None)
def attn_case(shape, fp8, segs_name):
    segs = BIG_SEGS if segs_name == "big" else SEGS[segs_name]
    c = build_case(shape, fp8, segs, seed=2000 + sum(shape) + 7 * fp8 + 31 * len(segs_name))
    c.ref = oracle_attn(c)
    return c


@functools.lru_cache(maxsize=None)
def chain_case(shape, fp8):
    c = build_case(shape, fp8, CHAIN_SEGS, seed=2500 + sum(shape) + 7 * fp8, rope=True)
    c.ref = oracle_attn(c)
    return c


# ---------------------------------------------------------------- input self-check (CPU)
def _cells(c, vis, bt, slot):
    """[M][n_pages * 64] bool: the physical cache cells (page, key) a row reads."""
    cell = bt[slot.long()].long().repeat_interleave(64, 1) * 64 + torch.arange(MAX_PAGES * 64) % 64
    return torch.zeros(c.M, c.n_pages * 64, dtype=torch.int32).scatter_add_(1, cell, vis.int()) > 0


def mutants(c):
    """(name, vis, bt, slot, rows): the oracle's inputs with one thing wrong.  rows: a mask of the
    rows the mutation is aimed at, or None for all."""
    M, rows_all = c.M, torch.arange(c.M)
    pos = c.pos.long()
    vis = c.vis.clone()
    vis[rows_all, pos + 1] = True
    yield "key p + 1 visible to row p", vis, c.bt, c.slot, None
    vis = c.vis.clone()
    vis[rows_all, pos] = False
    yield "key p dropped for row p", vis, c.bt, c.slot, None
    vis, vis4 = c.vis.clone(), c.vis.clone()
    for m0, n in c.tiles:
        last = int(pos[m0 + n - 1]) // 64
        vis[m0:m0 + n, :64 * (last + 1)] = True
        vis4[m0:m0 + n, 64 * last:] = False
    yield "partially visible pages treated as full", vis, c.bt, c.slot, None
    yield "the tile's last page dropped", vis4, c.bt, c.slot, None
    vis = c.vis.clone()
    for (s, p0, T), (row0, _) in zip(c.segs, c.rows):
        m0, n = [t for t in c.tiles if row0 <= t[0] < row0 + T][-1]
        vis[m0:m0 + n, p0 + T] = True
    yield "the stale slot past the tile's last row read", vis, c.bt, c.slot, None
    bt = c.bt.clone()
    for s, p0, T in c.segs:   # the page of the segment's first row with the first unused entry
        i, k = p0 // 64, c.need[s]
        bt[s, [i, k]] = bt[s, [k, i]]
    yield "two block-table entries swapped", c.vis, bt, c.slot, None
    slot = c.slot.clone()
    for (row0, T), nb in zip(c.rows, c.neighbour):
        slot[row0:row0 + T] = nb
    yield "the neighbouring segment's block table", c.vis, c.bt, slot, None
    for b in sorted(set().union(*c.bset)):
        vis = c.vis.clone()
        rows = torch.zeros(M, dtype=torch.bool)
        for (row0, T), bset in zip(c.rows, c.bset):
            if b in bset:
                rows[row0:row0 + T] = True
        vis[rows, b] = False
        yield f"boundary key {b} dropped", vis, c.bt, c.slot, rows


def check_mutants(c):
    assert torch.isfinite(_decode(c.kc)).all() and torch.isfinite(_decode(c.vc)).all()
    base = _cells(c, c.vis, c.bt, c.slot)
    worst = float("inf")
    for name, vis, bt, slot, rows in mutants(c):
        affected = (_cells(c, vis, bt, slot) != base).any(1)
        if rows is not None:
            assert not (affected & ~rows).any()
        assert affected.any(), (name, "changes no row's key set")
        r = _head_ratio(oracle_attn(c, vis=vis, bt=bt, slot=slot), c.ref)[affected]
        assert (r >= 10).all(), (name, float(r.min()), "rows", affected.nonzero().flatten().tolist()[:8])
        worst = min(worst, float(r.min()))
    return worst


PROPERTY_CASES = ([(s, "packed") for s in SHAPES] + [(s, n) for s in SEG_SHAPES for n in SEGS if n != "packed"]
                  + [(s, n) for s in FALLBACK_SHAPES if s not in SEG_SHAPES for n in ("mid",)] + [(BIG_SHAPE, "big")])


@kv_param
@pytest.mark.parametrize("shape,segs_name", PROPERTY_CASES, ids=[f"{sid(s)}-{n}" for s, n in PROPERTY_CASES])
def test_inputs_expose_one_wrong_key(shape, segs_name, fp8):
    """On the oracle alone, for every case the GPU tests use: each mutation moves EVERY query head of
    EVERY row whose set of cache cells it changes by at least 10x the output tolerance on some element,
    and changes the key set of at least one row -- so a GPU result within tolerance has read exactly
    the keys [0, pos] of the right slot through the right pages."""
    c = attn_case(shape, fp8, segs_name)
    worst = check_mutants(c)
    print(f"least margin {sid(shape)} {segs_name} {'fp8' if fp8 else 'f16'}: {worst:.1f}x the tolerance")


@kv_param
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=sid)
def test_inputs_expose_one_wrong_key_after_rope(shape, fp8):
    """The same for the second chunk of the rope_kv -> attn_prefill chain (the cache image is the
    rope_kv oracle's, written into poison)."""
    c = chain_case(shape, fp8)
    worst = check_mutants(c)
    print(f"least margin chain {sid(shape)} {'fp8' if fp8 else 'f16'}: {worst:.1f}x the tolerance")


# ---------------------------------------------------------------- GPU harness
def _v_dev(vc, blocked):
    from mipipe.ops.kernels import v_pages_to_blocked
    return (v_pages_to_blocked(vc) if blocked else vc).cuda()


def _v_host(vc_dev, blocked):
    from mipipe.ops.kernels import v_pages_from_blocked
    v = vc_dev.cpu()
    return v_pages_from_blocked(v) if blocked else v


def run_prefill(c, blocked, n_split=1, split_pages=1, q=None, kc=None, vc=None):
    """attn_prefill on fresh device copies; the launch must leave both caches as they were."""
    from mipipe.ops.kernels import attn_prefill, v_layout
    kc, vc = c.kc if kc is None else kc, c.vc if vc is None else vc
    kd, vd = kc.cuda(), _v_dev(vc, blocked)
    with v_layout(blocked):
        out = attn_prefill((c.q if q is None else q).cuda(), c.pos.cuda(), c.slot.cuda(), c.bt.cuda(), kd, vd, c.Hkv,
                           c.hd, segs=c.rows, n_split=n_split, split_pages=split_pages, kv_fp8=c.fp8)
        torch.cuda.synchronize()
    assert _same_bytes(kd.cpu(), kc) and _same_bytes(_v_host(vd, blocked), vc), "attention wrote into a cache"
    return out.cpu().double().view(c.M, c.Hq, c.hd)


def _assert_out(got, ref, what):
    r = _ratio(got, ref)
    print(f"error ratio {what}: {r:.3f}")
    assert torch.isfinite(got).all(), what
    bad = (got - ref).abs() > ATOL + RTOL * ref.abs()
    assert not bad.any(), (what, f"worst ratio {r:.2f}", "first (row, head, d):", bad.nonzero()[0].tolist(),
                           f"{int(bad.sum())} elements")


def _kv(fp8):
    return "fp8" if fp8 else "f16"


# ---------------------------------------------------------------- 4a. shapes
@gpu
@layout_param
@kv_param
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_prefill_shapes(cuda, native, shape, fp8, blocked):
    """Dp 64 / 128, padded head dims on both, G 1 .. 32 (tiles of 128, 42, 32, 25, 18, 16, 10, 8 and 4
    tokens; G 3, 5, 7 and 12 leave MFMA rows of the tile unused) on the packed chunk: four segments
    in non-monotonic slot order, block tables a random permutation with spare pages."""
    c = attn_case(shape, fp8, "packed")
    _assert_out(run_prefill(c, blocked), c.ref, f"prefill-1 {_kv(fp8)} shapes {sid(shape)}")


# ---------------------------------------------------------------- 4b. segment sets
@gpu
@kv_param
@pytest.mark.parametrize("segs_name", [n for n in SEGS if n != "packed"])
@pytest.mark.parametrize("shape", SEG_SHAPES, ids=sid)
def test_prefill_segments(cuda, native, shape, segs_name, fp8):
    """One row; a tile into the second page; a tile straddling a page edge; a mid-sequence start."""
    c = attn_case(shape, fp8, segs_name)
    _assert_out(run_prefill(c, True), c.ref, f"prefill-1 {_kv(fp8)} segs {segs_name} {sid(shape)}")


# ---------------------------------------------------------------- 4c. splits and the LSE merge
# (segments, n_split, split_pages, both): both = an empty split and a fully masked first row in a
# non-empty split must occur for every shape
SPLIT_CASES = [("one", 2, 1, False), ("t65", 2, 1, False), ("straddle", 2, 1, False), ("straddle", 3, 1, True),
               ("mid", 2, 3, False), ("mid", 3, 2, False), ("packed", 2, 2, False), ("packed", 3, 1, False)]


def split_situations(c, n_split, split_pages):
    """(a split wholly past a tile's last page, a split that holds pages of the tile but no key of
    the tile's first row), from the kernel's own split arithmetic."""
    empty = masked = False
    for m0, n in c.tiles:
        pmin, n_kt_all = int(c.pos[m0]), int(c.pos[m0 + n - 1]) // 64 + 1
        assert n_split * split_pages >= n_kt_all, "the splits do not cover the tile"
        for z in range(n_split):
            kt0 = min(z * split_pages, n_kt_all)
            kt1 = min(kt0 + split_pages, n_kt_all)
            empty |= kt1 == kt0
            masked |= kt1 > kt0 and kt0 * 64 > pmin
    return empty, masked


@pytest.mark.parametrize("shape", SEG_SHAPES, ids=sid)
def test_split_cases_reach_empty_and_masked_splits(shape):
    got = {(n, ns, sp): split_situations(attn_case(shape, False, n), ns, sp) for n, ns, sp, _ in SPLIT_CASES}
    assert any(e for e, _ in got.values()) and any(m for _, m in got.values()), got
    for n, ns, sp, both in SPLIT_CASES:
        assert not both or got[(n, ns, sp)] == (True, True), (n, ns, sp, got[(n, ns, sp)])


@gpu
@kv_param
@pytest.mark.parametrize("segs_name,n_split,split_pages,both", SPLIT_CASES,
                         ids=[f"{n}-s{ns}x{sp}" for n, ns, sp, _ in SPLIT_CASES])
@pytest.mark.parametrize("shape", SEG_SHAPES, ids=sid)
def test_prefill_splits(cuda, native, shape, segs_name, n_split, split_pages, both, fp8):
    """KV splits over workgroups + attn_combine: splits past a tile's last page (n_kt == 0) and rows
    that reach the merge with m = -inf, l = 0 from a split that was not empty for their tile."""
    c = attn_case(shape, fp8, segs_name)
    empty, masked = split_situations(c, n_split, split_pages)
    assert not both or (empty and masked)
    out = run_prefill(c, True, n_split, split_pages)
    _assert_out(out, c.ref, f"prefill-split {_kv(fp8)} {segs_name} s{n_split}x{split_pages} {sid(shape)} "
                            f"empty={int(empty)} masked={int(masked)}")


# ---------------------------------------------------------------- 4d. more than 256 tiles
@gpu
@kv_param
@pytest.mark.parametrize("n_split,split_pages", [(1, 5), (2, 3)], ids=["s1", "s2"])
def test_prefill_more_than_256_tiles(cuda, native, n_split, split_pages, fp8):
    """G = 128: one token per tile, 300 tiles, so the tile list is flushed once (two launches)."""
    c = attn_case(BIG_SHAPE, fp8, "big")
    assert len(c.tiles) == 300 and all(n == 1 for _, n in c.tiles)
    kind = "prefill-1" if n_split == 1 else "prefill-split"
    _assert_out(run_prefill(c, True, n_split, split_pages), c.ref, f"{kind} {_kv(fp8)} 300 tiles")


# ---------------------------------------------------------------- 4e. lazy rescale
# exp2-domain score of every key of 32-key chunk c, for every row.  A wave walks the chunks in order
# and moves its running maximum only when a chunk's largest score beats it by more than 8.
RESCALE = {
    "rise7": [7.0 * i for i in range(10)],        # every second chunk rescales; p up to 2^7 in between
    "rise8": [8.0 * i for i in range(10)],        # at the threshold: the 0.3 noise splits rows and heads
    "rise9": [9.0 * i for i in range(10)],        # every chunk rescales
    "high_first": [10.0] + [3.0] * 9,             # never after the first chunk: the maximum stays
    "fall_rise": [0.0, 9.0, 1.0, 1.0, 18.0, 10.0, 10.0, 27.0, 20.0, 36.0],
}
RESCALE_SEGS = [(0, 250, 40)]   # keys over 5 pages; rows on both sides of the chunk edges 256 and 288


@functools.lru_cache(maxsize=None)
def rescale_case(name, fp8):
    c = build_case((128, 32, 8), fp8, RESCALE_SEGS, seed=2700 + len(name) + 7 * fp8, levels=RESCALE[name],
                   stale=(max(RESCALE[name]) + 14.0) / LOG2E)
    c.ref = oracle_attn(c)
    return c


def test_rescale_rows_of_one_wave_disagree():
    """The inputs' side of the rescale cases: in one wave (4 consecutive tokens at G = 4) one row sees
    a chunk that lifts its maximum by more than 8 and another row sees none of that chunk."""
    c = rescale_case("rise9", False)
    (m0, n), pos = c.tiles[0], c.pos.tolist()
    assert any(pos[m0 + w] // 32 != pos[m0 + w + 3] // 32 for w in range(0, n - 3, 4))
    assert max(pos) // 64 + 1 >= 4


@gpu
@kv_param
@pytest.mark.parametrize("n_split,split_pages", [(1, 5), (2, 3)], ids=["s1", "s2"])
@pytest.mark.parametrize("name", list(RESCALE))
def test_prefill_lazy_rescale(cuda, native, name, n_split, split_pages, fp8):
    c = rescale_case(name, fp8)
    _assert_out(run_prefill(c, True, n_split, split_pages), c.ref, f"rescale {_kv(fp8)} {name} s{n_split}")


# ---------------------------------------------------------------- 4f. rope_kv
ROPE_RUNS = [(2, 0, 9), (0, 60, 7), (3, 120, 21), (2, 300, 3)]   # (slot, first position, rows): 40 rows, 3 slots


@functools.lru_cache(maxsize=None)
def rope_case(shape, fp8):
    """40 rows of 3 slots at positions 0..8, 60..66, 120..140 and 300..302: both sides of the 8-key
    block edges and the page edges; slot 3 ends at key 12 of its last page, in the middle of a block.
    The caches are the stale pages of build_case; q / k / v are random, with a few |values| > 448 in k
    and v (the e4m3 clamp)."""
    hd, Hq, Hkv = shape
    c = build_case(shape, fp8, [(2, 0, 303), (0, 0, 67), (3, 0, 141)], seed=2900 + sum(shape) + 7 * fp8)
    g = torch.Generator().manual_seed(2950 + sum(shape))
    c.rpos = torch.cat([torch.arange(p, p + n, dtype=torch.int32) for _, p, n in ROPE_RUNS])
    c.rslot = torch.cat([torch.full((n,), s, dtype=torch.int32) for s, _, n in ROPE_RUNS])
    n = (Hq + 2 * Hkv) * hd
    c.rqkv = torch.full((len(c.rpos), n + 12), -777.0, dtype=torch.float32)
    x = 2.0 * torch.randn(len(c.rpos), n, generator=g)
    big = torch.rand(len(c.rpos), n, generator=g) < 0.01
    big[:, :Hq * hd] = False
    c.rqkv[:, :n] = torch.where(big, 600.0 * torch.sign(x), x)
    c.rref = oracle_rope(c, c.rqkv, c.rpos, c.rslot, c.kc0, c.vc0)
    return c


def _zero_bits(t):
    return bool(((t if t.dtype == torch.uint8 else t.contiguous().view(torch.int16)) == 0).all())


def _assert_rope(c, q, kc_after, vc_after, ref, kc_before, vc_before, pos, slot):
    """q_out within the rope_kv tolerance with exactly zero padded dims; the cells at (page, kv head,
    pos % 64) hold the oracle's codes (one code off on at most 1 % of the elements: the kernel rotates
    in f32), V -- a plain conversion -- exactly; their padded dims are zero; every other byte of both
    caches is what it was."""
    hd = c.hd
    q_ref, kc_ref, vc_ref = ref
    assert _zero_bits(q[:, :, hd:]), "padded dims of q_out not zero"
    torch.testing.assert_close(q[:, :, :hd].double(), q_ref[:, :, :hd].double(), rtol=Q_RTOL, atol=Q_ATOL)
    ek, ev = kc_before.clone(), vc_before.clone()
    off, total = 0, 0
    for m in range(len(pos)):
        p = int(pos[m])
        page, idx = int(c.bt[int(slot[m]), p // 64]), p % 64
        gk, gv = kc_after[page, :, idx, :], vc_after[page, :, :, idx]
        assert _zero_bits(gk[:, hd:]) and _zero_bits(gv[:, hd:]), ("padded dims not zero", m, p)
        dk = (_codes(gk[:, :hd]) - _codes(kc_ref[page, :, idx, :hd])).abs()
        dv = (_codes(gv[:, :hd]) - _codes(vc_ref[page, :, :hd, idx])).abs()
        assert int(dk.max()) <= 1, ("K off by more than one code", m, p, int(dk.max()))
        assert int(dv.max()) == 0, ("V is not the rounded input", m, p, int(dv.max()))
        off += int(dk.sum())
        total += dk.numel()
        ek[page, :, idx, :], ev[page, :, :, idx] = gk, gv
    print(f"rope_kv {_kv(c.fp8)}: {off} of {total} K elements one code off")
    assert off <= 0.01 * total, (off, total)
    assert _same_bytes(kc_after, ek), "stray write into the K cache"
    assert _same_bytes(vc_after, ev), "stray write into the V cache"


def run_rope(c, blocked, qkv, pos, slot, kd, vd):
    from mipipe.ops.kernels import rope_kv, v_layout
    q_out = torch.full((len(pos), c.Hq, c.Dp), 77.0, dtype=torch.float16, device="cuda")
    with v_layout(blocked):
        q = rope_kv(qkv.cuda(), pos.cuda(), slot.cuda(), c.bt.cuda(), c.cs.cuda(), c.Hq, c.Hkv, c.hd, c.Dp, c.q_scale,
                    kd, vd, kv_fp8=c.fp8, q_out=q_out)
        torch.cuda.synchronize()
    return q


@gpu
@layout_param
@kv_param
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=sid)
def test_rope_kv_writes_its_cells_only(cuda, native, shape, fp8, blocked):
    c = rope_case(shape, fp8)
    kd, vd = c.kc0.cuda(), _v_dev(c.vc0, blocked)
    q = run_rope(c, blocked, c.rqkv, c.rpos, c.rslot, kd, vd)
    _assert_rope(c, q.cpu(), kd.cpu(), _v_host(vd, blocked), c.rref, c.kc0, c.vc0, c.rpos, c.rslot)


# ---------------------------------------------------------------- 4g. rope_kv then attn_prefill
@gpu
@layout_param
@kv_param
@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=sid)
def test_rope_kv_then_prefill(cuda, native, shape, fp8, blocked):
    """Two consecutive chunks of one sequence as the engine prefills them, both kernels on poisoned
    caches: rows [0, 100), then rows [100, 160) whose attention reads what both appends left."""
    from mipipe.ops.kernels import attn_prefill, v_layout
    c = chain_case(shape, fp8)
    p0 = c.p0
    kd, vd = c.kc0.cuda(), _v_dev(c.vc0, blocked)
    q1 = run_rope(c, blocked, c.qkv[:p0], c.pos_all[:p0], c.slot_all[:p0], kd, vd)
    _assert_rope(c, q1.cpu(), kd.cpu(), _v_host(vd, blocked), (c.q_first, c.kc_first, c.vc_first), c.kc0, c.vc0,
                 c.pos_all[:p0], c.slot_all[:p0])
    k1, v1 = kd.cpu(), _v_host(vd, blocked)
    q2 = run_rope(c, blocked, c.qkv[p0:], c.pos_all[p0:], c.slot_all[p0:], kd, vd)
    _assert_rope(c, q2.cpu(), kd.cpu(), _v_host(vd, blocked), (c.q, c.kc, c.vc), k1, v1, c.pos_all[p0:],
                 c.slot_all[p0:])
    with v_layout(blocked):
        out = attn_prefill(q2, c.pos.cuda(), c.slot.cuda(), c.bt.cuda(), kd, vd, c.Hkv, c.hd, segs=c.rows,
                           kv_fp8=fp8)
        torch.cuda.synchronize()
    _assert_out(out.cpu().double().view(c.M, c.Hq, c.hd), c.ref, f"chain {_kv(fp8)} {sid(shape)}")


# ---------------------------------------------------------------- 4h. the fallback attention kernel
@gpu
@layout_param
@pytest.mark.parametrize("mode", ["prefill", "decode-s1", "decode-s3"])
@pytest.mark.parametrize("segs_name", ["mid", "packed"])
@pytest.mark.parametrize("shape", FALLBACK_SHAPES, ids=sid)
def test_fallback_attention(cuda, native, shape, segs_name, mode, blocked):
    """attn_kernel (f16 pages): tq = max(1, 16 // G) tokens per row group and one launch per segment,
    as HipStage::attention runs prefill chunks; and tq = 1 over all rows, one split and three of 128
    keys + attn_combine, as it runs decode rows."""
    from mipipe.ops.kernels import attention, v_layout
    c = attn_case(shape, False, segs_name)
    kd, vd = c.kc.cuda(), _v_dev(c.vc, blocked)
    q, kvlen, slot, bt = c.q.cuda(), (c.pos + 1).cuda(), c.slot.cuda(), c.bt.cuda()
    with v_layout(blocked):
        if mode == "prefill":
            tq = max(1, 16 // c.G)
            out = torch.cat([attention(q[r0:r0 + T].contiguous(), kvlen[r0:r0 + T].contiguous(),
                                       slot[r0:r0 + T].contiguous(), bt, kd, vd, c.Hkv, c.hd, tq=tq,
                                       split_len=MAX_PAGES * 64, n_split=1) for r0, T in c.rows])
        else:
            n_split = int(mode[-1])
            assert n_split * 128 > int(c.pos.max()) or n_split == 1
            out = attention(q, kvlen, slot, bt, kd, vd, c.Hkv, c.hd, tq=1,
                            split_len=128 if n_split > 1 else MAX_PAGES * 64, n_split=n_split)
        torch.cuda.synchronize()
    assert _same_bytes(kd.cpu(), c.kc) and _same_bytes(_v_host(vd, blocked), c.vc), "attention wrote into a cache"
    got = out.cpu().double().view(c.M, c.Hq, c.hd)
    _assert_out(got, c.ref, f"fallback f16 {mode} {segs_name} {sid(shape)}")
