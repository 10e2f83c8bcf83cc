"""Context shift on the MI355X: the kv_shift kernel against a float64 oracle of its definition, and the
engine's shifted KV against a fresh engine / the CPU backend.

Definition (kernels_api.h, KvShiftParams).  A slot's cache holds positions [0, old_len).  After the
page edit of its block-table row, the entry of position p >= n_keep + n_discard is the entry of position
p - n_discard: V unchanged, K rotated by minus n_discard positions -- (c, s) = rope_cs[n_discard][j],
(x0, x1) -> (x0 c + x1 s, x1 c - x0 s) in f32 from the stored code, rounded to f16 / e4m3, dims hd..Dp
zero.  n_discard is a multiple of 64, so the tail pages stay where they are and are rotated in place;
with n_keep % 64 != 0 the page holding n_keep takes rows [n_keep % 64, 64) of the old page
n_keep / 64 + n_discard / 64 (K rotated, V copied, in either V layout).

Op level (1.-3.).  4 slots x 8 pages over a pool of 40, page ids scattered and interleaved over the
slots, unmapped entries TRASH (id 40); both caches are random finite codes everywhere (stale pages,
other slots, TRASH and padded dims included), so every byte the kernel must not write is live data to
the comparison.  The oracle is plain torch float64 on the CPU with the same f32 rope_cs_table values.
  1. (CPU) the records exercise what they are meant to: merge rows, a one-row tail, a tail that ends
     on a page boundary.
  2. (CPU) an f32 torch emulation of the kernel's arithmetic stays inside the cap of 3. against the
     oracle, so the cap is about f32-then-round, not about these inputs.  With plain normal values it
     does not: where a rotation cancels (|x0 c + x1 s| << |x|) the f32 error, about 3 * 2^-24 |x|, spans
     several f16 codes of the small result (2 codes off on ~1e-5 of the elements at hd 128 and 96).  So
     in the rows that move, a pair whose rotated component falls below 2^-9 max(|x0|, |x1|) is drawn
     again (0.4 % of the pairs): there the f32 error is at most 3 * 2^-15 of the result, a fifth of an
     f16 code, and a result can only be the oracle's code or its neighbour.  Every other cell keeps
     its plain normal value.
  3. (GPU) every K element of a moved row is the oracle's code or an adjacent one, adjacent on at most
     1 % of the moved elements (the cap test_attn_prefill_oracle_gpu applies to rope_kv's K cells: f32
     rotation, then rounding); padded dims zero; V rows of the merge equal the source bytes; every
     other byte of both caches -- other slots, rows < n_keep, rows past the new length, the freed pages,
     TRASH -- is what it was.
     Measured, K elements one code off of the moved K elements, summed over the five record sets
     (f32 emulation without fma | MI355X; fp8: 0 everywhere in both):
       hd 128, Hkv 8: 49 | 25 of 680960     hd 64, Hkv 4: 14 | 8 of 170240
       hd 48, Hkv 6:  16 | 5 of 191520      hd 96, Hkv 2: 16 | 5 of 127680      (the cap: 1 %)

Engine level (4.-6.), tiny models.
  4. n_layer = 1: the logits after context_shift match a GPU engine started on the spliced token list
     (nmse <= 5e-4 at f16 KV, 2e-2 at fp8 KV, the bounds of test_engine_gpu.py).
     Measured: f16 1.3e-7 (n_keep 5), 1.6e-7 (64); fp8 1.7e-4, 1.8e-4.
  5. 4 layers, tiny-gqa and tiny-qwen3 (NEOX by permutation, qk_norm, hd 128): GPU engine against the CPU
     backend after the same explicit shift, same bounds; no graph is re-captured.
     Measured nmse before | after the shift: tiny-gqa f16 3.8e-7 | 2.4e-7, fp8 2.0e-4 | 2.6e-4;
     tiny-qwen3 f16 7.3e-7 | 6.4e-7, fp8 8.1e-4 | 1.5e-3.
  6. "context_shift": true over 2 stages x 2 micro-batches x 2 sequences with graphs: 300 tokens at
     max_ctx 256 complete, shifts are counted, every page returns to the pool.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import make_model
from test_attn_decode_gpu import _codes, _decode, _rot, _round_cache, _same_bytes, _store
from test_kv_shift_cpu import _nmse, splice_nmse

gpu = pytest.mark.gpu

N_SLOTS, MAX_PAGES, N_PAGES = 4, 8, 40
TRASH = N_PAGES
SHAPES = [(128, 32, 8), (64, 32, 4), (48, 6, 6), (96, 8, 2)]
# (slot, n_keep, n_discard, old_len)
RECORDS = {
    "one-row": [(0, 0, 64, 65)],            # smallest tail: one row
    "aligned": [(1, 64, 128, 300)],         # aligned keep, no merge
    "merge": [(2, 5, 64, 200)],             # merge, r0 % 8 != 0
    "merge-edge": [(3, 70, 192, 448)],      # merge in page 1; the tail ends exactly on a page boundary
    "two": [(3, 5, 64, 200), (1, 64, 128, 300)],   # two records in one launch, on different slots
}
OTHER_LEN = 150   # positions of the slots a record set does not name

sid = lambda s: "hd%d-q%d-kv%d" % s
kv_param = pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
layout_param = pytest.mark.parametrize("blocked", [False, True], ids=["vt", "blocked"])
shape_param = pytest.mark.parametrize("shape", SHAPES, ids=sid)
rec_param = pytest.mark.parametrize("name", list(RECORDS))


class Case:
    pass


def shift_row(row, owned, n_keep, n_discard):
    """The page edit of one block-table row (the definition KvPager::shift implements): the new row,
    the pages it owns, the merge source page (-1: none)."""
    nd, r0 = n_discard // 64, n_keep % 64
    first = n_keep // 64 + (1 if r0 else 0)
    merge = row[first + nd - 1] if r0 else -1
    new = row[:first] + row[first + nd:owned] + [TRASH] * (MAX_PAGES - owned + nd)
    return new, owned - nd, merge


@functools.lru_cache(maxsize=None)
def build_case(shape, fp8, name):
    hd, Hq, Hkv = shape
    c = Case()
    c.hd, c.Hkv, c.Dp, c.fp8 = hd, Hkv, 64 if hd <= 64 else 128, fp8
    from mipipe.ops.kernels import rope_cs_table
    c.cs = rope_cs_table(MAX_PAGES * 64, hd, 10000.0)                 # f32 [pos][hd/2][2]
    g = torch.Generator().manual_seed(4100 + sum(shape) + 7 * fp8 + 13 * list(RECORDS).index(name))
    perm = torch.randperm(N_PAGES, generator=g).tolist()
    lens = {s: OTHER_LEN for s in range(N_SLOTS)}
    lens.update({s: L for s, _, _, L in RECORDS[name]})
    old = [[perm[k * N_SLOTS + s] if k * 64 < lens[s] else TRASH for k in range(MAX_PAGES)] for s in range(N_SLOTS)]
    new, c.recs = [list(r) for r in old], []
    for s, nk, nd, L in RECORDS[name]:
        new[s], _, merge = shift_row(old[s], (L + 63) // 64, nk, nd)
        c.recs.append((s, nk, nd, L, merge))
    c.old_bt, c.new_bt = old, torch.tensor(new, dtype=torch.int32)
    # random finite codes everywhere; K [page][Hkv][64][Dp], V as V^T [page][Hkv][Dp][64]
    c.kc0 = _store(_round_cache(3.0 * torch.randn(N_PAGES + 1, Hkv, 64, c.Dp, generator=g, dtype=torch.float64), fp8), fp8)
    c.vc0 = _store(_round_cache(3.0 * torch.randn(N_PAGES + 1, Hkv, c.Dp, 64, generator=g, dtype=torch.float64), fp8), fp8)
    _redraw_cancelling_pairs(c, g)
    return c


CANCEL = 2.0 ** -9


def _redraw_cancelling_pairs(c, g):
    """The value distribution of the rows that move (module docstring, 2.): a pair whose rotated
    x0 c + x1 s or x1 c - x0 s falls below CANCEL max(|x0|, |x1|) is drawn again."""
    for nd, sp, _, i in moves(c):
        for _ in range(16):
            x = _decode(c.kc0[sp, :, i, :c.hd])
            y = _rot(x, c.cs[nd], inverse=True)
            m = torch.maximum(x[:, 0::2].abs(), x[:, 1::2].abs())
            bad = (y[:, 0::2].abs() < CANCEL * m) | (y[:, 1::2].abs() < CANCEL * m)
            if not bool(bad.any()):
                break
            fresh = _round_cache(3.0 * torch.randn(c.Hkv, c.hd, generator=g, dtype=torch.float64), c.fp8)
            c.kc0[sp, :, i, :c.hd] = _store(torch.where(bad.repeat_interleave(2, dim=1), fresh, x), c.fp8)
        else:
            raise AssertionError("no pair without cancellation found")


def moves(c):
    """(record, source page, destination page, row) of every moved position."""
    for s, nk, nd, L, _ in c.recs:
        for p in range(nk + nd, L):
            yield nd, c.old_bt[s][p // 64], int(c.new_bt[s][(p - nd) // 64]), p % 64


def expected(c, f32=False):
    """The caches after the shift by the definition, in float64 (f32: the kernel's arithmetic instead:
    f32 products and sums, then the rounding), and the mask [page][row] of the moved rows."""
    ek, ev = c.kc0.clone(), c.vc0.clone()
    moved = torch.zeros(N_PAGES + 1, 64, dtype=torch.bool)
    for nd, sp, dp, i in moves(c):
        x = _decode(c.kc0[sp, :, i, :c.hd])
        if f32:
            cs = c.cs[nd]
            x0, x1, co, si = x[:, 0::2].float(), x[:, 1::2].float(), cs[:, 0], cs[:, 1]
            y = torch.empty_like(x)
            y[:, 0::2] = (x0 * co + x1 * si).double()
            y[:, 1::2] = (x1 * co - x0 * si).double()
        else:
            y = _rot(x, c.cs[nd], inverse=True)
        ek[dp, :, i, :c.hd] = _store(_round_cache(y, c.fp8), c.fp8)
        ek[dp, :, i, c.hd:] = 0
        ev[dp, :, :, i] = c.vc0[sp, :, :, i]
        assert not moved[dp, i], "a row is written twice"
        moved[dp, i] = True
    return ek, ev, moved


def _zero_bits(t):
    return bool(((t if t.dtype == torch.uint8 else t.contiguous().view(torch.int16)) == 0).all())


def check_k(c, ka, ek, moved, what):
    """ka's moved rows against the oracle's codes: at most one code off, on at most 1 % of the elements;
    padded dims zero; returns (off, total)."""
    rows = lambda t: t.permute(0, 2, 1, 3)[moved]                      # [n][Hkv][Dp]
    got, ref = rows(ka), rows(ek)
    assert _zero_bits(got[:, :, c.hd:]), "padded dims of a moved row are not zero"
    d = (_codes(got[:, :, :c.hd]) - _codes(ref[:, :, :c.hd])).abs()
    off, total = int(d.sum()), d.numel()
    print(f"kv_shift {what} {'fp8' if c.fp8 else 'f16'}: {off} of {total} moved K elements one code off")
    assert int(d.max()) <= 1, ("K off by more than one code", int(d.max()))
    assert off <= 0.01 * total, (off, total)
    return off, total


# ---------------------------------------------------------------- 1. the records
def test_records_cover_their_cases():
    c = build_case(SHAPES[0], False, "one-row")
    assert len(list(moves(c))) == 1 and c.recs[0][4] == -1
    c = build_case(SHAPES[0], False, "aligned")
    assert c.recs[0][4] == -1 and all(sp == dp for _, sp, dp, _ in moves(c))
    c = build_case(SHAPES[0], False, "merge")
    s, nk = c.recs[0][0], c.recs[0][1]
    src = {(sp, i) for _, sp, dp, i in moves(c) if sp != dp}
    assert src == {(c.recs[0][4], i) for i in range(nk % 64, 64)} and (nk % 64) % 8 != 0
    assert all(dp == c.old_bt[s][0] for _, sp, dp, _ in moves(c) if sp != dp)
    c = build_case(SHAPES[0], False, "merge-edge")
    assert (c.recs[0][3] - c.recs[0][2]) % 64 == 0 and c.recs[0][1] // 64 == 1 and c.recs[0][4] >= 0
    c = build_case(SHAPES[0], False, "two")
    assert len({r[0] for r in c.recs}) == 2
    for name in RECORDS:   # scattered ids, TRASH in the rows, the freed pages gone from them
        c = build_case(SHAPES[0], False, name)
        flat = [p for r in c.new_bt.tolist() for p in r]
        live = [p for p in flat if p != TRASH]
        assert TRASH in flat and len(set(live)) == len(live) and sorted(live) != live


# ---------------------------------------------------------------- 2. f32 emulation inside the cap
@kv_param
@shape_param
def test_f32_emulation_within_cap(shape, fp8):
    off = total = 0
    for name in RECORDS:
        c = build_case(shape, fp8, name)
        ek, _, moved = expected(c)
        ek32, _, _ = expected(c, f32=True)
        o, t = check_k(c, ek32, ek, moved, f"emulation {name}")
        off, total = off + o, total + t
    print(f"kv_shift emulation {sid(shape)} {'fp8' if fp8 else 'f16'}: {off} of {total} in all")


# ---------------------------------------------------------------- 3. the kernel
@gpu
@layout_param
@kv_param
@rec_param
@shape_param
def test_kv_shift_matches_oracle(cuda, native, shape, name, fp8, blocked):
    from mipipe.ops.kernels import kv_shift, v_layout, v_pages_from_blocked, v_pages_to_blocked
    c = build_case(shape, fp8, name)
    ek, ev, moved = expected(c)
    kd = c.kc0.cuda()
    vd = (v_pages_to_blocked(c.vc0) if blocked else c.vc0).cuda()
    with v_layout(blocked):
        kv_shift(kd, vd, c.new_bt.cuda(), c.cs.cuda(), c.recs, c.Hkv, c.hd, c.Dp, N_PAGES, kv_fp8=fp8)
        torch.cuda.synchronize()
    ka, va = kd.cpu(), (v_pages_from_blocked(vd.cpu()) if blocked else vd.cpu())
    check_k(c, ka, ek, moved, f"mi355x {sid(shape)} {name}")
    # V: the merge rows hold the source bytes, everything else is untouched
    assert _same_bytes(va, ev), "V: a merge row differs from its source, or a stray write"
    # K: every byte outside the moved rows is what it was
    rest = ek.clone()
    rest.permute(0, 2, 1, 3)[moved] = ka.permute(0, 2, 1, 3)[moved]
    assert _same_bytes(ka, rest), "stray write into the K cache"


@gpu
def test_kv_shift_refuses_bad_records(cuda, native):
    """Host-side checks only: nothing is launched for a record the kernel cannot take."""
    from mipipe.ops.kernels import kv_shift
    c = build_case(SHAPES[0], False, "merge")
    kd, vd, bt, cs = c.kc0.cuda(), c.vc0.cuda(), c.new_bt.cuda(), c.cs.cuda()
    s, nk, nd, L, mg = c.recs[0]
    for rec, msg in [((s, nk, 32, L, mg), "multiple of 64"), ((s, nk, nd, L, -1), "merge_src_page"),
                     ((s, nk, nd, L, TRASH), "merge_src_page"), ((s, 64, nd, L, mg), "merge_src_page"),
                     ((9, nk, nd, L, mg), "slot out of range"), ((s, nk, 256, L, mg), "n_keep \\+ n_discard > old_len"),
                     ((s, nk, nd, 600, mg), "old_len exceeds"), ((s, -1, nd, L, mg), "n_keep < 0")]:
        with pytest.raises(RuntimeError, match=msg):
            kv_shift(kd, vd, bt, cs, [rec], c.Hkv, c.hd, c.Dp, N_PAGES)
    with pytest.raises(RuntimeError, match="listed twice"):
        kv_shift(kd, vd, bt, cs, [c.recs[0], c.recs[0]], c.Hkv, c.hd, c.Dp, N_PAGES)
    torch.cuda.synchronize()
    assert _same_bytes(kd.cpu(), c.kc0) and _same_bytes(vd.cpu(), c.vc0)


# ---------------------------------------------------------------- 4. engine: splice equivalence
@gpu
@pytest.mark.parametrize("n_keep", [5, 64])
@pytest.mark.parametrize("kv_dtype,bound", [("f16", 5e-4), ("fp8", 2e-2)])
def test_gpu_splice_equivalence(cuda, native, model_dir, kv_dtype, bound, n_keep):
    path, _ = make_model(model_dir, "tiny-gqa", "Q8_0", n_layer=1)
    e = splice_nmse(path, n_keep, 64, kv_dtype=kv_dtype, prefill_chunk=64)
    print(f"gpu splice {kv_dtype} n_keep {n_keep}: nmse {e:.3g}")
    assert e <= bound, e


# ---------------------------------------------------------------- 5. engine: GPU against the CPU backend
def _graph_captures(eng):
    return [s["graph_captures"] for s in eng.health()["stages"]]


@gpu
@pytest.mark.parametrize("kv_dtype,bound", [("f16", 5e-4), ("fp8", 2e-2)])
@pytest.mark.parametrize("model", ["tiny-gqa", "tiny-qwen3"])
def test_gpu_shift_matches_cpu_backend(cuda, native, model_dir, model, kv_dtype, bound):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, model, "Q8_0")
    prompt = np.random.default_rng(11).integers(3, cfg.vocab, 150).tolist()
    with Engine(gguf=path, max_ctx=256, kv_dtype=kv_dtype) as eng, \
            Engine(gguf=path, max_ctx=256, backend="cpu", cpu_act="f32") as ref:
        for e in (eng, ref):
            e.start([prompt])
        assert eng.tokens()[0] == ref.tokens()[0]
        before = _nmse(eng.logits()[0], ref.logits()[0])
        caps = _graph_captures(eng)
        for e in (eng, ref):
            e.context_shift([0], [5], [64])
            e.decode(1)
        assert _graph_captures(eng) == caps and caps[0] >= 1
        assert eng.slot_position(0) == ref.slot_position(0) == 150 - 64 + 1
        after = _nmse(eng.logits()[0], ref.logits()[0])
        print(f"gpu vs cpu {model} {kv_dtype}: nmse {before:.3g} before the shift, {after:.3g} after")
        assert after <= bound, after


# ---------------------------------------------------------------- 6. endless generation
@gpu
def test_gpu_endless_generation(cuda, native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    rng = np.random.default_rng(3)
    prompts = [rng.integers(3, cfg.vocab, n).tolist() for n in (100, 30, 60, 7)]
    with Engine(gguf=path, max_ctx=256, n_mb=2, mb_size=2, stages=2, devices=[0, 0], link="local", graphs=True,
                context_shift=True, n_keep=4) as eng:
        free0 = eng.kv_stats()["kv_free_pages"]
        caps = _graph_captures(eng)
        out, stats = eng.generate(prompts, 300)
        assert [len(o) for o in out] == [300] * 4 and min(min(o) for o in out) >= 0
        assert eng.health()["context_shifts"] > 0 and eng.health()["ok"]
        assert [eng.slot_shifts(s) > 0 for s in range(4)] == [True, True, True, True]
        assert _graph_captures(eng) == caps
        for s in range(4):
            eng.release(s)
        assert eng.kv_stats()["kv_free_pages"] == free0
