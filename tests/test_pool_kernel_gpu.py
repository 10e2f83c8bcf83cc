"""The embedding pooling kernels (csrc/kernels/pool.hip) alone against a float64 numpy oracle.

Oracle, from the same f32 inputs in float64: h = x * (mean(x^2) + eps)^-1/2 * w per row; the pooled
vector v of a prompt (mean of its rows, row 0, last row, or every row); with normalisation
v / |v| (0 for the zero vector).

Bound.  u = 2^-24 is the unit roundoff of f32.  The kernel's error is bounded term by term:

  E_ROW = 33 u   one element of h.  Each thread sums at most 8 float4 of squares (5 roundings each:
                 40), the wave tree adds 6 and the 4 wave totals 3, the squares themselves 1: the sum
                 of squares is within 50 u; / d and + eps add 2 u; rsqrt halves that (26 u) and is
                 itself within 2 ulp (4 u); x * sc * w rounds twice (2 u).  26 + 4 + 2 + 1 spare.
  mean           v_c = (1 / L) sum_i h_ic over L rows, added one after the other (within a 32-row
                 block, then the blocks, then the chunks): at most (L - 1) u of sum_i |h_ic| / L, and
                 2 u for 1 / L and the product.  So |dv_c| <= REL * A_c with REL = E_ROW + (L + 1) u
                 and A_c = mean_i |h_ic|; for the single-row poolings REL = E_ROW and A_c = |h_c|.
  E_L2 = 34 u    the factor 1 / sqrt(s), s = sum v_c^2, given v: s within 52 u as above, sqrt halves
                 it (26 u), sqrt and the division are within 1 and 2.5 ulp (7 u), the product 1 u.

Normalised, w = v / |v|, and a perturbation dv of v moves w_c by at most |dv_c| / |v| + |w_c| |dv| / |v|,
so with |dv| <= REL |A|:

    |got_c - w_c| <= REL A_c / |v| + |w_c| (REL |A| / |v| + E_L2)

and without normalisation |got_c - v_c| <= REL A_c.  Both are asserted element by element (a zero
row has A = 0: it must come out as exact zeros, not NaN).  At the largest case here (L = 64, mean)
REL is 98 u = 5.8e-6; a wrong row, slot, scale or block order is an error of order 1."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
E_ROW = 33 * U
E_L2 = 34 * U
EPS = 1e-5
N_SLOTS = 8
POOLINGS = {"none": 0, "mean": 1, "cls": 2, "last": 3}
LAYOUTS = {"two": ([33, 31], [5, 2]), "three": ([1, 64, 33], [7, 0, 3]), "four": ([1, 31, 33, 64], [6, 1, 4, 2])}


def make_rows(d, T, seed):
    """unit-scale rows; where there are enough, row 3 all zero and row 5 scaled by 1e3"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, d, generator=g, dtype=torch.float32)
    if T > 3:
        x[3] = 0
    if T > 5:
        x[5] *= 1e3
    return x


def make_w(d):
    g = torch.Generator().manual_seed(99)
    return (1.0 + 0.1 * torch.randn(d, generator=g, dtype=torch.float32))


def oracle_h(x, w):
    x = x.double().numpy()
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + EPS) * w.double().numpy()


def expect(h, pooling, normalize):
    """(want, tol) for the rows h [L][d] of one prompt"""
    L = h.shape[0]
    if pooling == "mean":
        v, A, rel = h.mean(0), np.abs(h).mean(0), E_ROW + (L + 1) * U
    elif pooling == "none":
        v, A, rel = h, np.abs(h), E_ROW
    else:
        v = h[0] if pooling == "cls" else h[-1]
        A, rel = np.abs(v), E_ROW
    if not normalize:
        return v, rel * A
    nv = np.sqrt((v * v).sum(-1, keepdims=True))
    nA = np.sqrt((A * A).sum(-1, keepdims=True))
    inv = np.where(nv > 0, 1.0 / np.where(nv > 0, nv, 1.0), 0.0)
    wv = v * inv
    return wv, rel * A * inv + np.abs(wv) * (rel * nA * inv + E_L2)


def check(got, want, tol, what):
    got = got.double().cpu().numpy()
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    worst = float((err / np.maximum(tol, 1e-300)).max()) if (tol > 0).any() else 0.0
    print(f"measured {what}: max |err| {err.max():.3e}, max err / bound {worst:.3f}")
    assert (err <= tol).all(), (what, float(err.max()), worst)


class Bufs:
    def __init__(self, d, dev, chunk=160):
        nan = float("nan")
        self.h = torch.full((chunk, d), nan, device=dev)
        self.part = torch.full((chunk // 32 + N_SLOTS + 1, d), nan, device=dev)
        self.acc = torch.full((N_SLOTS, d), nan, device=dev)
        self.emb = torch.full((N_SLOTS, d), nan, device=dev)


def run(x, w, segs, pooling, normalize, b):
    from mipipe.ops import kernels as K
    K.pool_embed(x, w, EPS, segs, POOLINGS[pooling], normalize, N_SLOTS, h=b.h, part=b.part, pool_acc=b.acc, emb=b.emb)
    torch.cuda.synchronize()


@pytest.mark.parametrize("d", [384, 512, 8192])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_whole_prompts_in_one_chunk(cuda, native, d, layout):
    """Segments of 1, 31, 33 and 64 rows (33 crosses a 32-row block) of different slots in one chunk,
    each a whole prompt; every pooling, normalised and not.  The result rows of the slots that are
    not in the chunk, and h beyond the chunk, keep their NaN fill."""
    dev = torch.device("cuda")
    Ts, slots = LAYOUTS[layout]
    T = sum(Ts)
    x = make_rows(d, T, seed=d + T)
    w = make_w(d)
    # the zero row and the scaled row where last / cls look: the last row of the first segment with
    # more than one row is zero, its first row scaled
    r0 = [sum(Ts[:i]) for i in range(len(Ts))]
    big = next(i for i, t in enumerate(Ts) if t > 1)
    x[r0[big] + Ts[big] - 1] = 0
    x[r0[big]] *= 1e3
    h = oracle_h(x, w)
    segs = [(r0[i], Ts[i], slots[i], 0, Ts[i], 1) for i in range(len(Ts))]
    xd, wd = x.to(dev), w.to(dev)
    for pooling in POOLINGS:
        for normalize in (True, False):
            b = Bufs(d, dev)
            run(xd, wd, segs, pooling, normalize, b)
            what = f"d={d} {layout} {pooling} norm={normalize}"
            if pooling == "none":
                want, tol = expect(h, pooling, normalize)
                check(b.h[:T], want, tol, what)
                assert torch.isnan(b.h[T:]).all() and torch.isnan(b.emb).all()
                continue
            for i, sl in enumerate(slots):
                want, tol = expect(h[r0[i]:r0[i] + Ts[i]], pooling, normalize)
                check(b.emb[sl], want, tol, f"{what} T={Ts[i]}")
            rest = [s for s in range(N_SLOTS) if s not in slots]
            assert torch.isnan(b.emb[rest]).all(), what
            if pooling != "mean":
                assert torch.isnan(b.acc).all() and torch.isnan(b.h).all(), what


@pytest.mark.parametrize("d", [384, 512, 8192])
def test_prompt_split_over_three_calls(cuda, native, d):
    """A 37-token prompt as 16 + 16 + 5 rows over three chunks, each shared with a whole prompt of
    another slot.  mean: the first call stores into the NaN-filled accumulator, the second adds, the
    third adds, scales by 1 / 37 and normalises; last comes from the third call, cls from the first;
    none returns each call's rows."""
    dev = torch.device("cuda")
    w = make_w(d)
    xs = make_rows(d, 37, seed=7 * d)          # the split prompt, slot 3
    others = [make_rows(d, t, seed=d + t) for t in (9, 33, 2)]   # whole prompts in slots 0, 5, 6
    hs = oracle_h(xs, w)
    wd = w.to(dev)
    cuts = [(0, 16), (16, 16), (32, 5)]
    for pooling in POOLINGS:
        for normalize in (True, False):
            b = Bufs(d, dev)
            what = f"d={d} split {pooling} norm={normalize}"
            for c, (p0, t) in enumerate(cuts):
                o = others[c]
                oslot = (0, 5, 6)[c]
                # the split prompt's segment second in calls 0 and 2, first in call 1
                mine = (0 if c == 1 else o.shape[0], t, 3, p0, 37, int(p0 + t == 37))
                his = (t if c == 1 else 0, o.shape[0], oslot, 0, o.shape[0], 1)
                segs = [mine, his] if c == 1 else [his, mine]
                x = torch.cat([xs[p0:p0 + t], o] if c == 1 else [o, xs[p0:p0 + t]]).to(dev)
                run(x, wd, segs, pooling, normalize, b)
                if pooling == "none":
                    want, tol = expect(hs[p0:p0 + t], "none", normalize)
                    check(b.h[mine[0]:mine[0] + t], want, tol, f"{what} call {c}")
                else:
                    want, tol = expect(oracle_h(o, w), pooling, normalize)
                    check(b.emb[oslot], want, tol, f"{what} other prompt of call {c}")
                    done = {"mean": c == 2, "last": c == 2, "cls": True}[pooling]
                    assert bool(torch.isnan(b.emb[3]).any()) == (not done), (what, c)
            if pooling != "none":
                want, tol = expect(hs, pooling, normalize)
                check(b.emb[3], want, tol, what)


@pytest.mark.parametrize("d", [384, 8192])
@pytest.mark.parametrize("pooling", ["mean", "last", "cls"])
def test_bitwise_independent_of_the_rest_of_the_chunk(cuda, native, d, pooling):
    """The same 70-row prompt pooled alone, and in a chunk behind another slot's 33-row segment:
    identical bits (blocks are counted from the segment's first row, and nothing is shared)."""
    dev = torch.device("cuda")
    w = make_w(d).to(dev)
    x = make_rows(d, 70, seed=3).to(dev)
    other = make_rows(d, 33, seed=4).to(dev)
    alone, shared = Bufs(d, dev), Bufs(d, dev)
    run(x, w, [(0, 70, 2, 0, 70, 1)], pooling, True, alone)
    run(torch.cat([other, x]), w, [(0, 33, 6, 0, 33, 1), (33, 70, 2, 0, 70, 1)], pooling, True, shared)
    assert not torch.isnan(alone.emb[2]).any()
    assert torch.equal(alone.emb[2], shared.emb[2])
    again = Bufs(d, dev)
    run(x, w, [(0, 70, 2, 0, 70, 1)], pooling, True, again)
    assert torch.equal(alone.emb[2], again.emb[2])


def test_launcher_refuses_what_the_kernels_cannot_take(cuda, native):
    dev = torch.device("cuda")
    b = Bufs(512, dev)
    x, w = make_rows(512, 8, 0).to(dev), make_w(512).to(dev)
    bad = [
        (x[:, :100].contiguous(), w[:100], [(0, 8, 0, 0, 8, 1)], "multiple of 64"),
        (x, w, [(0, 8, N_SLOTS, 0, 8, 1)], "slot out of range"),
        (x, w, [(0, 4, 0, 0, 4, 1), (5, 3, 1, 0, 3, 1)], "tile the chunk"),
        (x, w, [(0, 4, 1, 0, 4, 1), (4, 4, 1, 0, 4, 1)], "two segments of one slot"),
        (x, w, [(0, 8, 0, 4, 8, 1)], "prompt_len"),
    ]
    for xx, ww, segs, msg in bad:
        with pytest.raises(RuntimeError, match=msg):
            run(xx, ww, segs, "mean", True, b)
    with pytest.raises(RuntimeError, match="pooling"):
        from mipipe.ops import kernels as K
        K.pool_embed(x, w, EPS, [(0, 8, 0, 0, 8, 1)], 4, True, N_SLOTS, h=b.h, part=b.part, pool_acc=b.acc, emb=b.emb)
    assert torch.isnan(b.emb).all()
