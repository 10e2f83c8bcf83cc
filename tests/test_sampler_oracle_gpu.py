"""sample_kernel (sample.hip) checked draw by draw against a float64 numpy oracle.

The draw is a pure function of (seed, step, row, logits), so nothing here is statistical.

Oracle.  Cuts are taken on the T = 1 distribution, in llama.cpp's chain order: top-k exactly, by
sort; top-p as the smallest descending prefix of the top-k survivors whose mass is >= top_p of
theirs; min-p relative to the maximum.  Weights are exp((l - max) / T) over the kept set.  The
uniform variate is the documented contract checkpoint resume depends on:
    u = (mix64(seed ^ mix64((step << 20) ^ row)) >> 40) / 2^24      (mix64: the splitmix64 finaliser)

Per draw, with cdf the oracle's normalised CDF in index order: the token t is in the kept set and
    cdf[t - 1] - TOL <= u <= cdf[t] + TOL,   TOL = 1e-4.
TOL is derived, not measured from the kernel: the kernel's f32 summation (ceil(n / 1024) serial adds
per thread plus 10 scan levels) is within ~8e-6 of the exact CDF at n = 128256, the fast exp on
arguments that carry mass adds ~4e-6 relative; an f32 numpy emulation of the kernel's summation order
stayed within 6.3e-6 of the float64 CDF over 256 draws at n = 128256.  Measured on the MI355X: over every
draw of this file, V = 128256 included, no u lay outside its oracle interval (worst distance 0.0,
printed by each case as `worst`); the draw that came nearest to an interval edge (`nearest edge`) was
9.7e-8 away from it at V = 1537 and 1.4e-7 at V = 128256 and still gave the oracle's token.

No case has a tie at a cut boundary: the kernel's thresholds keep ALL tokens tied at a cut, llama.cpp
keeps exactly k, and the oracle here does what llama.cpp does.  The small-vocabulary cases carry
explicit margins (asserted below) so the kept set is unambiguous and drawn-set equality can be
demanded.  At V = 128256 only the interval is asserted: for top_p deep in the tail the kernel's
24-step bisection cannot separate tokens whose probabilities relative to the maximum differ by less
than 2^-24 ~ 6e-8, so kept-set equality is not a property of the kernel there."""
import numpy as np
import pytest
import torch

TOL = 1e-4
MASK64 = (1 << 64) - 1
M_ROWS = 256
SEED = 0x9E3779B97F4A7C15          # a seed that needs all 64 bits


# ---------------------------------------------------------------- oracle (numpy, float64)
def mix64(x):
    x &= MASK64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK64
    x ^= x >> 31
    return x


def uniform(seed, step, row):
    r = mix64(seed ^ mix64(((step << 20) ^ row) & MASK64))
    return (r >> 40) / 16777216.0


def kept_set(logits, top_k=0, top_p=1.0, min_p=0.0):
    """Boolean mask of the tokens that survive the three cuts (taken at T = 1)."""
    l = np.asarray(logits, np.float64)
    n = l.size
    keep = l > -np.inf
    mx = l.max()
    if 0 < top_k < n:
        kth = np.sort(l)[::-1][top_k - 1]
        keep &= l >= kth
    p1 = np.where(keep, np.exp(l - mx), 0.0)
    if 0.0 < top_p < 1.0:
        order = np.argsort(-p1, kind="stable")
        cs = np.cumsum(p1[order])
        m = int(np.searchsorted(cs, top_p * cs[-1], side="left"))      # first prefix with mass >= top_p
        inp = np.zeros(n, bool)
        inp[order[:m + 1]] = True
        keep &= inp
    if min_p > 0.0:
        keep &= np.exp(l - mx) >= min_p
    return keep


def draw_cdf(logits, keep, temp):
    """Normalised CDF, in index order, of the weights exp((l - max) / T) over the kept set."""
    l = np.asarray(logits, np.float64)
    e = np.where(keep, (l - l.max()) / temp, -np.inf)
    w = np.exp(e)
    c = np.cumsum(w)
    return c / c[-1]


def interval_distance(cdf, t, u):
    """How far u lies outside [cdf[t - 1], cdf[t]] (0 inside); arrays of draws."""
    lo = np.where(t > 0, cdf[np.maximum(t - 1, 0)], 0.0)
    return np.maximum(0.0, np.maximum(lo - u, u - cdf[t]))


def edge_margin(cdf, t, u):
    """Distance from u to the nearer edge of [cdf[t - 1], cdf[t]] (negative outside): only a draw
    within the kernel's f32 error of an edge could come out differently from the oracle."""
    lo = np.where(t > 0, cdf[np.maximum(t - 1, 0)], 0.0)
    return np.minimum(u - lo, cdf[t] - u)


def test_oracle_on_hand_computed_cases():
    """CPU only: the oracle helpers on a 4-token distribution worked out by hand."""
    p = np.array([0.1, 0.4, 0.2, 0.3])
    l = np.log(p) + 3.0
    every = kept_set(l)
    assert every.tolist() == [True] * 4
    np.testing.assert_allclose(draw_cdf(l, every, 1.0), [0.1, 0.5, 0.7, 1.0], rtol=1e-12)
    k2 = kept_set(l, top_k=2)
    assert k2.tolist() == [False, True, False, True]
    np.testing.assert_allclose(draw_cdf(l, k2, 1.0), [0, 4 / 7, 4 / 7, 1], rtol=1e-12)
    np.testing.assert_allclose(draw_cdf(l, k2, 0.5), [0, 0.64, 0.64, 1], rtol=1e-12)      # weights .16, .09
    assert kept_set(l, top_k=4).all() and kept_set(l, top_k=9).all()
    assert kept_set(l, top_p=0.39).tolist() == [False, True, False, False]
    assert kept_set(l, top_p=0.65).tolist() == [False, True, False, True]                 # .4 + .3 >= .65
    assert kept_set(l, top_p=0.75).tolist() == [False, True, True, True]
    # top-p is taken on the top-k survivors: .75 of their .9 is .675 <= .7
    assert kept_set(l, top_k=3, top_p=0.75).tolist() == [False, True, False, True]
    mp = kept_set(l, min_p=0.6)                                                          # ratios .25 1 .5 .75
    assert mp.tolist() == [False, True, False, True]
    np.testing.assert_allclose(draw_cdf(l, mp, 2.0)[1], np.sqrt(.4) / (np.sqrt(.4) + np.sqrt(.3)), rtol=1e-12)
    assert kept_set(np.array([0.0, -np.inf, 1.0])).tolist() == [True, False, True]
    # the uniform variate: splitmix64's first output for state 0 is mix64 of the golden-ratio increment
    assert mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert uniform(0, 0, 0) == (mix64(mix64(0)) >> 40) / 2 ** 24 == 0.0                  # mix64(0) = 0
    us = [uniform(SEED, s, r) for s in (0, 5) for r in range(64)]
    assert all(0.0 <= u < 1.0 and u * 2 ** 24 == int(u * 2 ** 24) for u in us) and len(set(us)) == len(us)
    assert uniform(SEED, 1, 0) == uniform(SEED, 0, 1 << 20)                              # the documented packing
    cdf = np.array([0.0, 0.64, 0.64, 1.0])
    d = interval_distance(cdf, np.array([1, 1, 3, 3, 0]), np.array([0.0, 0.7, 0.64, 0.5, 0.25]))
    np.testing.assert_allclose(d, [0, 0.06, 0, 0.14, 0.25], atol=1e-15)


# ---------------------------------------------------------------- GPU side
def _launch(K, cuda, dev_logits, step, **kw):
    st = None if step is None else torch.tensor([step], dtype=torch.int32, device=cuda)
    out = K.sample(dev_logits, step=st, **kw).cpu().numpy().astype(np.int64)
    return out


def _check_case(K, cuda, rows, n, *, temp, top_k=0, top_p=1.0, min_p=0.0, seed=SEED, drawn_equals_kept=False,
                row_logits=None):
    """One case: rows is the CPU f32 tensor [256][ld]; launches step None, 0 and 5 and checks every
    draw against the oracle of its own row (row r follows row_logits[r % len(row_logits)] when given).
    Returns (tokens at step 0, worst interval distance)."""
    M = rows.shape[0]
    dev = rows.to(cuda)[:, :n]
    kw = dict(temp=temp, top_k=top_k, top_p=top_p, min_p=min_p, seed=seed)
    got = {s: _launch(K, cuda, dev, s, **kw) for s in (None, 0, 5)}
    assert np.array_equal(got[None], got[0]), "a null step pointer must mean step 0"
    oracles = {}
    for key, l in (row_logits or {None: rows[0, :n].numpy()}).items():
        keep = kept_set(l, top_k, top_p, min_p)
        oracles[key] = (keep, draw_cdf(l, keep, temp))
    worst, nearest, drawn = 0.0, 1.0, {k: set() for k in oracles}
    for s in (0, 5):
        t = got[s]
        assert ((t >= 0) & (t < n)).all(), "a token outside [0, n)"
        u = np.array([uniform(seed, s, r) for r in range(M)])
        for key, (keep, cdf) in oracles.items():
            sel = np.arange(M) % len(oracles) == (0 if key is None else key)
            ts, us = t[sel], u[sel]
            assert keep[ts].all(), f"step {s}: drew tokens outside the kept set: {sorted(set(ts[~keep[ts]]))}"
            dist = interval_distance(cdf, ts, us)
            worst = max(worst, float(dist.max()))
            nearest = min(nearest, float(edge_margin(cdf, ts, us).min()))
            assert (dist <= TOL).all(), f"step {s}: u outside the token's CDF interval by {dist.max():.3e}"
            drawn[key] |= set(ts.tolist())
    for key, (keep, _) in oracles.items():
        kept = set(np.flatnonzero(keep).tolist())
        if len(kept) > 1:
            assert not np.array_equal(got[0], got[5]), "step 5 must draw differently from step 0"
        else:
            assert np.array_equal(got[0], got[5])
        if drawn_equals_kept:
            assert drawn[key] == kept, f"drawn {sorted(drawn[key])} != kept {sorted(kept)}"
    print(f"sampler n={n} T={temp} k={top_k} p={top_p} min_p={min_p}: worst {worst:.3e}, nearest edge {nearest:.3e}, "
          f"kept {[int(o[0].sum()) for o in oracles.values()]}")
    return got[0], worst


# V = 1537: per = 2 elements per thread, the last chunk (thread 768) ragged.  Twelve heavy tokens,
# logits 5 - 0.06 j: pairs inside one thread's chunk (0/1, 2/3, 700/701, 1534/1535), a pair across a
# chunk boundary (1023/1024), the first and the last index (1536, alone in its chunk).
V_SMALL = 1537
HEAVY = [700, 1536, 0, 1023, 701, 3, 1534, 1, 1024, 2, 1535, 777]      # j-th heaviest token


def _small_logits(perm=0, seed=0):
    rng = np.random.default_rng(seed)
    l = rng.uniform(-9.0, -7.0, V_SMALL)
    idx = HEAVY[perm:] + HEAVY[:perm]
    l[idx] = 5.0 - 0.06 * np.arange(12)
    return l.astype(np.float32)


def _assert_margins(l, top_k, top_p, min_p):
    """The case keeps clear of every cut: see the module docstring."""
    l = l.astype(np.float64)
    p = np.exp(l - l.max())
    mass = p / p.sum()
    assert (np.sort(mass)[::-1][:12] >= 0.02).all()
    order = np.argsort(-l, kind="stable")
    surv = order
    if top_k:
        assert l[order[top_k - 1]] - l[order[top_k]] >= 0.01 and mass[order[top_k]] >= 0.01
        surv = order[:top_k]
    if top_p < 1.0:
        cs = np.cumsum(p[surv]) / p[surv].sum()
        m = int(np.searchsorted(cs, top_p))
        assert cs[m] - top_p >= 1e-3 and (m == 0 or top_p - cs[m - 1] >= 1e-3)
        assert mass[order[m + 1]] >= 0.01
    if min_p:
        below = p[p < min_p].max()
        assert min_p - below >= 1e-3 and p[p >= min_p].min() - min_p >= 1e-3
        assert mass[p == below][0] >= 0.01


SMALL_CASES = [
    # (temp, top_k, top_p, min_p), kept-set size
    ((1.0, 5, 1.0, 0.0), 5),            # top-k alone
    ((1.0, 0, 0.5, 0.0), 5),            # top-p alone
    ((1.0, 0, 1.0, 0.75), 5),           # min-p alone
    ((0.5, 4, 0.8, 0.72), 4),           # all three, top-k binds
    ((2.0, 4, 0.8, 0.72), 4),
    ((0.5, 9, 0.5, 0.72), 4),           # top-p binds (on the 9 survivors: 5 tokens without the top-k)
    ((2.0, 9, 0.5, 0.72), 4),
    ((0.5, 9, 0.8, 0.75), 5),           # min-p binds
    ((2.0, 9, 0.8, 0.75), 5),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case,size", SMALL_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_small_kept_sets(cuda, native, case, size):
    """Every draw inside its oracle interval, and over the 3 x 256 draws the set of drawn tokens EQUALS
    the oracle's kept set (each kept token carries >= 10 % of the kept mass; the seeds are fixed)."""
    from mipipe.ops import kernels as K
    temp, top_k, top_p, min_p = case
    l = _small_logits()
    _assert_margins(l, top_k, top_p, min_p)
    assert int(kept_set(l, top_k, top_p, min_p).sum()) == size
    rows = torch.from_numpy(l).repeat(M_ROWS, 1)
    _check_case(K, cuda, rows, V_SMALL, temp=temp, top_k=top_k, top_p=top_p, min_p=min_p, drawn_equals_kept=True)


@pytest.mark.gpu
def test_rows_use_their_own_logits(cuda, native):
    """Even and odd rows hold different logits (rows 0 and 1 differ): each row follows its own oracle."""
    from mipipe.ops import kernels as K
    a, b = _small_logits(0, seed=1), _small_logits(5, seed=2)
    rows = torch.from_numpy(np.stack([a, b])).repeat(M_ROWS // 2, 1)
    assert torch.equal(rows[2], rows[0]) and not torch.equal(rows[1], rows[0])
    for kw in (dict(temp=1.0, top_k=5), dict(temp=0.7, top_k=9, top_p=0.5, min_p=0.72)):
        _check_case(K, cuda, rows, V_SMALL, row_logits={0: a, 1: b}, drawn_equals_kept=True, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(temp=0.8), dict(temp=0.8, top_k=40, top_p=0.9, min_p=0.05)],
                         ids=["T0.8", "T0.8-k40-p0.9-minp0.05"])
def test_llama3_vocabulary(cuda, native, kw):
    """V = 128256 (per = 126), logits randn * 4: the interval assertion only (see the module docstring)."""
    from mipipe.ops import kernels as K
    l = (np.random.default_rng(128256).standard_normal(128256) * 4).astype(np.float32)
    rows = torch.from_numpy(l).repeat(M_ROWS, 1)
    _check_case(K, cuda, rows, 128256, **kw)


@pytest.mark.gpu
def test_tiny_vocabulary(cuda, native):
    """V = 5: per = 1 and 1019 threads own no element."""
    from mipipe.ops import kernels as K
    rows = torch.tensor([0.3, 1.2, -0.5, 0.9, 0.1]).repeat(M_ROWS, 1)
    _check_case(K, cuda, rows, 5, temp=1.0, drawn_equals_kept=True)
    _check_case(K, cuda, rows, 5, temp=1.5, top_k=2, drawn_equals_kept=True)


@pytest.mark.gpu
def test_padding_columns_and_minus_inf(cuda, native):
    """ld = n + 5 with +inf in the padding: never read (same draws as the packed rows); -inf logits
    carry no mass and are never drawn."""
    from mipipe.ops import kernels as K
    l = _small_logits(3, seed=4)
    l[[4, 5, 6, 699, 702, 1533]] = -np.inf
    packed = torch.from_numpy(l).repeat(M_ROWS, 1)
    padded = torch.full((M_ROWS, V_SMALL + 5), float("inf"))
    padded[:, :V_SMALL] = packed
    for kw in (dict(temp=1.5), dict(temp=1.0, top_k=9, top_p=0.8)):
        t0, _ = _check_case(K, cuda, packed, V_SMALL, **kw)
        t1, _ = _check_case(K, cuda, padded, V_SMALL, **kw)
        assert np.array_equal(t0, t1)
        assert np.isfinite(l[t0]).all()


@pytest.mark.gpu
def test_degenerate_settings(cuda, native):
    """top_k >= n is a no-op; top_k = 1, top_p = 1e-6 and min_p = 1 each give the argmax for every row,
    seed and step; temp = 0 is the lowest-index argmax."""
    from mipipe.ops import kernels as K
    l = _small_logits(7, seed=5)
    rows = torch.from_numpy(l).repeat(M_ROWS, 1)
    base, _ = _check_case(K, cuda, rows, V_SMALL, temp=1.0)
    assert len(set(base.tolist())) >= 12
    for k in (V_SMALL, V_SMALL + 100):
        t, _ = _check_case(K, cuda, rows, V_SMALL, temp=1.0, top_k=k)
        assert np.array_equal(t, base)
    am = int(np.argmax(l))
    for seed in (0, 1, 12345, SEED):
        for kw in (dict(top_k=1), dict(top_p=1e-6), dict(min_p=1.0)):
            t, _ = _check_case(K, cuda, rows, V_SMALL, temp=1.3, seed=seed, **kw)
            assert (t == am).all(), kw
    tie = l.copy()
    tie[[900, 40, 1536]] = 7.0                   # three equal maxima: the lowest index wins
    dev = torch.from_numpy(tie).repeat(M_ROWS, 1).to(cuda)
    for s in (None, 0, 5):
        assert (_launch(K, cuda, dev, s, temp=0.0, seed=SEED) == 40).all()
