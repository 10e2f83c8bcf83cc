"""sample_rows_kernel and row_adjust_kernel (sample_rows.hip): every row of one launch follows its
own record.  The draws are checked one by one against the float64 oracle of test_sampler_oracle_gpu
(same chain, same TOL: the kernels share one device function, so the summation structure that TOL was
derived for is unchanged), with the per-request variate u = uniform(seed_r, d_r, 0)."""
import numpy as np
import pytest
import torch

from test_sampler_oracle_gpu import (SEED, SMALL_CASES, TOL, V_SMALL, _assert_margins, _small_logits, draw_cdf,
                                     interval_distance, kept_set, uniform)

M = 64
# the three draw indices of row r are (7 r) % 23 + k * DRAW_STRIDE: with this stride the ORACLE's draws of every
# parameter set cover its kept set (asserted on the CPU below, before anything runs on the GPU)
DRAW_STRIDE = 31


def _rec(case, seed, **kw):
    temp, top_k, top_p, min_p = case
    return dict(temp=temp, top_k=top_k, top_p=top_p, min_p=min_p, seed=seed, **kw)


def _oracle_token(l, rec, d):
    """(token the exact chain draws, kept mask, cdf, u)."""
    keep = kept_set(l, rec["top_k"], rec["top_p"], rec["min_p"])
    cdf = draw_cdf(l, keep, rec["temp"])
    u = uniform(rec["seed"], d, 0)
    return int(np.searchsorted(cdf, u, side="right")), keep, cdf, u


def _run(K, cuda, logits, recs, draws, advance=False):
    """argmax of every row, then the sampled rows over it (the order of the stage's head)."""
    dev = logits.to(cuda) if logits.device.type == "cpu" else logits
    tok = K.argmax(dev)
    d = torch.tensor(draws, dtype=torch.int32, device=cuda)
    K.sample_rows(dev, K.row_records(recs, cuda), d, tokens=tok, advance=advance)
    return tok.cpu().numpy().astype(np.int64), d.cpu().numpy()


def _check_rows(tok, row_logits, recs, draws):
    """Every sampled row inside its own oracle interval, every greedy row the lowest-index argmax."""
    worst = 0.0
    for r, (rec, d) in enumerate(zip(recs, draws)):
        l = row_logits(r)
        if rec["temp"] <= 0:
            assert tok[r] == int(np.argmax(l)), f"greedy row {r}"
            continue
        _, keep, cdf, u = _oracle_token(l, rec, d)
        assert 0 <= tok[r] < l.size and keep[tok[r]], f"row {r}: token {tok[r]} outside its kept set"
        dist = float(interval_distance(cdf, np.array([tok[r]]), np.array([u]))[0])
        worst = max(worst, dist)
        assert dist <= TOL, f"row {r}: u outside the token's CDF interval by {dist:.3e}"
    return worst


def _mixed_rows():
    recs, base = [], []
    for r in range(M):
        case = SMALL_CASES[r % 9][0]
        recs.append(_rec(case if r % 4 != 3 else (0.0,) + case[1:], SEED + r))
        base.append((7 * r) % 23)
    return recs, base


@pytest.mark.gpu
def test_mixed_rows(cuda, native):
    """64 rows of the same logits, nine parameter sets, own seeds and draw indices, every fourth row greedy."""
    from mipipe.ops import kernels as K
    l = _small_logits()
    recs, base = _mixed_rows()
    for case, _ in SMALL_CASES:
        _assert_margins(l, *case[1:])
    # CPU precondition: the oracle's three draws per row cover every parameter set's kept set
    for s in range(9):
        rows = [r for r in range(M) if r % 9 == s and recs[r]["temp"] > 0]
        want = set(np.flatnonzero(kept_set(l, *SMALL_CASES[s][0][1:])).tolist())
        seen = {_oracle_token(l, recs[r], base[r] + k * DRAW_STRIDE)[0] for r in rows for k in range(3)}
        assert seen == want and len(want) == SMALL_CASES[s][1], (s, sorted(seen), sorted(want))
    logits = torch.from_numpy(l).repeat(M, 1)
    drawn = [set() for _ in range(9)]
    worst = 0.0
    for k in range(3):
        draws = [b + k * DRAW_STRIDE for b in base]
        tok, d_after = _run(K, cuda, logits, recs, draws)
        assert np.array_equal(d_after, draws), "advance = 0 must leave the draw indices alone"
        worst = max(worst, _check_rows(tok, lambda r: l, recs, draws))
        for r in range(M):
            if recs[r]["temp"] > 0:
                drawn[r % 9].add(int(tok[r]))
    for s in range(9):
        assert drawn[s] == set(np.flatnonzero(kept_set(l, *SMALL_CASES[s][0][1:])).tolist()), s
    print(f"sample_rows mixed: worst {worst:.3e}")
    # advance = 1: every row's index moves on by one, greedy rows included, and the tokens are the same
    draws = list(base)
    t0, _ = _run(K, cuda, logits, recs, draws)
    t1, d_after = _run(K, cuda, logits, recs, draws, advance=True)
    assert np.array_equal(t0, t1) and np.array_equal(d_after, np.asarray(draws) + 1)


@pytest.mark.gpu
def test_row_independence(cuda, native):
    """Permuting the rows (records, draw indices, logits) permutes the tokens exactly; changing one row's
    record changes no other row's token."""
    from mipipe.ops import kernels as K
    a, b = _small_logits(0, seed=1), _small_logits(5, seed=2)
    logits = torch.from_numpy(np.stack([a, b])).repeat(M // 2, 1)
    recs, draws = _mixed_rows()
    t0, _ = _run(K, cuda, logits, recs, draws)
    _check_rows(t0, lambda r: (a, b)[r % 2], recs, draws)
    perm = np.random.default_rng(3).permutation(M)
    assert (perm != np.arange(M)).sum() > M // 2 and ((perm % 2) != (np.arange(M) % 2)).any()
    t1, _ = _run(K, cuda, logits[torch.from_numpy(perm)], [recs[p] for p in perm], [draws[p] for p in perm])
    assert np.array_equal(t1, t0[perm])
    changed = [dict(r) for r in recs]
    changed[10] = _rec((1.7, 0, 1.0, 0.0), 99)
    changed[11] = dict(recs[11], temp=0.6) if recs[11]["temp"] <= 0 else dict(recs[11], temp=0.0)
    t2, _ = _run(K, cuda, logits, changed, draws)
    keep = np.ones(M, bool)
    keep[[10, 11]] = False
    assert np.array_equal(t2[keep], t0[keep])
    _check_rows(t2, lambda r: (a, b)[r % 2], changed, draws)


@pytest.mark.gpu
def test_llama3_and_tiny_vocabulary(cuda, native):
    """V = 128256 (the interval only, as test_llama3_vocabulary: kept-set equality is not a property of the
    24-step bisection there) and V = 5, 32 rows, per-row seeds."""
    from mipipe.ops import kernels as K
    l = (np.random.default_rng(128256).standard_normal(128256) * 4).astype(np.float32)
    sets = [(0.8, 0, 1.0, 0.0), (0.8, 40, 0.9, 0.05)]
    recs = [_rec(sets[r % 2], SEED ^ (r * 0x1234567)) for r in range(32)]
    draws = [(5 * r) % 17 for r in range(32)]
    tok, _ = _run(K, cuda, torch.from_numpy(l).repeat(32, 1), recs, draws)
    worst = 0.0
    for r in range(32):
        _, _, cdf, u = _oracle_token(l, recs[r], draws[r])
        assert 0 <= tok[r] < l.size
        dist = float(interval_distance(cdf, np.array([tok[r]]), np.array([u]))[0])
        worst = max(worst, dist)
        assert dist <= TOL, (r, dist)
    print(f"sample_rows V=128256: worst {worst:.3e}")
    tiny = np.array([0.3, 1.2, -0.5, 0.9, 0.1], np.float32)
    sets = [(1.0, 0, 1.0, 0.0), (1.5, 2, 1.0, 0.0)]
    recs = [_rec(sets[r % 2], 1000 + r) for r in range(32)]
    tok, _ = _run(K, cuda, torch.from_numpy(tiny).repeat(32, 1), recs, draws)
    _check_rows(tok, lambda r: tiny, recs, draws)


@pytest.mark.gpu
def test_padding_columns_and_minus_inf(cuda, native):
    """ld = n + 5 with +inf in the padding: never read; -inf logits are never drawn."""
    from mipipe.ops import kernels as K
    l = _small_logits(3, seed=4)
    l[[4, 5, 6, 699, 702, 1533]] = -np.inf
    recs = [_rec(((1.5, 0, 1.0, 0.0), (1.0, 9, 0.8, 0.0))[r % 2], 50 + r) for r in range(32)]
    draws = list(range(32))
    packed = torch.from_numpy(l).repeat(32, 1)
    padded = torch.full((32, V_SMALL + 5), float("inf"))
    padded[:, :V_SMALL] = packed
    t0, _ = _run(K, cuda, packed, recs, draws)
    t1, _ = _run(K, cuda, padded.to(cuda)[:, :V_SMALL], recs, draws)
    assert np.array_equal(t0, t1) and np.isfinite(l[t0]).all()
    _check_rows(t0, lambda r: l, recs, draws)


def _adjust_oracle(l, rec, window):
    """numpy f32 mirror of row_adjust_kernel.  Bias: one f32 add per listing, in list order.  Penalty per
    distinct window id with count c: ONE divide (l > 0) or multiply by repeat, then ONE FUSED
    multiply-subtract fma(-c, freq, l) (the product c * freq is exact in float64 and the sum of it and an
    f32 is rounded once to f32 here, as the fma does), then one f32 subtract of presence."""
    out = l.copy()
    for t, v in rec.get("bias", ()):
        out[t] = np.float32(out[t] + np.float32(v))
    rep, fq, pr = (np.float32(rec.get(k, d)) for k, d in (("repeat", 1.0), ("freq", 0.0), ("presence", 0.0)))
    if rep != 1 or fq != 0 or pr != 0:
        ids = [t for t in window if 0 <= t < l.size]
        for t in sorted(set(ids)):
            x = out[t]
            x = np.float32(x / rep) if x > 0 else np.float32(x * rep)
            x = np.float32(np.float64(x) - np.float64(ids.count(t)) * np.float64(fq))
            out[t] = np.float32(x - pr)
    return out


@pytest.mark.gpu
def test_row_adjust_matches_f32_oracle(cuda, native):
    """Penalties with per-row values over a window of 8 (repeats, empty slots, an id at n - 1), bias with
    0, 1 and 32 entries (a ban, an id that is also in the window; bias first): exactly equal.  Neutral
    rows are bit-identical to their input."""
    from mipipe.ops import kernels as K
    n = 1537
    rng = np.random.default_rng(9)
    base = (rng.standard_normal((8, n)) * 3).astype(np.float32)
    window = np.array([[5, 9, 5, -1, n - 1, 5, 9, -1]] * 8, np.int32)
    window[3] = [-1] * 8
    window[6] = [700, 700, 700, 700, 3, 2, 1, 0]
    b32 = [(int(t), float(v)) for t, v in zip(rng.permutation(n)[:32], rng.standard_normal(32) * 2)]
    b32[7] = (9, 1.25)            # also in the window
    b32[20] = (b32[3][0], -0.5)   # an id listed twice
    recs = [dict(repeat=1.3, freq=0.25, presence=0.5),
            dict(),                                                    # neutral
            dict(repeat=0.8, bias=[(5, -np.inf)]),
            dict(freq=0.7, bias=b32),                                  # empty window
            dict(bias=[(n - 1, 3.5)]),                                 # bias alone
            dict(presence=1.5, bias=[(9, -2.0), (n - 1, np.inf * -1)]),
            dict(repeat=1.1, freq=0.1, presence=0.1, bias=b32),
            dict(repeat=1.0, freq=0.0, presence=0.0)]                  # neutral, spelled out
    dev = torch.from_numpy(base).to(cuda)
    K.row_adjust(dev, K.row_records(recs, cuda), torch.from_numpy(window).to(cuda))
    got = dev.cpu().numpy()
    for r, rec in enumerate(recs):
        want = _adjust_oracle(base[r], rec, window[r].tolist())
        assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), (r, np.flatnonzero(got[r] != want)[:8])
    assert np.array_equal(got[1].view(np.uint32), base[1].view(np.uint32))
    assert np.array_equal(got[7].view(np.uint32), base[7].view(np.uint32))
    assert got[2][5] == -np.inf and got[5][n - 1] == -np.inf
    # a window narrower than its row stride (the stage keeps the bias ids behind the window): the tail is not read
    wide = np.full((8, 12), 11, np.int32)
    wide[:, :8] = window
    dev = torch.from_numpy(base).to(cuda)
    K.row_adjust(dev, K.row_records(recs, cuda), torch.from_numpy(wide).to(cuda), last_n=8)
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), got.view(np.uint32))


@pytest.mark.gpu
def test_bias_and_the_draw(cuda, native):
    """A ban on the heaviest token with top_k = 5 keeps the next five and never draws the banned id; +100
    on a light token makes a temp = 1 row draw only it."""
    from mipipe.ops import kernels as K
    l = _small_logits()
    heavy = int(np.argmax(l))
    banned = l.copy()
    banned[heavy] = -np.inf
    _assert_margins(l, 5, 1.0, 0.0)
    # the margins of _assert_margins' top-k cut for the row with the ban (eleven heavy tokens are left, so
    # its twelve-token mass line does not apply): the 5th / 6th survivors are 0.01 apart and the 6th is heavy
    order = np.argsort(-banned.astype(np.float64), kind="stable")
    mass = np.exp(banned.astype(np.float64) - banned.max())
    mass /= mass.sum()
    assert (mass[order[:11]] >= 0.02).all()
    assert banned[order[4]] - banned[order[5]] >= 0.01 and mass[order[5]] >= 0.01
    want = set(np.argsort(-l, kind="stable")[1:6].tolist())
    assert set(np.flatnonzero(kept_set(banned, 5)).tolist()) == want
    light = 1200
    assert l[light] < -6.0
    recs = [dict(temp=1.0, top_k=5, seed=SEED + r, bias=[(heavy, -np.inf)]) if r % 2 == 0 else
            dict(temp=1.0, seed=SEED + r, bias=[(light, 100.0)]) for r in range(M)]
    # CPU precondition: the oracle's 3 x 32 draws of the banned rows cover the five survivors
    full = [{**dict(top_k=0, top_p=1.0, min_p=0.0), **r} for r in recs]
    assert {_oracle_token(banned, full[r], r + k * M)[0] for r in range(0, M, 2) for k in range(3)} == want
    recs = full
    drawn = set()
    for k in range(3):
        draws = [r + k * M for r in range(M)]
        dev = torch.from_numpy(l).repeat(M, 1).to(cuda)
        K.row_adjust(dev, K.row_records(recs, cuda))
        tok, _ = _run(K, cuda, dev, recs, draws)
        adj = dev.cpu().numpy()
        assert np.array_equal(adj[0], banned) and adj[1][light] == np.float32(l[light] + np.float32(100.0))
        _check_rows(tok, lambda r: adj[r], recs, draws)
        assert (tok[1::2] == light).all()
        drawn |= set(tok[0::2].tolist())
    assert heavy not in drawn and drawn == want
