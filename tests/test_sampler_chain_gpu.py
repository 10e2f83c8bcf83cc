"""The later stages of the sampler chain (sample_chain.h through sample_rows): each token against a
float64 reference written from the definitions in kernels_api.h.  A draw is left out only where fp32
may land on the other side: u * total within 1e-4 * total of a CDF boundary, or a threshold statistic
within 1e-4 of its limit; at most 5 % of a case's draws, which the reference alone decides.  LOGITS was
chosen on the CPU for that: every case leaves out 0 or 1 of its 64 draws."""
import numpy as np
import pytest
import torch

M, SEED, MASK = 64, 0x5EED0BADC0FFEE, (1 << 64) - 1
# n -> (seed, sigma): the large rows are peaked, or an uncut row's draws all lie next to a CDF boundary
LOGITS = {37: (6, 2.0), 1029: (2, 6.0), 4099: (1, 6.0)}
CASES = {
    "top_n_sigma": dict(top_n_sigma=1.0),
    "typical": dict(typical_p=0.5),
    "xtc_always": dict(xtc_probability=1.0, xtc_threshold=0.05),
    "xtc_half": dict(xtc_probability=0.5, xtc_threshold=0.05),
    "dynatemp": dict(dynatemp_range=0.5, dynatemp_exponent=1.0),
    "dynatemp_clamped": dict(dynatemp_range=2.0, dynatemp_exponent=2.0),
    "all": dict(top_n_sigma=2.0, top_k=40, typical_p=0.9, top_p=0.9, min_p=0.02, xtc_probability=0.5, xtc_threshold=0.05,
                dynatemp_range=0.5, dynatemp_exponent=1.5),
}

def mix64(x):
    for shift, mul in ((30, 0xBF58476D1CE4E5B9), (27, 0x94D049BB133111EB)):
        x = ((x & MASK) ^ (x & MASK) >> shift) * mul & MASK
    return x ^ x >> 31

def logits(n):
    """Normal logits, three planted 2e-3, 4e-3 and 7e-3 below the maximum, every gap >= 1e-3."""
    rng = np.random.default_rng(LOGITS[n][0])
    l = rng.standard_normal(n) * LOGITS[n][1]
    l[rng.permutation(n)[:3]] = l.max() - np.array([2e-3, 4e-3, 7e-3])
    order = np.argsort(l)
    l[order] = np.maximum.accumulate(l[order] - 1e-3 * np.arange(n)) + 1e-3 * np.arange(n)
    assert np.diff(np.sort(l.astype(np.float32).astype(np.float64))).min() >= 0.99e-3
    return l.astype(np.float32)

def reference(l32, rec, d):
    """(token, near) of draw d, the chain in float64; near: fp32 may legitimately differ."""
    l, near = l32.astype(np.float64), False
    alive = np.ones(l.size, bool)
    r = mix64(rec["seed"] ^ mix64(d << 20))
    u, u2 = (r >> 40) / 2.0**24, (mix64(r ^ 0x9E3779B97F4A7C15) >> 40) / 2.0**24

    def prob():
        p = np.where(alive, np.exp(l - l.max()), 0.0)
        return p / p.sum()

    def mass_cut(order, p, limit):   # the leading tokens of `order` up to the one that reaches limit
        nonlocal near
        cum = np.cumsum(p[order])
        j = min(int(np.searchsorted(cum, limit)), len(order) - 1)
        near |= abs(cum[j] - limit) < 1e-4 or (j > 0 and abs(cum[j - 1] - limit) < 1e-4)
        alive[:] = False
        alive[order[:j + 1]] = True

    if rec.get("top_n_sigma", 0) > 0:
        alive &= l >= l.max() - rec["top_n_sigma"] * l.std()
    if 0 < rec.get("top_k", 0) < alive.sum():
        alive &= l >= np.sort(l[alive])[-rec["top_k"]]
    for key in ("typical_p", "top_p"):   # score: |-ln p - H|, then -p
        if 0 < rec.get(key, 1.0) < 1:
            p, idx = prob(), np.flatnonzero(alive)
            q = p[idx]
            score = np.abs(-np.log(q) + (q * np.log(q)).sum()) if key == "typical_p" else -q
            mass_cut(idx[np.argsort(score, kind="stable")], p, rec[key])
    if rec.get("min_p", 0) > 0:
        p = prob()
        near |= np.abs(p[alive] / p.max() - rec["min_p"]).min() < 1e-4
        alive &= p >= rec["min_p"] * p.max()
    if rec.get("xtc_probability", 0) > 0 and rec.get("xtc_threshold", 0.1) <= 0.5 and u2 < rec["xtc_probability"]:
        p = prob()
        near |= np.abs(p[alive] - rec["xtc_threshold"]).min() < 1e-4
        above = np.flatnonzero(alive & (p >= rec["xtc_threshold"]))
        if above.size >= 2:
            alive[above] = False
            alive[above[p[above] == p[above].min()].max()] = True
    T = rec["temp"]
    if rec.get("dynatemp_range", 0) > 0 and alive.sum() > 1:
        p = prob()[alive]
        t_lo, t_hi = max(0.0, T - rec["dynatemp_range"]), T + rec["dynatemp_range"]
        T = t_lo + (t_hi - t_lo) * (-(p * np.log(p)).sum() / np.log(p.size)) ** rec.get("dynatemp_exponent", 1.0)
    cdf = np.cumsum(np.where(alive, np.exp((l - l[alive].max()) / T), 0.0))
    x = u * cdf[-1]
    near |= np.abs(cdf[alive] - x).min() < 1e-4 * cdf[-1] or x < 1e-4 * cdf[-1]
    return int(np.searchsorted(cdf, x, side="right")), bool(near)

def run(cuda, l, recs):
    from mipipe.ops import kernels as K
    dev = torch.from_numpy(l).repeat(len(recs), 1).to(cuda)
    return K.sample_rows(dev, K.row_records(recs, cuda), torch.arange(len(recs), dtype=torch.int32, device=cuda)).cpu().numpy()

@pytest.mark.gpu
@pytest.mark.parametrize("n", list(LOGITS))
@pytest.mark.parametrize("case", list(CASES))
def test_chain_matches_reference(cuda, native, n, case):
    l, rec = logits(n), dict(temp=1.0, seed=SEED, **CASES[case])
    want = [reference(l, rec, d) for d in range(M)]
    left_out = sum(near for _, near in want)
    assert left_out <= 0.05 * M, f"the reference leaves out {left_out} of {M} draws"
    got = run(cuda, l, [rec] * M)
    print(f"chain {case} n={n}: {left_out}/{M} draws left out")
    bad = [(d, int(got[d]), t) for d, (t, near) in enumerate(want) if not near and got[d] != t]
    assert not bad, bad

@pytest.mark.gpu
@pytest.mark.parametrize("n", list(LOGITS))
def test_neutral_fields_change_nothing(cuda, native, n):
    """The existing cuts with the new fields left out, spelled out as neutral, and off in their other
    spellings (top_n_sigma = -1, an XTC threshold above 0.5, an exponent without a range): the same tokens."""
    cuts = [dict(temp=0.8), dict(temp=1.3, top_k=5), dict(temp=1.0, top_p=0.8), dict(temp=1.1, top_k=20, top_p=0.9, min_p=0.01)]
    plain = [dict(cuts[r % 4], seed=SEED + r % 7) for r in range(M)]
    neutral = dict(top_n_sigma=0.0, typical_p=1.0, xtc_probability=0.0, xtc_threshold=0.1, dynatemp_range=0.0, dynatemp_exponent=1.0)
    off = dict(top_n_sigma=-1.0, xtc_probability=1.0, xtc_threshold=0.6, dynatemp_exponent=3.0)
    base = run(cuda, logits(n), plain)
    assert len(set(base.tolist())) > 3
    for extra in (neutral, off):
        assert np.array_equal(base, run(cuda, logits(n), [dict(r, **extra) for r in plain]))
