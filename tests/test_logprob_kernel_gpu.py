"""logprob_kernel (logprob.hip) against a float64 numpy oracle.

Ids are exact against np.argsort(-x, kind="stable") (descending logit, ties to the lower index).
lse, target_lp and top_lp are within TOL = 1e-4 absolute of the oracle for |logit| <= 30.  The bound
is derived, not fitted: an f32 sum of <= 128256 exponentials in any partial / tree order plus the final
subtraction came to 2.8e-6 in a numpy f32 emulation; v_exp_f32 with its argument scaling adds about
|x| * 2^-24 * log2(e) <~ 5e-6 relative to the sum; 1e-4 is roughly ten times the total.
Every case prints its worst distance as `worst`.  Measured on the MI355X over every case of this
file: worst 4.9e-6 (n = 32771, M = 67, top_n = 20); 3.4e-6 at n = 128256, M = 3.

Decomposition the tie cases straddle: a lane reads 4 consecutive logits (16 bytes), a wave 256, the
1024-thread workgroup 4096 per load and 4 loads (16384) per batch; n % 4 trailing logits, or the
whole row when it is not 16-byte aligned, go through a scalar loop; the 16 waves' lists are merged by
wave 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
CANARY_I = 0x7FC5A5A5      # a quiet-NaN bit pattern, also an implausible id
PAD_ROWS, PAD_TOP = 2, 3


def oracle(x, n, target, top_n):
    """x: f32 [M][ld] -> (lse [M], target_lp [M], top_id [M][top_n], top_lp [M][top_n]) in float64."""
    M = x.shape[0]
    v = x[:, :n].astype(np.float64)
    v = np.where(np.isnan(v), -np.inf, v)
    mx = v.max(axis=1)
    lse = np.full(M, -np.inf)
    ok = np.isfinite(mx)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse[ok] = mx[ok] + np.log(np.exp(v[ok] - mx[ok, None]).sum(axis=1))
    tlp = np.full(M, -np.inf)
    tid = np.full((M, top_n), -1, np.int64)
    tl = np.full((M, top_n), -np.inf)
    for m in range(M):
        if not ok[m]:
            continue
        if target is not None and 0 <= target[m] < n:
            tlp[m] = v[m, target[m]] - lse[m]
        if top_n:
            order = np.argsort(-v[m], kind="stable")[:top_n]
            keep = v[m, order] > -np.inf
            k = int(keep.sum())
            tid[m, :k] = order[:k]
            tl[m, :k] = v[m, order[:k]] - lse[m]
    return lse, tlp, tid, tl


def run(cuda, x, n, target, top_n):
    """Launch on x (numpy f32 [M][ld]) with canary-filled, over-sized outputs; check the canaries and
    that the logits are bitwise unchanged; return the outputs as numpy."""
    from mipipe.ops import kernels as K
    M = x.shape[0]
    xd = torch.from_numpy(x).to(cuda)
    before = xd.view(torch.int32).clone()

    def can(shape, dtype):
        return torch.full(shape, CANARY_I, dtype=torch.int32, device=cuda).view(dtype)
    out = (can((M + PAD_ROWS,), torch.float32), can((M + PAD_ROWS,), torch.float32),
           can((M + PAD_ROWS, top_n + PAD_TOP), torch.int32), can((M + PAD_ROWS, top_n + PAD_TOP), torch.float32))
    td = None if target is None else torch.from_numpy(np.asarray(target, np.int32)).to(cuda)
    K.logprob(xd, n=n, target=td, top_n=top_n, rows=M, out=out)
    torch.cuda.synchronize()
    assert torch.equal(xd.view(torch.int32), before), "logits were written"
    lse, tlp, tid, tl = (o.view(torch.int32).cpu().numpy() for o in out)
    assert (lse[M:] == CANARY_I).all() and (tlp[M:] == CANARY_I).all(), "rows beyond M written"
    assert (tid[M:] == CANARY_I).all() and (tl[M:] == CANARY_I).all(), "rows beyond M written"
    assert (tid[:, top_n:] == CANARY_I).all() and (tl[:, top_n:] == CANARY_I).all(), "slots beyond top_n written"
    return (lse[:M].view(np.float32), tlp[:M].view(np.float32), tid[:M, :top_n], tl[:M, :top_n].view(np.float32))


def dist(a, b):
    """max |a - b| where -inf must meet -inf exactly."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    inf = np.isinf(b)
    assert np.array_equal(np.isinf(a), inf) and not np.isnan(a).any(), (a, b)
    assert (a[inf] == b[inf]).all()
    return float(np.abs(a[~inf] - b[~inf]).max()) if (~inf).any() else 0.0


def check(cuda, x, n, target, top_n, label):
    lse, tlp, tid, tl = run(cuda, x, n, target, top_n)
    olse, otlp, otid, otl = oracle(x, n, target, top_n)
    assert np.array_equal(tid, otid), f"{label}: top ids differ"
    worst = max(dist(lse, olse), dist(tlp, otlp), dist(tl, otl))
    print(f"{label}: worst {worst:.3g}")
    assert worst <= TOL, (label, worst)
    return worst


def padded(M, n, rng, fill=np.nan):
    ld = (n + 15) // 16 * 16
    x = np.full((M, ld), fill, np.float32)
    return x, ld


def distinct_rows(M, n, rng):
    """Every row a shuffled grid over [-30, 30]: distinct f32 values (the spacing at n = 128256 is
    4.7e-4, an f32 ulp at 30 is 1.9e-6)."""
    x, _ = padded(M, n, rng)
    grid = np.linspace(-30.0, 30.0, n).astype(np.float32) if n > 1 else np.array([1.5], np.float32)
    assert len(np.unique(grid)) == n
    for m in range(M):
        x[m, :n] = rng.permutation(grid)
    return x


SHAPES = [(n, M) for n in (1, 5, 63, 64, 65, 1023, 1024, 1025, 4099, 32771) for M in (1, 3, 67)] + [(128256, 3)]


@pytest.mark.parametrize("top_n", [0, 1, 5, 20])
@pytest.mark.parametrize("n,M", SHAPES)
def test_distinct_logits(cuda, native, n, M, top_n):
    rng = np.random.default_rng(n * 131 + M * 7 + top_n)
    x = distinct_rows(M, n, rng)
    target = rng.integers(0, n, M)
    check(cuda, x, n, target, top_n, f"n={n} M={M} top_n={top_n}")


@pytest.mark.parametrize("top_n", [1, 5, 20])
def test_ties_across_boundaries(cuda, native, top_n):
    """Exact duplicates of the row maximum on both sides of every boundary of the decomposition (13 of
    them: more than top_n = 1 and 5), over a second tie of a sixth of the row that straddles the cut at
    top_n = 20: the lower ids win, in order."""
    n = 16384 * 2 + 4096 + 256 + 7               # two batches, one more load, one more wave, a scalar tail
    n4 = n & ~3
    rng = np.random.default_rng(top_n)
    x = distinct_rows(3, n, rng)
    x[:, :n] = np.minimum(x[:, :n], 20.0)         # a second, much larger tie (a sixth of the row) below the first
    edges = [3, 4, 63 * 4 + 3, 256, 4095, 4096, 16383, 16384, 32767, 32768, n4 - 1, n4, n - 1]
    # row 0: all edges tie at the maximum; row 1: ties only late in the row, so lists are full of
    # smaller entries when they arrive; row 2: a tie BELOW a unique maximum, high ids placed first
    x[0, edges] = 25.0
    x[1, edges[5:]] = 25.0
    x[2, edges[::-1][:top_n + 2]] = 25.0
    x[2, 7] = 26.0
    check(cuda, x, n, [4, 4096, n - 1], top_n, f"ties top_n={top_n}")


def test_all_equal_row(cuda, native):
    """Every logit equal: the top-n are ids 0..top_n-1 and every logprob is -log(n)."""
    n = 4099
    x, _ = padded(2, n, None)
    x[:, :n] = 0.25
    lse, tlp, tid, tl = run(cuda, x, n, [n - 1, 0], 20)
    assert np.array_equal(tid, np.tile(np.arange(20), (2, 1)))
    assert np.abs(tl + np.log(n)).max() <= TOL and np.abs(tlp + np.log(n)).max() <= TOL


def edge_base(rng, M=3, n=1025):
    return distinct_rows(M, n, rng), n


def test_nan_entry(cuda, native):
    rng = np.random.default_rng(1)
    x, n = edge_base(rng)
    big = x[:, :n].argmax(axis=1)
    x[np.arange(3), big] = np.nan                 # the would-be maximum is ignored
    x[1, 0] = np.nan
    check(cuda, x, n, [int(big[0]), 0, 5], 5, "nan")
    _, tlp, _, _ = run(cuda, x, n, [int(big[0]), 0, 5], 5)
    assert tlp[0] == -np.inf and tlp[1] == -np.inf and np.isfinite(tlp[2])


def test_neg_inf_entries(cuda, native):
    rng = np.random.default_rng(2)
    x, n = edge_base(rng)
    x[:, rng.permutation(n)[:700]] = -np.inf
    check(cuda, x, n, [1, 2, 3], 20, "-inf entries")


@pytest.mark.parametrize("fill", [-np.inf, np.nan])
def test_dead_row(cuda, native, fill):
    """A row that is entirely -inf (or entirely NaN) between two ordinary rows."""
    rng = np.random.default_rng(3)
    x, n = edge_base(rng)
    x[1, :n] = fill
    check(cuda, x, n, [1, 2, 3], 5, f"dead row {fill}")
    lse, tlp, tid, tl = run(cuda, x, n, [1, 2, 3], 5)
    assert lse[1] == -np.inf and tlp[1] == -np.inf and (tid[1] == -1).all() and (tl[1] == -np.inf).all()
    assert np.isfinite(lse[[0, 2]]).all()


def test_top_n_exceeds_finite_entries(cuda, native):
    rng = np.random.default_rng(4)
    x, n = edge_base(rng)
    x[:, :n] = -np.inf
    x[0, [1000, 3, 512]] = [1.0, 2.0, 3.0]        # 3 finite entries
    x[1, 1024] = -4.0                             # 1 finite entry, in the scalar tail
    x[2, :20] = np.arange(20, dtype=np.float32)   # exactly top_n
    check(cuda, x, n, [3, 1024, 19], 20, "few finite")
    _, _, tid, tl = run(cuda, x, n, None, 20)
    assert list(tid[0][:4]) == [512, 3, 1000, -1] and (tl[0][3:] == -np.inf).all()
    assert list(tid[1][:2]) == [1024, -1]
    assert list(tid[2]) == list(range(19, -1, -1))


def test_targets_none_and_out_of_range(cuda, native):
    rng = np.random.default_rng(5)
    x, n = edge_base(rng)
    x[:, n:] = 1e30                               # padding that would win if it were read
    check(cuda, x, n, [-1, n, 7], 5, "targets")
    _, tlp, _, _ = run(cuda, x, n, [-1, n, 7], 5)
    assert tlp[0] == -np.inf and tlp[1] == -np.inf and np.isfinite(tlp[2])
    _, tlp, _, _ = run(cuda, x, n, None, 0)       # no target array at all
    assert (tlp == -np.inf).all()


def test_unaligned_rows_take_the_scalar_path(cuda, native):
    """A row stride that is no multiple of 16 bytes: same results through the scalar loop."""
    from mipipe.ops import kernels as K
    rng = np.random.default_rng(6)
    n, M = 4099, 3
    x = distinct_rows(M, n, rng)[:, :n].copy()    # ld = n = 4099
    xd = torch.from_numpy(x).to(cuda)
    lse, tlp, tid, tl = K.logprob(xd, target=torch.tensor([0, 1, 2], dtype=torch.int32, device=cuda), top_n=20)
    olse, otlp, otid, otl = oracle(x, n, [0, 1, 2], 20)
    assert np.array_equal(tid.cpu().numpy(), otid)
    assert max(dist(lse.cpu().numpy(), olse), dist(tlp.cpu().numpy(), otlp), dist(tl.cpu().numpy(), otl)) <= TOL


def test_generation_pair_reads_the_raw_logit(cuda, native):
    """Statistics before the in-place penalty, the chosen token's logprob after the sampler: it is
    the log-softmax of the RAW logits at the chosen id, also for ids the penalty rewrote."""
    from mipipe.ops import kernels as K
    rng = np.random.default_rng(7)
    n, M, last_n = 1025, 3, 8
    x = distinct_rows(M, n, rng)[:, :n].copy()
    top = np.argsort(-x, axis=1)
    hist = np.full((M, last_n), -1, np.int32)
    hist[0, :3] = [top[0, 0], 5, top[0, 0]]       # the raw argmax is penalised away ...
    hist[1, :2] = [top[1, 1], 9]
    hist[2, 5] = top[2, 0]
    x[2] *= 0.5
    x[2, top[2, 0]] = 30.0                        # ... except here, where it survives the penalty
    xd = torch.from_numpy(x).to(cuda)
    hd = torch.from_numpy(hist).to(cuda)

    def step(lg):
        K.penalize(lg, hd, repeat=1.5, freq=0.5, presence=0.5)
        return K.argmax(lg)
    tok, clp, tid, tl = K.logprob_generation(xd, hd, 5, step)
    tok = tok.cpu().numpy()
    assert tok[0] == top[0, 1] and tok[1] == top[1, 0] and tok[2] == top[2, 0]     # [2] was penalised and chosen
    olse, otlp, otid, otl = oracle(x, n, tok, 5)
    assert np.array_equal(tid.cpu().numpy(), otid)
    assert dist(clp.cpu().numpy(), otlp) <= TOL and dist(tl.cpu().numpy(), otl) <= TOL
    assert not np.array_equal(xd.cpu().numpy(), x), "the penalty did not run"


def test_top_n_out_of_range_is_an_error(cuda, native):
    from mipipe.ops import kernels as K
    x = torch.zeros(1, 16, device=cuda)
    with pytest.raises(Exception):
        K.logprob(x, top_n=21)
