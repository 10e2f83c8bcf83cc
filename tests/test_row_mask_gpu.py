"""row_mask_kernel (row_mask.hip): in a row that is on, every logit whose bit is clear becomes -inf and
nothing else is written.  Bit-exact against numpy over whole buffers (padding included), then the
stage's chain mask -> argmax -> sample_rows against the float64 oracle of test_sampler_oracle_gpu."""
import numpy as np
import pytest
import torch

from test_sample_rows_gpu import _check_rows, _rec, _run
from test_sampler_oracle_gpu import SEED, _small_logits

NAN_BITS = 0x7FC01234          # a quiet NaN with a payload: rows that are off must keep it bit for bit
KINDS = ("half", "sparse", "dense", "one", "ones", "off")


def _row_bits(kind, n, nw, rng):
    """uint32 words of one row's mask over n tokens (bits >= n clear)."""
    if kind in ("ones", "off"):
        allow = np.ones(n, bool) if kind == "ones" else rng.random(n) < 0.5
    elif kind == "one":
        allow = np.zeros(n, bool)
        allow[int(rng.integers(0, n))] = True
    else:
        allow = rng.random(n) < {"half": 1 / 2, "sparse": 1 / 64, "dense": 63 / 64}[kind]
    bits = np.zeros(nw * 32, bool)
    bits[:n] = allow
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint32).copy(), allow


def _case(n, M, run, rng):
    """(logits [M][ld] with +inf padding, bits [M][ldw], on [M], expected [M][ld]) for one run: the row
    kinds rotate with the run so that every kind meets every M; odd runs set the stray bits above n."""
    ld, nw = n + 5, (n + 31) // 32
    ldw = nw + 1                                   # one spare word per row: never read
    lg = np.full((M, ld), np.inf, np.float32)
    lg[:, :n] = (rng.standard_normal((M, n)) * 3).astype(np.float32)
    bits = np.zeros((M, ldw), np.uint32)
    on = np.ones(M, np.int32)
    want = lg.copy()
    for m in range(M):
        kind = KINDS[(m + run) % len(KINDS)]
        words, allow = _row_bits(kind, n, nw, rng)
        if run % 2 == 1:                           # stray bits: the last word above n, and the spare word
            if n % 32:
                words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
            bits[m, nw] = 0xFFFFFFFF
        bits[m, :nw] = words
        if kind == "off":
            on[m] = 0
            lg[m, :n].view(np.uint32)[::3] = NAN_BITS
            want[m] = lg[m]
        else:
            want[m, :n][~allow] = -np.inf
    return lg, bits, on, want


def _launch(K, cuda, lg, bits, on, n):
    """Row 0 starts 4 bytes past a 16-byte boundary and row m at 4 * (1 + m * ld) bytes, ld = n + 5.  With an
    even ld (n = 5, 31, 33, 1537) every row offset is an odd multiple of 4 bytes; with an odd ld (n = 32,
    128256) the rows alternate between odd and even multiples, so some rows there are 8- or 16-byte
    aligned.  Over the shapes below every alignment class (0, 4, 8, 12 bytes past a 16-byte boundary)
    occurs, and the first row is never aligned."""
    M, ld = lg.shape
    flat = torch.full((M * ld + 8,), 7.0, dtype=torch.float32, device=cuda)
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + M * ld].view(M, ld)
    view.copy_(torch.from_numpy(lg))
    assert view.data_ptr() % 16 == 4
    K.row_mask(view, torch.from_numpy(bits.view(np.int32)).to(cuda), torch.from_numpy(on).to(cuda), n=n)
    out = flat.cpu().numpy()
    assert out[0] == 7.0 and (out[1 + M * ld:] == 7.0).all(), "written outside the rows"
    return out[1:1 + M * ld].reshape(M, ld)


SHAPES = [(n, M) for n in (5, 31, 32, 33, 1537) for M in (1, 3, 64)] + [(128256, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,M", SHAPES)
def test_bit_exact(cuda, native, n, M):
    from mipipe.ops import kernels as K
    rng = np.random.default_rng(1000 * n + M)
    seen = set()
    for run in range(len(KINDS)):
        lg, bits, on, want = _case(n, M, run, rng)
        seen |= {KINDS[(m + run) % len(KINDS)] for m in range(M)}
        got = _launch(K, cuda, lg, bits, on, n)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (n, M, run, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
        assert np.isposinf(got[:, n:]).all()
    assert seen == set(KINDS)


@pytest.mark.gpu
def test_ldw_too_small_raises(cuda, native):
    from mipipe.ops import kernels as K
    lg = torch.zeros(2, 70, device=cuda)
    with pytest.raises(RuntimeError, match="ldw"):
        K.row_mask(lg, torch.zeros(2, 2, dtype=torch.int32, device=cuda), torch.ones(2, dtype=torch.int32, device=cuda))
    assert float(lg.abs().sum()) == 0.0


@pytest.mark.gpu
def test_chain_mask_argmax_sample_rows(cuda, native):
    """64 rows of the same logits, each with its own half-density mask (row 5: one token, row 6: all);
    every fourth row greedy, the others sampled without cuts at two temperatures.  Greedy rows give
    the lowest-index argmax over the allowed set, sampled rows fall inside the oracle interval of the
    masked logits (that file's TOL), and no banned token is drawn in 3 x 64 draws."""
    from mipipe.ops import kernels as K
    M = 64
    l = _small_logits()
    n = l.size
    nw = (n + 31) // 32
    rng = np.random.default_rng(77)
    bits = np.zeros((M, nw), np.uint32)
    allow = np.zeros((M, n), bool)
    for m in range(M):
        bits[m], allow[m] = _row_bits("one" if m == 5 else "ones" if m == 6 else "half", n, nw, rng)
    l[np.flatnonzero(allow[3])[:2]] = l.max() + 1.0   # a tie among row 3's allowed tokens: greedy takes the lower index
    masked = np.where(allow, l[None, :], -np.inf).astype(np.float32)
    recs = [_rec((0.0 if m % 4 == 3 else (0.8, 1.5)[m % 2], 0, 1.0, 0.0), SEED + m) for m in range(M)]
    assert allow.sum(1).min() == 1 and (~allow).any(1).sum() == M - 1
    drawn_banned = 0
    for k in range(3):
        draws = [(7 * m) % 23 + 31 * k for m in range(M)]
        dev = torch.from_numpy(l).repeat(M, 1).to(cuda)
        K.row_mask(dev, torch.from_numpy(bits.view(np.int32)).to(cuda), torch.ones(M, dtype=torch.int32, device=cuda))
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), masked.view(np.uint32))
        tok, _ = _run(K, cuda, dev, recs, draws)
        _check_rows(tok, lambda r: masked[r], recs, draws)
        drawn_banned += int((~allow[np.arange(M), tok]).sum())
        assert tok[5] == int(np.flatnonzero(allow[5])[0])
    assert drawn_banned == 0
    assert recs[3]["temp"] <= 0 and int(np.argmax(masked[3])) == int(np.flatnonzero(allow[3])[0])
