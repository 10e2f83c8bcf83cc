"""Qwen3 per-head Q/K RMSNorm kernel (`ops.kernels.qk_norm`, elementwise.hip qk_norm_kernel)
against an fp64 torch evaluation of the same f32 inputs.

Bound: |out - ref| <= 1e-5 |ref| + 1e-12 per element.  It is derived, not measured: an f32 sum of
at most 128 squares has relative error <= 129 * 2^-24 ~ 7.7e-6, the rsqrt halves that, and the
hardware rsqrt plus two multiplies add a few 2^-24: below 5e-6 in total."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-6
PAD = 24
# (hd, Hq, Hkv, M): one row; 9 heads (partly filled last workgroup); one element per lane; lanes
# masked in the second half with 6 heads
CASES = [(128, 8, 2, 1), (128, 6, 3, 37), (64, 4, 4, 3), (96, 5, 1, 17)]


def _inputs(hd, Hq, Hkv, M, seed):
    """qkv [M + 1][ld] f32 (row M is the guard row), wq, wk: on the CPU"""
    g = torch.Generator().manual_seed(seed)
    ld = (Hq + 2 * Hkv) * hd + PAD
    qkv = torch.randn(M + 1, ld, generator=g, dtype=torch.float32)
    if M > 1:                    # (a single row stays plain random)
        qkv[0] = 0.0             # the zero row
        qkv[M - 1] *= 1e3        # a row of large values
    wq = torch.rand(hd, generator=g, dtype=torch.float32) * 1.5 + 0.5
    wk = torch.rand(hd, generator=g, dtype=torch.float32) * 1.5 + 0.5
    return qkv, wq, wk


def _oracle(qkv, wq, wk, hd, Hq, Hkv, M):
    x = qkv[:M].double()
    out = x.clone()
    for H, off, w in ((Hq, 0, wq), (Hkv, Hq * hd, wk)):
        h = x[:, off:off + H * hd].reshape(M, H, hd)
        h = h * torch.rsqrt((h * h).mean(-1, keepdim=True) + EPS) * w.double()
        out[:, off:off + H * hd] = h.reshape(M, H * hd)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("hd,Hq,Hkv,M", CASES)
def test_qk_norm_matches_fp64_oracle(cuda, native, hd, Hq, Hkv, M):
    from mipipe.ops import kernels as K
    qkv, wq, wk = _inputs(hd, Hq, Hkv, M, seed=hd + M)
    ref = _oracle(qkv, wq, wk, hd, Hq, Hkv, M)
    buf = qkv.to(cuda)
    # the op sees M rows of the (M + 1)-row buffer: the last row is the guard
    got = K.qk_norm(buf[:M], wq.to(cuda), wk.to(cuda), Hq, Hkv, hd, EPS)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()   # in place
    out = buf.cpu()
    nqk = (Hq + Hkv) * hd
    o, r = out[:M, :nqk].double(), ref[:, :nqk]
    assert torch.isfinite(o).all()
    err = (o - r).abs()
    bound = 1e-5 * r.abs() + 1e-12
    worst = float((err / (r.abs() + 1e-30)).max())
    print(f"qk_norm hd={hd} Hq={Hq} Hkv={Hkv} M={M}: max rel err {worst:.3e}")
    assert (err <= bound).all(), worst
    # the zero row: exact zeros, not NaN
    if M > 1:
        assert (out[0, :nqk] == 0).all()
    # v columns, the padding and the guard row keep their bits
    assert torch.equal(_bits(out[:M, nqk:]), _bits(qkv[:M, nqk:]))
    assert torch.equal(_bits(out[M]), _bits(qkv[M]))
    # the norm did something (weights 0.5 .. 2, unit-variance input)
    assert not torch.equal(out[M // 2, :nqk], qkv[M // 2, :nqk])


@pytest.mark.parametrize("hd,Hq,Hkv,M", CASES)
def test_qk_norm_graph_replay_bitwise(cuda, native, hd, Hq, Hkv, M):
    from mipipe.ops import kernels as K
    qkv, wq, wk = _inputs(hd, Hq, Hkv, M, seed=7 * hd + M)
    wq_d, wk_d = wq.to(cuda), wk.to(cuda)
    eager = qkv.to(cuda)
    K.qk_norm(eager[:M], wq_d, wk_d, Hq, Hkv, hd, EPS)
    torch.cuda.synchronize()
    buf = qkv.to(cuda)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K.qk_norm(buf[:M], wq_d, wk_d, Hq, Hkv, hd, EPS)   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    buf.copy_(qkv)
    with torch.cuda.graph(g):
        K.qk_norm(buf[:M], wq_d, wk_d, Hq, Hkv, hd, EPS)
    for _ in range(2):
        buf.copy_(qkv)            # a fresh copy of the input
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(buf.cpu()), _bits(eager.cpu()))


@pytest.mark.parametrize("hd", [130, 256, 63, 0])
def test_qk_norm_rejects_bad_head_dim(cuda, native, hd):
    from mipipe.ops import kernels as K
    qkv = torch.zeros(2, 4 * max(hd, 1) + PAD, dtype=torch.float32, device=cuda)
    w = torch.ones(max(hd, 1), dtype=torch.float32, device=cuda)
    with pytest.raises(RuntimeError, match="qk_norm"):
        K.qk_norm(qkv, w, w, 2, 1, hd, EPS)
