"""The gemm4 epilogues (csrc/kernels/gemm4_kernel.h) element by element: the 16-byte store paths of
the dense STORE and SwiGLU epilogues, their element-store fallbacks (a misaligned base or row
stride) and the guards (rows >= M, columns / outputs >= n_valid, a 4-column or 8-output group that
straddles n_valid).

Every GEMM result here is exact in f32: Q8_0 weights k * 2^-10 with integer k (|k| <= 127, +-127
in every 32-block, so the block scale is 2^-10 and the quants are k), x small integers, and sums
far below 2^24 units of 2^-10.  A single misplaced element is then an inequality, not a small NMSE.
The outputs are slices of NaN-filled tensors: everything the kernel must not write stays NaN."""
import numpy as np
import pytest
import torch

from mipipe.utils import quants as Q

pytestmark = pytest.mark.gpu

N, K, K_SPLIT = 208, 1280, 2048   # 13 tiles: a partial 256-column (and 224-column) group
ROWS = [65, 129, 300]
# (row tile through set_gemm3_tuning, knobs): every dense geometry the plan can name at these shapes
FORMS = [(0, {}), (96, {}), (128, {}), (256, {}),
         (0, {"GEMM4_TW4": 1}), (0, {"GEMM4_TW4": 2}), (128, {"GEMM4_TW4": 2}), (0, {"GEMM4_TW4": 4}),
         (128, {"GEMM4_NW": 4}), (128, {"GEMM4_NW": 7}), (256, {"GEMM4_NW": 7, "GEMM4_TW4": 0}),
         (0, {"GEMM4_NW": 7, "GEMM4_TW4": 4})]
FORM_IDS = ["bm%d%s" % (bm, "".join("-%s%d" % (k[6:], v) for k, v in kn.items())) for bm, kn in FORMS]


def _int_weights(n, k, seed):
    """W[n][k] = q * 2^-10, integer |q| <= 127, both +127 and -127 in every 32-block."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-127, 128, (n, k)).astype(np.float32)
    q[:, 0::32] = 127.0
    q[:, 1::32] = -127.0
    w = q * np.float32(2.0 ** -10)
    raw = Q.quantize(w, Q.Q8_0)
    assert np.array_equal(Q.dequantize(raw, Q.Q8_0).reshape(n, k), w)   # precondition: the data is exact
    return raw, torch.from_numpy(w)


def _int_x(M, k, k_pad, seed):
    g = torch.Generator().manual_seed(seed)
    xh = torch.zeros(M, k_pad, dtype=torch.float16)
    xh[:, :k] = torch.randint(-2, 3, (M, k), generator=g).half()
    return xh


class _Case:
    def __init__(self, k, seed):
        from mipipe.ops.kernels import PackedWeight
        raw, w = _int_weights(N, k, seed)
        self.w = PackedWeight(raw, Q.Q8_0, N, k)
        self.x, self.ref = {}, {}
        for M in ROWS:
            xh = _int_x(M, k, self.w.k_pad, seed + M)
            r64 = xh[:, :k].double() @ w.double().T
            assert float(r64.abs().max()) * 1024 < 2 ** 24   # exact in f32
            self.x[M] = xh.cuda()
            self.ref[M] = r64.float()
            assert torch.equal(self.ref[M].double(), r64)


@pytest.fixture(scope="module")
def case(cuda, native):
    return _Case(K, 11)


@pytest.fixture(scope="module")
def case_split(cuda, native):
    return _Case(K_SPLIT, 12)


@pytest.fixture
def form(native, request):
    from mipipe import _native as Nv
    from mipipe.ops.kernels import set_gemm3_tuning
    bm, knobs = request.param
    try:
        set_gemm3_tuning(bm, 0, 0, 0)
        for name, v in knobs.items():
            Nv.check(native.mp_set_knob(name.encode(), v), "knob")
        yield request.param
    finally:
        set_gemm3_tuning(0, 0, 0, 0)
        for name in ("GEMM4_TW4", "GEMM4_NW"):
            native.mp_reset_knob(name.encode())


def _check_slice(buf, sl, n_valid, want):
    """buf (on the GPU) holds `want` in columns sl[:n_valid] and NaN everywhere else."""
    exp = torch.full(buf.shape, float("nan"), dtype=want.dtype)
    exp[:, sl][:, :n_valid] = want[:, :n_valid]
    got = buf.cpu()
    mask = torch.isnan(exp)
    assert torch.equal(torch.isnan(got), mask), "written outside the valid slice (or a hole inside it)"
    return got[~mask], exp[~mask]


# (buffer columns, first column of the slice): contiguous; 16-B aligned with ldy != n; base off by one
# float; ldy % 4 != 0
Y_PLACES = [(N, 0), (256, 16), (256, 1), (211, 0)]


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS, indirect=True)
def test_store_exact(case, form, M):
    from mipipe.ops.kernels import gemm, EPI_STORE
    for cols, c0 in Y_PLACES:
        for n_valid in (208, 206, 203):
            buf = torch.full((M, cols), float("nan"), dtype=torch.float32, device="cuda")
            gemm(case.w, case.x[M], EPI_STORE, y=buf[:, c0:c0 + N], n_valid=n_valid, v=4)
            got, exp = _check_slice(buf, slice(c0, c0 + N), n_valid, case.ref[M])
            assert torch.equal(got, exp), (cols, c0, n_valid, int((got != exp).sum()))


@pytest.mark.parametrize("M", ROWS)
def test_splitk_partials_exact(case_split, native, M):
    """Split-K partial stores (the 16-B store path into the scratch) + the fixed-order reduction onto
    an integer base: exact, and the same bits run to run."""
    from mipipe.ops.kernels import gemm_splitk
    g = torch.Generator().manual_seed(5 + M)
    base = torch.randint(-8, 9, (M, N), generator=g).float()
    outs = []
    for _ in range(2):
        y = base.clone().cuda()
        ns = gemm_splitk(case_split.w, case_split.x[M], y)
        assert ns >= 2, ns
        outs.append(y.cpu())
    assert torch.equal(outs[0], base + case_split.ref[M])
    assert torch.equal(outs[0], outs[1])


def _f16_order(t):
    """f16 -> integers in value order (adjacent floats differ by 1; +0 and -0 coincide)."""
    b = t.view(torch.int16).to(torch.int32)
    mag = b & 0x7FFF
    return torch.where(b < 0, -mag, mag)


# (buffer columns, first column of the slice): 16-B aligned; ldh % 8 != 0; base off by one element
H_PLACES = [(128, 8), (109, 0), (128, 1)]


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS, indirect=True)
def test_swiglu_exact(case, form, M):
    """h = f16(silu(g) * u) from the exact g and u; one f16 ulp for the device's exp."""
    from mipipe.ops.kernels import gemm, EPI_SWIGLU
    F = N // 2
    gi = torch.tensor([16 * (o // 8) + (o % 8) for o in range(F)])
    g, u = case.ref[M][:, gi], case.ref[M][:, gi + 8]
    prod = torch.nn.functional.silu(g) * u
    assert float(prod.abs().max()) < 6e3   # far below the f16 range
    href = prod.half()
    for cols, c0 in H_PLACES:
        for n_valid in (104, 100):
            buf = torch.full((M, cols), float("nan"), dtype=torch.float16, device="cuda")
            gemm(case.w, case.x[M], EPI_SWIGLU, y=buf[:, c0:c0 + F], n_valid=n_valid, v=4)
            got, exp = _check_slice(buf, slice(c0, c0 + F), n_valid, href)
            d = (_f16_order(got) - _f16_order(exp)).abs()
            assert int(d.max()) <= 1, (cols, c0, n_valid, int((d > 1).sum()), int(d.max()))
