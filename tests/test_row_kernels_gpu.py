"""The row kernels of elementwise.hip between the GEMMs, each against a float64 / exact CPU reference
of the same operation, through bindings that are the launcher and nothing else (ops.kernels
rmsnorm_fill, rmsnorm_acc, splitk_reduce, moe_combine, swiglu, f32_to_f16, act_pack / act_unpack,
advance) plus both argmax kernels.

Conventions: references are float64 (or exact IEEE f32 adds / conversions) on the CPU; every output
buffer is larger than the kernel may write and pre-filled with a canary (NaN for floats, a fixed bit
pattern for ints) that must survive outside the documented write set; padding that must not be READ
holds NaN (or +inf for argmax), so a stray read poisons a checked value.

Bounds.  RMSNorm `out` is compared with f16(x rsqrt(mean x^2 + eps) w) evaluated in float64 and must
be within ONE f16 ulp: the kernel's f32 evaluation (sum of <= 8196 squares, rsqrt, two multiplies) is
within ~1e-6 relative of the float64 value, far inside half an f16 ulp (4.9e-4), so its f16 rounding
can differ from the reference's only where the exact value sits next to a rounding boundary -- by one
ulp.  Everything that is an ordered f32 sum or a format conversion is compared bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
NAN = float("nan")
I8_CANARY, I16_CANARY, I32_CANARY = 0x55, 0x5A5A, -0x5A5A5A5B


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _is_canary(t):
    """Every element still holds the NaN bit pattern torch.full wrote."""
    return torch.equal(_bits(t), _bits(torch.full_like(t.detach().cpu(), NAN)))


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _f16_key(t):
    """f16 -> integers in value order (adjacent representable values differ by 1, -0 == +0)."""
    b = _bits(t.to(torch.float16)).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def _ulp_diff(got, ref):
    return (_f16_key(got) - _f16_key(ref)).abs()


def _pad4(d):
    return (d + 3) // 4 * 4


def _norm_ref(x64, w, d):
    """f16(x rsqrt(mean x^2 + eps) w) in float64; x64 [M][d] float64."""
    r = x64 * torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + EPS) * w.double()
    return r.to(torch.float16)


def _rows(M, d, ld, seed):
    """x f32 [M + 1][ld]: random rows (a zero row and a large row when M > 1), NaN in the padding
    columns and in the guard row M; w f32 [d]."""
    g = torch.Generator().manual_seed(seed)
    x = _nan(M + 1, ld)
    x[:M, :d] = torch.randn(M, d, generator=g) * 3
    if M > 1:
        x[M // 2, :d] = 0.0
        x[M - 1, :d] *= 1e3
    w = torch.rand(d, generator=g) + 0.5
    return x, w


def _check_out(out, ref, M, d):
    """out f16 [M + 1][ldo] from the device: rows < M, columns < d within one f16 ulp of ref, the rest canary."""
    out = out.cpu()
    got = out[:M, :d]
    assert torch.isfinite(got.float()).all()
    diff = _ulp_diff(got, ref)
    print(f"rmsnorm M={M} d={d}: {int((diff != 0).sum())} of {diff.numel()} elements one f16 ulp off, max {int(diff.max())}")
    assert int(diff.max()) <= 1
    # no looser than the plain test's rtol = atol = 2e-3
    torch.testing.assert_close(got.float(), ref.float(), rtol=2e-3, atol=2e-3)
    assert _is_canary(out[:M, d:]), "columns [d, ldo) written"
    assert _is_canary(out[M]), "row M written"


# ---------------------------------------------------------------- RMSNorm: shapes and output
# 288: one partly used float4 slot; 4096: second slot all masked; 4104: partly used; 8192: full;
# 4098 / 8196: the scalar path (d % 4 != 0, d > 8192), launch_rmsnorm only, ldx a multiple of 4
@pytest.mark.parametrize("M", [1, 7, 130])
@pytest.mark.parametrize("d", [288, 4096, 4104, 8192, 4098, 8196])
def test_rmsnorm_shapes(cuda, native, d, M):
    from mipipe.ops import kernels as K
    ldx, ldo = _pad4(d) + 8, _pad4(d) + 12
    x, w = _rows(M, d, ldx, seed=d + M)
    ref = _norm_ref(x[:M, :d].double(), w, d)
    xd, wd = x.to(cuda), w.to(cuda)
    out = _nan(M + 1, ldo, dtype=torch.float16).to(cuda)
    K.rmsnorm_fill(xd, ldx, wd, d, EPS, out, ldo, M)
    torch.cuda.synchronize()
    _check_out(out, ref, M, d)
    assert _same_bits(xd, x), "x written by the plain form"
    if M > 1:
        assert (out[M // 2, :d] == 0).all()   # the zero row: zeros, not NaN


# ---------------------------------------------------------------- RMSNorm: zero fill / bias fill
# (5, 1): a tail shorter than a float4; (32771, 1): three fill workgroups, one row (rows >= M exist
# only to fill); (100, 7): fewer fill workgroups than rows; (0, 7): a fill pointer with nothing to fill
@pytest.mark.parametrize("acc", [False, True], ids=["launch_rmsnorm", "launch_rmsnorm_acc"])
@pytest.mark.parametrize("zero_n,M", [(0, 7), (5, 1), (16384 * 2 + 3, 1), (100, 7)])
def test_rmsnorm_zero_fill(cuda, native, zero_n, M, acc):
    from mipipe.ops import kernels as K
    d = 288
    ldx, ldo = d + 8, d + 12
    x, w = _rows(M, d, ldx, seed=zero_n + M)
    ref = _norm_ref(x[:M, :d].double(), w, d)
    xd, wd = x.to(cuda), w.to(cuda)
    out = _nan(M + 1, ldo, dtype=torch.float16).to(cuda)
    zero = _nan(zero_n + 24).to(cuda)
    if acc:
        K.rmsnorm_acc(xd, ldx, wd, d, EPS, out, ldo, M, zero=zero, zero_n=zero_n)
    else:
        K.rmsnorm_fill(xd, ldx, wd, d, EPS, out, ldo, M, zero=zero, zero_n=zero_n)
    torch.cuda.synchronize()
    z = zero.cpu()
    assert _same_bits(z[:zero_n], torch.zeros(zero_n)), "the filled range is not exactly +0"
    assert _is_canary(z[zero_n:]), "a float after zero_n was written"
    _check_out(out, ref, M, d)
    assert _same_bits(xd, x)


# M = 400: 19200 floats, two fill workgroups, and 16384 % 48 != 0 (the modulo runs across the boundary)
@pytest.mark.parametrize("acc", [False, True], ids=["launch_rmsnorm", "launch_rmsnorm_acc"])
@pytest.mark.parametrize("M", [1, 7, 400])
def test_rmsnorm_bias_fill(cuda, native, M, acc):
    from mipipe.ops import kernels as K
    d, bias_n = 288, 48
    zero_n = M * bias_n
    ldx, ldo = d + 8, d + 12
    x, w = _rows(M, d, ldx, seed=M)
    ref = _norm_ref(x[:M, :d].double(), w, d)
    g = torch.Generator().manual_seed(3)
    bias = _nan(bias_n + 8)
    bias[:bias_n] = torch.randn(bias_n, generator=g)
    bias[5] = -0.0
    xd, wd, bd = x.to(cuda), w.to(cuda), bias.to(cuda)
    out = _nan(M + 1, ldo, dtype=torch.float16).to(cuda)
    zero = _nan(zero_n + 24).to(cuda)
    fn = K.rmsnorm_acc if acc else K.rmsnorm_fill
    fn(xd, ldx, wd, d, EPS, out, ldo, M, zero=zero, zero_n=zero_n, bias=bd, bias_n=bias_n)
    torch.cuda.synchronize()
    z = zero.cpu()
    assert _same_bits(z[:zero_n], bias[:bias_n].repeat(M)), "zero[i] != bias[i % 48]"
    assert _is_canary(z[zero_n:])
    _check_out(out, ref, M, d)


# ---------------------------------------------------------------- RMSNorm: partial absorb
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("d,M", [(288, 1), (288, 7), (4104, 7), (8192, 3)])
def test_rmsnorm_absorbs_partials(cuda, native, d, M, nsplit):
    """x <- ((x + p0) + p1) + p2 in f32, written back bit for bit, and out = norm of that sum.  Rows of
    `part` beyond M, its columns beyond d and the gap between splits hold NaN: they are not read."""
    from mipipe.ops import kernels as K
    ldx, ldo, ldp = d + 8, d + 12, d + 16
    ss = (M + 2) * ldp + 8                     # > M * ldp, a multiple of 4
    x, w = _rows(M, d, ldx, seed=31 * d + M + nsplit)
    g = torch.Generator().manual_seed(d + nsplit)
    part = _nan(nsplit, ss)
    for s in range(nsplit):
        part[s, :M * ldp].view(M, ldp)[:, :d] = torch.randn(M, d, generator=g) * (s + 1)
    want_x = x[:M, :d].clone()
    for s in range(nsplit):
        want_x = want_x + part[s, :M * ldp].view(M, ldp)[:, :d]      # IEEE f32 adds, split order
    ref = _norm_ref(want_x.double(), w, d)
    xd, wd, pd = x.to(cuda), w.to(cuda), part.to(cuda)
    out = _nan(M + 1, ldo, dtype=torch.float16).to(cuda)
    K.rmsnorm_acc(xd, ldx, wd, d, EPS, out, ldo, M, part=pd, nsplit=nsplit, ss=ss, ldp=ldp)
    torch.cuda.synchronize()
    got_x = xd.cpu()
    assert _same_bits(got_x[:M, :d], want_x), "the written-back residual is not the ordered f32 sum"
    assert _is_canary(got_x[:M, d:]) and _is_canary(got_x[M]), "x written outside [M][d]"
    assert _same_bits(pd, part), "part written"
    _check_out(out, ref, M, d)


# ---------------------------------------------------------------- RMSNorm: int8 output
@pytest.mark.parametrize("absorb", [False, True])
@pytest.mark.parametrize("d", [288, 4104, 8192])
def test_rmsnorm_int8_rows(cuda, native, d, absorb):
    """q8 / q8s are bitwise what quant_rows_i8 gives for the kernel's own f16 row (the promise in the
    kernel's comment); independently s = max|out| / 127 and q = round(out / s) in float64, where the
    kernel's multiply by the f32 reciprocal may land on the other side of a .5 on a few elements: off
    by at most 1, on at most 0.1 % of them (a CPU emulation of reciprocal-vs-division measures 5e-5;
    measured on the MI355X: 5 of 176160 elements = 2.8e-5 over the six cases, worst case 3.5e-5)."""
    from mipipe.ops import kernels as K
    M = 7
    ldx, ldo, ldq, ldp = d + 8, d + 12, d + 16, d + 4
    x, w = _rows(M, d, ldx, seed=d)            # row 3 is all zero
    part, ss = None, 0
    if absorb:
        ss = (M + 1) * ldp
        part = torch.zeros(1, ss)
        part[0, :M * ldp].view(M, ldp)[:, :d] = torch.randn(M, d, generator=torch.Generator().manual_seed(1))
        part[0, :M * ldp].view(M, ldp)[M // 2] = 0.0
        part = part.to(cuda)
    xd, wd = x.to(cuda), w.to(cuda)
    out = _nan(M + 1, ldo, dtype=torch.float16).to(cuda)
    q8 = torch.full((M + 1, ldq), I8_CANARY, dtype=torch.int8).to(cuda)
    q8s = _nan(M + 4).to(cuda)
    K.rmsnorm_acc(xd, ldx, wd, d, EPS, out, ldo, M, part=part, nsplit=1 if absorb else 0, ss=ss, ldp=ldp,
                  q8=q8, ldq8=ldq, q8s=q8s)
    torch.cuda.synchronize()
    ref = _norm_ref(xd.cpu()[:M, :d].double(), w, d)
    _check_out(out, ref, M, d)
    row16 = out[:M, :d].contiguous()
    q_ref, s_ref = K.quant_rows_i8(row16)
    torch.cuda.synchronize()
    q, s = q8.cpu(), q8s.cpu()
    assert _same_bits(q[:M, :d], q_ref), "q8 differs from quant_rows_i8 of the same f16 row"
    assert _same_bits(s[:M], s_ref), "q8s differs from quant_rows_i8's scale"
    assert (q[:M, d:] == I8_CANARY).all() and (q[M] == I8_CANARY).all(), "q8 written outside [M][d]"
    assert _is_canary(s[M:])
    o64 = row16.cpu().double()
    amax = o64.abs().amax(-1)
    nz = amax > 0
    assert nz.tolist() == [r != M // 2 for r in range(M)]
    torch.testing.assert_close(s[:M][nz].double(), amax[nz] / 127.0, rtol=1e-6, atol=0.0)
    assert float(s[M // 2]) == 1.0 and (q[M // 2, :d] == 0).all()      # the all-zero row
    want = torch.from_numpy(np.rint((o64 / s[:M].double()[:, None]).numpy()))
    off = (q[:M, :d].double() - want).abs()
    share = float((off != 0).double().mean())
    print(f"rmsnorm int8 d={d} absorb={absorb}: {int((off != 0).sum())} of {off.numel()} off by one ({share:.2e})")
    assert float(off.max()) <= 1
    assert share <= 1e-3
    assert int(q[:M, :d].abs().max()) == 127


# ---------------------------------------------------------------- splitk_reduce (all four kernels)
def _splitk_case(K, cuda, n, aligned, init, nsplit, M, bias_mode):
    ldp = n + 4
    ldy = n + 8 if aligned else n + 5          # n + 5: ldy % 4 != 0 -> the one-column kernels
    ss = (M + 1) * ldp + 4
    g = torch.Generator().manual_seed(n + 7 * nsplit + M)
    part = _nan(nsplit, ss)
    for s in range(nsplit):
        p = part[s, :M * ldp].view(M, ldp)
        p[:, :n] = torch.randn(M, n, generator=g)
        p[:, 0] = -0.0                          # a sum of -0 partials: +0 from a 0.f start, -0 from the first partial
    y = _nan(M + 1, ldy)
    if not init:
        y[:M, :n] = torch.randn(M, n, generator=g)
    bias_buf = _nan(n + 8)
    off = {None: 0, "aligned": 0, "offset": 1}[bias_mode]    # offset: a 4-byte aligned bias -> the one-column kernel
    bias = bias_buf[off:off + n]
    bias[:] = torch.randn(n, generator=g)
    if init:
        acc = (bias if bias_mode else torch.zeros(n)).expand(M, n).clone()
    else:
        acc = y[:M, :n].clone()
    for s in range(nsplit):
        acc = acc + part[s, :M * ldp].view(M, ldp)[:, :n]
    yd, pd, bd = y.to(cuda), part.to(cuda), bias_buf.to(cuda)
    K.splitk_reduce(pd, nsplit, ss, ldp, M, n, yd, ldy, init=init, bias=bd[off:off + n] if bias_mode else None)
    torch.cuda.synchronize()
    got = yd.cpu()
    what = f"n={n} aligned={aligned} init={init} nsplit={nsplit} M={M} bias={bias_mode}"
    assert _same_bits(got[:M, :n], acc), "not the ordered f32 sum: " + what
    assert _is_canary(got[:M, n:]) and _is_canary(got[M]), "Y written outside [M][n]: " + what
    assert _same_bits(pd, part) and _same_bits(bd, bias_buf)


@pytest.mark.parametrize("init", [False, True])
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("n", [20, 1028])
def test_splitk_reduce(cuda, native, n, aligned, init):
    """Bitwise the ordered f32 sum from Y (accumulate) or from bias-or-0 (init, where Y starts as NaN
    to show it is not read); 1028 columns: two workgroups in the one-column kernels, a partly filled
    second one in the four-column kernels."""
    from mipipe.ops import kernels as K
    for nsplit in (1, 4):
        for M in (1, 65):
            for bias_mode in ((None, "aligned", "offset") if init else (None,)):
                _splitk_case(K, cuda, n, aligned, init, nsplit, M, bias_mode)


def test_splitk_reduce_bias_needs_init(cuda, native):
    from mipipe.ops import kernels as K
    y = _nan(2, 24).to(cuda)
    part = torch.zeros(2 * 24).to(cuda)
    bias = torch.zeros(24).to(cuda)
    with pytest.raises(RuntimeError, match="init form"):
        K.splitk_reduce(part, 1, 48, 24, 2, 20, y, 24, init=False, bias=bias)
    torch.cuda.synchronize()
    assert _is_canary(y)


def test_rmsnorm_acc_rejects_scalar_shapes(cuda, native):
    """launch_rmsnorm_acc has no scalar path: d % 4 != 0 and d > 8192 are refused, nothing is launched."""
    from mipipe.ops import kernels as K
    for d in (4098, 8196):
        x = torch.zeros(1, d + 6).to(cuda)
        w = torch.ones(d).to(cuda)
        out = _nan(1, d + 6, dtype=torch.float16).to(cuda)
        with pytest.raises(RuntimeError, match="rmsnorm_acc"):
            K.rmsnorm_acc(x, _pad4(d) + 4, w, d, EPS, out, d + 6, 1)
        torch.cuda.synchronize()
        assert _is_canary(out)


# ---------------------------------------------------------------- moe_combine
@pytest.mark.parametrize("n", [100, 2048])
@pytest.mark.parametrize("k", [1, 8])
def test_moe_combine(cuda, native, k, n):
    from mipipe.ops import kernels as K
    lds, ldy = n + 4, n + 3
    for M in (1, 33):
        g = torch.Generator().manual_seed(n + k + M)
        ys = _nan(M * k + 1, lds)
        ys[:M * k, :n] = torch.randn(M * k, n, generator=g)
        y = _nan(M + 1, ldy)
        y[:M, :n] = torch.randn(M, n, generator=g)
        acc = y[:M, :n].clone()
        for e in range(k):
            acc = acc + ys[:M * k, :n].view(M, k, n)[:, e]
        yd, sd = y.to(cuda), ys.to(cuda)
        K.moe_combine(sd, lds, k, M, n, yd, ldy)
        torch.cuda.synchronize()
        got = yd.cpu()
        assert _same_bits(got[:M, :n], acc), f"not the ordered f32 sum at M={M}"
        assert _is_canary(got[:M, n:]) and _is_canary(got[M])
        assert _same_bits(sd, ys)


# ---------------------------------------------------------------- swiglu
@pytest.mark.parametrize("F", [100, 1024])
def test_swiglu(cuda, native, F):
    """silu(g) u in float64; the products past f16's range saturate at exactly +-65504.  Elsewhere:
    test_gemv_swiglu's NMSE < 1e-5, and per element half an f16 ulp (2^-11 relative, 2^-25 absolute in
    the subnormals) plus the f32 evaluation's ~1e-6: 5e-4 |ref| + 6e-8."""
    from mipipe.ops import kernels as K
    M = 3
    ld, ldh = 2 * F + 4, F + 5
    g = torch.Generator().manual_seed(F)
    gu = _nan(M + 1, ld)
    gu[:M, :2 * F] = torch.randn(M, 2 * F, generator=g) * 3
    special = torch.tensor([-100.0, -20.0, 0.0, 20.0, 100.0])
    for m in range(M):
        gu[m, 7 * m:7 * m + 5] = special
    gu[0, F - 1], gu[0, 2 * F - 1] = 100.0, 700.0        # 70000 -> 65504
    gu[1, F - 2], gu[1, 2 * F - 2] = 100.0, -700.0       # -70000 -> -65504
    gu[2, 50], gu[2, F + 50] = 30.0, 2183.5              # 65505 (rounds to 65504 unsaturated too)
    g64, u64 = gu[:M, :F].double(), gu[:M, F:2 * F].double()
    ref = g64 * torch.sigmoid(g64) * u64
    h = _nan(M + 1, ldh, dtype=torch.float16).to(cuda)
    gd = gu.to(cuda)
    K.swiglu(gd, ld, F, M, h, ldh)
    torch.cuda.synchronize()
    got = h.cpu()
    assert _is_canary(got[:M, F:]) and _is_canary(got[M])
    assert _same_bits(gd, gu)
    v = got[:M, :F].double()
    assert torch.isfinite(v).all()
    assert float(v[0, F - 1]) == 65504.0 and float(v[1, F - 2]) == -65504.0 and float(v[2, 50]) == 65504.0
    inr = ref.abs() <= 65504.0
    assert int((~inr).sum()) == 3
    err = (v - ref).abs()[inr]
    bound = (5e-4 * ref.abs() + 6e-8)[inr]
    print(f"swiglu F={F}: max err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert float(((v - ref)[inr] ** 2).sum() / (ref[inr] ** 2).sum()) < 1e-5


# ---------------------------------------------------------------- f32 -> f16 / bf16 conversions
CONV_N = [1, 3, 1023, 1024, 4099]
# a NaN, f16 ties (65520 -> inf, 1 + 2^-11 -> 1, 1 + 3 * 2^-11 -> 1 + 2^-9, 2^-25 -> 0, 1.5 * 2^-24 -> 2^-23),
# signed zeros, f16 subnormals, an f32 subnormal, values past 65504 (inf in f16: not saturating), the
# largest f16, bf16 ties (1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6) and the f32 maximum (inf in bf16)
SPECIALS = [NAN, 65520.0, -0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 1.5 * 2.0 ** -24, 0.0, 2.0 ** -24,
            -3.0e-6, 1e-40, 70000.0, -70000.0, 65504.0, 65519.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
            3.4028234e38, -1.0 - 2.0 ** -11, float("inf")]


def _conv_input(n, seed):
    """n values: the specials at the front and (reversed) at the back, random in between."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.tensor(10.0) ** torch.randint(-8, 5, (n,), generator=g).float()
    sp = torch.tensor(SPECIALS, dtype=torch.float32)
    k = min(n, len(sp))
    x[:k] = sp[:k]
    if n >= 2 * len(sp):
        x[n - len(sp):] = sp.flip(0)
    return x


def _same_bits_or_nan(got, want):
    """Bitwise equal; where the reference is NaN any NaN will do (the payload is not part of the contract)."""
    wn = torch.isnan(want.float())
    return bool((torch.isnan(got.float()) == wn).all()) and torch.equal(_bits(got)[~wn], _bits(want)[~wn])


@pytest.mark.parametrize("n", CONV_N)
def test_f32_to_f16(cuda, native, n):
    from mipipe.ops import kernels as K
    M, ldx, ldy = 3, n + 3, n + 5
    x = _nan(M + 1, ldx)
    for m in range(M):
        x[m, :n] = _conv_input(n, 10 * n + m)
    want = x[:M, :n].to(torch.float16)           # round to nearest even
    y = torch.full((M + 1, ldy), I16_CANARY, dtype=torch.int16).to(cuda)
    K.f32_to_f16(x.to(cuda), ldx, n, M, y, ldy)
    torch.cuda.synchronize()
    got = y.cpu()
    assert _same_bits_or_nan(got[:M, :n].contiguous().view(torch.float16), want)
    assert (got[:M, n:] == I16_CANARY).all() and (got[M] == I16_CANARY).all()
    if n >= 2:
        assert torch.isinf(got[0, 1:2].view(torch.float16)).all()      # 65520 -> inf, documented


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("n", CONV_N)
def test_act_pack_unpack(cuda, native, n, dt):
    """The stage-boundary wire format: pack is torch's round-to-nearest-even conversion bit for bit,
    unpack the exact widening; element n and after are never written."""
    from mipipe.ops import kernels as K
    tdt, code = (torch.float16, K.ACT_F16) if dt == "f16" else (torch.bfloat16, K.ACT_BF16)
    x = _conv_input(n, n)
    want = x.to(tdt)
    xd = torch.cat([x, _nan(8)]).to(cuda)        # NaN behind element n: not read into a checked value
    y = torch.full((n + 8,), I16_CANARY, dtype=torch.int16).to(cuda)
    K.act_pack(xd, y, n, code)
    torch.cuda.synchronize()
    got = y.cpu()
    assert _same_bits_or_nan(got[:n].view(tdt), want)
    assert (got[n:] == I16_CANARY).all(), "pack wrote past element n"
    assert bool(torch.isnan(got[:1].view(tdt)).all())                  # the NaN stays a NaN
    # unpack the reference encoding (subnormals, infinities and the NaN included)
    yin = torch.cat([want, torch.full((8,), NAN, dtype=tdt)]).to(cuda)
    back = _nan(n + 8).to(cuda)
    K.act_unpack(yin, back, n, code)
    torch.cuda.synchronize()
    b = back.cpu()
    assert _same_bits_or_nan(b[:n], want.float())
    assert _is_canary(b[n:]), "unpack wrote past element n"


# ---------------------------------------------------------------- advance
@pytest.mark.parametrize("M", [1, 64, 65, 300, 1024])
def test_advance(cuda, native, M):
    from mipipe.ops import kernels as K
    g = torch.Generator().manual_seed(M)
    pos = torch.randint(0, 5000, (M + 8,), generator=g, dtype=torch.int32)
    kv = torch.full((M + 8,), I32_CANARY, dtype=torch.int32)
    step = torch.tensor([41, I32_CANARY], dtype=torch.int32)
    pd, kd, sd = pos.to(cuda), kv.to(cuda), step.to(cuda)
    K.advance(pd, kd, M, sd)
    torch.cuda.synchronize()
    assert torch.equal(pd.cpu()[:M], pos[:M] + 1) and torch.equal(kd.cpu()[:M], pos[:M] + 2)
    assert torch.equal(pd.cpu()[M:], pos[M:]) and (kd.cpu()[M:] == I32_CANARY).all(), "rows >= M written"
    assert sd.cpu().tolist() == [42, I32_CANARY], "step advances exactly once"
    K.advance(pd, kd, M, None)                  # no step counter: rows advance, the counter does not
    torch.cuda.synchronize()
    assert torch.equal(pd.cpu()[:M], pos[:M] + 2) and torch.equal(kd.cpu()[:M], pos[:M] + 3)
    assert torch.equal(pd.cpu()[M:], pos[M:]) and (kd.cpu()[M:] == I32_CANARY).all()
    assert sd.cpu().tolist() == [42, I32_CANARY]


# ---------------------------------------------------------------- argmax, both kernels, and sample(temp = 0)
def _argmax_chunk(n):
    """Columns per workgroup of the two-level kernel: launch_argmax's arithmetic."""
    from mipipe.ops.kernels import ARGMAX_CHUNKS
    nchunk = min(max((n + 2047) // 2048, 1), ARGMAX_CHUNKS)
    return ((n + nchunk - 1) // nchunk + 3) & ~3


def _argmax_rows(n, ld, M, seed):
    """logits [M][ld] (+inf in the padding columns) and the expected token per row.  Rows 0-7: the
    maximum at 0, at n - 1, on either side of the first argmax2 chunk boundary, a tie across two chunks
    (lowest index wins), a row with NaNs, all -inf, all NaN; then random rows.
    The reference of a row with NaNs is the argmax over its comparable values (a NaN compares false
    against everything, so no kernel can select it); a row with no comparable maximum gives token 0."""
    chunk = _argmax_chunk(n)
    g = torch.Generator().manual_seed(seed)
    x = torch.full((M, ld), float("inf"))
    x[:, :n] = torch.randn(M, n, generator=g)
    lo, hi = (chunk - 1, chunk) if chunk < n else (n // 2, n // 2 + 1)
    x[0, 0] = 50.0
    x[1, n - 1] = 50.0
    x[2, lo] = 50.0
    x[3, hi] = 50.0
    a, b = (chunk // 2, chunk + 3) if chunk + 3 < n else (1, n - 1)
    x[4, a] = x[4, b] = 50.0
    x[5, 0] = x[5, n - 1] = x[5, n // 3] = NAN
    x[5, n // 2] = 50.0
    x[5, n // 2 - 1] = NAN
    x[6, :n] = float("-inf")
    x[7, :n] = NAN
    v = x[:, :n].numpy().copy()
    v[np.isnan(v)] = -np.inf
    want = np.where(np.isinf(v.max(-1)) & (v.max(-1) < 0), 0, v.argmax(-1))      # numpy: first occurrence
    assert want[:8].tolist() == [0, n - 1, lo, hi, a, n // 2, 0, 0]
    return x, want.astype(np.int64)


@pytest.mark.parametrize("pad", [0, 3], ids=["ld=n", "ld=n+3"])
@pytest.mark.parametrize("n", [5, 2047, 2049, 128256])
def test_argmax_kernels(cuda, native, n, pad):
    """One-level kernel on M = 70 rows, two-level kernel three rows at a time (its wrapper asserts the
    arrival counters are back at 0), greedy sampling on the same rows.  Only the returned ids are read."""
    from mipipe.ops import kernels as K
    M = 70
    x, want = _argmax_rows(n, n + pad, M, seed=n + pad)
    xd = x.to(cuda)[:, :n]                       # shape [M][n], row stride n + pad
    got = {"one-level": K.argmax(xd, two_level=False).cpu().tolist(),
           "two-level": sum((K.argmax(xd[r0:r0 + 3], two_level=True).cpu().tolist() for r0 in range(0, 9, 3)), []),
           "sample(temp=0)": K.sample(xd, temp=0.0).cpu().tolist()}
    # rows 6 and 7 (no comparable maximum) must come out as token 0, inside [0, n), on all three paths
    bad = {name: [(r, t) for r, (t, w) in enumerate(zip(toks, want.tolist())) if t != w] for name, toks in got.items()}
    assert not any(bad.values()), f"(row, token) pairs that differ from the reference: {bad}"
    assert len(got["two-level"]) == 9 and len(got["one-level"]) == len(got["sample(temp=0)"]) == M
