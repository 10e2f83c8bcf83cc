"""Thin torch wrappers over the HIP kernels (used by the T1 kernel tests and tools).

Every op launches the hand-written gfx950 kernel on torch's current HIP stream.  There is no
PyTorch fallback: if `libmipipe.so` is missing the import of the library raises.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _native as N
from ..utils import quants as Q

EPI_STORE, EPI_ATOMIC, EPI_SWIGLU = 0, 1, 2
P_F16, P_Q8_0, P_Q4_K, P_Q5_K, P_Q6_K, P_Q4_0, P_BF16, P_I8 = 0, 1, 2, 3, 4, 5, 6, 7
P_Q3_K, P_Q2_K = 8, 9
P_Q5_0, P_Q5_1, P_IQ4_NL, P_IQ4_XS = 10, 11, 12, 13


def _ptr(t: torch.Tensor | None):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def pack_type(ggml_type: int) -> int:
    return N.lib().mp_pack_type(ggml_type)


def packed_dims(ggml_type: int, n: int, k: int):
    n_pad = (n + 15) // 16 * 16
    k_pad = (k + 255) // 256 * 256
    return n_pad, k_pad, n_pad // 16, k_pad // 256


def pack_t16(raw: np.ndarray, ggml_type: int, n: int, k: int, gateup: bool = False) -> np.ndarray:
    """Pack a GGUF-native [n][k] tensor (bytes) into the T16 device layout (host, C++ packer)."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    nbytes = N.lib().mp_packed_bytes(ggml_type, n, k)
    out = np.empty(nbytes, np.uint8)
    rb = Q.row_bytes(ggml_type, k)
    N.check(N.lib().mp_pack_t16(ggml_type, n, k, raw.ctypes.data, rb, out.ctypes.data, int(gateup)), "pack_t16")
    return out


class PackedWeight:
    """A T16-packed weight resident on the GPU."""

    def __init__(self, raw: np.ndarray, ggml_type: int, n: int, k: int, device="cuda", gateup=False):
        self.ggml_type, self.n, self.k = ggml_type, n, k
        self.ptype = pack_type(ggml_type)
        self.n_pad, self.k_pad, self.ntiles, self.nsb = packed_dims(ggml_type, n, k)
        self.host = pack_t16(raw, ggml_type, n, k, gateup)
        self.dev = torch.from_numpy(self.host).to(device)

    @classmethod
    def random(cls, ggml_type: int, n: int, k: int, seed: int = 0, scale: float | None = None, device="cuda"):
        """Random-init blocks of the type generated on the device (mp_init_packed, the synthetic
        models' weights): no host copy."""
        self = cls.__new__(cls)
        self.ggml_type, self.n, self.k = ggml_type, n, k
        self.ptype = pack_type(ggml_type)
        self.n_pad, self.k_pad, self.ntiles, self.nsb = packed_dims(ggml_type, n, k)
        self.host = None
        nbytes = N.lib().mp_packed_bytes(ggml_type, n, k)
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        N.check(N.lib().mp_init_packed(_ptr(self.dev), nbytes, self.ptype, scale if scale else 1.0 / k ** 0.5, seed,
                                       _stream()), "init_packed")
        return self

    def unpack(self) -> torch.Tensor:
        out = torch.zeros(self.n_pad, self.k_pad, dtype=torch.float16, device=self.dev.device)
        N.check(N.lib().mp_op_unpack(self.ptype, _ptr(self.dev), self.ntiles, self.nsb, _ptr(out), self.k_pad,
                                     _stream()), "unpack")
        return out[: self.n, : self.k]


def gemv(w: PackedWeight, x: torch.Tensor, epi: int = EPI_STORE, y: torch.Tensor | None = None,
         nsplit: int = 1, n_valid: int | None = None) -> torch.Tensor:
    """x: f16 [M][K_pad] (zero tail). Returns f32 [M][n] (STORE/ATOMIC) or f16 [M][n/2] (SWIGLU)."""
    assert x.dtype == torch.float16 and x.shape[1] == w.k_pad and x.is_contiguous()
    M = x.shape[0]
    if epi == EPI_SWIGLU:
        F = w.n // 2
        h = torch.zeros(M, F, dtype=torch.float16, device=x.device) if y is None else y
        N.check(N.lib().mp_op_gemv(w.ptype, epi, _ptr(w.dev), w.ntiles, w.nsb, _ptr(x), w.k_pad, M, None, 0,
                                   _ptr(h), h.stride(0), F if n_valid is None else n_valid, 1, _stream()), "gemv")
        return h
    if y is None:
        y = torch.zeros(M, w.n, dtype=torch.float32, device=x.device)
    N.check(N.lib().mp_op_gemv(w.ptype, epi, _ptr(w.dev), w.ntiles, w.nsb, _ptr(x), w.k_pad, M, _ptr(y),
                               y.stride(0), None, 0, w.n if n_valid is None else n_valid, nsplit, _stream()),
            "gemv")
    return y


def gemv_small(w: PackedWeight, epi: int = EPI_STORE, *, x: torch.Tensor | None = None,
               xf: torch.Tensor | None = None, gamma: torch.Tensor | None = None, eps: float = 1e-5,
               bias: torch.Tensor | None = None, y: torch.Tensor | None = None, G: int = 0, nsplit: int = 0,
               deterministic: bool = False) -> torch.Tensor:
    """Small-M decode GEMV (gemvs.hip, M <= 4), the engine's single-stream path.
    xf/gamma: fused RMSNorm -- the GEMV runs on f16(xf * rsqrt(mean(xf^2) + eps) * gamma), the
    standalone rmsnorm kernel's rounding.  ATOMIC adds into `y`.  G (tiles per workgroup) and nsplit
    (k-splits over the grid, ATOMIC only) override the launcher's plan (0 = auto)."""
    if xf is not None:
        assert xf.dtype == torch.float32 and xf.is_contiguous()
        M, d = xf.shape
    else:
        assert x.dtype == torch.float16 and x.shape[1] == w.k_pad and x.is_contiguous()
        M, d = x.shape[0], 0
    F = w.n // 2
    if epi == EPI_SWIGLU:
        h = torch.zeros(M, F, dtype=torch.float16, device=w.dev.device) if y is None else y
        Y, ldy, H, ldh, nv = None, 0, h, h.stride(0), F
    else:
        y = torch.zeros(M, w.n, dtype=torch.float32, device=w.dev.device) if y is None else y
        Y, ldy, H, ldh, nv = y, y.stride(0), None, 0, w.n
    N.check(N.lib().mp_op_gemvs(w.ptype, epi, _ptr(w.dev), w.ntiles, w.nsb, _ptr(x), w.k_pad if x is not None else 0,
                                M, _ptr(Y), ldy, _ptr(H), ldh, nv, _ptr(xf), d, _ptr(gamma), eps, d, _ptr(bias),
                                G, nsplit, int(deterministic), _stream()), "gemv_small")
    return h if epi == EPI_SWIGLU else y


def gemm(w: PackedWeight, x: torch.Tensor, epi: int = EPI_STORE, y: torch.Tensor | None = None,
         n_valid: int | None = None, v: int = 3, allow_split: bool = True) -> torch.Tensor:
    """Prefill / wide-decode GEMM (any M): x f16 [M][K_pad]. Same outputs as gemv (ATOMIC adds).
    v=3: BM x BN in {128, 256}^2 workgroup tiles, weights dequantized once per workgroup into LDS
    (launch_gemm3; ATOMIC may split K over workgroups unless allow_split is False); v=4: the 32x32x16
    MFMA GEMM (launch_gemm4); v=1: the 64 x 64 tile GEMM.  (v=2, the 128-row form of the decode GEMV,
    is retired.)"""
    assert x.dtype == torch.float16 and x.shape[1] == w.k_pad and x.is_contiguous()
    M = x.shape[0]
    L = N.lib()
    if v == 3:
        fn = lambda *a: L.mp_op_gemm3(*a[:-1], int(allow_split), a[-1])
    elif v == 4:
        fn = lambda *a: L.mp_op_gemm4(*a[:-1], int(allow_split), a[-1])
    else:
        assert v == 1, "gemm: v must be 1, 3 or 4 (the v=2 form is retired)"
        fn = L.mp_op_gemm
    if epi == EPI_SWIGLU:
        F = w.n // 2
        h = torch.zeros(M, F, dtype=torch.float16, device=x.device) if y is None else y
        N.check(fn(w.ptype, epi, _ptr(w.dev), w.ntiles, w.nsb, _ptr(x), w.k_pad, M, None, 0,
                   _ptr(h), h.stride(0), F if n_valid is None else n_valid, _stream()), "gemm")
        return h
    if y is None:
        y = torch.zeros(M, w.n, dtype=torch.float32, device=x.device)
    N.check(fn(w.ptype, epi, _ptr(w.dev), w.ntiles, w.nsb, _ptr(x), w.k_pad, M, _ptr(y),
               y.stride(0), None, 0, w.n if n_valid is None else n_valid, _stream()), "gemm")
    return y


def gemm_splitk(w: PackedWeight, x: torch.Tensor, y: torch.Tensor, v: int = 4, max_splits: int = 16) -> int:
    """Split-K through per-split partial stores and the fixed-order reduction added into y (the
    engine's wide-decode path for qkv / o / down, gemm_splitk_store); returns the split count (0:
    the shape did not split, y untouched).  The scratch starts as NaN, so a partial element the
    kernel never writes poisons y instead of reading as a plausible value."""
    assert x.dtype == torch.float16 and x.shape[1] == w.k_pad and x.is_contiguous() and v == 4
    M = x.shape[0]
    scratch = torch.full((max_splits * M * w.ntiles * 16,), float("nan"), dtype=torch.float32, device=x.device)
    return N.check(N.lib().mp_op_gemm4_splitk(w.ptype, _ptr(w.dev), w.ntiles, w.nsb, _ptr(x), w.k_pad, M, _ptr(y),
                                               y.stride(0), w.n, _ptr(scratch), scratch.numel(), _stream()),
                   "gemm_splitk")


def moe_route(logits: torch.Tensor, k: int, list_cap: int | None = None):
    """Top-k routing of router logits [M][E] (f32, contiguous): returns (counts [E], lists [E][list_cap]
    of token-slot ids t * k + j, renormalised top-k weights [M * k])."""
    M, E = logits.shape
    list_cap = list_cap or M * k
    counts = torch.zeros(E, dtype=torch.int32, device=logits.device)
    lists = torch.full((E, list_cap), -1, dtype=torch.int32, device=logits.device)
    weights = torch.zeros(M * k, dtype=torch.float32, device=logits.device)
    N.check(N.lib().mp_op_moe_route(_ptr(logits), logits.stride(0), M, E, k, _ptr(counts), _ptr(lists), list_cap,
                                    _ptr(weights), _stream()), "moe_route")
    return counts, lists, weights


def moe_gemm(w_dev: torch.Tensor, estride: int, ptype: int, ntiles: int, nsb: int, n_valid: int, epi: int,
             x: torch.Tensor, M: int, E: int, k: int, counts, lists, weights=None, *, x_per_slot: bool = False,
             h: torch.Tensor | None = None, y: torch.Tensor | None = None) -> None:
    """Grouped expert GEMM (gemm4 MoE mode, K13) over E packed matrices estride bytes apart:
    EPI_SWIGLU writes h[slot] = SwiGLU(x[slot // k] W_e^T) for every routed slot; EPI_ATOMIC adds
    weights[slot] * (x[slot] W_e^T) into y[slot // k] (x_per_slot: x rows are slots)."""
    assert x.dtype == torch.float16 and x.is_contiguous()
    N.check(N.lib().mp_op_moe_gemm4(ptype, epi, _ptr(w_dev), estride, ntiles, nsb, _ptr(x), x.stride(0),
                                    int(x_per_slot), M, E, k, _ptr(counts), _ptr(lists), lists.shape[1],
                                    _ptr(weights), _ptr(y), y.stride(0) if y is not None else 0, _ptr(h),
                                    h.stride(0) if h is not None else 0, n_valid, _stream()), "moe_gemm4")


def moe_gemv(w_dev: torch.Tensor, estride: int, ptype: int, ntiles: int, nsb: int, n_valid: int, epi: int,
             x: torch.Tensor, M: int, E: int, k: int, counts, lists, weights=None, *, x_per_slot: bool = False,
             h: torch.Tensor | None = None, y: torch.Tensor | None = None, nsplit: int = 1) -> None:
    """Grouped expert GEMV (the decode route of the stages, M <= 64 tokens per call on the
    workgroup-shared kernel); operands as moe_gemm, `nsplit` K splits for the EPI_ATOMIC epilogue."""
    assert x.dtype == torch.float16 and x.is_contiguous()
    N.check(N.lib().mp_op_moe_gemv(ptype, epi, _ptr(w_dev), estride, ntiles, nsb, _ptr(x), x.stride(0),
                                   int(x_per_slot), M, E, k, _ptr(counts), _ptr(lists), lists.shape[1],
                                   _ptr(weights), _ptr(y), y.stride(0) if y is not None else 0, _ptr(h),
                                   h.stride(0) if h is not None else 0, n_valid, nsplit, _stream()), "moe_gemv")


def router_logits(x: torch.Tensor, r_dense: torch.Tensor) -> torch.Tensor:
    """logits [M][E] f32 = x [M][K] f16 . r_dense [E][K]^T (the dense-router kernel, E <= 64)."""
    M, K = x.shape[0], r_dense.shape[1]
    E = r_dense.shape[0]
    out = torch.zeros(M, 64, dtype=torch.float32, device=x.device)
    N.check(N.lib().mp_op_router_logits(_ptr(x), x.stride(0), _ptr(r_dense.contiguous()), K, E, M, _ptr(out), 64,
                                        _stream()), "router_logits")
    return out[:, :E]


def moe_router(x: torch.Tensor, r_dense: torch.Tensor, k: int, *, ld: int | None = None, list_cap: int | None = None,
               logits: torch.Tensor | None = None, lists: torch.Tensor | None = None):
    """Fused router for up to 128 experts: x [M][K] f16 and the dense f16 router r_dense [E][K] ->
    (logits [M][ld] f32, counts [E], lists [E][list_cap] of slot ids t * k + j, weights [M * k]).
    `logits` / `lists` may be passed pre-filled (the kernel leaves columns >= E and the list tails
    untouched); otherwise the padding columns are 0 and the list tails -1."""
    assert x.dtype == torch.float16 and r_dense.dtype == torch.float16 and x.stride(1) == 1
    M, (E, K) = x.shape[0], r_dense.shape
    r_dense = r_dense.contiguous()
    if logits is None:
        logits = torch.zeros(M, ld or (E + 63) // 64 * 64, dtype=torch.float32, device=x.device)
    if lists is None:
        lists = torch.full((E, list_cap or M * k), -1, dtype=torch.int32, device=x.device)
    counts = torch.zeros(E, dtype=torch.int32, device=x.device)
    weights = torch.zeros(M * k, dtype=torch.float32, device=x.device)
    sel = torch.zeros(M * k, dtype=torch.int32, device=x.device)
    N.check(N.lib().mp_op_moe_router(_ptr(x), x.stride(0), _ptr(r_dense), K, E, M, k, _ptr(logits), logits.stride(0),
                                     _ptr(counts), _ptr(lists), lists.stride(0), _ptr(weights), _ptr(sel), _stream()),
            "moe_router")
    return logits, counts, lists, weights


class I8Weight:
    """Per-row int8 re-quantization of a packed weight for the int8-activation GEMM prototype
    (SURVEY K15): w8[n][k] = round(w[n][k] / ws[n]), ws[n] = max_k |w[n][k]| / 127, packed into P_I8
    chunks (csrc/kernels/gemm3.hip W3<P_I8>: byte ((2 st + kk) * 64 + 16 g + r) * 16 + j of chunk
    (tile t, super-block sb) is row 16 t + r, k = 256 sb + 128 st + 64 kk + 16 g + j)."""

    ptype = P_I8

    def __init__(self, w: PackedWeight):
        dense = w.unpack().float()
        n, k = dense.shape
        self.n, self.k, self.n_pad, self.k_pad, self.ntiles, self.nsb = n, k, w.n_pad, w.k_pad, w.ntiles, w.nsb
        ws = dense.abs().amax(1).clamp_min(1e-30) / 127.0
        q = torch.zeros(self.n_pad, self.k_pad, dtype=torch.int8, device=dense.device)
        q[:n, :k] = torch.round(dense / ws[:, None]).clamp(-127, 127).to(torch.int8)
        self.ws = torch.ones(self.n_pad, dtype=torch.float32, device=dense.device)
        self.ws[:n] = ws
        self.q = q
        v = q.view(self.ntiles, 16, self.nsb, 2, 2, 4, 16)           # t, r, sb, st, kk, g, j
        self.dev = v.permute(0, 2, 3, 4, 5, 1, 6).contiguous().view(-1)   # t, sb, st, kk, g, r, j


def quant_rows_i8(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """f16 [M][K] -> (int8 [M][K], f32 row scales [M]): q = round(x / s), s = max|x| / 127 per row."""
    assert x.dtype == torch.float16 and x.is_contiguous()
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.int8, device=x.device)
    xs = torch.empty(M, dtype=torch.float32, device=x.device)
    N.check(N.lib().mp_op_quant_i8(_ptr(x), K, M, K, _ptr(q), K, _ptr(xs), _stream()), "quant_i8")
    return q, xs


def gemm_i8(w: I8Weight, x: torch.Tensor | None = None, epi: int = EPI_STORE, y: torch.Tensor | None = None,
            xq: tuple[torch.Tensor, torch.Tensor] | None = None, allow_split: bool = True) -> torch.Tensor:
    """int8-activation GEMM prototype: x f16 [M][K_pad] quantized per row (or xq = quant_rows_i8(x)
    given), v_mfma_i32_16x16x64_i8 against I8Weight, y = xs[m] ws[n] sum_k xq wq (exact int32 sums)."""
    q, xs = xq if xq is not None else quant_rows_i8(x)
    assert q.shape[1] == w.k_pad
    M = q.shape[0]
    L = N.lib()
    if epi == EPI_SWIGLU:
        F = w.n // 2
        h = torch.zeros(M, F, dtype=torch.float16, device=q.device) if y is None else y
        N.check(L.mp_op_gemm3_i8(epi, _ptr(w.dev), w.ntiles, w.nsb, _ptr(q), w.k_pad, M, None, 0, _ptr(h), h.stride(0),
                                 F, _ptr(xs), _ptr(w.ws), int(allow_split), _stream()), "gemm_i8")
        return h
    if y is None:
        y = torch.zeros(M, w.n, dtype=torch.float32, device=q.device)
    N.check(L.mp_op_gemm3_i8(epi, _ptr(w.dev), w.ntiles, w.nsb, _ptr(q), w.k_pad, M, _ptr(y), y.stride(0), None, 0,
                             w.n, _ptr(xs), _ptr(w.ws), int(allow_split), _stream()), "gemm_i8")
    return y


def set_gemm3_tuning(bm: int = 0, bn: int = 0, nsplit: int = 0, split_wg: int = 0) -> None:
    """Force the v3 GEMM's tile rows / columns (128 | 256) and ATOMIC split-K factor (0 = auto);
    split_wg: workgroup target of the automatic split.  0 restores a knob to the process's own value
    (its MIPIPE_* environment variable, else the default)."""
    N.check(N.lib().mp_set_gemm3_tuning(bm, bn, nsplit, split_wg), "set_gemm3_tuning")


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, k_pad: int | None = None) -> torch.Tensor:
    M, d = x.shape
    k_pad = k_pad or (d + 255) // 256 * 256
    out = torch.zeros(M, k_pad, dtype=torch.float16, device=x.device)
    N.check(N.lib().mp_op_rmsnorm(_ptr(x), x.stride(0), _ptr(w), d, eps, _ptr(out), k_pad, M, _stream()), "rmsnorm")
    return out


# Raw bindings of the row kernels for the kernel tests: every tensor is the caller's (nothing is
# allocated here), shapes are explicit, and a launcher's own argument check surfaces as RuntimeError.
ACT_F16, ACT_BF16 = 1, 2


def rmsnorm_fill(x, ldx, w, d, eps, out, ldo, M, zero=None, zero_n=0, bias=None, bias_n=0) -> None:
    """launch_rmsnorm: out f16 [M][ldo] = norm(x f32 [M][ldx]) * w; the same launch clears zero[:zero_n]
    (or, with bias, sets zero[i] = bias[i % bias_n])."""
    N.check(N.lib().mp_op_rmsnorm_fill(_ptr(x), ldx, _ptr(w), d, eps, _ptr(out), ldo, M, _ptr(zero), zero_n,
                                       _ptr(bias), bias_n, _stream()), "rmsnorm_fill")


def rmsnorm_acc(x, ldx, w, d, eps, out, ldo, M, zero=None, zero_n=0, part=None, nsplit=0, ss=0, ldp=0, bias=None,
                bias_n=0, q8=None, ldq8=0, q8s=None) -> None:
    """launch_rmsnorm_acc: x += part[0] + ... + part[nsplit - 1] (split s at part + s * ss, rows ldp
    apart) is written back, then normalised as rmsnorm_fill; q8 / q8s: the f16 row also as int8 + scale."""
    N.check(N.lib().mp_op_rmsnorm_acc(_ptr(x), ldx, _ptr(w), d, eps, _ptr(out), ldo, M, _ptr(zero), zero_n, _ptr(part),
                                      nsplit, ss, ldp, _ptr(bias), bias_n, _ptr(q8), ldq8, _ptr(q8s), _stream()),
            "rmsnorm_acc")


POOL_NONE, POOL_MEAN, POOL_CLS, POOL_LAST = 0, 1, 2, 3
POOL_BLOCK_ROWS = 32


def pool_embed(x, w, eps, segs, pooling, normalize, n_slots, h=None, part=None, pool_acc=None, emb=None) -> None:
    """launch_pool_embed (pool.hip): output RMSNorm of the chunk's rows x f32 [T][d] with weights w, then
    pooling per prompt.  segs: one (row0, T, slot, p0, prompt_len, ends_prompt) per segment, tiling the
    rows in order.  none: h [T][d] gets every row's vector; mean: h [T][d] scratch, part [>= blocks][d]
    scratch (32-row blocks per segment), pool_acc [n_slots][d] the running sums, emb [n_slots][d] the
    result of prompt-ending segments; cls / last: emb only.  Raises on a shape the kernel refuses."""
    T, d = x.shape
    tab = torch.tensor([list(map(int, s)) for s in segs], dtype=torch.int32).reshape(-1, 6).contiguous()
    seg_tab = torch.empty(max(tab.shape[0], 1) * 6, dtype=torch.int32, device=x.device)
    N.check(N.lib().mp_op_pool_embed(_ptr(x), x.stride(0), _ptr(w), d, float(eps), tab.data_ptr(), tab.shape[0],
                                     _ptr(seg_tab), T, int(pooling), int(bool(normalize)), int(n_slots), _ptr(h), _ptr(part),
                                     0 if part is None else part.shape[0], _ptr(pool_acc), _ptr(emb), _stream()),
            "pool_embed")


def splitk_reduce(part, nsplit, ss, ldp, M, n, y, ldy, init=False, bias=None) -> None:
    """y[m][j] (+)= sum_s part[s * ss + m * ldp + j] in split order; init: y starts from bias[j] or 0."""
    N.check(N.lib().mp_op_splitk_reduce(_ptr(part), nsplit, ss, ldp, M, n, _ptr(y), ldy, int(init), _ptr(bias),
                                        _stream()), "splitk_reduce")


def moe_combine(ys, lds, k, M, n, y, ldy) -> None:
    """y[t][j] += sum_{e < k} ys[(t * k + e) * lds + j], e ascending."""
    N.check(N.lib().mp_op_moe_combine(_ptr(ys), lds, k, M, n, _ptr(y), ldy, _stream()), "moe_combine")


def swiglu(gu, ld, F, M, h, ldh) -> None:
    """h f16 [M][ldh] = sat_f16(silu(gu[m][j]) * gu[m][F + j]) for j < F (gu f32 [M][ld])."""
    N.check(N.lib().mp_op_swiglu(_ptr(gu), ld, F, M, _ptr(h), ldh, _stream()), "swiglu")


def f32_to_f16(x, ldx, n, M, y, ldy) -> None:
    N.check(N.lib().mp_op_f32_to_f16(_ptr(x), ldx, n, M, _ptr(y), ldy, _stream()), "f32_to_f16")


def act_pack(x, y, n, dtype) -> None:
    """Stage-boundary wire format: n f32 elements of x -> f16 / bf16 (ACT_F16 / ACT_BF16) in y."""
    N.check(N.lib().mp_op_act_pack(_ptr(x), _ptr(y), n, dtype, _stream()), "act_pack")


def act_unpack(y, x, n, dtype) -> None:
    N.check(N.lib().mp_op_act_unpack(_ptr(y), _ptr(x), n, dtype, _stream()), "act_unpack")


def advance(pos, kvlen, M, step=None) -> None:
    """Decode-step advance: pos[i] += 1, kvlen[i] = pos[i] + 1 for i < M; step[0] += 1 when given."""
    N.check(N.lib().mp_op_advance(_ptr(pos), _ptr(kvlen), M, _ptr(step), _stream()), "advance")


def embed(raw_table: torch.Tensor, ggml_type: int, d: int, tokens: torch.Tensor) -> torch.Tensor:
    M = tokens.numel()
    x = torch.empty(M, d, dtype=torch.float32, device=tokens.device)
    rb = Q.row_bytes(ggml_type, d)
    N.check(N.lib().mp_op_embed(ggml_type, _ptr(raw_table), rb, d, _ptr(tokens), M, _ptr(x), d, _stream()), "embed")
    return x


def attn_prefill(q, pos, slot, block_table, k_cache, v_cache, Hkv, hd, segs=None, n_split=1, split_pages=1,
                 kv_fp8=False):
    """Prefill flash attention (attn_prefill.hip): q [M][Hq][Dp] f16 (q_scale applied), rows in
    `segs` = [(row0, T), ...] runs of consecutive positions of one sequence each (default: one run);
    n_split > 1 splits every tile's pages (split_pages each) over workgroups, merged by attn_combine.
    kv_fp8: the caches hold e4m3 bytes (uint8 tensors of the same element layout)."""
    M, Hq, Dp = q.shape
    segs = segs or [(0, M)]
    sa = np.asarray(segs, np.int32).reshape(-1)
    out = torch.zeros(M, Hq * hd, dtype=torch.float16, device=q.device)
    op = ml = None
    if n_split > 1:
        op = torch.full((n_split, M * Hq, Dp), float("nan"), dtype=torch.float32, device=q.device)
        ml = torch.full((n_split, M * Hq, 2), float("nan"), dtype=torch.float32, device=q.device)
    N.check(N.lib().mp_op_attn_prefill(_ptr(q), _ptr(pos), _ptr(slot), _ptr(block_table), block_table.shape[1],
                                       _ptr(k_cache), _ptr(v_cache), Hq, Hkv, hd, Dp,
                                       sa.ctypes.data, len(segs), _ptr(out), out.stride(0), n_split, split_pages,
                                       _ptr(op), _ptr(ml), M, int(kv_fp8), _stream()), "attn_prefill")
    return out


ARGMAX_CHUNKS = 64


def argmax(logits: torch.Tensor, two_level: bool = True) -> torch.Tensor:
    """Greedy token per row (lowest index on ties).  two_level: (chunk, row) grid + last-arriver
    reduce (the engine's path); otherwise one workgroup per row."""
    M, n = logits.shape
    out = torch.empty(M, dtype=torch.int32, device=logits.device)
    part = cnt = None
    if two_level:
        part = torch.empty(M, ARGMAX_CHUNKS, 2, dtype=torch.float32, device=logits.device)
        cnt = torch.zeros(M, dtype=torch.int32, device=logits.device)
    N.check(N.lib().mp_op_argmax(_ptr(logits), logits.stride(0), n, M, _ptr(out), _ptr(part), _ptr(cnt),
                                 _stream()), "argmax")
    if cnt is not None:
        assert int(cnt.abs().sum()) == 0, "argmax arrival counters did not reset"
    return out


def gemv_fused(w: PackedWeight, epi: int = EPI_STORE, *, x: torch.Tensor | None = None,
               xf: torch.Tensor | None = None, gamma: torch.Tensor | None = None, eps: float = 1e-5,
               bias: torch.Tensor | None = None, y: torch.Tensor | None = None, nsplit: int = 1,
               zero: torch.Tensor | None = None, ssq: torch.Tensor | None = None) -> torch.Tensor:
    """Decode GEMV (gemv2.hip) with the fusions the engine uses at single-stream decode.
    xf/gamma: deferred RMSNorm of the f32 rows xf (M <= 4, x unused) -- the GEMV runs on
    f16(xf * gamma); STORE/SWIGLU outputs are scaled by rsqrt(mean(xf^2) + eps), ATOMIC outputs are
    left unscaled and sum(xf^2) per row is added into `ssq` (f32 [M]).  bias: added once per output.
    zero: f32 tensor cleared after the GEMV."""
    if xf is not None:
        assert xf.dtype == torch.float32 and xf.is_contiguous()
        M, d = xf.shape
    else:
        assert x.dtype == torch.float16 and x.shape[1] == w.k_pad and x.is_contiguous()
        M, d = x.shape[0], 0
    F = w.n // 2
    if epi == EPI_SWIGLU:
        h = torch.zeros(M, F, dtype=torch.float16, device=w.dev.device) if y is None else y
        Y, ldy, H, ldh, nv = None, 0, h, h.stride(0), F
    else:
        y = torch.zeros(M, w.n, dtype=torch.float32, device=w.dev.device) if y is None else y
        Y, ldy, H, ldh, nv = y, y.stride(0), None, 0, w.n
    N.check(N.lib().mp_op_gemv_fused(w.ptype, epi, _ptr(w.dev), w.ntiles, w.nsb, _ptr(x), w.k_pad if x is not None else 0,
                                     M, _ptr(Y), ldy, _ptr(H), ldh, nv, nsplit, _ptr(xf), d, _ptr(gamma), eps, d,
                                     _ptr(ssq), _ptr(bias), _ptr(zero), 0 if zero is None else zero.numel(), _stream()),
            "gemv_fused")
    return H if epi == EPI_SWIGLU else Y


def sample(logits: torch.Tensor, temp: float, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0,
           seed: int = 0, step: torch.Tensor | None = None) -> torch.Tensor:
    M, n = logits.shape
    out = torch.empty(M, dtype=torch.int32, device=logits.device)
    N.check(N.lib().mp_op_sample(_ptr(logits), logits.stride(0), n, M, temp, top_k, top_p, min_p, seed, _ptr(step),
                                 _ptr(out), _stream()), "sample")
    return out


def penalize(logits: torch.Tensor, hist: torch.Tensor, repeat: float = 1.0, freq: float = 0.0,
             presence: float = 0.0) -> torch.Tensor:
    """In-place repetition penalties: logits f32 [M][n], hist int32 [M][last_n] (-1 = empty)."""
    M, n = logits.shape
    assert hist.dtype == torch.int32 and hist.shape[0] == M and hist.is_contiguous()
    N.check(N.lib().mp_op_penalize(_ptr(logits), logits.stride(0), n, M, _ptr(hist), hist.shape[1], repeat, freq,
                                   presence, _stream()), "penalize")
    return logits


MAX_LOGIT_BIAS = 32
# the device record of one row (RowSampling, csrc/runtime/kernels_api.h)
ROW_SAMPLING_DTYPE = np.dtype([("temp", "<f4"), ("top_k", "<i4"), ("top_p", "<f4"), ("min_p", "<f4"), ("repeat", "<f4"),
                               ("freq", "<f4"), ("presence", "<f4"), ("n_bias", "<i4"), ("seed", "<u8"), ("draw0", "<i4"),
                               ("pad", "<i4"), ("bias_id", "<i4", (MAX_LOGIT_BIAS,)), ("bias_val", "<f4", (MAX_LOGIT_BIAS,))])


def row_records(rows, device) -> torch.Tensor:
    """Device table (uint8 [M][304]) of per-row sampling records from dicts with the keys temp, top_k,
    top_p, min_p, repeat, freq, presence, seed, draw0 and bias (a list of (id, value) pairs, <= 32)."""
    assert ROW_SAMPLING_DTYPE.itemsize == N.lib().mp_row_sampling_bytes()
    a = np.zeros(len(rows), ROW_SAMPLING_DTYPE)
    a["top_p"], a["repeat"] = 1.0, 1.0
    for i, r in enumerate(rows):
        r = dict(r)
        bias = list(r.pop("bias", ()))
        assert len(bias) <= MAX_LOGIT_BIAS
        for k, v in r.items():
            a[k][i] = v
        a["n_bias"][i] = len(bias)
        for j, (t, v) in enumerate(bias):
            a["bias_id"][i, j], a["bias_val"][i, j] = t, v
    return torch.from_numpy(a.view(np.uint8).reshape(len(rows), -1).copy()).to(device)


def row_adjust(logits: torch.Tensor, records: torch.Tensor, hist: torch.Tensor | None = None,
               last_n: int | None = None) -> torch.Tensor:
    """In place, per row: logit bias, then the repetition penalties of the row's record over its window
    hist[m][:last_n] (int32 [M][hist_ld], -1 = empty; last_n defaults to the width).  logits f32 [M][n]."""
    M, n = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and records.shape[0] == M
    hist_ld = 0
    if hist is not None:
        assert hist.dtype == torch.int32 and hist.shape[0] == M and hist.is_contiguous()
        hist_ld = hist.shape[1]
    last_n = hist_ld if last_n is None else last_n
    N.check(N.lib().mp_row_adjust(_ptr(logits), logits.stride(0), n, M, _ptr(records), _ptr(hist), hist_ld, last_n,
                                  _stream()), "row_adjust")
    return logits


def sample_rows(logits: torch.Tensor, records: torch.Tensor, draw: torch.Tensor, tokens: torch.Tensor | None = None,
                advance: bool = False) -> torch.Tensor:
    """Per-row sampler: row m with temp > 0 draws tokens[m] by its own record at draw index draw[m]
    (int32 [M]); a greedy row leaves tokens[m] as given (-1 when tokens is None).  advance: draw += 1."""
    M, n = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and records.shape[0] == M
    assert draw.dtype == torch.int32 and draw.numel() == M and draw.is_contiguous()
    out = torch.full((M,), -1, dtype=torch.int32, device=logits.device) if tokens is None else tokens
    assert out.dtype == torch.int32 and out.numel() == M and out.is_contiguous()
    N.check(N.lib().mp_sample_rows(_ptr(logits), logits.stride(0), n, M, _ptr(records), _ptr(draw), int(advance),
                                   _ptr(out), _stream()), "sample_rows")
    return out


def row_mask(logits: torch.Tensor, bits: torch.Tensor, on: torch.Tensor, n: int | None = None) -> torch.Tensor:
    """In place: in every row m with on[m] != 0, logits[m][t] = -inf for each t < n whose bit
    bits[m][t >> 5] >> (t & 31) & 1 is clear.  logits f32 [M][>= n] (row stride free, 4-byte aligned),
    bits int32 [M][ldw] holding the uint32 words, on int32 [M].  Nothing else is written."""
    M = logits.shape[0]
    n = logits.shape[1] if n is None else n
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and n <= logits.shape[1]
    assert bits.dtype == torch.int32 and bits.shape[0] == M and bits.stride(1) == 1
    assert on.dtype == torch.int32 and on.numel() == M and on.is_contiguous()
    N.check(N.lib().mp_op_row_mask(_ptr(logits), logits.stride(0), n, M, _ptr(bits), bits.stride(0), _ptr(on),
                                   _stream()), "row_mask")
    return logits


LORA_TARGETS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")


def lora_rank_pad(r: int) -> int:
    """The rank the LoRA kernels see (A [r_pad][K], B [N][r_pad], zero-filled)."""
    return N.lib().mp_lora_rank_pad(int(r))


def lora_max_tiles(M: int, n_adapters: int) -> int:
    return N.lib().mp_lora_max_tiles(int(M), int(n_adapters))


def lora_tile_table(ids, scales=None, n_adapters: int = 8, max_tiles: int | None = None) -> np.ndarray:
    """The tile table of a row -> adapter list, built by the builder the stages use: ids[m] is row m's
    adapter or -1, scales[m] its user scale.  int32 words: [0] the tile count, then from word 4 tiles
    of (adapter, 3 unused, 16 row indices -1 padded, 16 f32 scales)."""
    ids = np.ascontiguousarray(ids, np.int32)
    sc = np.ascontiguousarray(np.ones(len(ids)) if scales is None else scales, np.float32)
    assert sc.shape == ids.shape
    mt = lora_max_tiles(len(ids), n_adapters) if max_tiles is None else int(max_tiles)
    out = np.zeros(N.lib().mp_lora_table_words(max(mt, 1)), np.int32)
    N.check(N.lib().mp_lora_build_tiles(ids.ctypes.data, sc.ctypes.data, len(ids), int(n_adapters), mt,
                                        out.ctypes.data), "lora_tile_table")
    return out


def lora_target_table(pairs: dict, n_adapters: int, n_layers: int, device) -> torch.Tensor:
    """The device table [n_adapters][n_layers][7] of (A pointer, B pointer, r_pad) from
    {(adapter, layer, target): (A f16 [r_pad][K], B f16 [N][r_pad])} of device tensors the caller
    keeps alive; a missing key leaves the target absent (null pointers)."""
    rec = np.zeros((n_adapters, n_layers, len(LORA_TARGETS)),
                   dtype=[("A", "<u8"), ("B", "<u8"), ("r_pad", "<i4"), ("pad", "<i4")])
    assert rec.dtype.itemsize == N.lib().mp_lora_target_rec_bytes()
    for (a, layer, t), (A, B) in pairs.items():
        assert A.dtype == torch.float16 and B.dtype == torch.float16 and A.is_contiguous() and B.is_contiguous()
        assert A.shape[0] == B.shape[1] and A.shape[0] % 32 == 0
        rec[a, layer, t] = (A.data_ptr(), B.data_ptr(), A.shape[0], 0)
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(device)


def lora_part(max_tiles: int, K: int, n_t: int, rcap: int, device) -> torch.Tensor:
    """Split-K partial scratch of one shrink / expand pair (deliberately not zeroed by the kernels'
    contract: every word expand reads was stored by shrink)."""
    n = N.lib().mp_lora_part_floats(int(max_tiles), int(K), int(n_t), int(rcap))
    return torch.full((max(n, 1),), float("nan"), dtype=torch.float32, device=device)


def _lora(which, tiles, max_tiles, targets, n_adapters, n_layers, layer, tgt, n_cols, yoff, x, K, y, part, rcap):
    assert x.dtype == torch.float16 and x.stride(1) == 1 and y.dtype == torch.float32 and y.stride(1) == 1
    assert tiles.dtype == torch.int32 and tiles.numel() >= N.lib().mp_lora_table_words(max_tiles)
    n_t = len(tgt)
    arr = lambda v: np.ascontiguousarray(v, np.int32)
    tg, nc, yo = arr(tgt), arr(n_cols), arr(yoff)
    assert len(nc) == n_t and len(yo) == n_t
    N.check(N.lib().mp_op_lora(which, _ptr(tiles), int(max_tiles), _ptr(targets), int(n_adapters), int(n_layers),
                               int(layer), n_t, tg.ctypes.data, nc.ctypes.data, yo.ctypes.data, _ptr(x), x.stride(0),
                               int(K), _ptr(y), y.stride(0), _ptr(part), part.numel(), int(rcap), _stream()),
            "lora_expand" if which else "lora_shrink")


def lora_shrink(tiles, max_tiles, targets, n_adapters, n_layers, layer, tgt, n_cols, yoff, x, K, y, part, rcap) -> None:
    """Per tile of `tiles` (device int32 table of lora_tile_table) and K split: part <- A x for the
    targets `tgt` (ids into LORA_TARGETS) of the tile's adapter at `layer`.  x f16 [M][ldx >= K]."""
    _lora(0, tiles, max_tiles, targets, n_adapters, n_layers, layer, tgt, n_cols, yoff, x, K, y, part, rcap)


def lora_expand(tiles, max_tiles, targets, n_adapters, n_layers, layer, tgt, n_cols, yoff, x, K, y, part, rcap) -> None:
    """y[row][yoff[i] + n] += scale[row] * B_i[n] . (the partials of lora_shrink summed in split order),
    n < n_cols[i], for the rows of the tiles; nothing else of y is written."""
    _lora(1, tiles, max_tiles, targets, n_adapters, n_layers, layer, tgt, n_cols, yoff, x, K, y, part, rcap)


LOGPROB_MAX_TOP = 20


def logprob(logits: torch.Tensor, n: int | None = None, target: torch.Tensor | None = None, top_n: int = 0,
            rows: int | None = None, out: tuple | None = None):
    """Log-softmax statistics of the first `rows` rows of f32 logits [M][ld] (columns n.. are padding):
    returns (lse [M], target_lp [M], top_id [M][w], top_lp [M][w]); the kernel writes the first `rows`
    rows and the first top_n slots of a row.  out: pre-filled buffers of those shapes (w >= top_n)."""
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    M = logits.shape[0] if rows is None else rows
    n = logits.shape[1] if n is None else n
    dev = logits.device
    if out is None:
        out = (torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev),
               torch.empty(M, max(top_n, 1), dtype=torch.int32, device=dev),
               torch.empty(M, max(top_n, 1), dtype=torch.float32, device=dev))
    lse, tlp, tid, tl = out
    assert tid.dtype == torch.int32 and tid.is_contiguous() and tl.is_contiguous() and tid.shape == tl.shape
    assert lse.numel() >= M and tlp.numel() >= M and tid.shape[0] >= M
    if target is not None:
        assert target.dtype == torch.int32 and target.numel() >= M and target.is_contiguous()
    N.check(N.lib().mp_op_logprob(_ptr(logits), logits.stride(0), n, M, _ptr(target), top_n, _ptr(lse), _ptr(tlp),
                                  _ptr(tid), _ptr(tl), tid.shape[1], _stream()), "logprob")
    return out


def logprob_generation(logits: torch.Tensor, hist: torch.Tensor | None, top_n: int, step):
    """The engine's generation sequence on f32 logits [M][n]: statistics of the raw logits (saving
    those of the penalty window `hist`), then step(logits) -> int32 tokens [M] (penalties in place
    and a sampler), then the chosen tokens' raw logprobs.  Returns (tokens, chosen_lp, top_id, top_lp)."""
    M, n = logits.shape
    dev = logits.device
    lse = torch.empty(M, dtype=torch.float32, device=dev)
    tid = torch.empty(M, max(top_n, 1), dtype=torch.int32, device=dev)
    tl = torch.empty(M, max(top_n, 1), dtype=torch.float32, device=dev)
    last_n = 0 if hist is None else hist.shape[1]
    raw = None if hist is None else torch.empty(M, last_n, dtype=torch.float32, device=dev)
    N.check(N.lib().mp_op_logprob_stats(_ptr(logits), logits.stride(0), n, M, top_n, _ptr(lse), _ptr(tid), _ptr(tl),
                                        tid.shape[1], _ptr(hist), last_n, _ptr(raw), _stream()), "logprob_stats")
    tokens = step(logits)
    clp = torch.empty(M, dtype=torch.float32, device=dev)
    N.check(N.lib().mp_op_logprob_chosen(_ptr(logits), logits.stride(0), n, M, _ptr(tokens), _ptr(lse), _ptr(hist),
                                         last_n, _ptr(raw), _ptr(clp), _stream()), "logprob_chosen")
    return tokens, clp, tid[:, :top_n], tl[:, :top_n]


def hist_push(hist: torch.Tensor, cnt: torch.Tensor, tokens: torch.Tensor) -> None:
    """hist[m][cnt[m] % last_n] = tokens[m]; cnt[m] += 1 (int32 device tensors)."""
    M, last_n = hist.shape
    N.check(N.lib().mp_op_hist_push(_ptr(hist), _ptr(cnt), last_n, _ptr(tokens), M, _stream()), "hist_push")


def rope_cs_table(max_pos: int, hd: int, base: float, freq_factors=None) -> torch.Tensor:
    inv = base ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)
    if freq_factors is not None:
        inv = inv / np.asarray(freq_factors, np.float64)
    ang = np.outer(np.arange(max_pos, dtype=np.float64), inv)
    cs = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)   # [pos][hd/2][2]
    return torch.from_numpy(cs)


class v_layout:
    """V page layout the V-touching ops of this thread use (rope_kv, attention, attn_prefill,
    attn_decode, attn_o, gemv_small_qkv) inside the `with` block: blocked=False (the default outside
    any block) is V^T [page][Hkv][Dp][64]; blocked=True is [page][Hkv][8][Dp][8], element (key, d) at
    (key >> 3) * Dp * 8 + d * 8 + (key & 7), the engine's default (`v_blocked`)."""

    def __init__(self, blocked: bool):
        self.blocked = bool(blocked)

    def __enter__(self):
        self.old = N.lib().mp_op_v_layout(int(self.blocked))
        return self

    def __exit__(self, *exc):
        N.lib().mp_op_v_layout(self.old)
        return False


def v_pages_to_blocked(v: torch.Tensor) -> torch.Tensor:
    """V^T pages [P][H][Dp][64] -> blocked pages (same shape and bytes, elements permuted)."""
    P, H, Dp, _ = v.shape
    return v.view(P, H, Dp, 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(P, H, Dp, 64)


def v_pages_from_blocked(v: torch.Tensor) -> torch.Tensor:
    P, H, Dp, _ = v.shape
    return v.view(P, H, 8, Dp, 8).permute(0, 1, 3, 2, 4).contiguous().view(P, H, Dp, 64)


def gemv_small_qkv(w: PackedWeight, xf, gamma, eps, pos, slot0, block_table, rope_cs, k_cache, v_cache, Hq, Hkv, hd, Dp,
                   *, bias=None, kv_fp8=False) -> torch.Tensor:
    """The single-stream q|k|v GEMV with the RoPE + KV append epilogue (gemvs QkvAppend): fused
    RMSNorm of xf f32 [M <= 4][d]; returns y f32 [M][(Hq + 2 Hkv) hd] whose q columns hold the rotated
    q (k / v columns are not written); k (rotated) and v land in the pages of slot slot0 + m at pos[m]."""
    assert xf.dtype == torch.float32 and xf.is_contiguous() and pos.dtype == torch.int32
    assert block_table.dtype == torch.int32 and block_table.is_contiguous()
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and w.n == (Hq + 2 * Hkv) * hd
    M, d = xf.shape
    y = torch.zeros(M, w.n, dtype=torch.float32, device=xf.device)
    N.check(N.lib().mp_op_gemvs_qkv(w.ptype, _ptr(w.dev), w.ntiles, w.nsb, M, _ptr(y), y.stride(0), w.n, _ptr(xf), d,
                                    _ptr(gamma), eps, d, _ptr(bias), _ptr(pos), int(slot0), _ptr(block_table),
                                    block_table.shape[1], _ptr(rope_cs), _ptr(k_cache), _ptr(v_cache), Hq, Hkv, hd, Dp,
                                    int(kv_fp8), _stream()), "gemv_small_qkv")
    return y


def rope_kv(qkv, pos, slot, block_table, rope_cs, Hq, Hkv, hd, Dp, q_scale, k_cache, v_cache, kv_fp8=False, q_out=None):
    """kv_fp8: the caches hold e4m3 bytes (uint8 tensors of the same element layout).  q_out: the
    f16 [M][Hq][Dp] buffer to write (the kernel writes every element of it); default a new one."""
    M = qkv.shape[0]
    if q_out is None:
        q_out = torch.zeros(M, Hq, Dp, dtype=torch.float16, device=qkv.device)
    assert q_out.shape == (M, Hq, Dp) and q_out.dtype == torch.float16 and q_out.is_contiguous()
    N.check(N.lib().mp_op_rope_kv(_ptr(qkv), qkv.stride(0), M, Hq, Hkv, hd, Dp, _ptr(pos), _ptr(slot),
                                  _ptr(block_table), block_table.shape[1], _ptr(rope_cs), q_scale, _ptr(q_out),
                                  _ptr(k_cache), _ptr(v_cache), int(kv_fp8), _stream()), "rope_kv")
    return q_out


def kv_shift(k_cache, v_cache, block_table, rope_cs, records, Hkv, hd, Dp, n_pages, kv_fp8=False):
    """Context shift of one layer's paged caches, in place.  records: (slot, n_keep, n_discard, old_len,
    merge_src_page) tuples naming distinct slots; block_table int32 [n_slots][max_pages] is the table
    AFTER the page edit (KvPager::shift): the tail pages of a record's slot are rotated in place by
    minus n_discard positions with rope_cs[n_discard] (f32 from the stored code, rounded to f16 /
    e4m3, dims hd..Dp zero); with n_keep % 64 != 0 the page holding n_keep takes rows
    [n_keep % 64, 64) of merge_src_page (K rotated, V copied in the thread's `v_layout`), else
    merge_src_page is -1.  n_pages: pool pages (ids >= n_pages are never touched).  The host checks
    the records and raises, naming the first bad one."""
    assert block_table.dtype == torch.int32 and block_table.is_contiguous() and block_table.dim() == 2
    assert k_cache.is_contiguous() and v_cache.is_contiguous()
    assert rope_cs.dtype == torch.float32 and rope_cs.is_contiguous() and rope_cs.shape[1] == hd // 2
    rec = np.ascontiguousarray(np.asarray(records, np.int32).reshape(-1, 5))
    N.check(N.lib().mp_op_kv_shift(_ptr(k_cache), _ptr(v_cache), _ptr(block_table), block_table.shape[0],
                                   block_table.shape[1], int(n_pages), Hkv, hd, Dp, int(kv_fp8), _ptr(rope_cs),
                                   rope_cs.shape[0], rec.ctypes.data, rec.shape[0], _stream()), "kv_shift")


def qk_norm(qkv, wq, wk, Hq, Hkv, hd, eps):
    """Qwen3 per-head RMSNorm of the q and k heads of the f32 rows qkv [M, >= (Hq + 2 Hkv) hd], in
    place, before RoPE; wq / wk: f32 [hd].  Returns qkv."""
    N.check(N.lib().mp_op_qk_norm(_ptr(qkv), qkv.stride(0), qkv.shape[0], Hq, Hkv, hd, _ptr(wq), _ptr(wk),
                                  float(eps), _stream()), "qk_norm")
    return qkv


def attention(q, kvlen, slot, block_table, k_cache, v_cache, Hkv, hd, tq=1, split_len=256, n_split=1):
    M, Hq, Dp = q.shape
    out = torch.zeros(M, Hq * hd, dtype=torch.float16, device=q.device)
    o_part = torch.zeros(max(n_split, 1), M * Hq, Dp, dtype=torch.float32, device=q.device)
    ml_part = torch.zeros(max(n_split, 1), M * Hq, 2, dtype=torch.float32, device=q.device)
    N.check(N.lib().mp_op_attention(_ptr(q), _ptr(kvlen), _ptr(slot), _ptr(block_table), block_table.shape[1],
                                    _ptr(k_cache), _ptr(v_cache), M, Hq, Hkv, hd, Dp, tq, split_len, n_split,
                                    _ptr(o_part), _ptr(ml_part), _ptr(out), out.stride(0), _stream()), "attention")
    return out


ATTN_FORM_PF4, ATTN_FORM_PF8, ATTN_FORM_NP, ATTN_FORM_WAVE = 0, 1, 2, 3


def attn_decode_form(M: int, Hkv: int, n_split: int) -> int:
    """The device form launch_attn_decode takes for this grid under the current knobs (ATTN_FORM_*)."""
    return N.check(N.lib().mp_attn_decode_form(M, Hkv, n_split), "attn_decode_form")


GEMM4_PLAN_FIELDS = ("ok", "bm", "nwv", "tw", "nsplit", "per", "wnt", "grid_x", "grid_y", "grid_z")


def _gemm4_plan(fn, what, *args) -> dict:
    out = (ctypes.c_int * len(GEMM4_PLAN_FIELDS))()
    in_table = N.check(fn(*args, out), what)
    return dict(zip(GEMM4_PLAN_FIELDS, out), in_table=in_table)


def gemm4_plan(ptype: int, epi: int, M: int, ntiles: int, nsb: int, allow_split: bool = True,
               partial_stores: bool = False) -> dict:
    """The launch launch_gemm4 (partial_stores: launch_gemm4_splitk) runs for this shape under the
    current knobs (host only): GEMM4_PLAN_FIELDS, plus in_table = 1 when the kernel geometry table
    holds the plan's (bm, nwv, tw)."""
    return _gemm4_plan(N.lib().mp_gemm4_plan, "gemm4_plan", ptype, epi, M, ntiles, nsb, int(allow_split),
                       int(partial_stores))


def moe_gemm4_plan(ptype: int, epi: int, M: int, k: int, E: int, ntiles: int, nsb: int, per_slot: bool = False) -> dict:
    """The same for launch_moe_gemm4 (M tokens, k of E experts each; per_slot: the deterministic down)."""
    return _gemm4_plan(N.lib().mp_moe_gemm4_plan, "moe_gemm4_plan", ptype, epi, M, k, E, ntiles, nsb, int(per_slot))


class DecodeAttnScratch:
    """Split partials and the self-resetting arrival counters of the fused decode attention; kept
    across calls as the engine keeps them (o_part / ml_part poisoned with NaN: never read unwritten)."""

    def __init__(self, M, Hq, Hkv, Dp, n_split, device="cuda"):
        self.o_part = torch.full((n_split, M * Hq, Dp), float("nan"), dtype=torch.float32, device=device)
        self.ml_part = torch.full((n_split, M * Hq, 2), float("nan"), dtype=torch.float32, device=device)
        self.counters = torch.zeros(max(M, 16) * Hkv, dtype=torch.int32, device=device)


def _decode_attn_args(qkv, pos, block_table, rope_cs, k_cache, v_cache, Hq, Hkv, hd, Dp, q_scale, split_len, n_split,
                      scratch, out, slot, slot0, ssq, eps, d_model, bias, kv_fp8, pre):
    M = qkv.shape[0]
    assert qkv.dtype == torch.float32 and qkv.stride(1) == 1 and pos.dtype == torch.int32
    assert block_table.dtype == torch.int32 and block_table.is_contiguous()
    assert rope_cs.dtype == torch.float32 and rope_cs.is_contiguous()
    assert k_cache.is_contiguous() and v_cache.is_contiguous()
    assert k_cache.dtype == v_cache.dtype == (torch.uint8 if kv_fp8 else torch.float16)
    assert (slot is None) != (slot0 is None), "exactly one of slot / slot0"
    assert out.dtype == torch.float16 and out.stride(1) == 1
    return (_ptr(qkv), qkv.stride(0), _ptr(pos), _ptr(slot), -1 if slot0 is None else int(slot0), _ptr(block_table),
            block_table.shape[1], _ptr(rope_cs), q_scale, _ptr(k_cache), _ptr(v_cache), M, Hq, Hkv, hd, Dp, split_len,
            n_split, _ptr(scratch.o_part), _ptr(scratch.ml_part), _ptr(scratch.counters), _ptr(out), out.stride(0),
            _ptr(ssq), eps, d_model, _ptr(bias), int(kv_fp8), int(pre))


def attn_decode(qkv, pos, block_table, rope_cs, k_cache, v_cache, Hq, Hkv, hd, Dp, q_scale, split_len, n_split,
                scratch, *, slot=None, slot0=None, ssq=None, eps=0.0, d_model=0, bias=None, kv_fp8=False, pre=False,
                out=None):
    """The fused decode attention step (attention.hip: RoPE of q and the new k, KV append, split
    flash-decoding, last-arriver merge) as the engine launches it: qkv f32 [M][>= (Hq + 2 Hkv) hd]
    pre-RoPE (with ssq: before the deferred RMSNorm scale / bias), row t in slot slot0 + t or slot[t]
    at position pos[t]; K pages [page][Hkv][64][Dp], V pages [page][Hkv][Dp][64] (or blocked, inside
    `with v_layout(True)`), f16 or (kv_fp8) e4m3 bytes.  pre: q rotated, the new K / V already in the cache.  Returns out f16 [M][Hq * hd];
    the form is chosen by the launcher (attn_decode_form)."""
    M = qkv.shape[0]
    if out is None:
        out = torch.zeros(M, Hq * hd, dtype=torch.float16, device=qkv.device)
    a = _decode_attn_args(qkv, pos, block_table, rope_cs, k_cache, v_cache, Hq, Hkv, hd, Dp, q_scale, split_len,
                          n_split, scratch, out, slot, slot0, ssq, eps, d_model, bias, kv_fp8, pre)
    N.check(N.lib().mp_op_attn_decode(*a, _stream()), "attn_decode")
    return out


def attn_o(w: PackedWeight, y, qkv, pos, block_table, rope_cs, k_cache, v_cache, Hq, Hkv, hd, Dp, q_scale, split_len,
           scratch, *, slot=None, slot0=None, ssq=None, eps=0.0, d_model=0, kv_fp8=False, pre=False):
    """Fused decode attention + o-projection (attn_o_kernel): y f32 [M][n] += attn . W_o^T with
    atomics; one split.  Raises where attn_o_supported is false."""
    M = qkv.shape[0]
    assert y.dtype == torch.float32 and y.stride(1) == 1 and y.shape == (M, w.n)
    out = torch.zeros(M, Hq * hd, dtype=torch.float16, device=qkv.device)   # unused by the fused kernel
    a = _decode_attn_args(qkv, pos, block_table, rope_cs, k_cache, v_cache, Hq, Hkv, hd, Dp, q_scale, split_len,
                          1, scratch, out, slot, slot0, ssq, eps, d_model, None, kv_fp8, pre)
    N.check(N.lib().mp_op_attn_o(*a, _ptr(w.dev), w.ptype, w.ntiles, w.nsb, _ptr(y), y.stride(0), w.n, _stream()),
            "attn_o")
    return y
