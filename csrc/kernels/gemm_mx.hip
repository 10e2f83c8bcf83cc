// MX-FP8 GEMM (opt-in mx8_gemm mode, M > 64): Y[M][N] (+)= X[M][K] W[N][K]^T with both operands in
// OCP MXFP8 -- e4m3 bytes with one e8m0 power-of-two scale per 32 k of a row -- on
// v_mfma_scale_f32_32x32x64_f8f6f4, which applies both block scales inside the instruction.
//
// Operand layout of the instruction (fp8 x fp8, measured with one-hot rows and per-block scales):
// lane l supplies row (A) / column (B) l % 32; its VGPRs 0-3 hold k = 16 (l / 32) .. + 15 and its
// VGPRs 4-7 k = 32 + 16 (l / 32) .. + 15 of the MFMA's 64.  The scale operand is a dword whose byte
// op_sel picks; the byte of lane l scales k-block l / 32 (k = 32 (l / 32) .. + 31), i.e. one MX block,
// whose values sit in the SAME register half of the two lanes l % 32 and l % 32 + 32.
// An fp4 (e2m1) B operand (blgp = 4; measured the same way: one-hot fp8 rows against fp4 columns whose
// nibble codes spell their position, scale bytes differing per lane half): lane l supplies column
// l % 32 from its VGPRs 0-3 only (4-7 are ignored), 32 nibbles = k 32 (l / 32) .. + 31 in order, k even
// in the low nibble of byte k / 2.  The lane's scale byte scales exactly those 32 k: one lane, one
// MX block, and op_sel picks the byte as for fp8.
//
// Work split: a workgroup of 8 waves computes BM (128 | 256) rows x 256 columns; every wave owns 32
// columns for all BM rows (BM / 32 accumulator fragments of 16 f32).  K runs in stages of 128 (two
// MFMAs per fragment), two stages per 256-k super-block.
//   W  never touches LDS: requant_mx8_kernel lays each wave's B operand of a 64-k block out as 2 KB
//      in fragment order, so a stage is four 1 KB wave loads global -> VGPR, one stage ahead.  The
//      column's 8 scale bytes of a super-block arrive as one dword per lane, already ordered so that
//      op_sel = 2 q + kk (stage q, MFMA kk) selects the lane's block.  An MXFP4 tensor's B image
//      (relayout_mx4_kernel: the file's nibbles and scale bytes, permuted) is 1 KB per 64-k block, so
//      the fp4 variant (BF = 1) loads two 1 KB pieces per stage and keeps 8 instead of 16 VGPRs of B
//      per stage in flight; the scale image and op_sel are the same.
//   X  (e4m3 rows, 128 B per row per stage) is shared by the 8 waves through LDS: global -> VGPR one
//      stage ahead, ds_write into the other of two stage buffers behind the MFMAs, one barrier per
//      stage.  Rows keep gemm3's 16-byte chunk swizzle (g3_off), so a fragment's two ds_read_b128 are
//      bank-conflict free.  The rows' scale dwords (4 blocks of the stage) ride along in the stage
//      buffer; a lane shifts its dword by 8 (l / 32), so op_sel = 2 kk selects its k-block.
// The global loads and the LDS writes are plain C++ (the compiler's own vmcnt waits: the prefetch
// registers are written at the top of a stage and first read behind its MFMAs); the LDS reads are
// asm with counted lgkmcnt waits, one fragment ahead of the MFMAs (gemm_mx_core.h: the stage, the image
// addressing and the workgroup id remap, shared with the grouped MoE kernel of moe_mx.hip).
// EPI_ATOMIC splits the super-block range over blockIdx.y; epilogues and output layouts are gemm3's
// (SwiGLU: tile rows 0-7 gate, 8-15 up of the same 8 outputs).
#include "kcommon.h"
#include "mx8.h"
#include "gemm_mx_core.h"
#include "../runtime/kernels_api.h"
#include "../runtime/tuning.h"

#include <algorithm>
#include <stdexcept>

namespace mpk {
using namespace mp;

// f16 rows -> MX-FP8 rows: one workgroup per row, 8 f16 (one 16-byte load) per lane per step, so a
// block is 4 adjacent lanes (cross-lane max), 8-byte stores, one scale byte per block
__global__ __launch_bounds__(256) void quant_rows_mx8_kernel(const f16* X, int ldx, int K, uint8_t* Q, int ldq, uint8_t* S,
                                                             int lds) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const f16* x = X + (size_t)m * ldx;
  for (int k = tid * 8; k < K; k += 2048) {   // K % 32 == 0: the 4 lanes of a block run the same trips
    const half8_t v = *reinterpret_cast<const half8_t*>(x + k);
    float mx = amax8(v);
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    const uint32_t e = mx8_scale_e(mx);
    *reinterpret_cast<u32x2*>(Q + (size_t)m * ldq + k) = mx8_pack8(v, mx8_scale_f32(e));
    if ((tid & 3) == 0) S[(size_t)m * lds + (k >> 5)] = (uint8_t)e;
  }
}

// Dense f16 weight -> the GEMM's B image (kernels_api.h): one lane per (column, 32-k block b of the
// chunk's two); the block's halves go to register half b of the lanes col and col + 32, so a wave
// writes one 2 KB chunk as two stores of 2 x 512 B
__global__ __launch_bounds__(256) void requant_mx8_kernel(const f16* W, int ldw, int n, int nsb, int nchunks, uint8_t* out,
                                                          uint8_t* scales) {
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (chunk >= nchunks) return;
  const int nkb = 4 * nsb, c = chunk / nkb, kb = chunk - c * nkb;
  const int col = 32 * c + (l & 31), k0 = 64 * kb + 32 * (l >> 5);
  half8_t v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (col < n) v[j] = *reinterpret_cast<const half8_t*>(W + (size_t)col * ldw + k0 + 8 * j);
    else v[j] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
  }
  const uint32_t e = mx8_scale_e(fmaxf(fmaxf(amax8(v[0]), amax8(v[1])), fmaxf(amax8(v[2]), amax8(v[3]))));
  const float s = mx8_scale_f32(e);
  uint8_t* dst = out + (size_t)chunk * 2048 + 1024 * (l >> 5) + (l & 31) * 16;
#pragma unroll
  for (int h = 0; h < 2; ++h) {   // k-half h of the block: lane 32 h + col % 32
    const u32x2 a = mx8_pack8(v[2 * h], s), b = mx8_pack8(v[2 * h + 1], s);
    *reinterpret_cast<u32x4*>(dst + 512 * h) = u32x4{a.x, a.y, b.x, b.y};
  }
  scales[((size_t)(c * nsb + (kb >> 2)) * 64 + l) * 4 + (kb & 3)] = (uint8_t)e;
}

// P_MXFP4 T16 image -> the fp4 B image (kernels_api.h): a permutation.  One lane per (column, 32-k
// block): its 16 source bytes are the T16 piece of lane 16 g + r, half h (block 2 g + h of the chunk),
// whose dwords hold elements j = 0..3 in the low and 4..7 in the high nibbles of their bytes
__global__ __launch_bounds__(256) void relayout_mx4_kernel(const uint8_t* W, int ntiles, int nsb, int nchunks, uint8_t* out,
                                                           uint8_t* scales) {
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
  if (chunk >= nchunks) return;
  const int nkb = 4 * nsb, c = chunk / nkb, kb = chunk - c * nkb;
  const int tile = 2 * c + ((l & 31) >> 4), r = l & 15, sb = kb >> 2, bi = 2 * (kb & 3) + (l >> 5);
  u32x4 o = {0u, 0u, 0u, 0u};
  uint32_t e = 127;
  if (tile < ntiles) {   // (an odd tile count leaves the last group's upper 16 columns empty)
    const uint8_t* src = W + ((size_t)tile * nsb + sb) * chunk_bytes(P_MXFP4);
    const u32x4 q = *reinterpret_cast<const u32x4*>(src + (bi & 1) * 1024 + (16 * (bi >> 1) + r) * 16);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const uint32_t lo = q[s] & 0x0F0F0F0Fu, hi = (q[s] >> 4) & 0x0F0F0F0Fu;
      o[s] = __builtin_amdgcn_perm(hi | (hi >> 4), lo | (lo >> 4), 0x06040200u);   // bytes (j0 j1, j2 j3, j4 j5, j6 j7)
    }
    e = src[2048 + 8 * r + bi];
  }
  *reinterpret_cast<u32x4*>(out + (size_t)chunk * 1024 + l * 16) = o;
  scales[((size_t)(c * nsb + sb) * 64 + l) * 4 + (kb & 3)] = (uint8_t)e;
}

template <int EPI, int BM, int BF>   // BF: B operand format, 0 = e4m3 (2 KB per 64-k block), 1 = fp4 (1 KB)
__global__ __launch_bounds__(512) void gemm_mx_kernel(const Mx8Params p, const int n_mb, const int sb_per_split) {
  constexpr int NB = MxB<BF>::NB;    // 16-byte B pieces per lane per stage
  constexpr int FM = BM / 32;        // accumulator fragments (32 rows each) per wave
  constexpr int AP = BM / 64;        // 16-byte x pieces per thread per stage
  constexpr int A_BYTES = BM * 128, STAGE = A_BYTES + 2048;   // x rows + a scale dword slot per thread (BM used)
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, cl = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware logical id (bijective for any grid size): the row blocks of one column group share an XCD
  const int lid = mx_xcd_lid(blockIdx.x, gridDim.x);
  const int cg = lid / n_mb, mb = lid - cg * n_mb;
  const int m0 = mb * BM, M = p.M;
  const int sb_begin = blockIdx.y * sb_per_split, sb_end = min(sb_begin + sb_per_split, p.nsb);
  if (sb_begin >= sb_end) return;   // uniform over the workgroup

  // this wave's 32 columns: group grp of the B image (clamped: a wave past the last group computes a
  // copy of it and stores nothing)
  const int grp = min(cg * 8 + wave, (p.ntiles + 1) / 2 - 1);
  const uint8_t* wb = MxB<BF>::pieces(p.W, grp, p.nsb, lane);
  const uint32_t* wsp = MxB<BF>::scales(p.wscale, grp, p.nsb, lane);
  // x piece i of this thread: row (tid + 512 i) >> 3, 16-byte chunk tid & 7 (rows clamped to M - 1)
  const int xrow = tid >> 3, xch = tid & 7;
  // (threads >= BM fetch a clamped row's dword into their own, unread slot: no branch in the loop, which
  // would split its block and let the MFMAs sink past the scheduling fences)
  const uint8_t* xsa = p.xscale + (size_t)min(m0 + min(tid, BM - 1), M - 1) * p.ldxs;

  // stage s (128 k): this thread's x pieces and x scale dword, this lane's four B half-fragments (fp4: two fragments)
  auto fetch = [&](int s, u32x4 (&a)[AP], uint32_t& as, u32x4 (&b)[NB]) {
#pragma unroll
    for (int i = 0; i < AP; ++i) a[i] = ld16(p.X + (size_t)min(m0 + xrow + 64 * i, M - 1) * p.ldx + 16 * xch + (size_t)s * 128);
    as = *reinterpret_cast<const uint32_t*>(xsa + 4 * s);
    MxB<BF>::fetch(wb, s, b);
  };
  auto store_a = [&](int buf, const u32x4 (&a)[AP], uint32_t as) {
    char* A = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < AP; ++i) *reinterpret_cast<u32x4*>(A + g3_off(xrow + 64 * i, xch)) = a[i];
    reinterpret_cast<uint32_t*>(A + A_BYTES)[tid] = as;
  };

  f32x16 acc[FM][1];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[i][0][v] = 0.f;

  // stage q of a super-block from buffer q: gemm_mx_core.h's mx_stage (fragment i's rows 32 i + cl)
  const MxLdsAddr la(smem, A_BYTES, cl, h);
  auto compute = [&](auto qc, const u32x4 (&b)[1][NB], const uint32_t (&wsc)[1]) {
    mx_stage<BF, FM, 1, STAGE, decltype(qc)::value, false>(la, h, b, wsc, acc, FM);
  };

  u32x4 an[AP], b[2][1][NB];
  uint32_t asn, wsc[1] = {wsp[(size_t)sb_begin * 64]};
  fetch(2 * sb_begin, an, asn, b[0][0]);
  store_a(0, an, asn);
  __syncthreads();
  for (int sb = sb_begin; sb < sb_end; ++sb) {
    fetch(2 * sb + 1, an, asn, b[1][0]);
    compute(std::integral_constant<int, 0>{}, b[0], wsc);
    store_a(1, an, asn);   // buffer 1's last readers passed the barrier that ended the previous stage
    __syncthreads();
    const int nx = min(sb + 1, sb_end - 1);   // (the last trip re-reads its own super-block: in bounds, unused)
    fetch(2 * nx, an, asn, b[0][0]);
    const uint32_t wsn = wsp[(size_t)nx * 64];
    compute(std::integral_constant<int, 1>{}, b[1], wsc);
    store_a(0, an, asn);
    __syncthreads();
    wsc[0] = wsn;
  }

  // epilogue: lane holds C[row 32 i + 8 (v >> 2) + 4 h + (v & 3)][col cl] of the wave's 32 columns
  const int rowb = m0 + 4 * h;
  const int n = (cg * 8 + wave) * 32 + cl;
  if constexpr (EPI == EPI_SWIGLU) {
    const int o = (n >> 4) * 8 + (cl & 15);   // tile rows 0-7 gate, 8-15 up of the same 8 outputs
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float other = __shfl_xor(acc[i][0][v], 8);
        const int m = rowb + 32 * i + 8 * (v >> 2) + (v & 3);
        if ((cl & 8) == 0 && m < M && o < p.n_valid) p.H[(size_t)m * p.ldh + o] = sat_f16(silu(acc[i][0][v]) * other);
      }
  } else if (n < p.n_valid) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int m = rowb + 32 * i + 8 * (v >> 2) + (v & 3);
        if (m < M) {
          float* dst = p.Y + (size_t)m * p.ldy + n;
          if constexpr (EPI == EPI_ATOMIC) unsafeAtomicAdd(dst, acc[i][0][v]);
          else *dst = acc[i][0][v];
        }
      }
  }
}

}  // namespace mpk

namespace mp {

void launch_quant_rows_mx8(const f16* X, int ldx, int M, int K, uint8_t* Q, int ldq, uint8_t* S, int lds, hipStream_t st) {
  if (M <= 0 || K <= 0 || (K & 31) || (ldx & 7) || (ldq & 7) || ldx < K || ldq < K || lds < K / 32 ||
      (reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(Q) & 7))
    throw std::runtime_error("quant_rows_mx8: K must be a multiple of 32, rows 16-byte aligned");
  hipLaunchKernelGGL(mpk::quant_rows_mx8_kernel, dim3(M), dim3(256), 0, st, X, ldx, K, Q, ldq, S, lds);
}

void launch_requant_mx8(const f16* W, int ldw, int n, int ntiles, int nsb, uint8_t* out, uint8_t* scales, hipStream_t st) {
  if (n <= 0 || n > ntiles * 16 || nsb <= 0 || ldw < nsb * 256 || (ldw & 7) || (reinterpret_cast<uintptr_t>(W) & 15) ||
      (reinterpret_cast<uintptr_t>(out) & 15))
    throw std::runtime_error("requant_mx8: bad weight shape or alignment");
  const int nchunks = mx8_groups(ntiles) * 4 * nsb;
  hipLaunchKernelGGL(mpk::requant_mx8_kernel, dim3((nchunks + 3) / 4), dim3(256), 0, st, W, ldw, n, nsb, nchunks, out,
                     scales);
}

void launch_relayout_mx4(const uint8_t* W, int ntiles, int nsb, uint8_t* out, uint8_t* scales, hipStream_t st) {
  if (ntiles <= 0 || nsb <= 0 || (reinterpret_cast<uintptr_t>(W) & 15) || (reinterpret_cast<uintptr_t>(out) & 15))
    throw std::runtime_error("relayout_mx4: bad weight shape or alignment");
  const int nchunks = mx8_groups(ntiles) * 4 * nsb;
  hipLaunchKernelGGL(mpk::relayout_mx4_kernel, dim3((nchunks + 3) / 4), dim3(256), 0, st, W, ntiles, nsb, nchunks, out, scales);
}

template <int EPI, int BM>
static void gemm_mx_go(const Mx8Params& p, bool allow_split, hipStream_t st) {
  const int n_cg = (p.ntiles + 15) / 16, n_mb = (p.M + BM - 1) / BM, wgs = n_cg * n_mb;
  int nsplit = 1;
  // split-K by gemm3's rule: fill the grid up to the split target, >= 1024 k (4 super-blocks) per split
  const int split_wg = knob(KNOB_GEMM2_SPLIT_WG);
  if (EPI == EPI_ATOMIC && allow_split && wgs < split_wg) nsplit = std::max(1, std::min(split_wg / wgs, p.nsb / 4));
  const int per = (p.nsb + nsplit - 1) / nsplit;
  nsplit = (p.nsb + per - 1) / per;
  if (p.bfmt) hipLaunchKernelGGL((mpk::gemm_mx_kernel<EPI, BM, 1>), dim3(wgs, nsplit), dim3(512), 0, st, p, n_mb, per);
  else hipLaunchKernelGGL((mpk::gemm_mx_kernel<EPI, BM, 0>), dim3(wgs, nsplit), dim3(512), 0, st, p, n_mb, per);
}

template <int EPI>
static void gemm_mx_shape(const Mx8Params& p, bool allow_split, hipStream_t st) {
  // 128-row tiles when one holds M, or when 256-row tiles would leave more than half the CUs without
  // a workgroup and the epilogue cannot split K to fill them
  const int wg256 = (p.ntiles + 15) / 16 * ((p.M + 255) / 256);
  const bool splits = EPI == EPI_ATOMIC && allow_split;
  if (p.M <= 128 || (wg256 < 128 && !splits)) gemm_mx_go<EPI, 128>(p, allow_split, st);
  else gemm_mx_go<EPI, 256>(p, allow_split, st);
}

void launch_gemm_mx8(int epi, const Mx8Params& p, hipStream_t st, bool allow_split) {
  const bool swiglu = epi == EPI_SWIGLU;
  if (p.M <= 0 || p.ntiles <= 0 || p.nsb <= 0 || p.ldx < p.nsb * 256 || (p.ldx & 15) || p.ldxs < p.nsb * 8 || (p.ldxs & 3) ||
      (reinterpret_cast<uintptr_t>(p.X) & 15) || (reinterpret_cast<uintptr_t>(p.xscale) & 3) ||
      (reinterpret_cast<uintptr_t>(p.W) & 15) || (reinterpret_cast<uintptr_t>(p.wscale) & 3) || !(swiglu ? (void*)p.H : (void*)p.Y) ||
      p.n_valid > (swiglu ? p.ntiles * 8 : p.ntiles * 16) || (p.bfmt != 0 && p.bfmt != 1))
    throw std::runtime_error("gemm_mx8: bad operand shape or alignment");
  switch (epi) {
    case EPI_STORE: return gemm_mx_shape<EPI_STORE>(p, allow_split, st);
    case EPI_ATOMIC: return gemm_mx_shape<EPI_ATOMIC>(p, allow_split, st);
    case EPI_SWIGLU: return gemm_mx_shape<EPI_SWIGLU>(p, allow_split, st);
    default: throw std::runtime_error("gemm_mx8: unknown epilogue");
  }
}

}  // namespace mp
