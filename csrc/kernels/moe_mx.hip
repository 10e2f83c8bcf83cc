// Grouped MoE expert GEMM on the scaled MFMA (mx8_gemm mode, M > 64 tokens): for every expert e, the
// rows the router listed for it (MX-FP8: e4m3 bytes + one e8m0 scale per 32 k) times that expert's B
// image -- launch_requant_mx8's e4m3 image or launch_relayout_mx4's fp4 image -- on
// v_mfma_scale_f32_32x32x64_f8f6f4, one launch per projection.  gemm_mx.hip's pipeline (W global ->
// VGPR one stage ahead, x through two swizzled LDS stage buffers with its scale dwords, counted
// lgkmcnt reads; the stage itself is gemm_mx_core.h's mx_stage) with gemm4_kernel<MOE>'s grouping:
//   grid      blockIdx.z = expert e, M_e = counts[e]; the x grid is n_cg * ceil(M / BM) (a token lists
//             an expert at most once), XCD-remapped; row block mb exits at once when mb * BM >= M_e.
//   A         row r of a tile is slot lists[e][min(m0 + r, M_e - 1)], read from x row slot (down) or
//             slot / k (gate/up): every thread's x piece and scale dword addresses are computed once
//             before the K loop.  List entries at or past counts[e] are never read.
//   B         W + e * estride_w, wscale + e * estride_s.
//   epilogue  SWIGLU scatters to H[slot] (tile rows 0-7 gate, 8-15 up), ATOMIC adds weights[slot] * acc
//             into Y[slot / k], K split over blockIdx.y (the router weight is linear in the sum).
// Row fragments (32 rows) wholly past M_e run no MFMA (uniform branch); their LDS reads stay.
//
// Tiles.  BM = 128: 8 waves x 32 columns, 4 row fragments per wave -- the dense kernel's 128-row form.
// BM = 64 (at most 64 rows per expert on average: Qwen3-MoE at 256 tokens has 16): a wave keeps TWO
// column groups (64 columns) and feeds both from each A fragment, so the workgroup spans 512 columns.
// With one group per wave a 64-row tile would issue the dense tile's LDS reads and barriers for half
// its MFMAs; two groups keep the 4 MFMAs per fragment read of the 128-row form, the same 64
// accumulator registers, and halve the workgroups that re-stage the same gathered rows.  The price is
// twice the B registers in flight (64 for e4m3).  The host picks the tile from M * k / E alone, so a
// captured launch serves any table contents.
//
// The down projection reads H re-quantized by launch_quant_rows_mx8 (one small launch per layer): a
// block of 32 H columns spans two waves' outputs under the SwiGLU tile layout, so the quantization
// does not fuse into the gate/up epilogue without a cross-wave exchange.
#include "gemm_mx_core.h"
#include "../runtime/kernels_api.h"
#include "../runtime/tuning.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mpk {
using namespace mp;

template <int EPI, int BM, int NPR, int BF>
__global__ __launch_bounds__(512) void moe_mx_kernel(const MoeMxParams p, const int n_mb, const int sb_per_split) {
  constexpr int NB = MxB<BF>::NB;    // 16-byte B pieces per lane per stage and column group
  constexpr int FM = BM / 32;        // row fragments per wave
  constexpr int AP = BM / 64;        // 16-byte x pieces per thread per stage
  constexpr int A_BYTES = BM * 128, STAGE = A_BYTES + 2048;   // x rows + a scale dword slot per thread (BM used)
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, cl = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lid = mx_xcd_lid(blockIdx.x, gridDim.x);
  const int cg = lid / n_mb, mb = lid - cg * n_mb;
  const int m0 = mb * BM, e = blockIdx.z;
  const int M = min(p.counts[e], p.list_cap);
  if (m0 >= M) return;   // uniform: this expert has fewer routed rows
  const int sb_begin = blockIdx.y * sb_per_split, sb_end = min(sb_begin + sb_per_split, p.nsb);
  if (sb_begin >= sb_end) return;
  const int fr_live = min(FM, (M - m0 + 31) >> 5);
  const int32_t* list = p.lists + (size_t)e * p.list_cap;

  // the wave's column groups (clamped: a group past the last computes a copy of it and stores nothing)
  const uint8_t* wb[NPR];
  const uint32_t* wsp[NPR];
#pragma unroll
  for (int pp = 0; pp < NPR; ++pp) {
    const int grp = min((cg * 8 + wave) * NPR + pp, (p.ntiles + 1) / 2 - 1);
    wb[pp] = MxB<BF>::pieces(p.W + (size_t)e * p.estride_w, grp, p.nsb, lane);
    wsp[pp] = MxB<BF>::scales(p.wscale + (size_t)e * p.estride_s, grp, p.nsb, lane);
  }
  // gathered x: piece i of this thread is tile row (tid >> 3) + 64 i, chunk tid & 7; thread t < BM also
  // carries row t's scale dword (threads >= BM fetch row BM - 1's into their own, unread slot)
  auto src_row = [&](int r) {
    const int slot = list[min(m0 + r, M - 1)];
    return p.x_per_slot ? slot : slot / p.k;
  };
  const int xrow = tid >> 3, xch = tid & 7;
  const uint8_t* xp[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) xp[i] = p.X + (size_t)src_row(xrow + 64 * i) * p.ldx + 16 * xch;
  const uint8_t* xsa = p.xscale + (size_t)src_row(min(tid, BM - 1)) * p.ldxs;

  auto fetch = [&](int s, u32x4 (&a)[AP], uint32_t& as, u32x4 (&b)[NPR][NB]) {
#pragma unroll
    for (int i = 0; i < AP; ++i) a[i] = ld16(xp[i] + (size_t)s * 128);
    as = *reinterpret_cast<const uint32_t*>(xsa + 4 * s);
#pragma unroll
    for (int pp = 0; pp < NPR; ++pp) MxB<BF>::fetch(wb[pp], s, b[pp]);
  };
  auto store_a = [&](int buf, const u32x4 (&a)[AP], uint32_t as) {
    char* A = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < AP; ++i) *reinterpret_cast<u32x4*>(A + g3_off(xrow + 64 * i, xch)) = a[i];
    reinterpret_cast<uint32_t*>(A + A_BYTES)[tid] = as;
  };

  f32x16 acc[FM][NPR];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int pp = 0; pp < NPR; ++pp)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[i][pp][v] = 0.f;

  const MxLdsAddr la(smem, A_BYTES, cl, h);
  u32x4 an[AP], b[2][NPR][NB];
  uint32_t asn, wsc[NPR], wsn[NPR];
#pragma unroll
  for (int pp = 0; pp < NPR; ++pp) wsc[pp] = wsp[pp][(size_t)sb_begin * 64];
  fetch(2 * sb_begin, an, asn, b[0]);
  store_a(0, an, asn);
  __syncthreads();
  for (int sb = sb_begin; sb < sb_end; ++sb) {
    fetch(2 * sb + 1, an, asn, b[1]);
    mx_stage<BF, FM, NPR, STAGE, 0, true>(la, h, b[0], wsc, acc, fr_live);
    store_a(1, an, asn);   // buffer 1's last readers passed the barrier that ended the previous stage
    __syncthreads();
    const int nx = min(sb + 1, sb_end - 1);   // (the last trip re-reads its own super-block: in bounds, unused)
    fetch(2 * nx, an, asn, b[0]);
#pragma unroll
    for (int pp = 0; pp < NPR; ++pp) wsn[pp] = wsp[pp][(size_t)nx * 64];
    mx_stage<BF, FM, NPR, STAGE, 1, true>(la, h, b[1], wsc, acc, fr_live);
    store_a(0, an, asn);
    __syncthreads();
#pragma unroll
    for (int pp = 0; pp < NPR; ++pp) wsc[pp] = wsn[pp];
  }

  // epilogue: lane holds C[row 32 i + 8 (v >> 2) + 4 h + (v & 3)][col cl] of each column group; row m of
  // the expert is slot list[m]
  const int rowb = m0 + 4 * h;
#pragma unroll
  for (int pp = 0; pp < NPR; ++pp) {
    const int n = ((cg * 8 + wave) * NPR + pp) * 32 + cl;
    if constexpr (EPI == EPI_SWIGLU) {
      const int o = (n >> 4) * 8 + (cl & 15);   // tile rows 0-7 gate, 8-15 up of the same 8 outputs
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const float other = __shfl_xor(acc[i][pp][v], 8);
          const int m = rowb + 32 * i + 8 * (v >> 2) + (v & 3);
          if ((cl & 8) == 0 && m < M && o < p.n_valid)
            p.H[(size_t)list[m] * p.ldh + o] = sat_f16(silu(acc[i][pp][v]) * other);
        }
    } else if (n < p.n_valid) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int m = rowb + 32 * i + 8 * (v >> 2) + (v & 3);
          if (m < M) {
            const int slot = list[m];
            unsafeAtomicAdd(p.Y + (size_t)(slot / p.k) * p.ldy + n, p.weights[slot] * acc[i][pp][v]);
          }
        }
    }
  }
}

}  // namespace mpk

namespace mp {

// 128-row tiles above 64 routed rows per expert on average (M * k / E), the 64-row two-group form at or
// below: host-only, from the launch's shape, never from the routing tables
int moe_mx_tile_rows(int M, int k, int E) { return (int64_t)M * k > (int64_t)64 * E ? 128 : 64; }

// Where the stages take this route instead of gemm4's MoE mode: from 128 routed rows per expert on average.
// Measured alone on an MI355X (tools/moe_bench.py, gate/up + down, us, gemm4 -> this kernel;
// profiles/moe_mx_bench.txt): Mixtral 8x7B at 512 tokens (128 rows per expert) Q4_K 1314 -> 1024, MXFP4
// 1296 -> 832; at 256 tokens (64) 465 -> 672 and 413 -> 490; at 96 (24) 318 -> 346 and 284 -> 235.
// Qwen3-30B-A3B (6, 16, 32 rows per expert at 96, 256, 512 tokens) is slower everywhere with the fp8 image
// and from 256 tokens with the fp4 image.  Below the threshold only the fp4 image at very few rows wins,
// and not on both models at the same M k / E, so the rule keeps to what held on every shape measured.
bool moe_mx_route(int M, int k, int E) { return (int64_t)M * k >= (int64_t)128 * E; }

template <int EPI, int BM, int NPR>
static void moe_mx_go(const MoeMxParams& p, hipStream_t st) {
  const int n_cg = (mx8_groups(p.ntiles) + 8 * NPR - 1) / (8 * NPR), n_mb = (p.M + BM - 1) / BM;
  int nsplit = 1;
  if (EPI == EPI_ATOMIC) {
    // split-K by gemm_mx's rule over the workgroups that can be busy: every routed expert has a row
    // block, and M k rows fill at least M k / BM of them
    const int64_t rows = (int64_t)p.M * p.k;
    const int64_t wgs = n_cg * std::max<int64_t>(std::min<int64_t>(p.E, rows), (rows + BM - 1) / BM);
    const int split_wg = knob(KNOB_GEMM2_SPLIT_WG);
    if (wgs < split_wg) nsplit = std::max(1, std::min((int)(split_wg / wgs), p.nsb / 4));
  }
  const int per = (p.nsb + nsplit - 1) / nsplit;
  nsplit = (p.nsb + per - 1) / per;
  const dim3 grid(n_cg * n_mb, nsplit, p.E);
  if (p.bfmt) hipLaunchKernelGGL((mpk::moe_mx_kernel<EPI, BM, NPR, 1>), grid, dim3(512), 0, st, p, n_mb, per);
  else hipLaunchKernelGGL((mpk::moe_mx_kernel<EPI, BM, NPR, 0>), grid, dim3(512), 0, st, p, n_mb, per);
}

void launch_moe_gemm_mx(int epi, const MoeMxParams& p, hipStream_t st) {
  auto bad = [](const std::string& what) { throw std::runtime_error("moe_gemm_mx: " + what); };
  const bool swiglu = epi == EPI_SWIGLU;
  if (epi != EPI_SWIGLU && epi != EPI_ATOMIC) bad("epilogue must be SWIGLU (gate/up) or ATOMIC (down)");
  if (p.bfmt != 0 && p.bfmt != 1) bad("bfmt must be 0 (e4m3) or 1 (fp4)");
  if (p.M <= 0 || p.ntiles <= 0 || p.nsb <= 0) bad("empty shape");
  if (p.E < 1 || p.E > 128) bad("E out of range (1..128)");
  if (p.k < 1 || p.k > 8 || p.k > p.E) bad("k out of range (1..min(8, E))");
  if (p.list_cap < p.M) bad("list_cap < M (an expert can list every token)");
  if (p.ldx < p.nsb * 256) bad("ldx < nsb * 256");
  if (p.ldxs < p.nsb * 8) bad("ldxs < nsb * 8");
  if ((p.ldx & 15) || (p.ldxs & 3) || (reinterpret_cast<uintptr_t>(p.X) & 15) || (reinterpret_cast<uintptr_t>(p.xscale) & 3) ||
      (reinterpret_cast<uintptr_t>(p.W) & 15) || (p.estride_w & 15) || (reinterpret_cast<uintptr_t>(p.wscale) & 3) ||
      (p.estride_s & 3))
    bad("bad alignment (x rows and images 16 bytes, scale rows and images 4)");
  if (!p.X || !p.xscale || !p.W || !p.wscale || !p.counts || !p.lists) bad("missing operand pointer");
  if (!(swiglu ? (void*)p.H : (void*)p.Y)) bad("missing output pointer");
  if (!swiglu && !p.weights) bad("missing router weights");
  if (p.n_valid <= 0 || p.n_valid > (swiglu ? p.ntiles * 8 : p.ntiles * 16)) bad("n_valid exceeds the image's columns");
  const bool wide = moe_mx_tile_rows(p.M, p.k, p.E) == 128;
  if (swiglu) wide ? moe_mx_go<EPI_SWIGLU, 128, 1>(p, st) : moe_mx_go<EPI_SWIGLU, 64, 2>(p, st);
  else wide ? moe_mx_go<EPI_ATOMIC, 128, 1>(p, st) : moe_mx_go<EPI_ATOMIC, 64, 2>(p, st);
}

}  // namespace mp
