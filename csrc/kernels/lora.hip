// LoRA on gfx950: Y[row] += user_scale[row] * B (A x[row]) for the rows of a call that are bound to an
// adapter (engine key "lora_adapters").  Rows are grouped by adapter, MoE-style, through the device
// tile table of lora.h: a tile count, then tiles of (adapter id, 16 row indices, -1 padded, the rows'
// scales).  A second table gives, per (adapter, layer, target), the f16 images A [r_pad][K] and
// B [N][r_pad] (alpha / r folded into B, ranks zero-filled to a multiple of 32); a null A means the
// adapter has no pair for that target.  A launch covers one group of up to three targets that share
// their input rows ({q, k, v}, {o}, {gate, up}, {down}).
//
// Grids are sized for the worst-case tile count, which is fixed when a decode graph is captured;
// workgroups past the count stored in the table return at once.  Nothing here uses float atomics:
//
//   shrink  t[row][j] = sum_k A[j][k] x[row][k] on v_mfma_f32_16x16x32_f16.  Both operands are
//           K-contiguous, so a lane's 8-element fragment is one 16-byte global load in the MFMA's own
//           layout (A operand: x row = lane & 15, B operand: rank j = lane & 15, k = 8 (lane >> 4) ..).
//           grid (tile, K split of 1024): each of the 4 waves keeps the x fragments of its 256-wide
//           K slice in registers (x is read once for all targets of the group) and walks the 16-rank
//           blocks of every target; the four wave sums meet in LDS (fixed order) and go out as that
//           split's partial [16 rows][rcap] -- no zero fill, every word expand reads was stored.
//   expand  sums the split partials in ascending order into LDS as an f16 hi + lo pair (the pair
//           carries t to ~2^-22, so the rounding of t adds nothing to the f16 rounding of x, A and B),
//           then Y += scale * (t B^T) with the rank as the MFMA's reduction axis (B is r_pad-contiguous).
//           grid (tile, 1024 output columns of the stacked targets).  Each output element is a plain
//           f32 read-modify-write by the one lane that owns it: rows of no tile, columns of absent
//           targets and padding are never touched.
#include <algorithm>
#include <stdexcept>
#include <string>

#include "kcommon.h"
#include "../runtime/kernels_api.h"

namespace mpk {
using namespace mp;

constexpr int kLoraThreads = 256, kLoraWaves = 4;
constexpr int kShrinkWaveK = 256;                             // 8 MFMA k-steps per wave
constexpr int kShrinkWgK = kShrinkWaveK * kLoraWaves;
constexpr int kExpandTilesPerWave = 16;                       // 16-column tiles per wave
constexpr int kExpandTilesPerWg = kExpandTilesPerWave * kLoraWaves;
constexpr int kLdT = kLoraMaxRank + 8;                        // LDS row stride of t (f16)

__device__ __forceinline__ half8_t zero8() { return half8_t{0, 0, 0, 0, 0, 0, 0, 0}; }
__device__ __forceinline__ half8_t ldh8(const f16* p) { return __builtin_bit_cast(half8_t, ld16(p)); }

__device__ __forceinline__ int pick3(const int* v, int i) { return i == 0 ? v[0] : i == 1 ? v[1] : v[2]; }

__global__ __launch_bounds__(kLoraThreads) void lora_shrink_kernel(const LoraGroupParams p) {
  __shared__ float red[2][kLoraWaves][256];
  const int tile = blockIdx.x;
  if (tile >= p.tiles[0]) return;
  const LoraTile* T = reinterpret_cast<const LoraTile*>(p.tiles + kLoraTabHeader) + tile;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int row = T->rows[r];
  const int kb = ((int)blockIdx.y * kLoraWaves + w) * kShrinkWaveK + g * 8;
  half8_t xf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int k = kb + s * 32;
    xf[s] = row >= 0 && k < p.K ? ldh8(p.X + (size_t)row * p.ldx + k) : zero8();
  }
  const LoraTargetRec* rec = p.targets + ((size_t)T->adapter * p.n_layers + p.layer) * LORA_N_TARGETS;
  const int nsplit = gridDim.y;
  int it = 0;
#pragma unroll
  for (int ti = 0; ti < 3; ++ti) {
    if (ti >= p.n_t) break;
    const LoraTargetRec tr = rec[p.tgt[ti]];
    if (!tr.A || tr.r_pad > p.rcap) continue;   // (a rank past the partial stride cannot come from the loader)
    float* out = p.part + ((((size_t)tile * nsplit + blockIdx.y) * p.n_t + ti) * kLoraTileRows) * p.rcap;
    for (int jb = 0; jb < tr.r_pad / 16; ++jb, ++it) {
      const f16* a = reinterpret_cast<const f16*>(tr.A) + (size_t)(jb * 16 + r) * p.K;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int k = kb + s * 32;
        const half8_t af = k < p.K ? ldh8(a + k) : zero8();
        acc = mfma16x16x32(xf[s], af, acc);
      }
      float* buf = red[it & 1][w];
#pragma unroll
      for (int i = 0; i < 4; ++i) buf[(g * 4 + i) * 16 + r] = acc[i];   // [x row][rank]
      __syncthreads();
      if (w == (it & 3)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = lane + 64 * i;
          const float v = ((red[it & 1][0][e] + red[it & 1][1][e]) + red[it & 1][2][e]) + red[it & 1][3][e];
          out[(size_t)(e >> 4) * p.rcap + jb * 16 + (e & 15)] = v;
        }
      }
      // (the buffer written two blocks from now is this one: every wave has passed the next
      // block's barrier by then, and the wave that read it did so before that barrier)
    }
  }
}

__global__ __launch_bounds__(kLoraThreads) void lora_expand_kernel(const LoraGroupParams p, const int nsplit) {
  __shared__ __attribute__((aligned(16))) f16 th[3][kLoraTileRows][kLdT];
  __shared__ __attribute__((aligned(16))) f16 tl[3][kLoraTileRows][kLdT];
  const int tile = blockIdx.x;
  if (tile >= p.tiles[0]) return;
  const LoraTile* T = reinterpret_cast<const LoraTile*>(p.tiles + kLoraTabHeader) + tile;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const LoraTargetRec* rec = p.targets + ((size_t)T->adapter * p.n_layers + p.layer) * LORA_N_TARGETS;
  const size_t split_stride = (size_t)p.n_t * kLoraTileRows * p.rcap;
#pragma unroll
  for (int ti = 0; ti < 3; ++ti) {
    if (ti >= p.n_t) break;
    const LoraTargetRec tr = rec[p.tgt[ti]];
    if (!tr.A || tr.r_pad > p.rcap) continue;   // (a rank past the partial stride cannot come from the loader)
    const float* src = p.part + (((size_t)tile * nsplit) * p.n_t + ti) * kLoraTileRows * p.rcap;
    for (int e = tid; e < kLoraTileRows * tr.r_pad; e += kLoraThreads) {
      const int row = e / tr.r_pad, j = e - row * tr.r_pad;
      float s = 0.f;
      for (int sp = 0; sp < nsplit; ++sp) s += src[sp * split_stride + (size_t)row * p.rcap + j];
      const f16 h = (f16)s;
      th[ti][row][j] = h;
      tl[ti][row][j] = (f16)(s - (float)h);
    }
  }
  __syncthreads();
  const int nct0 = (p.N[0] + 15) >> 4, nct1 = p.n_t > 1 ? (p.N[1] + 15) >> 4 : 0, nct2 = p.n_t > 2 ? (p.N[2] + 15) >> 4 : 0;
  const int total = nct0 + nct1 + nct2;
  for (int q = 0; q < kExpandTilesPerWave; ++q) {
    int c = (int)blockIdx.y * kExpandTilesPerWg + q * kLoraWaves + w;
    if (c >= total) break;
    int ti = 0;
    if (c >= nct0) { c -= nct0; ti = 1; if (c >= nct1) { c -= nct1; ti = 2; } }
    const LoraTargetRec tr = rec[pick3(p.tgt, ti)];
    if (!tr.A || tr.r_pad > p.rcap) continue;
    const int N = pick3(p.N, ti), n = c * 16 + r;
    const f16* b = reinterpret_cast<const f16*>(tr.B) + (size_t)n * tr.r_pad + g * 8;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < tr.r_pad / 32; ++s) {
      const half8_t bf = n < N ? ldh8(b + s * 32) : zero8();
      const half8_t hi = *reinterpret_cast<const half8_t*>(&th[ti][r][s * 32 + g * 8]);
      const half8_t lo = *reinterpret_cast<const half8_t*>(&tl[ti][r][s * 32 + g * 8]);
      acc = mfma16x16x32(hi, bf, acc);
      acc = mfma16x16x32(lo, bf, acc);
    }
    if (n >= N) continue;
    float* ycol = p.Y + pick3(p.yoff, ti) + n;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = T->rows[g * 4 + i];
      if (row < 0) continue;
      float* y = ycol + (size_t)row * p.ldy;
      *y += T->scale[g * 4 + i] * acc[i];
    }
  }
}

constexpr int kLoraTabBatch = 24;   // tiles per launch, by value (under the 4 KiB of kernel arguments)
struct LoraTileBatch { LoraTile t[kLoraTabBatch]; };

__global__ __launch_bounds__(256) void lora_table_kernel(int32_t* tab, const LoraTileBatch b, int first, int n, int total) {
  if (first == 0 && threadIdx.x == 0) tab[0] = total;
  int32_t* dst = tab + kLoraTabHeader + (size_t)first * kLoraTileWords;
  const int32_t* src = reinterpret_cast<const int32_t*>(&b);
  for (int i = threadIdx.x; i < n * kLoraTileWords; i += blockDim.x) dst[i] = src[i];
}

}  // namespace mpk

namespace mp {

int lora_ksplits(int K) { return (K + mpk::kShrinkWgK - 1) / mpk::kShrinkWgK; }

size_t lora_part_floats(int max_tiles, int K, int n_t, int rcap) {
  return (size_t)max_tiles * lora_ksplits(K) * n_t * kLoraTileRows * rcap;
}

static void lora_check(const LoraGroupParams& p, const char* who) {
  auto bad = [&](const std::string& m) { throw std::runtime_error(std::string(who) + ": " + m); };
  if (!p.tiles || !p.targets || !p.X || !p.Y || !p.part) bad("null pointer");
  if (p.max_tiles < 1) bad("max_tiles must be positive");
  if (p.n_t < 1 || p.n_t > 3) bad("a group holds 1..3 targets");
  if (p.n_adapters < 1 || p.n_adapters > kLoraMaxAdapters || p.layer < 0 || p.layer >= p.n_layers) bad("bad adapter / layer index");
  if (p.K < 8 || p.K % 8 || p.ldx < p.K || p.ldx % 8 || (reinterpret_cast<uintptr_t>(p.X) & 15)) bad("x rows must be 16-byte aligned, K a multiple of 8");
  if (p.rcap < 32 || p.rcap > kLoraMaxRank || p.rcap % 32) bad("rcap must be a multiple of 32 up to " + std::to_string(kLoraMaxRank));
  for (int i = 0; i < p.n_t; ++i) {
    if (p.tgt[i] < 0 || p.tgt[i] >= LORA_N_TARGETS || p.N[i] < 1 || p.yoff[i] < 0 || p.yoff[i] + p.N[i] > p.ldy) bad("bad target columns");
  }
  if (p.part_floats < lora_part_floats(p.max_tiles, p.K, p.n_t, p.rcap)) bad("partial buffer too small");
}

void launch_lora_shrink(const LoraGroupParams& p, hipStream_t st) {
  lora_check(p, "lora_shrink");
  hipLaunchKernelGGL(mpk::lora_shrink_kernel, dim3(p.max_tiles, lora_ksplits(p.K)), dim3(mpk::kLoraThreads), 0, st, p);
}

void launch_lora_expand(const LoraGroupParams& p, hipStream_t st) {
  lora_check(p, "lora_expand");
  int ct = 0;
  for (int i = 0; i < p.n_t; ++i) ct += (p.N[i] + 15) / 16;
  hipLaunchKernelGGL(mpk::lora_expand_kernel, dim3(p.max_tiles, (ct + mpk::kExpandTilesPerWg - 1) / mpk::kExpandTilesPerWg),
                     dim3(mpk::kLoraThreads), 0, st, p, lora_ksplits(p.K));
}

void launch_lora_table(int32_t* dev_tab, const int32_t* host_tab, int max_tiles, hipStream_t st) {
  const int n = host_tab[0];
  if (!dev_tab || n < 0 || n > max_tiles) throw std::runtime_error("lora_table: bad tile count");
  const LoraTile* tiles = reinterpret_cast<const LoraTile*>(host_tab + kLoraTabHeader);
  int first = 0;
  do {
    mpk::LoraTileBatch b{};
    const int m = std::min(mpk::kLoraTabBatch, n - first);
    for (int i = 0; i < m; ++i) b.t[i] = tiles[first + i];
    hipLaunchKernelGGL(mpk::lora_table_kernel, dim3(1), dim3(256), 0, st, dev_tab, b, first, m, n);
    first += m;
  } while (first < n);
}

}  // namespace mp
