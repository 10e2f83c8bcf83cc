// Context shift over the paged KV cache (Engine::context_shift): positions [n_keep, n_keep + n_discard)
// of a slot leave the cache and every later entry moves n_discard positions back.  V is position-free
// and K is stored post-RoPE in adjacent pairs, so the move is a block-table edit (KvPager::shift) plus
// one pass over the slot's tail K rows that rotates each pair by minus n_discard positions:
//   (c, s) = rope_cs[n_discard][j]      (x0, x1) -> (x0 c + x1 s, x1 c - x0 s)
// in f32 from the stored code, rounded back to the cache's element type (f16 or e4m3); pairs j >= hd / 2
// (the padding of a row up to Dp) are written as zero.
//
// n_discard is a multiple of the page size, so a row keeps its index inside its page.  With the NEW
// block table, entry t >= n_keep / 64 of the slot's row is a tail page:
//   * rotated in place -- every 16-byte piece is read and written by the same lane, no workgroup
//     touches another's rows;
//   * except the page holding n_keep when r0 = n_keep % 64 != 0: its rows [r0, 64) take the rotated K
//     rows and the V rows [r0, 64) of the record's merge_src_page (the old page n_keep/64 + n_discard/64,
//     free afterwards); rows < r0 keep their bytes.
// Rows at or past the new length (the never-live end of the last page) are not touched either.
//
// Geometry: workgroup (t, kv head, record) owns one page of one head: 64 rows of Dp / 8 (f16) or
// Dp / 16 (e4m3) 16-byte pieces.  The block has 16 lanes per piece column -- 16 x pieces per row = 64,
// 128 or 256 threads, so every wave has work at every Dp and type -- and a lane keeps its column over
// its 4 rows (row = tid / pieces per row + 16 i): it reads its 4 (f16) or 8 (e4m3) pairs of
// rope_cs[n_discard] once for the page, issues its 4 row loads together, then rotates and stores.  The
// merge page also copies its V rows: an 8-key run of one dim is contiguous in both V layouts
// (kernels_api.h), 16 B of f16 or 8 B of e4m3, and a lane moves 4 or 8 runs, loads first.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "kcommon.h"
#include "../runtime/kernels_api.h"

namespace mpk {
using namespace mp;

constexpr int kShiftMaxThreads = 256;
constexpr int kShiftRowLanes = 16;   // lanes per piece column
constexpr int kShiftIter = 64 / kShiftRowLanes;   // rows per lane

__device__ __forceinline__ bool is_pad(float2 c) { return c.x == 0.f && c.y == 0.f; }

// threads of a workgroup: 16 per 16-byte piece of a row
inline int kv_shift_threads(int Dp, bool fp8) { return kShiftRowLanes * (Dp / (fp8 ? 16 : 8)); }

template <bool FP8>
__global__ __launch_bounds__(kShiftMaxThreads) void kv_shift_kernel(const KvShiftParams p) {
  constexpr int EB = FP8 ? 1 : 2;          // bytes per element
  constexpr int EPP = 16 / EB;             // elements per 16-byte piece
  constexpr int PPP = EPP / 2;             // pairs per piece
  const KvShiftRec r = p.rec[blockIdx.z];
  const int kk = r.n_keep >> 6, r0 = r.n_keep & 63;
  const int new_len = r.old_len - r.n_discard;
  const int t = kk + (int)blockIdx.x;
  const bool merge = t == kk && r0 != 0;
  // first moved position of this page; nothing at or past the new length is live
  if (t >= p.max_pages || (merge ? r.n_keep : t * 64) >= new_len) return;
  const int row_lo = merge ? r0 : 0, row_hi = min(64, new_len - t * 64);   // the page's moved rows
  const int dst_page = p.block_table[(size_t)r.slot * p.max_pages + t];
  const int src_page = merge ? r.merge_src_page : dst_page;
  if (dst_page < 0 || dst_page >= p.n_pages || src_page < 0 || src_page >= p.n_pages) return;   // never a live page
  const int h = blockIdx.y;
  const size_t head_elems = (size_t)64 * p.Dp;
  const size_t src_head = ((size_t)src_page * p.Hkv + h) * head_elems * EB;
  const size_t dst_head = ((size_t)dst_page * p.Hkv + h) * head_elems * EB;

  // ---- K rows
  const int ppr = p.Dp / EPP;              // pieces per row: 4, 8 or 16 (blockDim.x = 16 ppr)
  const int col = threadIdx.x % ppr, row0 = threadIdx.x / ppr;
  const int hd2 = p.hd >> 1;
  float2 cs[PPP];
#pragma unroll
  for (int i = 0; i < PPP; ++i) {
    const int j = col * PPP + i;
    // (0, 0), which no table entry is, marks a padding pair: stored as zero
    cs[i] = j < hd2 ? p.rope_cs[(size_t)r.n_discard * hd2 + j] : make_float2(0.f, 0.f);
  }
  const uint8_t* ks = reinterpret_cast<const uint8_t*>(p.k_cache) + src_head + (size_t)col * 16;
  uint8_t* kd = reinterpret_cast<uint8_t*>(p.k_cache) + dst_head + (size_t)col * 16;
  const size_t row_bytes = (size_t)p.Dp * EB;
  u32x4 in[kShiftIter];
#pragma unroll
  for (int it = 0; it < kShiftIter; ++it) {
    const int row = row0 + kShiftRowLanes * it;
    if (row >= row_lo && row < row_hi) in[it] = ld16(ks + row * row_bytes);
  }
#pragma unroll
  for (int it = 0; it < kShiftIter; ++it) {
    const int row = row0 + kShiftRowLanes * it;
    if (row < row_lo || row >= row_hi) continue;
    u32x4 out;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if constexpr (FP8) {
        const half2_t a = f8x2_lo(in[it][w]), b = f8x2_hi(in[it][w]);
        const float2 ca = cs[2 * w], cb = cs[2 * w + 1];
        const float a0 = (float)a.x, a1 = (float)a.y, b0 = (float)b.x, b1 = (float)b.y;
        const uint32_t lo = is_pad(ca) ? 0u : f8x2_pack(a0 * ca.x + a1 * ca.y, a1 * ca.x - a0 * ca.y);
        const uint32_t hi = is_pad(cb) ? 0u : f8x2_pack(b0 * cb.x + b1 * cb.y, b1 * cb.x - b0 * cb.y);
        out[w] = lo | (hi << 16);
      } else {
        const half2_t a = as_h2(in[it][w]);
        const float2 c = cs[w];
        const float x0 = (float)a.x, x1 = (float)a.y;
        out[w] = is_pad(c) ? 0u : as_u32(half2_t{(f16)(x0 * c.x + x1 * c.y), (f16)(x1 * c.x - x0 * c.y)});
      }
    }
    *reinterpret_cast<u32x4*>(kd + row * row_bytes) = out;
  }
  if (!merge) return;

  // ---- V rows [r0, row_hi) of the merge page: 8 Dp runs of 8 keys, 4 (f16) or 8 (e4m3) per lane, all
  // loaded before the first store.  A run that r0 or the new length splits is blended in registers with
  // the destination's own run and stored whole: its other keys are rewritten with the bytes they hold
  // (this lane is the only writer of the run).
  typedef typename std::conditional<FP8, u32x2, u32x4>::type run_t;   // 8 keys of one dim
  constexpr int VIT = FP8 ? 8 : 4;         // 8 Dp / blockDim.x
  constexpr int EPW = 4 / EB;              // elements per 32-bit word
  const uint8_t* __restrict__ vs = reinterpret_cast<const uint8_t*>(p.v_cache) + src_head;
  uint8_t* __restrict__ vd = reinterpret_cast<uint8_t*>(p.v_cache) + dst_head;
  run_t sv[VIT], dv[VIT];
#pragma unroll
  for (int it = 0; it < VIT; ++it) {
    const int u = threadIdx.x + it * blockDim.x, kb = u / p.Dp, d = u % p.Dp;
    const int k_lo = max(0, r0 - kb * 8), k_hi = min(8, row_hi - kb * 8);   // keys of the run that move
    const size_t off = ((size_t)kb * p.v_kb + (size_t)d * p.v_d) * EB;
    if (k_lo < k_hi) sv[it] = *reinterpret_cast<const run_t*>(vs + off);
    if (k_lo < k_hi && (k_lo > 0 || k_hi < 8)) dv[it] = *reinterpret_cast<const run_t*>(vd + off);
  }
#pragma unroll
  for (int it = 0; it < VIT; ++it) {
    const int u = threadIdx.x + it * blockDim.x, kb = u / p.Dp, d = u % p.Dp;
    const int k_lo = max(0, r0 - kb * 8), k_hi = min(8, row_hi - kb * 8);
    if (k_lo >= k_hi) continue;
    const size_t off = ((size_t)kb * p.v_kb + (size_t)d * p.v_d) * EB;
    run_t out = sv[it];
    if (k_lo > 0 || k_hi < 8) {
#pragma unroll
      for (int w = 0; w < 8 / EPW; ++w) {
        uint32_t m = 0;
#pragma unroll
        for (int b = 0; b < EPW; ++b) {
          const int e = w * EPW + b;
          if (e >= k_lo && e < k_hi) m |= (EB == 2 ? 0xFFFFu : 0xFFu) << (8 * EB * b);
        }
        out[w] = (sv[it][w] & m) | (dv[it][w] & ~m);
      }
    }
    *reinterpret_cast<run_t*>(vd + off) = out;
  }
}

}  // namespace mpk

namespace mp {

void launch_kv_shift(const KvShiftParams& p_in, hipStream_t st) {
  KvShiftParams p = p_in;
  auto bad = [](const std::string& what) { throw std::runtime_error("kv_shift: " + what); };
  if (p.n_rec <= 0) return;
  if (p.n_rec > kKvShiftMaxRec) bad("more than " + std::to_string(kKvShiftMaxRec) + " records in one launch");
  if (!p.k_cache || !p.v_cache || !p.block_table || !p.rope_cs) bad("null pointer");
  if (p.Dp != 64 && p.Dp != 128) bad("Dp must be 64 or 128");
  if (p.hd < 2 || (p.hd & 1) || p.hd > p.Dp) bad("hd must be even and <= Dp");
  if (p.Hkv < 1 || p.max_pages < 1 || p.n_pages < 1 || p.n_slots < 1) bad("bad geometry");
  v_strides_or_legacy(p.v_kb, p.v_d);
  const bool legacy = p.v_kb == 8 && p.v_d == 64, blocked = p.v_kb == p.Dp * 8 && p.v_d == 8;
  if (!legacy && !blocked) bad("V strides are neither the legacy nor the blocked layout");
  int tail_max = 0;
  for (int i = 0; i < p.n_rec; ++i) {
    const KvShiftRec& r = p.rec[i];
    const std::string id = "record " + std::to_string(i) + ": ";
    if (r.slot < 0 || r.slot >= p.n_slots) bad(id + "slot out of range");
    for (int k = 0; k < i; ++k)
      if (p.rec[k].slot == r.slot) bad(id + "slot listed twice");
    if (r.n_keep < 0) bad(id + "n_keep < 0");
    if (r.n_discard <= 0 || r.n_discard % 64 != 0) bad(id + "n_discard must be a positive multiple of 64");
    if (r.n_discard >= p.rope_rows) bad(id + "n_discard is outside the rope table");
    if (r.old_len > p.max_pages * 64) bad(id + "old_len exceeds the slot's table row");
    if (r.n_keep + r.n_discard > r.old_len) bad(id + "n_keep + n_discard > old_len");
    const bool merge = r.n_keep % 64 != 0;
    if (merge ? (r.merge_src_page < 0 || r.merge_src_page >= p.n_pages) : r.merge_src_page != -1)
      bad(id + "merge_src_page must be a pool page when n_keep % 64 != 0, and -1 otherwise");
    const int new_len = r.old_len - r.n_discard;
    tail_max = std::max(tail_max, (new_len + 63) / 64 - r.n_keep / 64);
  }
  if (tail_max <= 0) return;   // nothing after the discarded range
  const dim3 grid(tail_max, p.Hkv, p.n_rec), block(mpk::kv_shift_threads(p.Dp, p.kv_fp8 != 0));
  if (p.kv_fp8) hipLaunchKernelGGL(mpk::kv_shift_kernel<true>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(mpk::kv_shift_kernel<false>, grid, block, 0, st, p);
}

}  // namespace mp
