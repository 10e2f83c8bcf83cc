// Embedding pooling (last stage of an embed chunk): output RMSNorm of the chunk's residual rows,
// pooling of each prompt's rows (mean / cls / last / none), optional L2 normalisation.
//
// Memory-bound row kernels in the style of elementwise.hip: f32 rows read and written as float4,
// one 256-thread workgroup (4 waves) per row or per column slab.  Every sum has a fixed order: no
// float atomics, and nothing a prompt's vector depends on is shared with another prompt of the
// chunk, so a prompt pools to the same bits whatever else its chunks carry.
//
//   last / cls : pool_row_kernel, one workgroup per segment that holds the kept row
//   none       : pool_row_kernel, one workgroup per row of the chunk -> h [T][d]
//   mean       : pool_row_kernel -> h [T][d], then pool_colsum_kernel over (32-row block of a segment,
//                1024-column slab) -> part [block][d], then pool_finish_kernel, one workgroup per
//                segment: the segment's blocks added in block order onto pool_acc[slot] (stored, not
//                added, by the p0 == 0 segment), and on the prompt-ending segment scaled by
//                1 / prompt_len and normalised -> emb[slot]
#include "kcommon.h"
#include <algorithm>
#include <stdexcept>
#include <string>
#include "../runtime/kernels_api.h"

namespace mpk {
using namespace mp;

constexpr int PT = 256;                 // threads per workgroup
constexpr int PV = kPoolMaxD / 4 / PT;  // float4 per thread of a whole row (d <= 8192)

// the 4 waves' values added in wave order; every thread gets the total
__device__ __forceinline__ float pool_block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}

struct PoolSegBatch { PoolSeg s[kPoolSegBatch]; };

// the segment table reaches the device through the kernel arguments: no host buffer has to outlive
// the call, and the write is ordered on the stream like everything else that uses the table
__global__ void pool_table_kernel(PoolSeg* tab, const PoolSegBatch b, int n) {
  const int i = threadIdx.x;
  if (i < n) tab[i] = b.s[i];
}

// h = x * rsqrt(mean(x^2) + eps) * w of one row (launch_rmsnorm's f32 arithmetic), then with
// `normalize` h * (s > 0 ? 1 / sqrt(s) : 0), s = sum h^2.
// by_seg = 0: row blockIdx.x of the chunk -> dst + row * d.
// by_seg = 1: segment blockIdx.x: POOL_LAST keeps the final row of a prompt-ending segment, POOL_CLS
//             row 0 of a p0 == 0 segment -> dst + slot * d; other segments write nothing.
__global__ __launch_bounds__(PT) void pool_row_kernel(const float* x, int ldx, const float* w, int d, float eps,
                                                      const PoolSeg* segs, int by_seg, int pooling, int normalize,
                                                      float* dst) {
  __shared__ float red[4];
  int row = blockIdx.x, orow = blockIdx.x;
  if (by_seg) {
    const PoolSeg sg = segs[blockIdx.x];
    if (pooling == POOL_LAST) {
      if (!sg.ends_prompt) return;
      row = sg.row0 + sg.T - 1;
    } else {
      if (sg.p0 != 0) return;
      row = sg.row0;
    }
    orow = sg.slot;
  }
  const float* xr = x + (size_t)row * ldx;
  const int tid = threadIdx.x;
  float4 v[PV], ww[PV];
#pragma unroll
  for (int k = 0; k < PV; ++k) {
    const int i = (tid + PT * k) * 4;
    v[k] = i < d ? *reinterpret_cast<const float4*>(xr + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    ww[k] = i < d ? *reinterpret_cast<const float4*>(w + i) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < PV; ++k) ss += v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z + v[k].w * v[k].w;
  const float sc = rsqrtf(pool_block_sum(ss, red) / (float)d + eps);
  float s2 = 0.f;
#pragma unroll
  for (int k = 0; k < PV; ++k) {
    v[k].x = v[k].x * sc * ww[k].x; v[k].y = v[k].y * sc * ww[k].y;
    v[k].z = v[k].z * sc * ww[k].z; v[k].w = v[k].w * sc * ww[k].w;
    s2 += v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z + v[k].w * v[k].w;
  }
  float l2 = 1.f;
  if (normalize) {
    const float s = pool_block_sum(s2, red);
    l2 = s > 0.f ? 1.f / sqrtf(s) : 0.f;
  }
  float* o = dst + (size_t)orow * d;
#pragma unroll
  for (int k = 0; k < PV; ++k) {
    const int i = (tid + PT * k) * 4;
    if (i < d) *reinterpret_cast<float4*>(o + i) = make_float4(v[k].x * l2, v[k].y * l2, v[k].z * l2, v[k].w * l2);
  }
}

// mean: part[block][c] = sum of h[r][c] over the block's rows, r ascending.  Blocks are numbered
// segment by segment, kPoolBlockRows rows each counted from the segment's first row (so a prompt's
// blocks do not depend on where its segment sits in the chunk); grid.y = 1024-column slabs.
__global__ __launch_bounds__(PT) void pool_colsum_kernel(const float* h, int d, const PoolSeg* segs, int n_seg,
                                                         float* part) {
  const int c = (blockIdx.y * PT + threadIdx.x) * 4;
  if (c >= d) return;
  int b = blockIdx.x, s = 0;
  for (; s < n_seg; ++s) {
    const int nb = (segs[s].T + kPoolBlockRows - 1) / kPoolBlockRows;
    if (b < nb) break;
    b -= nb;
  }
  if (s == n_seg) return;
  const int r0 = segs[s].row0 + b * kPoolBlockRows;
  const int nr = min(kPoolBlockRows, segs[s].T - b * kPoolBlockRows);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* hp = h + (size_t)r0 * d + c;
#pragma unroll 8
  for (int r = 0; r < nr; ++r) {
    const float4 t = *reinterpret_cast<const float4*>(hp + (size_t)r * d);
    a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
  }
  *reinterpret_cast<float4*>(part + (size_t)blockIdx.x * d + c) = a;
}

// mean: one workgroup per segment
__global__ __launch_bounds__(PT) void pool_finish_kernel(const float* part, int d, const PoolSeg* segs, int normalize,
                                                         float* pool_acc, float* emb) {
  __shared__ float red[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  int b0 = 0;
  for (int j = 0; j < s; ++j) b0 += (segs[j].T + kPoolBlockRows - 1) / kPoolBlockRows;
  const PoolSeg sg = segs[s];
  const int nb = (sg.T + kPoolBlockRows - 1) / kPoolBlockRows;
  float* acc = pool_acc + (size_t)sg.slot * d;
  float4 v[PV];
#pragma unroll
  for (int k = 0; k < PV; ++k) {
    const int i = (tid + PT * k) * 4;
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i >= d) continue;
    if (sg.p0 != 0) v[k] = *reinterpret_cast<const float4*>(acc + i);
    for (int b = 0; b < nb; ++b) {
      const float4 t = *reinterpret_cast<const float4*>(part + (size_t)(b0 + b) * d + i);
      v[k].x += t.x; v[k].y += t.y; v[k].z += t.z; v[k].w += t.w;
    }
    *reinterpret_cast<float4*>(acc + i) = v[k];
  }
  if (!sg.ends_prompt) return;
  const float inv = 1.f / (float)sg.prompt_len;
  float s2 = 0.f;
#pragma unroll
  for (int k = 0; k < PV; ++k) {
    v[k].x *= inv; v[k].y *= inv; v[k].z *= inv; v[k].w *= inv;
    s2 += v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z + v[k].w * v[k].w;
  }
  float l2 = 1.f;
  if (normalize) {
    const float t = pool_block_sum(s2, red);
    l2 = t > 0.f ? 1.f / sqrtf(t) : 0.f;
  }
  float* o = emb + (size_t)sg.slot * d;
#pragma unroll
  for (int k = 0; k < PV; ++k) {
    const int i = (tid + PT * k) * 4;
    if (i < d) *reinterpret_cast<float4*>(o + i) = make_float4(v[k].x * l2, v[k].y * l2, v[k].z * l2, v[k].w * l2);
  }
}

}  // namespace mpk

namespace mp {

int pool_blocks(const PoolSeg* segs, int n_seg) {
  int n = 0;
  for (int i = 0; i < n_seg; ++i) n += (segs[i].T + kPoolBlockRows - 1) / kPoolBlockRows;
  return n;
}

void launch_pool_embed(const PoolParams& p, hipStream_t st) {
  auto bad = [](const std::string& m) { throw std::runtime_error("pool_embed: " + m); };
  if (p.pooling < POOL_NONE || p.pooling > POOL_LAST) bad("pooling must be none, mean, cls or last");
  if (p.d < 64 || p.d % 64 || p.d > kPoolMaxD) bad("d must be a multiple of 64 up to " + std::to_string(kPoolMaxD));
  if (p.ldx < p.d || p.ldx % 4) bad("bad row stride");
  if (!p.x || !p.w || !p.segs || !p.seg_tab) bad("missing buffer");
  if (p.T < 1 || p.n_seg < 1 || p.n_seg > p.seg_cap) bad("bad chunk shape");
  // the table is checked here, on the host, before anything indexes device memory by it
  int row = 0;
  for (int i = 0; i < p.n_seg; ++i) {
    const PoolSeg& s = p.segs[i];
    if (s.row0 != row || s.T < 1) bad("segments must tile the chunk's rows in order");
    if (s.slot < 0 || s.slot >= p.n_slots) bad("slot out of range");
    if (s.p0 < 0 || (s.ends_prompt && s.prompt_len != s.p0 + s.T) || (!s.ends_prompt && s.prompt_len < s.p0 + s.T))
      bad("segment positions do not fit prompt_len");
    for (int j = 0; j < i; ++j)
      if (p.segs[j].slot == s.slot) bad("two segments of one slot in a chunk");
    row += s.T;
  }
  if (row != p.T) bad("segments must tile the chunk's rows in order");
  if (p.pooling == POOL_NONE || p.pooling == POOL_MEAN) {
    if (!p.h) bad("missing row buffer");
  }
  if (p.pooling != POOL_NONE && !p.emb) bad("missing result buffer");
  const int nblk = pool_blocks(p.segs, p.n_seg);
  if (p.pooling == POOL_MEAN && (!p.part || !p.pool_acc || nblk > p.part_cap)) bad("missing or short partial buffers");

  for (int i0 = 0; i0 < p.n_seg; i0 += kPoolSegBatch) {
    mpk::PoolSegBatch b{};
    const int n = std::min(kPoolSegBatch, p.n_seg - i0);
    for (int i = 0; i < n; ++i) b.s[i] = p.segs[i0 + i];
    hipLaunchKernelGGL(mpk::pool_table_kernel, dim3(1), dim3(64), 0, st, p.seg_tab + i0, b, n);
  }
  const int norm = p.normalize ? 1 : 0;
  if (p.pooling == POOL_NONE) {
    hipLaunchKernelGGL(mpk::pool_row_kernel, dim3(p.T), dim3(mpk::PT), 0, st, p.x, p.ldx, p.w, p.d, p.eps, p.seg_tab, 0,
                       p.pooling, norm, p.h);
  } else if (p.pooling == POOL_MEAN) {
    hipLaunchKernelGGL(mpk::pool_row_kernel, dim3(p.T), dim3(mpk::PT), 0, st, p.x, p.ldx, p.w, p.d, p.eps, p.seg_tab, 0,
                       p.pooling, 0, p.h);
    hipLaunchKernelGGL(mpk::pool_colsum_kernel, dim3(nblk, (p.d + mpk::PT * 4 - 1) / (mpk::PT * 4)), dim3(mpk::PT), 0, st,
                       (const float*)p.h, p.d, p.seg_tab, p.n_seg, p.part);
    hipLaunchKernelGGL(mpk::pool_finish_kernel, dim3(p.n_seg), dim3(mpk::PT), 0, st, (const float*)p.part, p.d, p.seg_tab,
                       norm, p.pool_acc, p.emb);
  } else {
    hipLaunchKernelGGL(mpk::pool_row_kernel, dim3(p.n_seg), dim3(mpk::PT), 0, st, p.x, p.ldx, p.w, p.d, p.eps, p.seg_tab, 1,
                       p.pooling, norm, p.emb);
  }
}

}  // namespace mp
