// Per-row token masks on the last stage (engine key "row_masks"): a row that is on gets -inf in every
// logit whose bit is clear, so the arg-max and the sampler that follow can only choose allowed tokens
// (grammar- and schema-constrained generation; the host computes the bits, grammar.h).
//   row m: bits + m * ldw, token t allowed iff bits[t >> 5] >> (t & 31) & 1
// The kernel reads the bits and stores -inf; it never reads a logit, never writes an allowed one,
// a column >= n or a row whose on[m] is 0 (the row and its flag are uniform per workgroup: one
// scalar load, then the workgroup returns).
//
// Geometry: (chunk, row) workgroups of 256 lanes as launch_argmax.  A lane owns 4 consecutive
// logits, one 16-byte store when all four are banned, so a wave instruction covers 1 KiB of the row
// without gaps; kRowMaskIter such groups per lane make a chunk 4096 logits (a 128k vocabulary: 32
// chunks per row, 128 workgroups at 4 rows, 2048 at 64).  A row base is only 4-byte aligned: the
// groups start at the row's first 16-byte boundary (h = 0..3 logits in), the h logits before it
// and the groups that cross n or hold an allowed token go out as scalar stores.
#include <stdexcept>

#include "kcommon.h"
#include "../runtime/kernels_api.h"

namespace mpk {
using namespace mp;

constexpr int kRowMaskThreads = 256;
constexpr int kRowMaskIter = 4;
constexpr int kRowMaskChunk = kRowMaskThreads * kRowMaskIter * 4;   // logits per workgroup

__global__ __launch_bounds__(kRowMaskThreads) void row_mask_kernel(const RowMaskParams p) {
  const int row = blockIdx.y;
  if (p.on[row] == 0) return;
  float* lg = p.logits + (size_t)row * p.ld;
  const uint32_t* bits = p.bits + (size_t)row * p.ldw;
  const int n = p.n;
  const int nw = (n + 31) >> 5;
  const float ninf = -__builtin_huge_valf();
  // logits before the row's first 16-byte boundary
  const int h = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(lg) & 15u)) & 15u) >> 2);
  if (blockIdx.x == 0 && (int)threadIdx.x < h && (int)threadIdx.x < n) {
    const int c = threadIdx.x;
    if (!((bits[0] >> c) & 1u)) lg[c] = ninf;
  }
  const int g0 = blockIdx.x * (kRowMaskThreads * kRowMaskIter) + threadIdx.x;
#pragma unroll
  for (int it = 0; it < kRowMaskIter; ++it) {
    const int c = h + 4 * (g0 + it * kRowMaskThreads);   // first column of the lane's group
    if (c >= n) break;
    const int wi = c >> 5, sh = c & 31;
    uint32_t v = bits[wi] >> sh;
    if (sh > 28 && wi + 1 < nw) v |= bits[wi + 1] << (32 - sh);
    v &= 0xFu;
    if (c + 4 <= n) {
      if (v == 0u) {
        *reinterpret_cast<float4*>(lg + c) = make_float4(ninf, ninf, ninf, ninf);
        continue;
      }
      if (v == 0xFu) continue;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < n && !((v >> j) & 1u)) lg[c + j] = ninf;
  }
}

}  // namespace mpk

namespace mp {
void launch_row_mask(const RowMaskParams& p, hipStream_t st) {
  if (p.M <= 0 || p.n <= 0) return;
  if (p.ldw < (p.n + 31) / 32) throw std::runtime_error("row_mask: ldw is smaller than ceil(n / 32)");
  if (p.ld < p.n) throw std::runtime_error("row_mask: ld is smaller than n");
  if (!p.logits || !p.bits || !p.on) throw std::runtime_error("row_mask: null pointer");
  // + 3: the groups start up to 3 logits into the row
  const int chunks = (p.n + 3 + mpk::kRowMaskChunk - 1) / mpk::kRowMaskChunk;
  hipLaunchKernelGGL(mpk::row_mask_kernel, dim3(chunks, p.M), dim3(mpk::kRowMaskThreads), 0, st, p);
}
}  // namespace mp
