// Per-request sampling on the last stage (engine key "row_sampling"): every row of a launch reads
// its own record (RowSampling, kernels_api.h) from a device table, so the rows of one micro-batch mix
// greedy and sampled requests, each with its own cuts, penalties, logit bias and random stream, and
// the captured decode graphs never change when a request is admitted.
//   row_adjust_kernel:  logit bias, then the repetition penalties of penalize_kernel, per row
//   sample_rows_kernel: the chain of sample_kernel (sample_chain.h) with the row's parameters
// The record is uniform per workgroup: the compiler reads it with a handful of scalar loads.
#include <stdexcept>

#include "kcommon.h"
#include "sample_chain.h"
#include "../runtime/kernels_api.h"

namespace mpk {
using namespace mp;

__global__ __launch_bounds__(256) void row_adjust_kernel(const RowAdjustParams p) {
  const int row = blockIdx.x;
  const RowSampling& rs = p.rows[row];
  const int nb = min(rs.n_bias, kMaxLogitBias);
  const float repeat = rs.repeat, freq = rs.freq, presence = rs.presence;
  const bool pen = p.last_n > 0 && (repeat != 1.f || freq != 0.f || presence != 0.f);
  if (nb <= 0 && !pen) return;   // neutral row: its logits stay bit-identical
  float* lg = p.logits + (size_t)row * p.ld;
  // bias first: the first listing of an id owns it and adds every listing's value in list order
  if ((int)threadIdx.x < nb) {
    const int i = threadIdx.x, t = rs.bias_id[i];
    bool first = t >= 0 && t < p.n;
    for (int j = 0; j < i; ++j) first &= rs.bias_id[j] != t;
    if (first) {
      float l = lg[t];
      for (int j = i; j < nb; ++j)
        if (rs.bias_id[j] == t) l += rs.bias_val[j];
      lg[t] = l;
    }
  }
  if (!pen) return;
  __syncthreads();   // the biased logits are visible to the whole workgroup
  const int32_t* h = p.hist + (size_t)row * p.hist_ld;
  for (int i = threadIdx.x; i < p.last_n; i += blockDim.x) {
    const int t = h[i];
    if (t < 0 || t >= p.n) continue;
    int c = 0;
    bool first = true;
    for (int j = 0; j < p.last_n; ++j)
      if (h[j] == t) {
        ++c;
        first &= j >= i;
      }
    if (!first) continue;   // the first occurrence in the window owns the token
    float l = lg[t];
    l = l > 0.f ? l / repeat : l * repeat;
    // one fused multiply-subtract, then one subtract (what penalize_kernel's expression contracts to)
    lg[t] = __fmaf_rn(-(float)c, freq, l) - presence;
  }
}

__global__ __launch_bounds__(ST) void sample_rows_kernel(const SampleRowsParams p) {
  const int row = blockIdx.x;
  const RowSampling& rs = p.rows[row];
  const float temp = rs.temp;
  const int32_t d = p.draw[row];
  if (temp > 0.f) {
    const uint64_t r = mix64(rs.seed ^ mix64((uint64_t)(uint32_t)d << 20));
    sample_chain(p.logits + (size_t)row * p.ld, p.n, temp, rs.top_k, rs.top_p, rs.min_p, r, p.tokens + row);
  }
  // (every thread read draw[row] before the chain's first barrier; a greedy row's other threads do
  // not use it)
  if (p.advance && threadIdx.x == 0) p.draw[row] = d + 1;
}

}  // namespace mpk

namespace mp {
void launch_row_adjust(const RowAdjustParams& p, hipStream_t st) {
  if (p.M <= 0) return;
  if (p.last_n < 0 || p.hist_ld < p.last_n || (p.last_n > 0 && !p.hist)) throw std::runtime_error("row_adjust: window");
  hipLaunchKernelGGL(mpk::row_adjust_kernel, dim3(p.M), dim3(256), 0, st, p);
}
void launch_sample_rows(const SampleRowsParams& p, hipStream_t st) {
  if (p.M <= 0) return;
  hipLaunchKernelGGL(mpk::sample_rows_kernel, dim3(p.M), dim3(mpk::ST), 0, st, p);
}
}  // namespace mp
