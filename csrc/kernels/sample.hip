// On-GPU sampler for the last stage (K12): temperature, top-k, min-p, top-p, then inverse-CDF
// draw with a counter-based RNG.  Only int32 token ids leave the GPU (the reference copies the
// 501 KiB logit row of Llama-3 to the host every token and samples on the CPU).
// One 1024-thread workgroup per row; thresholds by bisection (no sort), so the kernel is a few
// streaming passes over the row (L2-resident after the first).
#include "kcommon.h"
#include "sample_chain.h"
#include "../runtime/kernels_api.h"

namespace mpk {
using namespace mp;

// the chain itself (cuts + draw) is sample_chain.h, shared with sample_rows.hip
__global__ __launch_bounds__(ST) void sample_kernel(const SampleParams p) {
  const int row = blockIdx.x;
  const int32_t step = p.step ? p.step[0] : 0;
  const uint64_t r = mix64(p.seed ^ mix64(((uint64_t)step << 20) ^ (uint64_t)row));
  sample_chain(p.logits + (size_t)row * p.ld, p.n, p.temp, p.top_k, p.top_p, p.min_p, r, p.tokens + row);
}

__global__ __launch_bounds__(256) void penalize_kernel(const PenaltyParams p) {
  const int row = blockIdx.x;
  const int32_t* h = p.hist + (size_t)row * p.last_n;
  float* lg = p.logits + (size_t)row * p.ld;
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
    l = l > 0.f ? l / p.repeat : l * p.repeat;
    lg[t] = l - (float)c * p.freq - p.presence;
  }
}

__global__ void hist_push_kernel(int32_t* hist, int ld, int32_t* cnt, int last_n, const int32_t* tokens, int M) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int c = cnt[m];
  hist[(size_t)m * ld + c % last_n] = tokens[m];
  cnt[m] = c + 1;
}

}  // namespace mpk

namespace mp {
void launch_penalize(const PenaltyParams& p, hipStream_t st) {
  hipLaunchKernelGGL(mpk::penalize_kernel, dim3(p.M), dim3(256), 0, st, p);
}
void launch_hist_push(int32_t* hist, int32_t* cnt, int last_n, const int32_t* tokens, int M, hipStream_t st) {
  launch_hist_push_ld(hist, last_n, cnt, last_n, tokens, M, st);
}
void launch_hist_push_ld(int32_t* hist, int hist_ld, int32_t* cnt, int last_n, const int32_t* tokens, int M,
                         hipStream_t st) {
  if (M <= 0 || last_n <= 0) return;
  hipLaunchKernelGGL(mpk::hist_push_kernel, dim3((M + 63) / 64), dim3(64), 0, st, hist, hist_ld, cnt, last_n, tokens, M);
}
void launch_sample(const SampleParams& p, hipStream_t st) {
  hipLaunchKernelGGL(mpk::sample_kernel, dim3(p.M), dim3(mpk::ST), 0, st, p);
}
}  // namespace mp
