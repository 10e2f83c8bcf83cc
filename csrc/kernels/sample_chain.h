// The sampler chain of one logit row, shared by sample_kernel (sample.hip: one setting for the whole
// launch) and sample_rows_kernel (sample_rows.hip: a record per row): the cuts top-k, top-p and
// min-p on the T = 1 distribution, then the inverse-CDF draw at temperature T.  One 1024-thread
// workgroup per row; thresholds by bisection (no sort), so the chain is a few streaming passes over
// the row (L2-resident after the first).
#pragma once
#include "kcommon.h"

namespace mpk {

constexpr int ST = 1024;

__device__ __forceinline__ float block_reduce(float v, float* sh, bool is_max) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float x = __shfl_xor(v, o);
    v = is_max ? fmaxf(v, x) : v + x;
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  float r = is_max ? -INFINITY : 0.f;
  for (int i = 0; i < ST / 64; ++i) r = is_max ? fmaxf(r, sh[i]) : r + sh[i];
  return r;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL; x ^= x >> 27; x *= 0x94d049bb133111ebULL; x ^= x >> 31;
  return x;
}

// lg[0, n): the row.  r: the row's 64 random bits; the variate is (r >> 40) / 2^24.  Called by all
// ST threads of the workgroup (the arguments are uniform); thread 0 writes *tok.
__device__ __forceinline__ void sample_chain(const float* lg, int n, float temp, int top_k, float top_p, float min_p,
                                             uint64_t r, int32_t* tok) {
  __shared__ float sh[ST / 64];
  __shared__ float scan[ST];
  // chunk of contiguous indices per thread (for the ordered CDF walk)
  const int per = (n + ST - 1) / ST;
  const int i0 = threadIdx.x * per, i1 = min(n, i0 + per);

  float mx = -INFINITY;
  int am = 0x7fffffff;
  for (int i = i0; i < i1; ++i) if (lg[i] > mx) { mx = lg[i]; am = i; }
  // argmax (also the temp <= 0 path)
  float gmx = block_reduce(mx, sh, true);
  if (temp <= 0.f) {
    __shared__ int best;
    if (threadIdx.x == 0) best = 0x7fffffff;
    __syncthreads();
    if (mx == gmx) atomicMin(&best, am);
    __syncthreads();
    if (threadIdx.x == 0) *tok = best == 0x7fffffff ? 0 : best;   // all -inf / NaN: token 0, as argmax
    return;
  }
  const float invT = 1.f / temp;
  // llama.cpp sampler-chain semantics (common_sampler defaults: top-k -> top-p -> min-p -> temp ->
  // dist): the three cuts are taken on the T = 1 distribution, the draw uses temperature T.
  // top-k threshold on logits: largest thr with count(l >= thr) >= k
  float thr = -INFINITY;
  if (top_k > 0 && top_k < n) {
    float lo = gmx - 60.f, hi = gmx;
    for (int it = 0; it < 28; ++it) {
      const float mid = 0.5f * (lo + hi);
      float c = 0.f;
      for (int i = i0; i < i1; ++i) c += lg[i] >= mid ? 1.f : 0.f;
      c = block_reduce(c, sh, false);
      if (c >= (float)top_k) lo = mid; else hi = mid;
    }
    thr = lo;
  }
  // T = 1 probabilities (relative to the max) of the top-k survivors
  auto p1 = [&](float l) { return l >= thr ? __expf(l - gmx) : 0.f; };
  // top-p: largest q with sum_{p1 >= q} p1 >= top_p * sum p1
  float pthr = 0.f;
  if (top_p > 0.f && top_p < 1.f) {
    float tot = 0.f;
    for (int i = i0; i < i1; ++i) tot += p1(lg[i]);
    tot = block_reduce(tot, sh, false);
    float lo = 0.f, hi = 1.f;
    for (int it = 0; it < 24; ++it) {
      const float mid = 0.5f * (lo + hi);
      float s = 0.f;
      for (int i = i0; i < i1; ++i) { const float q = p1(lg[i]); s += q >= mid ? q : 0.f; }
      s = block_reduce(s, sh, false);
      if (s >= top_p * tot) lo = mid; else hi = mid;
    }
    pthr = lo;
  }
  // min-p: p1 >= min_p (the max has p1 = 1)
  pthr = fmaxf(pthr, min_p);
  auto keep = [&](float l) { return l >= thr && __expf(l - gmx) >= pthr ? __expf((l - gmx) * invT) : 0.f; };
  float mine = 0.f;
  for (int i = i0; i < i1; ++i) mine += keep(lg[i]);
  // inclusive scan of per-thread sums (Hillis-Steele in LDS)
  scan[threadIdx.x] = mine;
  __syncthreads();
  for (int o = 1; o < ST; o <<= 1) {
    const float v = threadIdx.x >= (unsigned)o ? scan[threadIdx.x - o] : 0.f;
    __syncthreads();
    scan[threadIdx.x] += v;
    __syncthreads();
  }
  const float total = scan[ST - 1];
  const float u = (float)((r >> 40) * (1.0 / 16777216.0)) * total;
  const float before = scan[threadIdx.x] - mine;
  __shared__ int pick;
  if (threadIdx.x == 0) pick = -1;   // fallback: global argmax below
  __syncthreads();
  if (mine > 0.f && u >= before && u < scan[threadIdx.x]) {
    float c = before;
    int sel = -1;
    for (int i = i0; i < i1; ++i) {
      c += keep(lg[i]);
      if (u < c) { sel = i; break; }
    }
    if (sel < 0) for (int i = i1 - 1; i >= i0; --i) if (keep(lg[i]) > 0.f) { sel = i; break; }
    pick = sel;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = pick;
    if (t < 0 || t >= n) {  // u landed on total (rounding): take the global argmax
      t = 0;
      for (int i = 0; i < n; ++i) if (lg[i] == gmx) { t = i; break; }
    }
    *tok = t;
  }
}

}  // namespace mpk
