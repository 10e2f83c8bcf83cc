// Token log-probabilities next to the sampler (K13): per logit row the log-sum-exp, the
// log-probability of one target token and the top-n (id, logprob) pairs, so that a few floats and
// ints leave the GPU instead of the row.  The logits are read-only here.
//
// One 1024-thread workgroup per row, ONE streaming pass (16-byte loads, four in flight per lane):
//  - every lane keeps an online (max, sum exp) pair, merged over the wave and then over the block;
//  - every wave keeps its best 64 (logit, id) pairs sorted across its 64 lanes.  An element is
//    offered to the list only when it beats the list's top_n-th entry, which after the first few
//    hundred elements is rare (about top_n * ln(n / top_n) times per wave), so the pass stays a
//    plain stream.  An offer is a wave-uniform insert: rank by ballot, shift by one lane.
//  - wave 0 merges the 16 lists through LDS with the same insert.
// Order: descending logit, exact ties to the lower id (the comparator is on (logit, id), so the
// result does not depend on which lane or wave met an element first).  NaN counts as -inf and
// -inf never enters a list.  No workgroup talks to another one.
#include "kcommon.h"
#include "../runtime/kernels_api.h"

namespace mpk {
using namespace mp;

constexpr int LT = 1024;            // threads per row
constexpr int LW = LT / 64;         // waves per row
constexpr int LU = 4;               // 16-byte loads in flight per lane

struct TopList {                    // one entry per lane, best first
  float v; int id;                  // this lane's entry (-inf, -1 = empty)
  float tv; int ti;                 // the top_n-th entry: what an element has to beat
};

__device__ __forceinline__ void list_insert(TopList& L, float cv, int ci, int lane) {
  // entries that stay ahead of the candidate form a prefix of the lanes
  const bool ahead = L.v > cv || (L.v == cv && (unsigned)L.id < (unsigned)ci);
  const int pos = __popcll(__ballot(ahead));
  const float uv = __shfl_up(L.v, 1);
  const int ui = __shfl_up(L.id, 1);
  if (lane == pos) { L.v = cv; L.id = ci; }
  else if (lane > pos) { L.v = uv; L.id = ui; }
}

// offer one element per lane (wave-uniform control flow; x = -inf never passes)
__device__ __forceinline__ void list_offer(TopList& L, float x, int idx, int top_n, int lane) {
  const bool pass = x > L.tv || (x == L.tv && idx < L.ti);
  unsigned long long mk = __ballot(pass);
  if (!mk) return;
  while (mk) {
    const int l = __ffsll(mk) - 1;
    mk &= mk - 1;
    list_insert(L, __shfl(x, l), __shfl(idx, l), lane);
  }
  L.tv = __shfl(L.v, top_n - 1);
  L.ti = __shfl(L.id, top_n - 1);
}

__device__ __forceinline__ float no_nan(float x) { return x == x ? x : -INFINITY; }

// online log-sum-exp state (m, s): sum of exp(x - m) over what was seen; m = -inf while empty
__device__ __forceinline__ void lse_add4(float& m, float& s, float a, float b, float c, float d) {
  const float m4 = fmaxf(fmaxf(a, b), fmaxf(c, d));
  if (m4 > m) { s *= __expf(m - m4); m = m4; }
  if (m > -INFINITY) s += (__expf(a - m) + __expf(b - m)) + (__expf(c - m) + __expf(d - m));
}
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  if (mm > -INFINITY) s = s * __expf(m - mm) + s2 * __expf(m2 - mm);
  m = mm;
}

__global__ __launch_bounds__(LT) void logprob_kernel(const LogprobParams p) {
  __shared__ float sh_m[LW], sh_s[LW];
  __shared__ float sh_v[LW * kLogprobMaxTop];
  __shared__ int sh_i[LW * kLogprobMaxTop];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lg = p.logits + (size_t)row * p.ld;
  const int n = p.n, top_n = p.top_n;
  const bool want_top = top_n > 0;

  float m = -INFINITY, s = 0.f;
  TopList L{-INFINITY, -1, -INFINITY, -1};

  // 16-byte loads need a 16-byte aligned row; otherwise the whole row takes the scalar tail loop
  const bool vec = (((uintptr_t)p.logits | ((uintptr_t)p.ld * 4)) & 15) == 0;
  const int n4 = vec ? n & ~3 : 0;
  for (int base = 0; base < n4; base += LT * 4 * LU) {   // wave-uniform trip count
    f32x4 x[LU];
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      const int i = base + u * LT * 4 + tid * 4;
      x[u] = i < n4 ? *reinterpret_cast<const f32x4*>(lg + i) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    }
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      const int i = base + u * LT * 4 + tid * 4;
      const float a = no_nan(x[u].x), b = no_nan(x[u].y), c = no_nan(x[u].z), d = no_nan(x[u].w);
      lse_add4(m, s, a, b, c, d);
      if (want_top) {
        const float m4 = fmaxf(fmaxf(a, b), fmaxf(c, d));
        // exact ties with the top_n-th entry are settled inside list_offer
        if (__ballot(m4 >= L.tv && m4 > -INFINITY)) {
          list_offer(L, a, i, top_n, lane);
          list_offer(L, b, i + 1, top_n, lane);
          list_offer(L, c, i + 2, top_n, lane);
          list_offer(L, d, i + 3, top_n, lane);
        }
      }
    }
  }
  for (int base = n4; base < n; base += LT) {
    const int i = base + tid;
    const float a = i < n ? no_nan(lg[i]) : -INFINITY;
    lse_add4(m, s, a, -INFINITY, -INFINITY, -INFINITY);
    if (want_top) list_offer(L, a, i, top_n, lane);
  }

  // block log-sum-exp
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o), __shfl_xor(s, o));
  if (lane == 0) { sh_m[wave] = m; sh_s[wave] = s; }
  if (want_top && wave > 0 && lane < top_n) {
    sh_v[wave * kLogprobMaxTop + lane] = L.v;
    sh_i[wave * kLogprobMaxTop + lane] = L.id;
  }
  __syncthreads();
  if (wave != 0) return;
  m = lane < LW ? sh_m[lane] : -INFINITY;
  s = lane < LW ? sh_s[lane] : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o), __shfl_xor(s, o));
  // a row without a finite maximum (all -inf / NaN, or a +inf) has no distribution
  const bool dead = !(fabsf(m) < INFINITY);
  const float lse = dead ? -INFINITY : m + logf(s);

  if (lane == 0) {
    p.lse[row] = lse;
    if (p.target_lp) {
      const int t = p.target ? p.target[row] : -1;
      float lp = -INFINITY;
      if (!dead && t >= 0 && t < n) lp = no_nan(lg[t]) - lse;
      p.target_lp[row] = lp;
    }
  }
  // raw logits at the ids of the row's penalty window, for the gather after the sampler
  if (p.hist)
    for (int i = lane; i < p.last_n; i += 64) {
      const int t = p.hist[(size_t)row * p.last_n + i];
      p.hist_raw[(size_t)row * p.last_n + i] = t >= 0 && t < n ? lg[t] : 0.f;
    }
  if (!want_top) return;
  for (int base = top_n; base < LW * top_n; base += 64) {
    const int e = base + lane;
    const bool ok = e < LW * top_n;
    const int w = ok ? e / top_n : 0, j = ok ? e - w * top_n : 0;
    const float v = ok ? sh_v[w * kLogprobMaxTop + j] : -INFINITY;
    const int id = ok ? sh_i[w * kLogprobMaxTop + j] : -1;
    list_offer(L, v, id, top_n, lane);
  }
  if (lane < top_n) {
    const bool have = !dead && L.id >= 0;
    p.top_id[(size_t)row * p.ld_top + lane] = have ? L.id : -1;
    p.top_lp[(size_t)row * p.ld_top + lane] = have ? L.v - lse : -INFINITY;
  }
}

// after the sampler: the chosen token's log-probability from the RAW logit.  The penalty step
// edits the logits of the window's ids in place, so for those the value saved before it is used.
__global__ void logprob_chosen_kernel(const LogprobChosenParams p) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= p.M) return;
  const int t = p.tokens[row];
  float lp = -INFINITY;
  if (t >= 0 && t < p.n) {
    float raw = p.logits[(size_t)row * p.ld + t];
    if (p.hist)
      for (int i = 0; i < p.last_n; ++i)
        if (p.hist[(size_t)row * p.last_n + i] == t) { raw = p.hist_raw[(size_t)row * p.last_n + i]; break; }
    const float lse = p.lse[row];
    if (lse > -INFINITY) lp = no_nan(raw) - lse;
  }
  p.chosen_lp[row] = lp;
}

}  // namespace mpk

namespace mp {
void launch_logprob(const LogprobParams& p, hipStream_t st) {
  if (p.top_n < 0 || p.top_n > kLogprobMaxTop) throw std::runtime_error("logprob: top_n out of range");
  if (p.top_n > 0 && (p.ld_top < p.top_n || !p.top_id || !p.top_lp)) throw std::runtime_error("logprob: top-n buffers");
  if (p.n < 1 || p.ld < p.n || !p.lse) throw std::runtime_error("logprob: bad shape");
  if (p.hist && (!p.hist_raw || p.last_n < 1)) throw std::runtime_error("logprob: history buffers");
  if (p.M <= 0) return;
  hipLaunchKernelGGL(mpk::logprob_kernel, dim3(p.M), dim3(mpk::LT), 0, st, p);
}
void launch_logprob_chosen(const LogprobChosenParams& p, hipStream_t st) {
  if (p.M <= 0) return;
  hipLaunchKernelGGL(mpk::logprob_chosen_kernel, dim3((p.M + 63) / 64), dim3(64), 0, st, p);
}
}  // namespace mp
