// The sampler chain of one logit row, shared by sample_kernel (sample.hip: one setting for the whole
// launch) and sample_rows_kernel (sample_rows.hip: a record per row), in llama.cpp's order:
//   top-n-sigma -> top-k -> typical-p -> top-p -> min-p -> XTC -> (dynamic) temperature -> draw
// Every cut works on the T = 1 distribution of the survivors of the cuts before it; the inverse-CDF
// draw uses temperature T.  One 1024-thread workgroup per row; thresholds by bisection (no sort), so
// the chain is a few streaming passes over the row (L2-resident after the first).
//
// The cuts never mark tokens: each one only tightens the scalars of one survivor predicate alive(l, i),
// which every later pass evaluates.
//   floor            top-n-sigma, top-k, top-p and min-p are bounds on the logit (p is monotone in l)
//   tmean, tdev      typical-p: -ln p_i - H = E_p[l] - l_i, so its score cut is |l - gmx - tmean| <= tdev
//   ceil_l, ceil_i   XTC removes every l above the least probable token that reaches its threshold
// A cut that is off is a uniform branch around its passes: a row with none of top-n-sigma, typical-p,
// XTC and dynamic temperature runs the passes of top-k / top-p / min-p and the draw alone.
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

// three sums in one trip through the wave shuffles and LDS (sh: 3 * ST / 64 floats)
__device__ __forceinline__ void block_reduce3(float& a, float& b, float& c, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    b += __shfl_xor(b, o);
    c += __shfl_xor(c, o);
  }
  constexpr int W = ST / 64;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) { sh[w] = a; sh[W + w] = b; sh[2 * W + w] = c; }
  __syncthreads();
  a = b = c = 0.f;
  for (int i = 0; i < W; ++i) { a += sh[i]; b += sh[W + i]; c += sh[2 * W + i]; }
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL; x ^= x >> 27; x *= 0x94d049bb133111ebULL; x ^= x >> 31;
  return x;
}

// the members of the chain beyond top-k / top-p / min-p; the defaults switch each of them off
struct ChainExtra {
  float top_n_sigma = 0.f;     // <= 0: off
  float typical_p = 1.f;       // <= 0 or >= 1: off
  float xtc_q = 0.f, xtc_t = 0.1f;   // probability and threshold; q <= 0 or t > 0.5: off
  float dyn_range = 0.f, dyn_exp = 1.f;   // range <= 0: off
};

// lg[0, n): the row.  r: the row's 64 random bits; the variate of the draw is (r >> 40) / 2^24, that
// of XTC (mix64(r ^ 0x9E3779B97F4A7C15) >> 40) / 2^24.  Called by all ST threads of the workgroup (the
// arguments are uniform); thread 0 writes *tok.
__device__ __forceinline__ void sample_chain(const float* lg, int n, float temp, int top_k, float top_p, float min_p,
                                             const ChainExtra x, uint64_t r, int32_t* tok) {
  __shared__ float sh[3 * ST / 64];
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
  const bool typ_on = x.typical_p > 0.f && x.typical_p < 1.f;
  const bool xtc_on = x.xtc_q > 0.f && x.xtc_t <= 0.5f;

  // the survivor predicate and its scalars (all uniform)
  float floor_l = -INFINITY;
  bool typ = false, xtc = false;
  float tmean = 0.f, tdev = INFINITY;
  float ceil_l = INFINITY;
  int ceil_i = 0;
  auto alive = [&](float l, int i) {
    bool a = l >= floor_l;
    if (typ) a = a && fabsf(l - gmx - tmean) <= tdev;
    if (xtc) a = a && (l < ceil_l || (l == ceil_l && i >= ceil_i));
    return a;
  };
  // T = 1 probability of a survivor, relative to the row's maximum
  auto p1 = [&](float l, int i) { return alive(l, i) ? __expf(l - gmx) : 0.f; };
  // survivors: sum of p1, sum of p1 * (l - gmx), count -- one pass, one reduction
  auto moments = [&](float& z, float& s, float& c) {
    z = s = c = 0.f;
    for (int i = i0; i < i1; ++i) {
      const float l = lg[i];
      if (!alive(l, i) || l == -INFINITY) continue;
      const float d = l - gmx, e = __expf(d);
      z += e;
      s += e > 0.f ? e * d : 0.f;
      c += 1.f;
    }
    block_reduce3(z, s, c, sh);
  };

  // top-n-sigma: l >= max - s * sigma, sigma over the finite logits (moments of l - gmx)
  if (x.top_n_sigma > 0.f) {
    float s1 = 0.f, s2 = 0.f, c = 0.f;
    for (int i = i0; i < i1; ++i) {
      const float l = lg[i];
      if (!(fabsf(l) < INFINITY)) continue;
      const float d = l - gmx;
      s1 += d; s2 += d * d; c += 1.f;
    }
    block_reduce3(s1, s2, c, sh);
    if (c > 0.f) {
      const float mean = s1 / c, var = fmaxf(s2 / c - mean * mean, 0.f);
      floor_l = gmx - x.top_n_sigma * sqrtf(var);
    }
  }
  // top-k threshold on logits: largest thr with count(l >= thr) >= k (the k largest of the row are
  // the k largest of the survivors of a floor, so the two bounds just combine)
  if (top_k > 0 && top_k < n) {
    float lo = gmx - 60.f, hi = gmx;
    for (int it = 0; it < 28; ++it) {
      const float mid = 0.5f * (lo + hi);
      float c = 0.f;
      for (int i = i0; i < i1; ++i) c += lg[i] >= mid ? 1.f : 0.f;
      c = block_reduce(c, sh, false);
      if (c >= (float)top_k) lo = mid; else hi = mid;
    }
    floor_l = fmaxf(floor_l, lo);
  }
  // typical-p: the tokens nearest to the expected surprise until their mass reaches typical_p.
  // -ln p_i - H = E_p[l] - l_i, so the score is the distance of l - gmx from its mean under p.
  // smallest dev with sum_{|l - gmx - tmean| <= dev} p1 >= typical_p * Z (the crossing token stays)
  float amx = gmx;   // the largest surviving logit: the reference of min-p and of the draw
  if (typ_on) {
    float z, s, c;
    moments(z, s, c);
    if (z > 0.f) {
      tmean = s / z;
      float lo = -1.f, hi = 128.f;   // exp(l - gmx) > 0 needs l - gmx > -104; |tmean| <= 104
      for (int it = 0; it < 28; ++it) {
        const float mid = 0.5f * (lo + hi);
        float q = 0.f;
        for (int i = i0; i < i1; ++i) {
          const float l = lg[i];
          q += l >= floor_l && fabsf(l - gmx - tmean) <= mid ? __expf(l - gmx) : 0.f;
        }
        q = block_reduce(q, sh, false);
        if (q >= x.typical_p * z) hi = mid; else lo = mid;
      }
      tdev = hi;
      typ = true;
      float m = -INFINITY;
      for (int i = i0; i < i1; ++i) if (alive(lg[i], i)) m = fmaxf(m, lg[i]);
      amx = block_reduce(m, sh, true);
    }
  }
  // top-p: largest q with sum_{p1 >= q} p1 >= top_p * sum p1
  float pthr = 0.f;
  if (top_p > 0.f && top_p < 1.f) {
    float tot = 0.f;
    for (int i = i0; i < i1; ++i) tot += p1(lg[i], i);
    tot = block_reduce(tot, sh, false);
    float lo = 0.f, hi = 1.f;
    for (int it = 0; it < 24; ++it) {
      const float mid = 0.5f * (lo + hi);
      float s = 0.f;
      for (int i = i0; i < i1; ++i) { const float q = p1(lg[i], i); s += q >= mid ? q : 0.f; }
      s = block_reduce(s, sh, false);
      if (s >= top_p * tot) lo = mid; else hi = mid;
    }
    pthr = lo;
  }
  // min-p: p1 >= min_p * p1 of the largest survivor (the row's maximum, p1 = 1, unless typical-p cut it)
  pthr = fmaxf(pthr, typ ? min_p * __expf(amx - gmx) : min_p);
  // the probability bound as a logit floor: the smallest surviving logit that passes it
  if (pthr > 0.f) {
    float m = INFINITY;
    for (int i = i0; i < i1; ++i) {
      const float l = lg[i];
      if (alive(l, i) && __expf(l - gmx) >= pthr) m = fminf(m, l);
    }
    m = -block_reduce(-m, sh, true);
    if (m < INFINITY) floor_l = fmaxf(floor_l, m);
  }
  // XTC: with probability q, of the survivors with p >= t all but the least probable one go
  if (xtc_on) {
    const uint64_t r2 = mix64(r ^ 0x9E3779B97F4A7C15ULL);
    if ((float)((r2 >> 40) * (1.0 / 16777216.0)) < x.xtc_q) {
      float z = 0.f;
      for (int i = i0; i < i1; ++i) z += p1(lg[i], i);
      z = block_reduce(z, sh, false);
      const float pt = x.xtc_t * z;
      float c = 0.f, m = INFINITY;
      for (int i = i0; i < i1; ++i) {
        const float l = lg[i];
        if (alive(l, i) && __expf(l - gmx) >= pt) { c += 1.f; m = fminf(m, l); }
      }
      c = block_reduce(c, sh, false);
      m = -block_reduce(-m, sh, true);
      if (c >= 2.f) {
        float last = -1.f;   // equal logits: the higher index stays (ids are exact in a float below 2^24)
        for (int i = i0; i < i1; ++i) if (lg[i] == m && alive(m, i)) last = (float)i;
        last = block_reduce(last, sh, true);
        ceil_l = m; ceil_i = (int)last;
        xtc = true;
        amx = m;
      }
    }
  }
  // temperature; dynamic: T_lo + (T_hi - T_lo) * (H / ln(survivors)) ^ exponent
  float T = temp;
  if (x.dyn_range > 0.f) {
    float z, s, c;
    moments(z, s, c);
    if (c > 1.f && z > 0.f) {
      const float H = fmaxf(logf(z) - s / z, 0.f);
      const float t_lo = fmaxf(0.f, temp - x.dyn_range), t_hi = temp + x.dyn_range;
      T = t_lo + (t_hi - t_lo) * powf(fminf(H / logf(c), 1.f), x.dyn_exp);
      T = fmaxf(T, 1e-6f);   // T_lo = 0 and no entropy: the largest survivor
    }
  }
  const float invT = 1.f / T;
  auto keep = [&](float l, int i) { return alive(l, i) ? __expf((l - amx) * invT) : 0.f; };
  float mine = 0.f;
  for (int i = i0; i < i1; ++i) mine += keep(lg[i], i);
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
  if (threadIdx.x == 0) pick = -1;   // fallback: the largest survivor below
  __syncthreads();
  if (mine > 0.f && u >= before && u < scan[threadIdx.x]) {
    float c = before;
    int sel = -1;
    for (int i = i0; i < i1; ++i) {
      c += keep(lg[i], i);
      if (u < c) { sel = i; break; }
    }
    if (sel < 0) for (int i = i1 - 1; i >= i0; --i) if (keep(lg[i], i) > 0.f) { sel = i; break; }
    pick = sel;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = pick;
    if (t < 0 || t >= n) {  // u landed on total (rounding): take the largest survivor
      t = 0;
      for (int i = 0; i < n; ++i) if (lg[i] == amx && alive(amx, i)) { t = i; break; }
    }
    *tok = t;
  }
}

}  // namespace mpk
