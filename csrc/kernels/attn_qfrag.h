// The q-fragment builder of the fused decode attention kernels (attention.hip, attn_shared.hip):
// q of the G query heads of one kv head for one token, deferred norm / bias and RoPE applied in
// registers, scaled by q_scale * log2(e), as the B operand of S^T = K Q^T.
#pragma once
#include <type_traits>

#include "kcommon.h"
#include "../runtime/kernels_api.h"

namespace mpk {
using namespace mp;

// ROT = false: q is already rotated (the qkv GEMV's append epilogue, DecodeAttnParams::pre)
template <int KK, bool ROT = true>
__device__ __forceinline__ void decode_q_frags(const DecodeAttnParams& p, const float* row, const float2* cs, float nrs,
                                               int kvh, int G, int q4, int col, half8_t (&qf)[KK]) {
  const int g = col;
  const bool rvalid = col < G;
  const int h = kvh * G + g;
  const float qsc = p.q_scale * 1.4426950408889634f;   // exp2-domain scores (softmax_chunk)
  auto qkv_at = [&](int i) { return p.bias ? fmaf(nrs, row[i], p.bias[i]) : nrs * row[i]; };
  // q fragments with RoPE applied in registers: lane holds q[h][d = 32kk + 8q4 + j].  Built
  // before the append so its loads overlap the append's, and (head_dim % 8 == 0) from
  // unconditional 16-byte loads issued together: written as guarded scalar reads (qkv_at per
  // element) the compiler serialised ~32 dependent load round trips here, ~10 us of fixed cost per
  // call whatever the context (measured: 12.7 us at 20 keys, mb64).
  if ((p.hd & 7) == 0) {
    const int hs = rvalid ? h : kvh * G;          // idle MFMA columns read a valid head, then zero
    // bias / no-bias as two straight-line bodies: a bias branch inside the loop split the loads
    // into per-kk groups, each waited for before the next was issued
    // two k-slices per batch of loads: all KK at once peaked at ~180 VGPRs for DP=128 (occupancy 2)
    constexpr int KH = KK < 2 ? KK : 2;
    auto build = [&](auto with_bias) {
      constexpr bool HB = decltype(with_bias)::value;
#pragma unroll
      for (int k0 = 0; k0 < KK; k0 += KH) {
      float4 xa[KH][2], ca[KH][2], ba[KH][2];
#pragma unroll
      for (int kh = 0; kh < KH; ++kh) {
        const int kk = k0 + kh;
        const int d0 = 32 * kk + 8 * q4;
        const int dl = d0 < p.hd ? d0 : 0;
        const float4* xs = reinterpret_cast<const float4*>(row + hs * p.hd + dl);
        const float4* cp = reinterpret_cast<const float4*>(cs + dl / 2);
        xa[kh][0] = xs[0]; xa[kh][1] = xs[1];
        if constexpr (ROT) { ca[kh][0] = cp[0]; ca[kh][1] = cp[1]; }
        if constexpr (HB) {
          const float4* bs = reinterpret_cast<const float4*>(p.bias + hs * p.hd + dl);
          ba[kh][0] = bs[0]; ba[kh][1] = bs[1];
        }
      }
#pragma unroll
      for (int kh = 0; kh < KH; ++kh) {
        const int kk = k0 + kh;
        const int d0 = 32 * kk + 8 * q4;
        const bool ok = rvalid && d0 < p.hd;
        float x[8] = {xa[kh][0].x, xa[kh][0].y, xa[kh][0].z, xa[kh][0].w, xa[kh][1].x, xa[kh][1].y, xa[kh][1].z, xa[kh][1].w};
        float c[8] = {};
        if constexpr (ROT) {
          const float cc[8] = {ca[kh][0].x, ca[kh][0].y, ca[kh][0].z, ca[kh][0].w, ca[kh][1].x, ca[kh][1].y, ca[kh][1].z, ca[kh][1].w};
#pragma unroll
          for (int j = 0; j < 8; ++j) c[j] = cc[j];
        }
        if constexpr (HB) {
          const float b[8] = {ba[kh][0].x, ba[kh][0].y, ba[kh][0].z, ba[kh][0].w, ba[kh][1].x, ba[kh][1].y, ba[kh][1].z, ba[kh][1].w};
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = fmaf(nrs, x[j], b[j]);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] *= nrs;
        }
        half8_t v = {};
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          if constexpr (ROT) {
            v[j] = ok ? (f16)((x[j] * c[j] - x[j + 1] * c[j + 1]) * qsc) : (f16)0.f;
            v[j + 1] = ok ? (f16)((x[j] * c[j + 1] + x[j + 1] * c[j]) * qsc) : (f16)0.f;
          } else {
            v[j] = ok ? (f16)(x[j] * qsc) : (f16)0.f;
            v[j + 1] = ok ? (f16)(x[j + 1] * qsc) : (f16)0.f;
          }
        }
        qf[kk] = v;
      }
      }
    };
    if (p.bias) build(std::true_type{});
    else build(std::false_type{});
  } else {
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      half8_t v = {};
      if (rvalid) {
        const int d0 = 32 * kk + 8 * q4;
        const int qr = h * p.hd;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          const int d = d0 + j;
          if (d < p.hd) {
            const float x0 = qkv_at(qr + d), x1 = qkv_at(qr + d + 1);
            const float2 c = ROT ? cs[d >> 1] : make_float2(1.f, 0.f);
            v[j] = (f16)((x0 * c.x - x1 * c.y) * qsc);
            v[j + 1] = (f16)((x0 * c.y + x1 * c.x) * qsc);
          }
        }
      }
      qf[kk] = v;
    }
  }

}

}  // namespace mpk
