// Decode attention over a shared prompt prefix (cascade decode, phase 1).
//
// Rows of a decode micro-batch whose slots name the same leading KV pages (KvPager::share) form a
// group.  The fused decode kernel gives every (row, kv head) its own pass over those pages: N rows
// stream N times the same bytes and feed G of the 16 MFMA columns.  Here one 512-thread workgroup =
// (group, block of up to 128 query rows, kv head, page split):
//   * its query rows are the (member row, g) pairs of the group, 16 / G member rows per 16-column
//     MFMA tile, one tile per wave; each member's q is built by decode_q_frags at that row's own
//     position (deferred norm, RoPE, q_scale * log2 e), exactly the fused decode kernel's operand;
//   * each 64-key K page [64][Dp] and V page of the kv head is read from HBM ONCE per workgroup,
//     through the LEADER's block-table row, as raw cache bytes (f16 or e4m3) into padded,
//     double-buffered LDS tiles (register prefetch of page j + 1 under page j's MFMAs; the padded
//     rows that keep the 16 key rows of a fragment on distinct banks rule out the contiguous
//     LDS-DMA of gemm_lds.h); all 8 waves read their fragments from them and convert e4m3 at the read;
//   * S^T = K Q^T with the key-row permutation pi(c, R) = 8(R>>2) + 4c + (R&3) of attention.hip,
//     so the exponentiated scores are the B operand of O^T += V^T P^T; online softmax in registers
//     in the exp2 domain with the lazy rescale;
//   * no mask: kv_begin <= pos for every member, every key of a shared page is visible.
// Coverage: a workgroup holds 8 tiles x (16 / G) member rows = 128 query rows when G divides 16;
// otherwise (G = 3, 5, 6, 7, 9 ..) a tile's last 16 % G columns idle and it covers 8 (16 / G) G < 128.
// LDS: 2 x (64 x (Dp + 8) + Dp x 72) elements, 70 KB for f16 at Dp = 128 (35 KB e4m3): above the
// 64 KB of earlier CDNA parts; on gfx950 (160 KB per CU) two 512-thread workgroups fit a CU.
// Output: unnormalised (O, m, l) per (member row, head, page split) in the layout of the decode
// kernel's o_part / ml_part, merged by the decode kernel's last arriver (DecodeAttnParams::pfx_*),
// which runs after this kernel in stream order.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "kcommon.h"
#include "attn_qfrag.h"
#include "../runtime/kernels_api.h"

namespace mpk {
using namespace mp;

template <int DP, bool F8>
__global__ __launch_bounds__(512) void attn_shared_kernel(const SharedAttnParams p, const int max_rb) {
  using KR = std::conditional_t<F8, u32x2, u32x4>;     // raw 8-element chunk, as staged
  using FR = std::conditional_t<F8, u32x2, half8_t>;   // raw 8-element fragment, as read back
  constexpr int KK = DP / 32;    // k-steps of S^T over d
  constexpr int DT = DP / 16;    // 16-row d tiles of O^T
  constexpr int EB = F8 ? 1 : 2; // bytes per cached element
  constexpr int KLD = (DP + 8) * EB;   // K tile row stride in bytes (16 key rows of a fragment: distinct banks)
  constexpr int VLD = (64 + 8) * EB;   // V^T tile row stride in bytes
  constexpr int NT = 512;
  constexpr int KCH = 64 * DP / 8 / NT;   // 8-element K chunks per thread per page (= V chunks)
  __shared__ __attribute__((aligned(16))) uint8_t ks[2][64 * KLD];
  __shared__ __attribute__((aligned(16))) uint8_t vs[2][DP * VLD];

  const DecodeAttnParams& d = p.d;
  const int gi = blockIdx.x / max_rb, rb = blockIdx.x - gi * max_rb;
  const int kvh = blockIdx.y, z = blockIdx.z;
  const int4 rec = *reinterpret_cast<const int4*>(p.groups + gi);   // the one load idle workgroups pay
  const int n_pages = rec.x, n_rows = rec.y, row_off = rec.z, leader = rec.w;
  const int G = d.Hq / d.Hkv;
  const int rpt = 16 / G;                    // member rows per MFMA tile
  if (rb * 8 * rpt >= n_rows) return;        // unused record (n_rows = 0) or row block past the group

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q4 = lane >> 4, col = lane & 15;
  const int tile = rb * 8 + wave;
  const bool live = tile * rpt < n_rows;     // wave-uniform: idle waves only stage pages
  const int mi = tile * rpt + col / G;       // member index of this lane's column
  const int g = col % G;
  const bool rvalid = col < rpt * G && mi < n_rows;
  const int t = p.rows[row_off + (rvalid ? mi : 0)];
  const int pos = d.pos[t];
  const int prow = d.pfx_row[t];
  const float* row = d.qkv + (size_t)t * d.ldqkv;
  const float2* cs = d.rope_cs + (size_t)pos * (d.hd / 2);
  const float nrs = d.ssq ? rsqrtf(d.ssq[t] / (float)d.d_model + d.eps) : 1.f;

  // pages [kt0, kt1) of the group's prefix belong to split z
  const int spp = (n_pages + d.n_psplit - 1) / d.n_psplit;
  const int kt0 = min(z * spp, n_pages), kt1 = min(kt0 + spp, n_pages);
  const int n_kt = kt1 - kt0;
  const int32_t* bt = d.block_table + (size_t)leader * d.max_pages;

  // page staging: thread owns K chunks (key = c / (DP/8), d8 = c % (DP/8)) and V chunks (dim, key
  // block), c = tid + NT j; consecutive threads read consecutive bytes of the page in either V
  // layout (kernels_api.h).  The LDS image is V^T [Dp][VLD] for both.
  KR kr[KCH], vr[KCH];
  const bool vblk = d.v_d == 8;
  auto v_d_of = [&](int c) { return vblk ? c % DP : c / 8; };
  auto v_k8_of = [&](int c) { return vblk ? c / DP : c % 8; };
  auto load_page = [&](int kt) {
    const int page = bt[kt];
    const uint8_t* kb = reinterpret_cast<const uint8_t*>(d.k_cache) + ((size_t)page * d.Hkv + kvh) * 64 * DP * EB;
    const uint8_t* vb = reinterpret_cast<const uint8_t*>(d.v_cache) + ((size_t)page * d.Hkv + kvh) * DP * 64 * EB;
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
      const int c = tid + NT * j;
      kr[j] = *reinterpret_cast<const KR*>(kb + (size_t)c * 8 * EB);
      vr[j] = *reinterpret_cast<const KR*>(vb + (size_t)(v_k8_of(c) * d.v_kb + v_d_of(c) * d.v_d) * EB);
    }
  };
  auto store_page = [&](int buf) {
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
      const int c = tid + NT * j;
      *reinterpret_cast<KR*>(&ks[buf][(c / (DP / 8)) * KLD + (c % (DP / 8)) * 8 * EB]) = kr[j];
      *reinterpret_cast<KR*>(&vs[buf][v_d_of(c) * VLD + v_k8_of(c) * 8 * EB]) = vr[j];
    }
  };
  auto cvt = [](const FR& r) -> half8_t {
    if constexpr (F8) return f8x8_to_h8(r);
    else return r;
  };

  if (n_kt > 0) load_page(kt0);   // in flight during the q build

  half8_t qf[KK] = {};
  if (live) decode_q_frags<KK>(d, row, cs, nrs, kvh, G, q4, rvalid ? g : G, qf);   // column G: a zero fragment

  f32x4 o[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const int krow0 = 8 * (col >> 2) + (col & 3);   // pi(c, R) - 4c

  if (n_kt > 0) {
    store_page(0);
    __syncthreads();
    if (n_kt > 1) load_page(kt0 + 1);
  }
  for (int kt = 0; kt < n_kt; ++kt) {
    const int buf = kt & 1;
    const uint8_t* kt_s = ks[buf];
    const uint8_t* vt_s = vs[buf];
    if (live) {
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        f32x4 s[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < KK; ++kk) {
            const half8_t kf =
                cvt(*reinterpret_cast<const FR*>(kt_s + (32 * kc + krow0 + 4 * c) * KLD + (32 * kk + 8 * q4) * EB));
            s[c] = mfma16x16x32(kf, qf[kk], s[c]);
          }
        }
        // lane holds the scores of query row `col` for keys 32 kc + 8 q4 + 4 c + i of the page
        float mx = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])),
                         fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        // lazy rescale: the reference moves only when a score exceeds it by > 8 (p <= 2^8 in f16)
        const bool resc = mx > m_run + 8.f;
        if (__any(resc)) {
          const float m_new = resc ? mx : m_run;
          const float alpha = m_run == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
          l_run *= alpha;
          m_run = m_new;
        }
        half8_t pf;
        float psum = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float e = __builtin_amdgcn_exp2f(s[c][i] - m_run);
            psum += e;
            pf[4 * c + i] = (f16)e;
          }
        l_run += psum;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const half8_t vf = cvt(*reinterpret_cast<const FR*>(vt_s + (16 * dt + col) * VLD + (32 * kc + 8 * q4) * EB));
          o[dt] = mfma16x16x32(vf, pf, o[dt]);
        }
      }
    }
    if (kt + 1 < n_kt) {
      store_page(buf ^ 1);   // page kt + 1 (loaded one page ago); buf ^ 1 was released by the last barrier
      __syncthreads();
      if (kt + 2 < n_kt) load_page(kt0 + kt + 2);
    }
  }
  l_run += __shfl_xor(l_run, 16);
  l_run += __shfl_xor(l_run, 32);
  if (!rvalid || prow < 0) return;
  // lane (q4, col) holds O^T[d = 16 dt + 4 q4 + i][query row col]; an empty split publishes (0, -inf, 0)
  const size_t rid = (size_t)prow * d.Hq + kvh * G + g, stride = (size_t)d.M * d.Hq;
  float* op = d.pfx_o + ((size_t)z * stride + rid) * DP;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
    *reinterpret_cast<float4*>(op + 16 * dt + 4 * q4) = make_float4(o[dt][0], o[dt][1], o[dt][2], o[dt][3]);
  if (q4 == 0) {
    float* ml = d.pfx_ml + ((size_t)z * stride + rid) * 2;
    ml[0] = m_run;
    ml[1] = l_run;
  }
}

}  // namespace mpk

namespace mp {

int attn_shared_splits(int n_groups, int Hkv, int max_pages, int max_split) {
  static const int n_cu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
      n = 256;
    return n;
  }();
  const int wgs = std::max(1, n_groups * Hkv);
  int ns = std::min(max_split, std::max(1, (n_cu + wgs - 1) / wgs));
  return std::max(1, std::min(ns, max_pages / 2));
}

void launch_attn_shared(const SharedAttnParams& p_in, hipStream_t st) {
  SharedAttnParams p = p_in;
  DecodeAttnParams& d = p.d;
  v_strides_or_legacy(d.v_kb, d.v_d);
  auto need = [](bool ok, const char* field) {
    if (!ok) throw std::runtime_error(std::string("launch_attn_shared: unsupported ") + field);
  };
  need(d.M >= 2, "M (a group has two rows)");
  need(d.Hkv >= 1 && d.Hq >= d.Hkv && d.Hq % d.Hkv == 0 && d.Hq / d.Hkv <= 16, "Hq / Hkv (G = 1 to 16)");
  need(d.Dp == 64 || d.Dp == 128, "Dp (64 or 128)");
  need(d.hd >= 2 && d.hd <= d.Dp && d.hd % 2 == 0, "hd (even, <= Dp)");
  need(d.n_psplit >= 1, "n_psplit");
  need(d.max_pages >= 1 && p.max_groups >= 1, "max_pages, max_groups");
  need(d.qkv && d.pos && d.block_table && d.rope_cs && d.k_cache && d.v_cache, "decode inputs (null)");
  need(p.groups && p.rows && d.pfx_row && d.pfx_o && d.pfx_ml, "group table or partial buffers (null)");
  need(!d.ssq || d.d_model > 0, "d_model with ssq");
  need(!d.pre, "pre (q must arrive unrotated)");
  const int rpt = 16 / (d.Hq / d.Hkv);
  const int max_rb = ((d.M + rpt - 1) / rpt + 7) / 8;   // row blocks of a group holding every row
  const dim3 grid(p.max_groups * max_rb, d.Hkv, d.n_psplit);
  if (d.Dp == 128) {
    if (d.kv_fp8) hipLaunchKernelGGL((mpk::attn_shared_kernel<128, true>), grid, dim3(512), 0, st, p, max_rb);
    else hipLaunchKernelGGL((mpk::attn_shared_kernel<128, false>), grid, dim3(512), 0, st, p, max_rb);
  } else {
    if (d.kv_fp8) hipLaunchKernelGGL((mpk::attn_shared_kernel<64, true>), grid, dim3(512), 0, st, p, max_rb);
    else hipLaunchKernelGGL((mpk::attn_shared_kernel<64, false>), grid, dim3(512), 0, st, p, max_rb);
  }
}

}  // namespace mp
