// Non-causal (bidirectional) flash attention on MFMA for embed chunks of models trained without the
// causal mask (<arch>.attention.causal = false: gte-Qwen2, GritLM, LLM2Vec conversions).
//
// Every row of a prompt attends to keys [0, kv_len) of its slot, whatever its own position, so the
// kernel never reads a position: a tile (m0 | n << 16, n <= 128 / G consecutive rows of ONE prompt)
// carries the prompt's length beside it, and there is no diagonal.  What follows from that:
//   * work: one 512-thread workgroup per (tile, kv head, page split) owns 128 MFMA rows
//     rho = t * G + g (16 per wave) and walks ALL ceil(kv_len / 64) pages of the prompt, or pages
//     [z, z + 1) * split_pages of them (grid.z; partials in the attn_combine layout).  The tiles of a
//     prompt are neighbours in blockIdx.x and read the same pages in the same order, so all but the
//     first reader of a page find it in L2 / MALL;
//   * masking: every page but the prompt's last is full for every row -- the page loop has no
//     compare at all, and the partial page runs after it (inside the loop the two bodies cost 164
//     VGPRs, one workgroup per CU).  The last page holds `keys` = kv_len - 64 kt live keys.  Its dead columns get
//     P = 0 by select (the score is replaced, never multiplied: stale K bytes may decode to NaN / Inf),
//     a 32-key chunk with no live key is not computed at all, and the dead columns of the V^T tile
//     are zeroed while the page is staged into LDS -- the P.V MFMA multiplies every column, and
//     0 x (a stale NaN) would be NaN.  Pages past the last are never touched;
//   * data movement as in attn_prefill.hip, which measured it: the page's K [64][Dp] and V^T [Dp][64]
//     are loaded once per workgroup (page j + 1 into registers while page j is consumed), converted
//     from e4m3 with v_cvt_scalef32_pk_f16_fp8 on the way for fp8 pages, into padded, double-buffered
//     LDS tiles shared by the 8 waves; per 32-key chunk a wave computes S^T = K Q^T with the key rows in
//     the permuted order pi(c, R) = 8 (R >> 2) + 4 c + (R & 3), so the exponentiated scores are the B
//     operand of O^T += V^T P^T as they stand; online softmax in the exp2 domain with the lazy rescale.
#include "kcommon.h"
#include "../runtime/kernels_api.h"

#include <string>
#include <type_traits>
#include <stdexcept>

namespace mpk {
using namespace mp;

// F8: e4m3 KV pages (kv_dtype "fp8").  4 waves per SIMD (<= 128 VGPRs): two workgroups per CU, so one
// computes while the other waits at its page barrier
template <int DP, bool F8>
__global__ __launch_bounds__(512, 4) void attn_encode_kernel(const EncodeAttnParams p) {
  using KR = std::conditional_t<F8, u32x2, u32x4>;   // raw 8-element chunk
  constexpr int KK = DP / 32;    // k-steps of S^T over d
  constexpr int DT = DP / 16;    // 16-row d tiles of O^T
  constexpr int KLD = DP + 8;    // K tile row stride (f16): 16 key rows of a fragment hit distinct banks
  constexpr int VLD = 64 + 8;    // V^T tile row stride (f16)
  constexpr int NT = 512;
  constexpr int KCH = 64 * DP / 8 / NT;   // 16 B K chunks per thread per page (= V chunks)
  constexpr int EB = F8 ? 1 : 2;          // bytes per cached element
  __shared__ __attribute__((aligned(16))) f16 ks[2][64 * KLD];
  __shared__ __attribute__((aligned(16))) f16 vs[2][DP * VLD];

  const int tile = blockIdx.x, kvh = blockIdx.y, z = blockIdx.z;
  if (tile >= p.n_tiles) return;
  const int m0 = (int)(p.tiles[tile] & 0xFFFFu), n = (int)(p.tiles[tile] >> 16);
  const int kv_len = p.kv_len[tile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q4 = lane >> 4, col = lane & 15;
  const int G = p.Hq / p.Hkv;
  const int R = 16 * wave + col;   // MFMA row of this lane's column
  const int t = R / G, g = R - t * G;
  const bool rvalid = t < n && R < (128 / G) * G;
  const int m = m0 + (rvalid ? t : 0), h = kvh * G + g;
  const int32_t* bt = p.block_table + (size_t)p.slot[m0] * p.max_pages;
  const int n_pg = (kv_len + 63) >> 6;
  // KV split z takes pages [kt0, kt1); its (m, l, O) partials are merged by attn_combine
  const int sp = p.n_split > 1 ? p.split_pages : n_pg;
  const int kt0 = min(z * sp, n_pg), kt1 = min(kt0 + sp, n_pg);
  const int n_kt = kt1 - kt0;

  // Q^T fragments: lane holds q[m][h][d = 32kk + 8q4 + j] (q_scale already applied), times log2(e)
  half8_t qf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    half8_t v = rvalid ? *reinterpret_cast<const half8_t*>(p.q + ((size_t)m * p.Hq + h) * DP + 32 * kk + 8 * q4) : half8_t{};
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (f16)((float)v[j] * 1.4426950408889634f);
    qf[kk] = v;
  }

  // page staging: thread owns K chunks (key = c / (DP/8), d8 = c % (DP/8)) and V chunks (dim d, key
  // block k8), c = tid + NT j; consecutive threads read consecutive 16 B of the page in either V layout
  // (kernels_api.h), the LDS image is V^T [Dp][VLD] for both
  KR kr[KCH], vr[KCH];
  const bool vblk = p.v_d == 8;
  auto v_d_of = [&](int c) { return vblk ? c % DP : c / 8; };
  auto v_k8_of = [&](int c) { return vblk ? c / DP : c % 8; };
  auto load_page = [&](int kt) {
    const int page = bt[kt];
    const uint8_t* kb = reinterpret_cast<const uint8_t*>(p.k_cache) + ((size_t)page * p.Hkv + kvh) * 64 * DP * EB;
    const uint8_t* vb = reinterpret_cast<const uint8_t*>(p.v_cache) + ((size_t)page * p.Hkv + kvh) * DP * 64 * EB;
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
      const int c = tid + NT * j;
      kr[j] = *reinterpret_cast<const KR*>(kb + (size_t)c * 8 * EB);
      vr[j] = *reinterpret_cast<const KR*>(vb + (size_t)(v_k8_of(c) * p.v_kb + v_d_of(c) * p.v_d) * EB);
    }
  };
  auto as16 = [](const KR& r) -> u32x4 {
    if constexpr (F8) return __builtin_bit_cast(u32x4, f8x8_to_h8(r));
    else return r;
  };
  // keys: live keys of the page (64 but for the prompt's last page, whose dead V columns become +0)
  auto store_page = [&](int buf, int keys) {
#pragma unroll
    for (int j = 0; j < KCH; ++j) {
      const int c = tid + NT * j;
      *reinterpret_cast<u32x4*>(&ks[buf][(c / (DP / 8)) * KLD + (c % (DP / 8)) * 8]) = as16(kr[j]);
      u32x4 v = as16(vr[j]);
      if (keys < 64) {
        const int live = keys - 8 * v_k8_of(c);   // of the chunk's 8 keys (word w: keys 2w, 2w + 1)
#pragma unroll
        for (int w = 0; w < 4; ++w) v[w] &= live >= 2 * w + 2 ? 0xFFFFFFFFu : live == 2 * w + 1 ? 0xFFFFu : 0u;
      }
      *reinterpret_cast<u32x4*>(&vs[buf][v_d_of(c) * VLD + v_k8_of(c) * 8]) = v;
    }
  };
  auto page_keys = [&](int kt) { return min(64, kv_len - 64 * kt); };

  f32x4 o[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;   // m_run in the base-2 domain
  const int krow0 = 8 * (col >> 2) + (col & 3);   // pi(c, R) - 4c

  // one staged page: MASK only for the prompt's last, partial page (keys < 64)
  auto page = [&](auto mask_tag, int buf, int keys) {
    constexpr bool MASK = decltype(mask_tag)::value;
    const f16* kt_s = ks[buf];
    const f16* vt_s = vs[buf];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      if (MASK && 32 * kc >= keys) break;   // no live key in the chunk (its first key is live otherwise)
      f32x4 s[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          const half8_t kf = *reinterpret_cast<const half8_t*>(kt_s + (32 * kc + krow0 + 4 * c) * KLD + 32 * kk + 8 * q4);
          s[c] = mfma16x16x32(kf, qf[kk], s[c]);
        }
      }
      // lane holds the scores of row `col` for keys 32 kc + 8 q4 + 4c + i of the page
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (MASK && 32 * kc + 8 * q4 + 4 * c + i >= keys) s[c][i] = -INFINITY;
          mx = fmaxf(mx, s[c][i]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      // lazy rescale: the running max only moves when a score exceeds it by > 8 (2^8: P stays far
      // inside f16 range), so the O^T rescale (DT x 4 multiplies) is skipped on most chunks
      const bool resc = mx > m_run + 8.f;
      if (__any(resc)) {
        const float m_new = resc ? mx : m_run;
        const float alpha = m_run == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_run - m_new);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
        l_run *= alpha;
        m_run = m_new;
      }
      // every computed chunk has a live key, so m_run is finite from the first chunk on
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
        const half8_t vf = *reinterpret_cast<const half8_t*>(vt_s + (16 * dt + col) * VLD + 32 * kc + 8 * q4);
        o[dt] = mfma16x16x32(vf, pf, o[dt]);
      }
    }
  };

  if (n_kt > 0) {
    load_page(kt0);
    store_page(0, page_keys(kt0));
    __syncthreads();
    if (n_kt > 1) load_page(kt0 + 1);
  }
  // the full pages, then (the split that holds it) the prompt's partial last page
  const int n_full = n_kt > 0 && page_keys(kt1 - 1) < 64 ? n_kt - 1 : n_kt;
  for (int kt = 0; kt < n_full; ++kt) {
    const int buf = kt & 1;
    page(std::false_type{}, buf, 64);
    if (kt + 1 < n_kt) {
      store_page(buf ^ 1, page_keys(kt0 + kt + 1));   // loaded one page ago; buf^1 was released by the last barrier
      __syncthreads();
      if (kt + 2 < n_kt) load_page(kt0 + kt + 2);
    }
  }
  if (n_full < n_kt) page(std::true_type{}, n_full & 1, page_keys(kt1 - 1));

  float l = l_run;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (!rvalid) return;
  if (p.n_split > 1) {   // unnormalised partials, the attn_combine layout [z][m * Hq + h][Dp]
    const size_t rid = (size_t)m * p.Hq + h, stride = (size_t)p.M * p.Hq;
    float* op = p.o_part + ((size_t)z * stride + rid) * DP;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      *reinterpret_cast<float4*>(op + 16 * dt + 4 * q4) = make_float4(o[dt][0], o[dt][1], o[dt][2], o[dt][3]);
    if (q4 == 0) {   // a split past the prompt's pages (a shorter prompt of the chunk): (-inf, 0)
      float* ml = p.ml_part + ((size_t)z * stride + rid) * 2;
      ml[0] = n_kt > 0 ? m_run * 0.6931471805599453f : -INFINITY;   // natural log
      ml[1] = n_kt > 0 ? l : 0.f;
    }
    return;
  }
  const float inv = l > 0.f ? 1.f / l : 0.f;
  f16* orow = p.out + (size_t)m * p.ldo + (size_t)h * p.hd;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int d0 = 16 * dt + 4 * q4;   // lane holds O^T[d0 + i][row]
    if (d0 + 4 <= p.hd) {
      typedef _Float16 h4 __attribute__((ext_vector_type(4)));
      *reinterpret_cast<h4*>(orow + d0) = h4{(f16)(o[dt][0] * inv), (f16)(o[dt][1] * inv), (f16)(o[dt][2] * inv),
                                             (f16)(o[dt][3] * inv)};
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (d0 + i < p.hd) orow[d0 + i] = (f16)(o[dt][i] * inv);
    }
  }
}

}  // namespace mpk

namespace mp {

void launch_attn_combine(const AttnParams& p, hipStream_t st);

void launch_attn_encode(const EncodeAttnParams& p_in, hipStream_t st) {
  if (p_in.n_tiles <= 0) return;
  EncodeAttnParams p = p_in;
  v_strides_or_legacy(p.v_kb, p.v_d);
  auto need = [](bool ok, const std::string& what) {
    if (!ok) throw std::runtime_error("launch_attn_encode: " + what);
  };
  need(p.n_tiles <= kEncodeAttnMaxTiles, "too many tiles");
  need(p.Hkv >= 1 && p.Hq >= p.Hkv && p.Hq % p.Hkv == 0 && p.Hq / p.Hkv <= 128, "bad GQA group");
  need(p.Dp == 64 || p.Dp == 128, "Dp must be 64 or 128");
  need(p.hd >= 2 && p.hd <= p.Dp && p.hd % 2 == 0, "head dim (even, <= Dp)");
  need(p.q && p.slot && p.block_table && p.k_cache && p.v_cache && p.out, "null pointer");
  need(p.max_pages >= 1 && p.M >= 1 && p.ldo >= p.Hq * p.hd, "max_pages, M, ldo");
  need(p.n_split >= 1 && (p.n_split == 1 || (p.o_part && p.ml_part && p.split_pages >= 1)),
       "split without partial buffers");
  const int bt = prefill_attn_rows_per_tile(p.Hq / p.Hkv);
  for (int i = 0; i < p.n_tiles; ++i) {
    const int m0 = (int)(p.tiles[i] & 0xFFFFu), n = (int)(p.tiles[i] >> 16);
    need(n >= 1 && n <= bt && m0 + n <= p.M, "tile " + std::to_string(i) + ": rows outside the chunk");
    need(p.kv_len[i] >= 1 && p.kv_len[i] <= p.max_pages * 64,
         "tile " + std::to_string(i) + ": kv_len " + std::to_string(p.kv_len[i]) + " outside the block table");
  }
  const dim3 grid(p.n_tiles, p.Hkv, p.n_split);
  if (p.kv_fp8) {
    if (p.Dp == 128) hipLaunchKernelGGL((mpk::attn_encode_kernel<128, true>), grid, dim3(512), 0, st, p);
    else hipLaunchKernelGGL((mpk::attn_encode_kernel<64, true>), grid, dim3(512), 0, st, p);
  } else if (p.Dp == 128) hipLaunchKernelGGL((mpk::attn_encode_kernel<128, false>), grid, dim3(512), 0, st, p);
  else hipLaunchKernelGGL((mpk::attn_encode_kernel<64, false>), grid, dim3(512), 0, st, p);
  if (p.n_split > 1) {   // LSE merge of the splits into out (attention.hip)
    AttnParams a{};
    a.M = p.M; a.Hq = p.Hq; a.hd = p.hd; a.Dp = p.Dp; a.n_split = p.n_split;
    a.o_part = p.o_part; a.ml_part = p.ml_part; a.out = p.out; a.ldo = p.ldo;
    launch_attn_combine(a, st);
  }
}

}  // namespace mp
