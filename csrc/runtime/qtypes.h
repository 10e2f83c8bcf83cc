// ggml block types (GGUF) and mipipe's MI355X-native packed weight layout.
//
// Packed layout ("T16"): a weight W[N][K] (row n = output feature) is cut into tiles of 16 rows
// and super-blocks of 256 k.  Tile t's super-blocks are contiguous, so one wavefront streams a
// tile with 16-B-per-lane coalesced loads.  Inside a (tile, super-block) chunk the bytes are
// arranged so that lane l = 16*g + r (g = l>>4, r = l&15) of a wave gets, with ONE 16-B load per
// 128-k half, exactly the 32 quantized weights of row r that feed its B-operand fragments of four
// consecutive v_mfma_f32_16x16x32_f16 (k = 128h + 32s + 8g + j, s = 0..3, j = 0..7).  Nibble order
// inside a dword lets ((w >> 4i) & 0x000F000F) | 0x64006400 produce a packed f16 pair (1024+q)
// directly.  Bytes per chunk equal 16 x the ggml block bytes (no bandwidth overhead), except F16
// which stores plain f16.
//
// The two low-bit K-quants (GGUF side, 256 weights per block; element e = 128 n + 32 j + l with
// n = 0..1, j = 0..3, l = 0..31, 16-wide sub-block e / 16 = 8 n + 2 j + l / 16):
//   Q2_K, 84 B:  scales[16], qs[64], f16 d, f16 dmin.  q = (qs[32 n + l] >> 2 j) & 3,
//                sc = scales[e / 16] & 15, m = scales[e / 16] >> 4, w = d sc q - dmin m.
//   Q3_K, 110 B: hmask[32], qs[64], scales[12], f16 d.  lo = (qs[32 n + l] >> 2 j) & 3,
//                hi = (hmask[l] >> (4 n + j)) & 1, q = lo + 4 hi - 4 in [-4, 3]; the 6-bit scale of
//                sub-block k: low4 = k < 8 ? scales[k] & 15 : scales[k - 8] >> 4,
//                high2 = (scales[8 + k % 4] >> (2 (k / 4))) & 3, s_k = (low4 | high2 << 4) - 32,
//                w = d s_k q.
// Packed, both keep the k-mapping above with 2-bit fields: ONE 16-B piece per lane holds the lane's
// 64 quants of the super-block, fragment (h, s) in dword 2 (s >> 1) + h, element j at bit
// 16 (j & 1) + 8 (s & 1) + 2 (j >> 1), so that four masks on w and on w >> 8 give 16 weights
// (csrc/kernels/dequant.h).  Chunk sections:
//   P_Q3_K (1760 B): quants [lane] 16 B | high bits [lane] 8 B (dword h, bit 8 s + 4 (j & 1) + (j >> 1))
//                    | scales [r] 12 B: byte b of v_g at 4 b + g, v_g = the four 6-bit (s_k + 32) of
//                    lane group g's sub-blocks 4g..4g+3, 6 bits each | d [r] 2 B
//   P_Q2_K (1344 B): quants [lane] 16 B | scale bytes [r] 16 B (dword g = sub-blocks 4g..4g+3, as
//                    in GGUF) | (d, dmin) [r] 4 B
//
// The 32-weight-block types with a fifth bit, and the two codebook types (GGUF side, recalled from
// upstream; in every 32-weight block element l < 16 is the low nibble of qs[l] and element l + 16
// the high nibble of qs[l], as in Q4_0):
//   Q5_0, 22 B / 32:    f16 d, u8 qh[4] (one 32-bit word, 2-byte aligned), qs[16].
//                       q = nibble | ((qh >> e) & 1) << 4 for element e, w = d (q - 16).
//   Q5_1, 24 B / 32:    f16 d, f16 m, qh[4], qs[16].  q as Q5_0, w = d q + m.
//   IQ4_NL, 18 B / 32:  f16 d, qs[16].  w = d kvalues[nibble], kvalues = {-127, -104, -83, -65, -49,
//                       -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113}.
//   IQ4_XS, 136 B / 256: f16 d, u16 scales_h, scales_l[4], qs[128].  Sub-block ib = 0..7 (32 weights,
//                       qs[16 ib ..]): ls = ((scales_l[ib / 2] >> 4 (ib % 2)) & 15) | ((scales_h >> 2 ib) & 3) << 4,
//                       w = d (ls - 32) kvalues[nibble].
// Packed, all four keep the k-mapping and the two 16-B quant pieces per lane of Q4_K.  Q5_0 / Q5_1
// keep Q4_K's nibble order and Q5_K's high-bit plane (the exponent magic applies).  The codebook
// types are looked up four nibbles at a time (w & 0x0F0F0F0F and (w >> 4) & 0x0F0F0F0F index a
// 16-byte register table through v_perm), so element j sits at bit 8 (j & 3) + 4 (j >> 2): the even
// nibbles are j = 0..3, the odd ones j = 4..7, each already in fragment order.  Chunk sections:
//   P_Q5_0 (2816 B):   quants [h][lane] 16 B | high bits [h][lane] 4 B (bit 8 s + 4 (j & 1) + (j >> 1))
//                      | d [r] 16 B (f16 of blocks 0..7: dword g = lane group g's blocks 2g, 2g + 1)
//   P_Q5_1 (3072 B):   as P_Q5_0 | m [r] 16 B (same order as d)
//   P_IQ4_NL (2304 B): quants [h][lane] 16 B | d [r] 16 B (as P_Q5_0)
//   P_IQ4_XS (2176 B): quants [h][lane] 16 B | header [r] 8 B as in GGUF (d, scales_h, scales_l)
// A block past a ragged K stays zero (d = 0, m = 0: w = 0).
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define MP_HD __host__ __device__
#else
#define MP_HD
#endif

namespace mp {

enum GgmlType : int {
  T_F32 = 0, T_F16 = 1, T_Q4_0 = 2, T_Q4_1 = 3, T_Q5_0 = 6, T_Q5_1 = 7, T_Q8_0 = 8, T_Q8_1 = 9,
  T_Q2_K = 10, T_Q3_K = 11, T_Q4_K = 12, T_Q5_K = 13, T_Q6_K = 14, T_Q8_K = 15, T_IQ4_NL = 20, T_IQ4_XS = 23,
  T_BF16 = 30,
};

inline const char* type_name(int t) {
  switch (t) {
    case T_F32: return "F32"; case T_F16: return "F16"; case T_BF16: return "BF16";
    case T_Q8_0: return "Q8_0"; case T_Q4_0: return "Q4_0"; case T_Q4_K: return "Q4_K";
    case T_Q5_K: return "Q5_K"; case T_Q6_K: return "Q6_K";
    case T_Q2_K: return "Q2_K"; case T_Q3_K: return "Q3_K";
    case T_Q5_0: return "Q5_0"; case T_Q5_1: return "Q5_1";
    case T_IQ4_NL: return "IQ4_NL"; case T_IQ4_XS: return "IQ4_XS"; default: return "?";
  }
}

// elements per block, bytes per block; 0 if unsupported
MP_HD inline int block_elems(int t) {
  switch (t) {
    case T_F32: case T_F16: case T_BF16: return 1;
    case T_Q8_0: case T_Q4_0: case T_Q5_0: case T_Q5_1: case T_IQ4_NL: return 32;
    case T_Q2_K: case T_Q3_K: case T_Q4_K: case T_Q5_K: case T_Q6_K: case T_IQ4_XS: return 256;
    default: return 0;
  }
}
MP_HD inline int block_bytes(int t) {
  switch (t) {
    case T_F32: return 4; case T_F16: case T_BF16: return 2;
    case T_Q8_0: return 34; case T_Q4_0: return 18;
    case T_Q2_K: return 84; case T_Q3_K: return 110;
    case T_Q5_0: return 22; case T_Q5_1: return 24; case T_IQ4_NL: return 18; case T_IQ4_XS: return 136;
    case T_Q4_K: return 144; case T_Q5_K: return 176; case T_Q6_K: return 210;
    default: return 0;
  }
}
inline size_t row_bytes(int t, int64_t n) { return (size_t)(n / block_elems(t)) * block_bytes(t); }

// Packed kernel types (what the GEMV/GEMM kernels stream).  F32 weights are packed as F16; BF16
// weights stay bf16 (P_BF16, same chunk layout as F16): no narrowing at pack time, the kernels run
// the bf16 MFMA on them.  P_I8 is not a GGUF type: per-row int8 re-quantized weights (one f32 scale
// per output row, kept beside the matrix) for the int8-activation GEMM prototype (gemm3.hip, K15).
enum PackType : int { P_F16 = 0, P_Q8_0 = 1, P_Q4_K = 2, P_Q5_K = 3, P_Q6_K = 4, P_Q4_0 = 5, P_BF16 = 6, P_I8 = 7,
                      P_Q3_K = 8, P_Q2_K = 9, P_Q5_0 = 10, P_Q5_1 = 11, P_IQ4_NL = 12, P_IQ4_XS = 13 };
constexpr bool is16(int p) { return p == P_F16 || p == P_BF16; }

inline int pack_type_of(int ggml_type) {
  switch (ggml_type) {
    case T_F32: case T_F16: return P_F16;
    case T_BF16: return P_BF16;
    case T_Q8_0: return P_Q8_0; case T_Q4_0: return P_Q4_0;
    case T_Q4_K: return P_Q4_K; case T_Q5_K: return P_Q5_K; case T_Q6_K: return P_Q6_K;
    case T_Q3_K: return P_Q3_K; case T_Q2_K: return P_Q2_K;
    case T_Q5_0: return P_Q5_0; case T_Q5_1: return P_Q5_1;
    case T_IQ4_NL: return P_IQ4_NL; case T_IQ4_XS: return P_IQ4_XS;
    default: return -1;
  }
}

// bytes of one (16-row tile, 256-k super-block) chunk
constexpr int chunk_bytes(int p) {
  return is16(p) ? 8192 : p == P_Q8_0 ? 4352 : p == P_Q4_K ? 2304 : p == P_Q5_K ? 2816
       : p == P_Q6_K ? 3360 : p == P_Q4_0 ? 2304 : p == P_I8 ? 4096
       : p == P_Q3_K ? 1760 : p == P_Q2_K ? 1344 : p == P_Q5_0 ? 2816 : p == P_Q5_1 ? 3072
       : p == P_IQ4_NL ? 2304 : p == P_IQ4_XS ? 2176 : 0;
}

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

struct PackedDims {
  int64_t N, K, N_pad, K_pad, ntiles, nsb;
  size_t bytes;
};

inline PackedDims packed_dims(int ptype, int64_t N, int64_t K) {
  PackedDims d;
  d.N = N; d.K = K;
  d.N_pad = round_up(N, 16);
  d.K_pad = round_up(K, 256);
  d.ntiles = d.N_pad / 16;
  d.nsb = d.K_pad / 256;
  d.bytes = (size_t)d.ntiles * d.nsb * chunk_bytes(ptype);
  return d;
}

}  // namespace mp
