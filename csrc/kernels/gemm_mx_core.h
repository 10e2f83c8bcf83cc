// Device pieces the scaled-MFMA GEMMs share (gemm_mx.hip: dense, moe_mx.hip: grouped MoE): the
// workgroup id remap, the addressing of the B / scale images (kernels_api.h) and one 128-k stage of a
// wave -- counted LDS reads of the x fragments and their scale dwords, one fragment ahead of the
// v_mfma_scale_f32_32x32x64_f8f6f4 that consume them.  Operand layouts: gemm_mx.hip's header.
#pragma once
#include "kcommon.h"
#include "gemm_lds.h"

namespace mpk {
using namespace mp;

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int OFF>   // ds_read_b32 with an immediate byte offset (asm, as gemm_lds.h's ds_b128o)
__device__ __forceinline__ void ds_b32o(uint32_t& v, uint32_t addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset");
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF) : "memory");
}

// XCD-aware logical workgroup id (bijective for any grid size): consecutive ids share an XCD and its L2
__device__ __forceinline__ int mx_xcd_lid(int bx, int nwg) {
  const int xcd = bx & 7, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bx >> 3);
}

// B operand format BF: 0 = e4m3 (2 KB per 64-k block), 1 = fp4 (1 KB).  NB 16-byte pieces per lane
// per 128-k stage, 1 KB apart; one scale dword per lane per 256-k super-block
template <int BF>
struct MxB {
  static constexpr int NB = BF ? 2 : 4;
  static constexpr int STAGE_BYTES = 1024 * NB;
  // lane's first piece of column group grp
  __device__ static __forceinline__ const uint8_t* pieces(const uint8_t* W, int grp, int nsb, int lane) {
    return W + (size_t)grp * nsb * (2048 * NB) + lane * 16;
  }
  __device__ static __forceinline__ const uint32_t* scales(const uint8_t* S, int grp, int nsb, int lane) {
    return reinterpret_cast<const uint32_t*>(S) + (size_t)grp * nsb * 64 + lane;
  }
  __device__ static __forceinline__ void fetch(const uint8_t* wb, int s, u32x4 (&b)[NB]) {
#pragma unroll
    for (int j = 0; j < NB; ++j) b[j] = ld16(wb + (size_t)s * STAGE_BYTES + 1024 * j);
  }
  // MFMA kk's B operand from the stage's pieces
  __device__ static __forceinline__ i32x8 frag(const u32x4 (&b)[NB], int kk) {
    if constexpr (BF) {   // the lane's 32 nibbles; the operand's upper four registers are not read
      const u32x4 bl = b[kk];
      return i32x8{(int)bl.x, (int)bl.y, (int)bl.z, (int)bl.w, 0, 0, 0, 0};
    } else {
      const u32x4 bl = b[2 * kk], bh = b[2 * kk + 1];
      return i32x8{(int)bl.x, (int)bl.y, (int)bl.z, (int)bl.w, (int)bh.x, (int)bh.y, (int)bh.z, (int)bh.w};
    }
  }
};

// per-lane LDS addresses of a stage image (x rows of 128 B with the g3_off swizzle, then a scale dword
// slot per row at a_bytes): row 32 i + cl has the swizzle of cl, so a lane's four chunk addresses
// (MFMA kk, register half e: chunk 4 kk + 2 e + h) are fixed and fragment / buffer are immediate offsets
struct MxLdsAddr {
  uint32_t fa[4], sa;
  __device__ __forceinline__ MxLdsAddr(const char* smem, int a_bytes, int cl, int h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) fa[c] = lds_addr(smem) + g3_off(cl, 4 * (c >> 1) + 2 * (c & 1) + h);
    sa = lds_addr(smem) + a_bytes + 4 * cl;
  }
};

// Stage Q (0 | 1) of a super-block from stage buffer Q: FM row fragments x NPR column groups of the
// wave, two MFMAs each.  The LDS reads are asm: left to the compiler, every fragment's reads are
// hoisted to the top of the stage; fragment i + 1 is read ahead of fragment i's MFMAs under a counted
// lgkmcnt.  SKIP: fragments >= fr_live (uniform) run no MFMA (their reads stay: the waits count them).
template <int BF, int FM, int NPR, int STAGE, int Q, bool SKIP>
__device__ __forceinline__ void mx_stage(const MxLdsAddr& la, int h, const u32x4 (&b)[NPR][MxB<BF>::NB],
                                         const uint32_t (&wsc)[NPR], f32x16 (&acc)[FM][NPR], int fr_live) {
  i32x8 bf[NPR][2];
#pragma unroll
  for (int pp = 0; pp < NPR; ++pp)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) bf[pp][kk] = MxB<BF>::frag(b[pp], kk);
  u32x4 fr[2][4];
  uint32_t asc[2];
  auto read = [&](auto ic, u32x4 (&f)[4], uint32_t& sc) {   // 5 LDS reads
    constexpr int I = decltype(ic)::value;
    ds_b32o<Q * STAGE + 128 * I>(sc, la.sa);
    static_for<4>([&](auto cc) { ds_b128o<Q * STAGE + 4096 * I>(f[decltype(cc)::value], la.fa[decltype(cc)::value]); });
  };
  read(std::integral_constant<int, 0>{}, fr[0], asc[0]);
  static_for<FM>([&](auto ic) {
    constexpr int I = decltype(ic)::value;
    if constexpr (I + 1 < FM) {
      read(std::integral_constant<int, I + 1>{}, fr[(I + 1) & 1], asc[(I + 1) & 1]);
      wait_lgkm<5>();   // fragment I in, I + 1's five reads in flight
    } else {
      wait_lgkm<0>();
    }
    if (!SKIP || I == 0 || I < fr_live) {
      const int as_i = (int)(asc[I & 1] >> (8 * h));
      static_for<2>([&](auto kc) {
        constexpr int KK = decltype(kc)::value;
        const u32x4 lo = fr[I & 1][2 * KK], hi = fr[I & 1][2 * KK + 1];
        const i32x8 af = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
#pragma unroll
        for (int pp = 0; pp < NPR; ++pp)
          acc[I][pp] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af, bf[pp][KK], acc[I][pp], 0, BF ? 4 : 0, 2 * KK, as_i,
                                                                       2 * Q + KK, (int)wsc[pp]);
      });
    }
    __builtin_amdgcn_sched_barrier(0);   // the next fragment's reads stay behind these MFMAs
  });
}

}  // namespace mpk
