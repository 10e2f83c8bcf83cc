// gemm4: from a launch plan (csrc/runtime/gemm4_plan.h) to the kernel instantiation it names.
// gemm4_<type>.hip instantiate gemm4_run per weight type (Q3_K beside Q5_K, Q2_K beside Q6_K, IQ4_NL
// and IQ4_XS beside F16, Q5_0 and Q5_1 beside Q8_0);
// gemm4.hip switches on the type.
#pragma once
#include "gemm4_kernel.h"
#include "../runtime/tuning.h"   // the probe-build knobs only: every launch decision is the plan's

#include <algorithm>
#include <stdexcept>
#include <string>

namespace mp {

// The geometries that exist, X(BM, MOE, NWV, TW): rows per workgroup, grouped MoE mode, compute
// waves, T16 tiles per wave.  Exactly the set plan_gemm4 / plan_moe_gemm4 can name.
#define GEMM4_GEOMETRIES(X)                                                                     \
  X(96, false, 8, 2) X(96, false, 7, 2)                                                         \
  X(128, false, 8, 2) X(128, false, 7, 2) X(128, false, 4, 2)                                   \
  X(128, false, 4, 4) X(128, false, 8, 4) X(128, false, 7, 4)                                   \
  X(256, false, 8, 2) X(256, false, 7, 2) X(256, false, 4, 4)                                   \
  X(64, true, 8, 2) X(96, true, 8, 2) X(128, true, 8, 2) X(128, true, 7, 2) X(128, true, 4, 4)  \
  X(256, true, 8, 2)

// 16-bit weights have the 128-row 8 x 32 tile only: their raw stage images leave LDS for no other
constexpr bool g4_type_has(int ptype, int bm, int nwv, int tw) {
  return !is16(ptype) || (bm == 128 && nwv == 8 && tw == 2);
}

template <int PT, int EPI, int BM, bool MOE, int NWV, int TW>
static void gemm4_go(const Gemm4Plan& pl, const GemvParams& p, const mpk::G4Moe& mo, hipStream_t st) {
  const int n_mb = (p.M + BM - 1) / BM;   // MoE: p.M = the most rows one expert can get
  const int n_stages = p.nsb * 4, per = pl.per;
  // the kernel's DMA offsets are 32-bit per lane: the weight matrix (one expert's) and the x rows
  // it addresses must stay under 4 GiB
  if ((size_t)p.ntiles * p.nsb * mpk::W3<PT>::CB >= (size_t(1) << 32) ||
      (size_t)std::max(p.M * std::max(1, mo.k), 1) * p.ldx * 2 >= (size_t(1) << 32))
    throw std::runtime_error("gemm4: operand over 4 GiB (32-bit DMA offsets)");
  const bool wnt = pl.wnt;
  const dim3 grid(pl.grid_x, pl.grid_y, pl.grid_z), block(64 * NWV);
#define G4_LAUNCH(F) hipLaunchKernelGGL((mpk::gemm4_kernel<PT, EPI, BM, MOE, NWV, F, TW>), grid, block, 0, st, p, n_mb, per, n_stages, mo)
#ifdef MIPIPE_TIMING_PROBES
  // timing probes (knob GEMM4_PROBE): Q4_K dense gate/up (SwiGLU, 256 rows), split-K stores and the
  // 256-row store.  Bits 0-2 are FL bits 3-5; bit 3 (no epilogue stores, FL bit 6) goes alone or on
  // top of the whole skeleton (8, 15)
  if constexpr (PT == P_Q4_K && ((!MOE && ((EPI == EPI_SWIGLU && BM == 256) || (EPI == EPI_STORE && BM == 128) ||
                                           (EPI == EPI_STORE && BM == 256 && NWV == 4))) ||
                                 (MOE && EPI == EPI_SWIGLU && BM == 128 && NWV == 8))) {
    const int pk = knob(KNOB_GEMM4_PROBE);
    if (pk) {
      const int w4 = wnt ? 4 : 0;
      switch (pk) {
        case 1: if (w4) G4_LAUNCH(4 | 8); else G4_LAUNCH(8); return;
        case 2: if (w4) G4_LAUNCH(4 | 16); else G4_LAUNCH(16); return;
        case 3: if (w4) G4_LAUNCH(4 | 24); else G4_LAUNCH(24); return;
        case 4: if (w4) G4_LAUNCH(4 | 32); else G4_LAUNCH(32); return;
        case 5: if (w4) G4_LAUNCH(4 | 40); else G4_LAUNCH(40); return;
        case 6: if (w4) G4_LAUNCH(4 | 48); else G4_LAUNCH(48); return;
        case 7: if (w4) G4_LAUNCH(4 | 56); else G4_LAUNCH(56); return;
        case 8: if (w4) G4_LAUNCH(4 | 64); else G4_LAUNCH(64); return;
        case 15: if (w4) G4_LAUNCH(4 | 56 | 64); else G4_LAUNCH(56 | 64); return;
        default: throw std::runtime_error("gemm4: GEMM4_PROBE bit 3 goes alone (8) or with bits 0-2 all set (15)");
      }
    }
  }
  // the LM head of a Q4_K file is Q6_K (dense 256-row store, 4 waves x 64 columns): bit 3 only
  if constexpr (PT == P_Q6_K && !MOE && EPI == EPI_STORE && BM == 256 && NWV == 4) {
    if (knob(KNOB_GEMM4_PROBE) == 8) {
      if (wnt) G4_LAUNCH(4 | 64); else G4_LAUNCH(64);
      return;
    }
  }
  // the LDS-DMA spread schedules (knob GEMM4_SPREAD, measured no faster: PERFORMANCE.md) exist in
  // the probe build only
  if constexpr (NWV >= 7) {   // (the 4-wave forms issue more DMA per wave than a stage's spread slots)
    switch (knob(KNOB_GEMM4_SPREAD) | (wnt ? 4 : 0)) {
      case 1: G4_LAUNCH(1); return;
      case 2: G4_LAUNCH(2); return;
      case 5: G4_LAUNCH(5); return;
      case 6: G4_LAUNCH(6); return;
      default: break;
    }
  }
#endif
  if (wnt) G4_LAUNCH(4);
  else G4_LAUNCH(0);
#undef G4_LAUNCH
}

// the one map from a plan's geometry to its instantiation; a geometry outside the table throws
template <int PT, int EPI, bool MOE>
static void gemm4_geom(const Gemm4Plan& pl, const GemvParams& p, const mpk::G4Moe& mo, hipStream_t st) {
#define G4_CASE(BM, MOE_, NWV, TW)                                                \
  if constexpr (MOE_ == MOE && g4_type_has(PT, BM, NWV, TW))                      \
    if (pl.bm == BM && pl.nwv == NWV && pl.tw == TW) return gemm4_go<PT, EPI, BM, MOE_, NWV, TW>(pl, p, mo, st);
  GEMM4_GEOMETRIES(G4_CASE)
#undef G4_CASE
  throw std::runtime_error("gemm4: no kernel for the geometry bm " + std::to_string(pl.bm) + ", " + std::to_string(pl.nwv) +
                           " waves x " + std::to_string(pl.tw) + " tiles" + (MOE ? " (MoE)" : "") + ", weight type " +
                           std::to_string(PT));
}

// Launch plan pl with the kernel epilogue epi on weights of type PT; mo: the grouped MoE mode
// (SWIGLU / ATOMIC), nullptr for a dense launch
template <int PT>
void gemm4_run(const Gemm4Plan& pl, int epi, const GemvParams& p, const mpk::G4Moe* mo, hipStream_t st) {
  static_assert(mpk::g4_supported<PT>(), "gemm4: weight type");
  if (mo && epi == EPI_SWIGLU) return gemm4_geom<PT, EPI_SWIGLU, true>(pl, p, *mo, st);
  if (mo && epi == EPI_ATOMIC) return gemm4_geom<PT, EPI_ATOMIC, true>(pl, p, *mo, st);
  if (!mo && epi == EPI_STORE) return gemm4_geom<PT, EPI_STORE, false>(pl, p, mpk::G4Moe{}, st);
  if (!mo && epi == EPI_ATOMIC) return gemm4_geom<PT, EPI_ATOMIC, false>(pl, p, mpk::G4Moe{}, st);
  if (!mo && epi == EPI_SWIGLU) return gemm4_geom<PT, EPI_SWIGLU, false>(pl, p, mpk::G4Moe{}, st);
  throw std::runtime_error("gemm4: epilogue " + std::to_string(epi));
}

// instantiated in gemm4_<type>.hip
extern template void gemm4_run<P_Q4_K>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_Q5_K>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_Q6_K>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_Q8_0>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_Q3_K>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_Q2_K>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_Q5_0>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_Q5_1>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_IQ4_NL>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_IQ4_XS>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_F16>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
extern template void gemm4_run<P_BF16>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);

}  // namespace mp
