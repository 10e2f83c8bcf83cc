#include "gemm4_plan.h"

#include "kernels_api.h"
#include "qtypes.h"
#include "tuning.h"

#include <algorithm>

namespace mp {

namespace {

// K splits wanted by a launch of `wgs` workgroups: enough for one round over the 256 CUs (one 8-wave
// workgroup per CU: the 3-stage LDS ring takes ~130 KB), >= 16 stages (1024 k) per split
int auto_splits(int wgs, int n_stages, int target) {
  if (wgs >= target) return 1;
  return std::max(1, std::min(target / wgs, n_stages / 16));
}

// share of the 256 CUs busy over the whole rounds that w workgroups take
double cu_fill(long w) { return (double)w / ((w + 255) / 256 * 256); }

// The part every launch shares: the split count clamped to whole stages, the weight DMA mode, the grid.
Gemm4Plan finish(int bm, int nwv, int tw, int nsplit, int per, int M, int ntiles, bool moe, int E, int k_wnt) {
  const int n_mb = (M + bm - 1) / bm;   // MoE: M = the most rows one expert can get
  Gemm4Plan pl{};
  pl.ok = true;
  pl.bm = bm; pl.nwv = nwv; pl.tw = tw; pl.nsplit = nsplit; pl.per = per;
  // non-temporal weight DMA where one row block reads each weight (GEMM4_WNT 0 = auto, 1 on, 2 off):
  // 70B gate/up 322 -> 287 us cold, +0.8 % / +1.4 % tok/s on 70B mb256 / Mixtral in the engine; with
  // two row blocks per column group (8B gate/up at M = 256) the second read needs the L2 copy (86.5
  // -> 89.7 us): profiles/r8k_wnt_ab.txt
  pl.wnt = k_wnt == 1 || (k_wnt == 0 && (moe || n_mb == 1));
  pl.grid_x = (ntiles + tw * nwv - 1) / (tw * nwv) * n_mb;
  pl.grid_y = nsplit;
  pl.grid_z = E;
  return pl;
}

// `want` K splits over n_stages stages: whole stages per split, no empty split
void clamp_splits(int want, int n_stages, int* nsplit, int* per) {
  want = std::max(1, std::min(want, n_stages));
  *per = (n_stages + want - 1) / want;
  *nsplit = (n_stages + *per - 1) / *per;
}

}  // namespace

Gemm4Plan plan_gemm4(int ptype, int epi, int M, int ntiles, int nsb, bool allow_split, bool partial_stores) {
  const int k_bm = knob(KNOB_GEMM3_BM), k_nw = knob(KNOB_GEMM4_NW), k_tw4 = knob(KNOB_GEMM4_TW4);
  const int k_split = knob(KNOB_GEMM3_SPLIT), k_wg = knob(KNOB_GEMM2_SPLIT_WG), k_wnt = knob(KNOB_GEMM4_WNT);
  if (!gemm4_supported(ptype) || (epi != EPI_STORE && epi != EPI_ATOMIC && epi != EPI_SWIGLU)) return Gemm4Plan{};
  if (partial_stores) epi = EPI_ATOMIC;   // the accumulating shapes' geometry
  const bool quant = !is16(ptype);
  const int n_stages = nsb * 4;

  // 8 waves x 64 columns on 128-row tiles (GEMM4_TW4 4: every dense shape, 5: the whole-K SwiGLU
  // gate/up only, 6: the split-K shapes only): a 128 x 512 workgroup tile whose A fragments each feed
  // two MFMAs (half the A-fragment LDS reads per MFMA of the 8 x 32 form) at two waves per SIMD (128
  // accumulators + ~110 registers: 237 VGPRs, no spills)
  // (A 7-wave 128-row tile at two workgroups per CU -- 81408 B of LDS fits, but the 128-register
  // cap it needs spilled VGPRs that hold in-flight asm LDS reads: tools/isa_lint.py, 82 findings.
  // Not shipped; the 96-row MoE tile reaches two per CU within its registers, r12i.)
  const bool w8x64 = quant && (k_tw4 == 4 || (k_tw4 == 5 && epi == EPI_SWIGLU) || (k_tw4 == 6 && epi != EPI_SWIGLU));

  // rows per workgroup: 256 unless one 128-row block holds M, or 256-row tiles leave most of the 256
  // CUs idle (8B gate/up at M = 256: 112 workgroups of 256 rows, 112 us, against 224 of 128 rows,
  // 78 us: profiles/r8a_gemm_microbench.txt).  16-bit weights: always 128, their raw stage images
  // leave no room for three 256-row x images in LDS
  int bm = 128;
  if (quant && !w8x64) {
    const int cgs = (ntiles + 15) / 16;
    if (k_bm) bm = k_bm;
    else if (M > 128) bm = cgs * ((M + 255) / 256) < 192 && cgs * ((M + 127) / 128) <= 512 ? 128 : 256;
  }
  const int n_mb = (M + bm - 1) / bm;

  // waves x tiles per wave, before the 7-wave choice below
  int nwv = 8, tw = 2;
  if (w8x64) {
    tw = 4;
  } else if (quant && (((k_tw4 & 1) && bm == 256) || (k_tw4 == 2 && bm >= 128))) {
    // 4 waves of 64 columns (one per SIMD): every A fragment read from LDS feeds two MFMAs (half the
    // LDS A traffic of 8 waves x 32 columns); the same 256-column workgroup tile and grid
    nwv = 4; tw = 4;
  } else if (quant && bm == 128 && k_nw == 4) {
    // GEMM4_NW=4: 4 waves x 32 columns (64 KB of LDS, <= 256 registers): two independent workgroups
    // per CU, so one's stage barrier and DMA waits overlap the other's MFMAs
    nwv = 4;
  }
  // workgroups resident per CU: 2 for the 96-row tiles (~72 KB of LDS) and the 4 x 32 form
  const int per_cu = bm == 96 || (nwv == 4 && tw == 2) ? 2 : 1;

  int want = 1;
  if (partial_stores || (epi == EPI_ATOMIC && allow_split))
    want = k_split > 0 ? k_split : auto_splits((ntiles + tw * nwv - 1) / (tw * nwv) * n_mb, n_stages, k_wg * per_cu);
  int nsplit, per;
  clamp_splits(want, n_stages, &nsplit, &per);
  if (partial_stores && nsplit < 2) return Gemm4Plan{};

  // 7 compute waves (224 columns, or 448 of the 8 x 64 form) when that fills more of the 256 CUs in
  // whole rounds (70B gate/up at M = 256: 224 -> 256 workgroups), else 8; knob GEMM4_NW.  The 8 x 32
  // forms take it for unsplit launches only.
  if (quant && nwv == 8 && (tw == 4 || nsplit == 1)) {
    auto fill = [&](int nw) { return cu_fill((long)(ntiles + tw * nw - 1) / (tw * nw) * n_mb * nsplit); };
    if (k_nw == 7 || (k_nw == 0 && fill(7) > fill(8) + 0.05)) nwv = 7;
  }
  return finish(bm, nwv, tw, nsplit, per, M, ntiles, false, 1, k_wnt);
}

Gemm4Plan plan_moe_gemm4(int ptype, int epi, int M, int k, int E, int ntiles, int nsb, bool per_slot) {
  const int k_moe64 = knob(KNOB_GEMM4_MOE64), k_nw = knob(KNOB_GEMM4_NW), k_tw4 = knob(KNOB_GEMM4_TW4);
  const int k_split = knob(KNOB_GEMM3_SPLIT), k_wg = knob(KNOB_GEMM2_SPLIT_WG), k_wnt = knob(KNOB_GEMM4_WNT);
  if (!gemm4_supported(ptype) || (epi != EPI_SWIGLU && epi != EPI_ATOMIC)) return Gemm4Plan{};
  // row tile from the mean rows per expert (M k / E): 128 up to 128, else 256; split-K (down, atomics
  // only) for the grid the ACTIVE row blocks form, except at 128-row tiles (unsplit, below).  The
  // GEMM3_SPLIT knob forces the count (A/B runs).
  const int avg = std::max(1, M * k / std::max(1, E));
  const int n_cg = (ntiles + 15) / 16, n_stages = nsb * 4;
  const bool splits = epi == EPI_ATOMIC && !per_slot;
  auto auto_or_knob = [&](int wgs) { return !splits ? 1 : k_split > 0 ? k_split : auto_splits(wgs, n_stages, k_wg); };
  int bm = 128, nwv = 8, tw = 2, want = 1;
  if (is16(ptype)) {
    want = auto_or_knob(n_cg * E * ((avg + 127) / 128));
  } else if (avg <= 64 && k_moe64 == 1) {
    // opt-in 64-row tile: drops the padding rows of Mixtral's 64 rows per expert at 256 tokens but
    // halves the MFMAs per stage for the same per-stage overhead: gate/up 499 vs 454 us, 8036 vs 8920
    // tok/s (profiles/r8ij_engine_ab.txt)
    // (64-row tiles with 64 columns per wave, TW = 4, measured 33 % slower still: twice the Q4_K
    // dequant per live MFMA, VALU-bound; profiles/r10c_moe_tile64x64.txt)
    bm = 64;
    want = auto_or_knob(n_cg * E);
  } else if (avg <= 128) {
    // the down projection unsplit: Mixtral at 256 tokens 10225-10246 vs 10091-10093 tok/s with the
    // 2 K splits that fill the 256 CUs (half the float atomics into the residual; r9i)
    want = splits && k_split > 0 ? k_split : 1;
    if (k_moe64 >= 2 && avg <= 80) {
      // GEMM4_MOE64 = 2: 96-row expert tiles (three 32-row fragments) at <= 80 mean rows per expert:
      // Mixtral's ~64 routed rows per expert at 256 tokens fill 2 of 3 fragments instead of 2 of 4,
      // and an expert rarely needs a second row block (which re-streams its weights)
      // and the down projection split 4 ways over K (float atomics into the token rows, which the two
      // slots of a token share anyway): its ~16 column groups x 8 experts are ~128 live workgroups on
      // 256 CUs.  Mixtral mb256 13495 -> 14546 tok/s with GEMM3_SPLIT=4 (r12m); GEMM4_MOE64=3: unsplit
      bm = 96;
      if (splits && k_split == 0 && k_moe64 == 2) want = 4;
    } else if (k_tw4 == 3) {
      nwv = 4; tw = 4;   // 4 waves x 64 columns
    } else if (k_nw == 7) {
      nwv = 7;           // 224-column tiles
    }
  } else {
    bm = 256;
    want = auto_or_knob(n_cg * E * ((avg + 255) / 256));
  }
  int nsplit, per;
  clamp_splits(want, n_stages, &nsplit, &per);
  return finish(bm, nwv, tw, nsplit, per, M, ntiles, true, E, k_wnt);
}

}  // namespace mp
