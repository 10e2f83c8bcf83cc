// Launch plan of the v4 dequant GEMM (csrc/kernels/gemm4*.hip): a pure host function of the shape,
// the weight type and the tuning knobs.  The launchers run exactly what the plan says, the stage
// sizes its split-K scratch from it, and the tests query it through the C API (mp_gemm4_plan).
#pragma once

namespace mp {

struct Gemm4Plan {
  bool ok;            // false (every other field 0): type or epilogue not supported, or partial stores
                      // of a shape that does not split
  int bm, nwv, tw;    // rows per workgroup, compute waves, T16 tiles per wave
  int nsplit, per;    // K splits (after the clamp to whole stages) and 64-k stages per split
  bool wnt;           // non-temporal weight DMA
  int grid_x, grid_y, grid_z;
};

// Dense launch.  partial_stores: the deterministic split-K form (split s stores its own partial);
// it takes the geometry of the accumulating epilogue whatever epi says, and is not ok below 2 splits.
Gemm4Plan plan_gemm4(int ptype, int epi, int M, int ntiles, int nsb, bool allow_split, bool partial_stores);
// Grouped MoE launch over E experts, k slots per token, M tokens (SWIGLU or ATOMIC; per_slot: the
// down projection stores one row per slot, so it does not split K).
Gemm4Plan plan_moe_gemm4(int ptype, int epi, int M, int k, int E, int ntiles, int nsb, bool per_slot);

}  // namespace mp
