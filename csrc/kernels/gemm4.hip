// Dequant GEMM v4, the launchers: plan (csrc/runtime/gemm4_plan.cpp) -> per-type kernel unit
// (gemm4_<type>.hip through gemm4_dispatch.h).  The device code is gemm4_kernel.h.
#include "gemm4_dispatch.h"

namespace mp {

bool gemm4_supported(int ptype) {
  return ptype == P_Q4_K || ptype == P_Q5_K || ptype == P_Q6_K || ptype == P_Q8_0 || ptype == P_F16 || ptype == P_BF16 ||
         ptype == P_Q3_K || ptype == P_Q2_K || ptype == P_Q5_0 || ptype == P_Q5_1 || ptype == P_IQ4_NL ||
         ptype == P_IQ4_XS;
}

bool gemm4_has_geometry(int ptype, int bm, int nwv, int tw, bool moe) {
#define G4_IS(BM, MOE, NWV, TW) if (bm == BM && moe == MOE && nwv == NWV && tw == TW) return g4_type_has(ptype, bm, nwv, tw);
  if (gemm4_supported(ptype)) { GEMM4_GEOMETRIES(G4_IS) }
#undef G4_IS
  return false;
}

int gemm4_geometry_count() {
#define G4_ONE(BM, MOE, NWV, TW) +1
  return 0 GEMM4_GEOMETRIES(G4_ONE);
#undef G4_ONE
}

static void run(int ptype, const Gemm4Plan& pl, int epi, const GemvParams& p, const mpk::G4Moe* mo, hipStream_t st) {
  switch (ptype) {
    case P_Q4_K: return gemm4_run<P_Q4_K>(pl, epi, p, mo, st);
    case P_Q5_K: return gemm4_run<P_Q5_K>(pl, epi, p, mo, st);
    case P_Q6_K: return gemm4_run<P_Q6_K>(pl, epi, p, mo, st);
    case P_Q8_0: return gemm4_run<P_Q8_0>(pl, epi, p, mo, st);
    case P_Q3_K: return gemm4_run<P_Q3_K>(pl, epi, p, mo, st);
    case P_Q2_K: return gemm4_run<P_Q2_K>(pl, epi, p, mo, st);
    case P_Q5_0: return gemm4_run<P_Q5_0>(pl, epi, p, mo, st);
    case P_Q5_1: return gemm4_run<P_Q5_1>(pl, epi, p, mo, st);
    case P_IQ4_NL: return gemm4_run<P_IQ4_NL>(pl, epi, p, mo, st);
    case P_IQ4_XS: return gemm4_run<P_IQ4_XS>(pl, epi, p, mo, st);
    case P_F16: return gemm4_run<P_F16>(pl, epi, p, mo, st);
    case P_BF16: return gemm4_run<P_BF16>(pl, epi, p, mo, st);
    default: throw std::runtime_error("gemm4: weight type " + std::to_string(ptype));
  }
}

void run_gemm4(int ptype, const Gemm4Plan& pl, int epi, const GemvParams& p, hipStream_t st) {
  run(ptype, pl, epi, p, nullptr, st);
}

bool launch_gemm4(int ptype, int epi, GemvParams p, hipStream_t st, bool allow_split) {
  const Gemm4Plan pl = plan_gemm4(ptype, epi, p.M, p.ntiles, p.nsb, allow_split, false);
  if (pl.ok) run_gemm4(ptype, pl, epi, p, st);
  return pl.ok;
}

// split-K partial stores of a partial-store plan: split s writes scratch + s * M * ldp.  init: the
// reduction writes Y = p.bias + the partials instead of adding them onto Y (which then needs no fill)
void run_gemm4_splitk(int ptype, const Gemm4Plan& pl, GemvParams p, float* scratch, hipStream_t st, bool reduce, bool init) {
  if (init && !reduce) throw std::runtime_error("gemm4 split-K: the init form reduces at once");
  if (p.bias && !init) throw std::runtime_error("gemm4 split-K: a bias takes the init form");
  const int ldp = p.ntiles * 16;
  GemvParams q = p;
  q.Y = scratch; q.ldy = ldp; q.split_stride = (int64_t)p.M * ldp;
  q.bias = nullptr;   // (init: added by the reduction)
  run(ptype, pl, EPI_STORE, q, nullptr, st);
  if (reduce) launch_splitk_reduce(scratch, pl.nsplit, q.split_stride, ldp, p.M, p.n_valid, p.Y, p.ldy, st, init, p.bias);
}

// plans itself; false (nothing launched) when the shape does not split or the partials do not fit
// scratch_n floats
bool launch_gemm4_splitk(int ptype, GemvParams p, float* scratch, size_t scratch_n, hipStream_t st, bool reduce,
                         int* nsplit_out, bool init) {
  if (p.bias && !init) return false;
  const Gemm4Plan pl = plan_gemm4(ptype, EPI_ATOMIC, p.M, p.ntiles, p.nsb, true, true);
  if (!pl.ok || (size_t)pl.nsplit * p.M * p.ntiles * 16 > scratch_n) return false;
  run_gemm4_splitk(ptype, pl, p, scratch, st, reduce, init);
  if (nsplit_out) *nsplit_out = pl.nsplit;
  return true;
}

// Grouped MoE GEMM (K13): q.M = tokens of the call (the most rows one expert can receive)
bool launch_moe_gemm4(int ptype, int epi, const MoeGemvParams& q, hipStream_t st) {
  const Gemm4Plan pl = plan_moe_gemm4(ptype, epi, q.M, q.k, q.E, q.ntiles, q.nsb, q.Yslot != nullptr);
  if (!pl.ok) return false;
  GemvParams p{};
  p.W = q.W; p.X = q.X; p.ldx = q.ldx; p.M = q.M; p.Y = q.Y; p.ldy = q.ldy; p.H = q.H; p.ldh = q.ldh;
  p.ntiles = q.ntiles; p.nsb = q.nsb; p.n_valid = q.n_valid;
  mpk::G4Moe mo;
  mo.counts = q.counts; mo.lists = q.lists; mo.list_cap = q.list_cap; mo.estride = q.estride; mo.k = q.k;
  mo.x_per_slot = q.x_per_slot; mo.weights = q.weights; mo.Yslot = q.Yslot;
  run(ptype, pl, epi, p, &mo, st);
  return true;
}

}  // namespace mp
