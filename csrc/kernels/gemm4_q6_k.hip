// gemm4 kernels for Q6_K and Q2_K weights, the two K-quants with per-16 sub-block scale bytes (the
// geometry table of gemm4_dispatch.h)
#include "gemm4_dispatch.h"

namespace mp {
template void gemm4_run<P_Q6_K>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
template void gemm4_run<P_Q2_K>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
}
