// gemm4 kernels for Q8_0, Q5_0 and Q5_1 weights, the 32-weight-block types with f16 block scales
// (the geometry table of gemm4_dispatch.h)
#include "gemm4_dispatch.h"

namespace mp {
template void gemm4_run<P_Q8_0>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
template void gemm4_run<P_Q5_0>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
template void gemm4_run<P_Q5_1>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
}
