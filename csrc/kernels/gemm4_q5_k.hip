// gemm4 kernels for Q5_K and Q3_K weights, the two K-quants with a separate high-bit plane (the
// geometry table of gemm4_dispatch.h)
#include "gemm4_dispatch.h"

namespace mp {
template void gemm4_run<P_Q5_K>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
template void gemm4_run<P_Q3_K>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
}
