// gemm4 kernels for Q4_K weights (the geometry table of gemm4_dispatch.h)
#include "gemm4_dispatch.h"

namespace mp {
template void gemm4_run<P_Q4_K>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
}
