// gemm4 kernels for F16 weights, and for the two codebook types IQ4_NL and IQ4_XS: F16 has the one
// 128-row geometry, so this unit has the room, and the Q4_K unit stays as it is (the geometry table
// of gemm4_dispatch.h)
#include "gemm4_dispatch.h"

namespace mp {
template void gemm4_run<P_F16>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
template void gemm4_run<P_IQ4_NL>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
template void gemm4_run<P_IQ4_XS>(const Gemm4Plan&, int, const GemvParams&, const mpk::G4Moe*, hipStream_t);
}
