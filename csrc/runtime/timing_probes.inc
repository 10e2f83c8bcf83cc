// Timing-probe knobs (tuning.cpp, `make PROBES=1` builds only): they skip work, so results are wrong.
    {"GEMM3_PROBE", 0, 0, 7, nullptr},
    {"ATTN_PROBE", 0, 0, 7, nullptr},   // bit 2: printf per-phase s_memrealtime stamps (decode attention, block 0)
    {"GEMM4_PROBE", 0, 0, 15, nullptr},  // bit 0: no dequant (raw bits), bit 1: no MFMA, bit 2: no LDS-DMA, bit 3: no epilogue stores
    {"GEMVS_PROBE", 0, 0, 7, nullptr},  // bit 0: no dequant / MFMA, bit 1: no x prologue, bit 2: plain epilogue store
