// LoRA adapters, host side: the llama.cpp adapter GGUF reader, the f16 images the kernels read, and the
// tables that tell the kernels which rows of a micro-batch use which adapter.  No GPU dependency.
//
// An adapter adds scale * B (A x) to the outputs of up to seven projections per layer (attn_q, attn_k,
// attn_v, attn_output, ffn_gate, ffn_up, ffn_down).  scale follows llama.cpp: alpha != 0 ?
// user_scale * alpha / r : user_scale, r the rank of that tensor pair; alpha / r is folded into B when
// the file is read, user_scale stays a run-time value per sequence slot.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "model.h"

namespace mp {

class GgufFile;

enum LoraTarget : int { LORA_Q = 0, LORA_K, LORA_V, LORA_O, LORA_GATE, LORA_UP, LORA_DOWN, LORA_N_TARGETS };
constexpr int kLoraMaxAdapters = 8;
constexpr int kLoraMaxRank = 128;
constexpr int kLoraTileRows = 16;
const char* lora_target_name(int t);                     // "attn_q", ..
// input (K) and output (N) width of a target's base projection
void lora_target_dims(const ModelConfig& cfg, int target, int* K, int* N);
// the rank the kernels see: a multiple of 32 (the expand MFMA's reduction step), zero-filled
inline int lora_rank_pad(int r) { return (r + 31) / 32 * 32; }

struct LoraPair {
  int layer = 0, target = 0;
  int r = 0, K = 0, N = 0;
  std::vector<float> A;   // [r][K]
  std::vector<float> B;   // [N][r], alpha / r folded in
};

struct LoraFile {
  std::string path;
  float alpha = 0.f;
  int r_min = 0, r_max = 0;       // over every pair of the file
  int n_pairs = 0;                // pairs in the file (all layers)
  std::vector<LoraPair> pairs;    // the pairs of the layers asked for
};

// Reads and checks an adapter file against the base model; converts the pairs of layers
// [layer_begin, layer_end) only.  Every refusal throws a runtime_error naming the tensor or field.
LoraFile lora_read(const GgufFile& f, const ModelConfig& cfg, int max_rank, int layer_begin, int layer_end);

// The kernels' images of a pair: A as f16 [r_pad][K], B as f16 [N][r_pad] (zero-filled ranks).
// neox_hd > 0: the rows of B are permuted like the rows of the base q / k weights (neox_src_row).
void lora_pack_f16(const LoraPair& p, int neox_hd, std::vector<uint16_t>* A16, std::vector<uint16_t>* B16);

// ---- device tables (plain data; the kernels of lora.hip read them)
// per (adapter, layer of the stage, target): null A = the target is absent
struct LoraTargetRec {
  const void* A = nullptr;   // f16 [r_pad][K]
  const void* B = nullptr;   // f16 [N][r_pad]
  int32_t r_pad = 0;
  int32_t pad_ = 0;
};
// The tile table: word 0 = the tile count, words 1..3 unused, then the tiles.
struct LoraTile {
  int32_t adapter;
  int32_t pad_[3];
  int32_t rows[kLoraTileRows];    // row indices of the call's X / Y, -1 padded
  float scale[kLoraTileRows];     // the rows' user_scale
};
constexpr int kLoraTileWords = sizeof(LoraTile) / 4;
constexpr int kLoraTabHeader = 4;
// worst case for M rows over n_adapters: every adapter leaves one partly filled tile
inline int lora_max_tiles(int M, int n_adapters) { return M / kLoraTileRows + (n_adapters < M ? n_adapters : M); }
inline size_t lora_table_words(int max_tiles) { return kLoraTabHeader + (size_t)max_tiles * kLoraTileWords; }
// Groups rows by adapter (ascending id, rows ascending) into tiles of 16.  ids[m] = -1: row m is in no
// tile.  Throws on an id >= n_adapters or more tiles than max_tiles.  out: lora_table_words(max_tiles)
// words; returns the tile count.
int lora_build_tiles(const int32_t* ids, const float* scales, int M, int n_adapters, int max_tiles, int32_t* out);

}  // namespace mp
