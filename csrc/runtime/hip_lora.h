// HipLora: a stage's adapter state (StageOptions::lora_adapters > 0; lora.h, lora.hip).  Per adapter id
// its device images; the target table [capacity][layers][7] on the device and its host copy; per
// micro-batch the decode tile table (rebuilt from the slots' bindings by set_row_adapters) and one table
// for the prefill chunk in flight (written on the stream by launch_lora_table); the shrink partials.
#pragma once
#include "hip_stage.h"
#include "lora.h"

namespace mp {

class HipLora {
 public:
  // checks the options against the kernels' limits (throws naming the key); n_layers, scratch_rows: the stage's
  HipLora(HipStage& stage, int n_layers, int scratch_rows);
  ~HipLora();

  // both return the adapter's bytes on the device (the stage counts them as weights)
  size_t load_adapter(int id, const GgufFile& f);
  size_t unload_adapter(int id);
  void set_row_adapters(const std::vector<int>& slots, const std::vector<int>& ids, const std::vector<float>& scales);

  // the tile table of a decode step of micro-batch mb / of the prefill chunk `segs` of T rows -> f
  void bind_decode(int mb, Fwd& f) const { f.lora_tab = tab_[mb]; f.lora_tiles = tiles_dec_; }
  void bind_prefill(int mb, const std::vector<PrefillSeg>& segs, int T, Fwd& f);
  // one shrink + one expand launch for a group of targets reading X [M][ldx] and adding into Y
  void group(int li, const Fwd& f, int n_t, const int* tgt, const int* N, const int* yoff, const f16* X, int ldx,
             int K, float* Y, int ldy);

 private:
  struct LoraDev { bool used = false; std::vector<void*> bufs; size_t bytes = 0; };
  HipStage& s_;
  const ModelConfig& cfg_;
  const StageOptions& opt_;
  int n_layers_;
  DevAllocs mem_;
  std::vector<LoraDev> ad_;
  LoraTargetRec* tgt_ = nullptr;
  std::vector<LoraTargetRec> tgt_host_;
  std::vector<int32_t*> tab_;
  int32_t* tab_pf_ = nullptr;
  int32_t* tab_host_ = nullptr;   // pinned mirror of the decode tables [n_mb][lora_table_words]
  int rcap_ = 0, tiles_dec_ = 0;
  float* part_ = nullptr; size_t part_n_ = 0;
  std::vector<int32_t> row_ad_;   // per slot: bound adapter (-1: none) and user scale
  std::vector<float> row_sc_;
};

}  // namespace mp
