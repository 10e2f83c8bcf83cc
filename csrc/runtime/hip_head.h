// HipHead: everything the last stage does after the LM head's logits.  It exists only on a stage with
// spec().last() and owns that stage's head state: the logits and arg-max scratch, the penalty windows,
// the per-request sampling table and draw indices, the token masks and their pinned mirrors, the
// logprob records, the score / verify chunk buffers, the kept last prompt rows and the pooling buffers.
// The stage keeps lm_head() (GEMV routing, xn_), the sampler step and the decode graphs.
#pragma once
#include "hip_stage.h"

namespace mp {

class HipHead {
 public:
  explicit HipHead(HipStage& stage);   // the buffers every last stage has, and those of row_sampling / row_masks
  ~HipHead();

  const float* logits() const { return logits_; }
  int logits_ld() const { return logits_ld_; }
  const void* logprob_rec(int mb) const { return lp_rec_.empty() ? nullptr : lp_rec_[mb]; }

  // The head of M rows x of micro-batch mb -> tok_out: LM head, then raw-logit statistics (n_probs) ->
  // adjust -> mask -> choose -> the chosen tokens' logprobs -> the windows.  advance: a decode step
  // (row_sampling: the rows' draw indices move on)
  void run(int mb, int M, const float* x, int32_t* tok_out, uint64_t salt, hipStream_t st, bool advance = false);
  // the last-stage part of a prefill chunk of T rows x: verify, score and embed chunks, else the rows
  // that end a prompt are kept for prefill_finish()
  void prefill_chunk(int mb, const std::vector<PrefillSeg>& segs, const float* x, int T, hipStream_t st);
  // the head over the kept rows -> tok[b]; with `rows`, only those rows' tokens change
  void prefill_finish(int mb, int32_t* tok, hipStream_t st, const std::vector<int>* rows);

  // (the stage calls these when the engine-wide penalties or n_probs change)
  void ensure_hist();
  void ensure_logprob();

  void set_history(int mb, const std::vector<std::vector<int32_t>>& seqs);
  void set_row_sampling(int mb, int row, const RowSampling& r);
  void set_row_draws(int mb, const std::vector<int32_t>& draws);
  void set_row_masks(const std::vector<int>& slots, const uint32_t* const* bits);
  void set_score_targets(int mb, const int32_t* host, int n, int top_n);
  void copy_scores(int mb, int n, float* target_lp, int32_t* top_id, float* top_lp);
  void copy_verify_tokens(int mb, int32_t* host, int n);
  void copy_embeddings(const std::vector<int>& slots, float* host);
  void copy_token_embeddings(int mb, int n_rows, float* host);

 private:
  bool rows_on() const { return row_tab_ != nullptr; }
  void ensure_chunk_head();
  void ensure_pool(int mb);
  void pool_chunk(int mb, const std::vector<PrefillSeg>& segs, const float* x, int T, hipStream_t st);

  HipStage& s_;
  const ModelConfig& cfg_;
  const StageOptions& opt_;
  DevAllocs mem_;

  float* logits_ = nullptr; int logits_ld_ = 0;       // [mb_size][logits_ld_]
  ArgmaxScratch am_{nullptr, nullptr, 0};             // two-level argmax partials / arrival counters
  int32_t* tok_tmp_ = nullptr;                        // row-selective prefill_finish
  std::vector<float*> last_h_;                        // [mb][B][d] final prompt rows
  // repetition-penalty windows: [n_mb][mb_size][hist_ld_] token ring, -1 = empty, and the per-row
  // count of accepted tokens (ring position)
  int32_t* hist_ = nullptr;
  int32_t* hist_cnt_ = nullptr;
  int hist_n_ = 0;
  int hist_ld_ = 0;   // row stride of hist_: hist_n_, plus kMaxLogitBias with row_sampling (the row's bias ids
                      // follow its window, so launch_logprob saves their raw logits with the window's)
  // per-request sampling (opt_.row_sampling): the slots' records [n_mb][mb_size] on the device and
  // their host copy, and each slot's draw index
  RowSampling* row_tab_ = nullptr;
  std::vector<RowSampling> row_host_;
  int32_t* row_draw_ = nullptr;
  // per-slot token masks (opt_.row_masks): the table [n_mb * mb_size][mask_ldw_] and the slots' on
  // flags on the device, and their pinned host mirrors (the source of the stream copies)
  uint32_t* mask_tab_ = nullptr; uint32_t* mask_host_ = nullptr;
  int32_t* mask_on_ = nullptr; int32_t* mask_on_host_ = nullptr;
  int mask_ldw_ = 0;
  // speculative verify / score chunks: [chunk][logits_ld_], and [n_mb][chunk] greedy token after each row
  float* vlogits_ = nullptr;
  int32_t* vtok_ = nullptr;
  // token logprobs (n_probs != 0): per micro-batch record (Stage::logprob_rec), the rows' log-sum-exp
  // and the raw logits of the penalty window's ids saved before the in-place penalty
  std::vector<float*> lp_rec_;
  float* lp_lse_ = nullptr;                           // [mb_size]
  float* lp_hist_raw_ = nullptr; int lp_hist_n_ = 0;  // [mb_size][hist_ld_]
  // prompt scoring: per micro-batch targets and results of a score chunk
  int32_t* sc_tgt_ = nullptr; float* sc_lp_ = nullptr; float* sc_lse_ = nullptr;   // [n_mb][chunk]
  int32_t* sc_top_id_ = nullptr; float* sc_top_lp_ = nullptr;                      // [n_mb][chunk][kMaxProbs]
  int sc_top_n_ = 0;
  // embeddings (allocated by the first embed chunk): the chunk's segment table, the slots' running
  // sums and results [n_slots][d], the mean's block sums, and per micro-batch the chunk's normed rows
  // [chunk][d] (none: the result; mean: the rows the block sums are taken over)
  PoolSeg* pool_tab_ = nullptr; int pool_tab_cap_ = 0;
  float* pool_acc_ = nullptr; float* pool_emb_ = nullptr;
  float* pool_part_ = nullptr; int pool_part_cap_ = 0;
  std::vector<float*> pool_h_;
};

}  // namespace mp
