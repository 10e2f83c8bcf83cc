// Stage interface: one pipeline stage (contiguous layer range) on one device.
//   HipStage: MI355X, hand-written HIP kernels, hipGraph decode (hip_stage.h)
//   CpuStage: host reference / plumbing backend (BASELINE.json config 1: "single-stage via
//             orchestrator on the CPU backend"; also the CPU test vehicle of the pipeline runtime)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "kernels_api.h"
#include "model.h"

namespace mp {

class GgufFile;

struct StageOptions {
  int n_mb = 1;             // micro-batches in flight
  int mb_size = 1;          // sequences per micro-batch
  int max_ctx = 2048;       // KV capacity per sequence (multiple of 64)
  int prefill_chunk = 512;  // max tokens per prefill chunk (8B: 31.5k prompt tok/s vs 24.3k at 256)
  bool use_graphs = true;
  int attn_split_len = 0;   // decode flash-decoding split length (multiple of 128; 0 = auto)
  int threads = 0;          // CPU backend worker threads (0 = hardware concurrency)
  bool cpu_q8 = true;       // CPU backend: quantized weights x int8 activation blocks (cpu_qdot.cpp); false: f32
                            // dequant + f32 dot (exact to the fp32 oracle)
  bool fused_attn = true;   // decode: one fused RoPE + KV-append + attention + merge kernel
  int attn_o_max_ctx = 512;   // single-stream decode: attention + o-projection in one launch up to this max_ctx (0 = off)
  bool prefill_gemm = true; // prompt chunks > 16 rows: MFMA dequant-GEMM instead of 16-row GEMVs
  bool int8_gemm = false;   // M > 64 GEMMs on v_mfma_i32_16x16x64_i8: per-row int8 activations x per-row int8
                            // re-quantized weights (+1 B/weight of HBM; reduced precision, opt-in)
  bool gemm_splitk_store = true;   // M > 64 split-K GEMMs: per-split partial stores + a fixed-order reduction
                                   // (into the residual: absorbed by the next RMSNorm) instead of float atomics
  int prefill_gemm_v = 0;    // 0: auto (16-bit weights: gemm3; the quantized types gemm4 takes: gemm4; the rest: the
                             // 64 x 64 GEMM); 4: gemm4 (32x32x16) for every type it takes; 3: gemm3; 2: as 4 (the
                             // 128 x 256 gemm2 is retired); 1: 64 x 64
  bool prefill_flash = true; // prompt chunks: the LDS-tiled prefill flash attention (attn_prefill.hip)
  bool kv_fp8 = false;       // kv_dtype "fp8": KV pages hold OCP e4m3 bytes
  bool v_blocked = true;     // HIP V pages blocked [8][Dp][8] (a token's V lands in one 2 KB key block, a 32-key
                             // chunk is contiguous) instead of V^T [Dp][64]; the saved state format is V^T either way
  int kv_pages = 0;          // KV pool pages per stage (64 tokens each; 0: n_slots x max_ctx / 64)
  bool deterministic = false;  // split-K and MoE partials reduced in a fixed order (no float atomics
                               // on shared outputs): bitwise-reproducible logits, PP=1 == PP=S
  bool fused_norm = false;  // M <= 4 rows: deferred RMSNorm folded into the qkv / gate-up GEMVs (gemv2.hip);
                            // off by default: 8B mb1 470.7 vs 473.7 tok/s, 70B mb1 92.5 vs 104.8 (r2i)
  bool moe_gemm = true;     // M > 64 MoE FFN on the grouped expert GEMM (gemm4.hip) instead of 64-row GEMV slices
  bool row_sampling = false;   // per-request sampling: the last stage keeps a RowSampling record and a draw
                               // index per sequence slot, and head() reads them (set_row_sampling)
  bool row_masks = false;      // per-slot token masks (needs row_sampling): the last stage keeps a table of
                               // ceil(vocab / 32) words per sequence slot, and head() bans the tokens whose
                               // bit is clear in the rows that are on (set_row_masks)
  bool small_gemv = true;   // M <= 4 rows: the gemvs kernels (gemvs.hip: x staged once per workgroup,
                            // RMSNorm fused into the qkv / gate-up / LM-head GEMVs, in-workgroup split-K)
  int lora_adapters = 0;    // LoRA adapter capacity (0: off, <= 8).  > 0: the stage keeps complete, un-rotated f32
                            // projection outputs and f16 input rows at every target (gate / up unfused, no RoPE +
                            // append in the qkv GEMV, no deferred-norm qkv, no fused attention + o), whatever is
                            // loaded or bound
  int lora_max_rank = 64;   // largest rank an adapter tensor pair may have (<= 128)
};

struct PrefillSeg {
  int b = 0;          // sequence row within the micro-batch
  int p0 = 0;         // first position of this segment
  int T = 0;          // tokens
  bool last = false;  // ends the prompt
  bool score = false;   // prompt scoring chunk: the last stage runs the LM head over EVERY row and keeps the
                        // log-probability of each row's target token (set_score_targets -> copy_scores)
  bool verify = false;  // speculative verification chunk: the last stage scores EVERY row (greedy
                        // argmax after each row -> verify_tokens), nothing is kept for prefill_finish
  bool embed = false;   // embedding chunk (every segment from position 0 of its prompt on, no prefix reuse): the
                        // last stage norms and pools the rows by set_embed (-> copy_embeddings /
                        // copy_token_embeddings); no LM head, nothing kept for prefill_finish, no sampler state
};

inline const char* pooling_name(int p) {
  static const char* n[] = {"none", "mean", "cls", "last", "rank"};
  return p >= 0 && p <= 4 ? n[p] : "?";
}

// throws naming the field a record is out of range in
inline void check_row_sampling(const RowSampling& r, int vocab) {
  auto bad = [](const char* f) { throw std::runtime_error(std::string("row sampling: bad value for ") + f); };
  if (!(r.temp == r.temp)) bad("temp");
  if (r.top_k < 0) bad("top_k");
  if (!(r.top_p > 0.f && r.top_p <= 1.f)) bad("top_p");
  if (!(r.min_p >= 0.f && r.min_p <= 1.f)) bad("min_p");
  if (!(r.repeat > 0.f) || std::isinf(r.repeat)) bad("repeat");
  if (!std::isfinite(r.freq)) bad("freq");
  if (!std::isfinite(r.presence)) bad("presence");
  if (r.draw0 < 0) bad("draw0");
  if (r.n_bias < 0 || r.n_bias > kMaxLogitBias) bad("n_bias");
  for (int i = 0; i < r.n_bias; ++i) {
    if (r.bias_id[i] < 0 || r.bias_id[i] >= vocab) bad("logit_bias id");
    if (r.bias_val[i] != r.bias_val[i] || r.bias_val[i] == INFINITY) bad("logit_bias value");
  }
}

class Stage {
 public:
  virtual ~Stage() = default;
  virtual bool is_gpu() const = 0;
  virtual const StageSpec& spec() const = 0;
  virtual hipStream_t stream() const = 0;                 // nullptr on CPU
  virtual void load_gguf(const GgufFile& f) = 0;
  virtual void init_synthetic(const std::string& ftype, uint64_t seed) = 0;
  virtual void alloc_runtime() = 0;
  virtual void capture_graphs() {}

  // per micro-batch buffers (device memory for HIP, host memory for CPU)
  virtual float* act(int mb) = 0;          // [rows][d] f32 residual in/out
  virtual int32_t* tokens(int mb) = 0;     // [mb_size]
  virtual int32_t* prompt_buf() = 0;       // [n_slots][max_ctx] token ids (first stage)
  virtual void set_positions(int mb, const std::vector<int32_t>& pos) = 0;
  // Packed prefill: one chunk = segments of several sequences of micro-batch mb (rows stacked in
  // segment order, sum of T <= prefill_chunk).  The projections run as ONE GEMM over all rows
  // (weights read once per chunk, not per sequence); attention runs per segment.  The first
  // stage embeds the tokens from prompt_buf(); for a segment with `last` set, the last stage
  // keeps the final row's hidden state for prefill_finish().
  virtual void prefill(int mb, const std::vector<PrefillSeg>& segs, hipStream_t st) = 0;
  // last stage: LM head + sampling over the kept rows -> tokens(mb)[b] for every sequence of mb;
  // with `rows`, only those rows' tokens change (continuous batching admits sequences into some
  // rows while the others are mid-generation)
  virtual void prefill_finish(int mb, hipStream_t st, const std::vector<int>* rows = nullptr) = 0;
  virtual void decode(int mb, hipStream_t st) = 0;
  // last stage, after a prefill() of verify segments of micro-batch mb: the greedy next token after
  // each of the chunk's n rows (row order = segment order) -> host
  virtual void copy_verify_tokens(int mb, int32_t* host, int n) = 0;
  // Token log-probabilities (log-softmax of the RAW logits: before penalties, temperature and cuts).
  // n_probs: 0 = off (nothing is recorded or enqueued), -1 = the chosen token's logprob only,
  // 1..kMaxProbs = plus that many most likely tokens.  Last stage: every head() then leaves one
  // record per row of micro-batch mb, logprob_rec(mb) (device memory for HIP, host for CPU):
  //   f32 chosen_lp[mb_size] | i32 top_id[mb_size][kMaxProbs] | f32 top_lp[mb_size][kMaxProbs]
  static constexpr int kMaxProbs = 20;
  static size_t logprob_rec_words(int mb_size) { return (size_t)mb_size * (1 + 2 * kMaxProbs); }
  virtual void set_n_probs(int n) { n_probs_ = n; }
  virtual const void* logprob_rec(int mb) const { (void)mb; return nullptr; }
  // prompt scoring, last stage: the target token of each of the n rows of micro-batch mb's next
  // score chunk (-1 = none) and how many alternatives to keep; after that prefill(), the rows'
  // target logprobs (and top_n ids / logprobs, [n][top_n]) -> host
  virtual void set_score_targets(int mb, const int32_t* host, int n, int top_n) = 0;
  virtual void copy_scores(int mb, int n, float* target_lp, int32_t* top_id, float* top_lp) = 0;
  // Embeddings, last stage.  set_embed: how the following embed chunks pool (POOL_NONE .. POOL_LAST of
  // kernels_api.h; throws on anything else, naming it) and whether vectors are L2-normalised.  After
  // the chunks that end the prompts of `slots`: their vectors, [slots.size()][d] -> host.  POOL_NONE:
  // after each chunk of micro-batch mb, its n_rows rows' vectors [n_rows][d] -> host.
  virtual void set_embed(int pooling, bool normalize) {
    if (pooling < POOL_NONE || pooling > POOL_LAST)
      throw std::runtime_error(std::string("embed: pooling \"") + pooling_name(pooling) + "\" (" + std::to_string(pooling) +
                               ") is not supported (none, mean, cls, last)");
    embed_pool_ = pooling; embed_norm_ = normalize;
  }
  virtual void copy_embeddings(const std::vector<int>& slots, float* host) = 0;
  virtual void copy_token_embeddings(int mb, int n_rows, float* host) = 0;
  virtual const float* logits_ptr() const = 0;   // last computed logits (device/host)
  virtual int logits_ld() const = 0;
  virtual size_t weight_bytes() const = 0;
  virtual size_t kv_bytes() const = 0;
  // sampling configuration for the last stage (temp <= 0: greedy)
  virtual void set_sampling(float temp, int top_k, float top_p, float min_p, uint64_t seed) {
    temp_ = temp; top_k_ = top_k; top_p_ = top_p; min_p_ = min_p; seed_ = seed;
  }
  // repetition penalties (llama.cpp penalties sampler, applied before the cuts): every distinct
  // token among the last `last_n` accepted tokens of a sequence (prompt included) with count c
  // gets l = l > 0 ? l / repeat : l * repeat, then l -= c * freq + presence
  virtual void set_penalties(int last_n, float repeat, float freq, float presence) {
    pen_last_n_ = last_n < 0 ? 0 : last_n; pen_repeat_ = repeat; pen_freq_ = freq; pen_presence_ = presence;
  }
  bool penalties_on() const {
    return pen_last_n_ > 0 && (pen_repeat_ != 1.f || pen_freq_ != 0.f || pen_presence_ != 0.f);
  }
  // last stage: seed the penalty window of micro-batch mb (row b <- seqs[b], its last tokens)
  virtual void set_history(int mb, const std::vector<std::vector<int32_t>>& seqs) { (void)mb; (void)seqs; }

  // Per-request sampling (StageOptions::row_sampling), last stage, between engine calls: the record of
  // row `row` of micro-batch mb; its draw index becomes r.draw0.  head() then samples every row by its
  // own record; a decode step advances every row's draw index, prefill_finish() none (the engine
  // sets the indices of a micro-batch after an admission: set_row_draws).  Other stages ignore both.
  virtual void set_row_sampling(int mb, int row, const RowSampling& r) { (void)mb; (void)row; (void)r; }
  virtual void set_row_draws(int mb, const std::vector<int32_t>& draws) { (void)mb; (void)draws; }
  // Per-slot token masks (StageOptions::row_masks), last stage, between engine calls.  bits[i] is the
  // mask of sequence slot slots[i] (= mb * mb_size + row): ceil(vocab / 32) words, token t allowed iff
  // bits[i][t >> 5] >> (t & 31) & 1; a null entry switches the slot's mask off.  From the next head()
  // on, a row that is on gets -inf in every banned logit after the bias and the penalties and before
  // the arg-max, the cuts and the draw.  The caller guarantees an allowed token < vocab per mask.
  // Captured graphs are not touched.  Throws on a stage built without the option.
  virtual void set_row_masks(const std::vector<int>& slots, const uint32_t* const* bits) {
    (void)slots; (void)bits;
  }
  // LoRA adapters (StageOptions::lora_adapters > 0), every stage, between engine calls.  load_adapter
  // reads the pairs of this stage's layers from an adapter file (lora.h) into id `id` (free, < the
  // capacity) and returns the bytes they take; unload_adapter frees them.  set_row_adapters binds
  // sequence slot slots[i] (= mb * mb_size + row) to adapter ids[i] (-1: none) at user scale
  // scales[i]: from the next prefill chunk / decode step on, the slot's rows get scale * B (A x) added
  // to the projections the adapter covers.  None of the three touches a captured graph.  The defaults
  // throw: the stage was built without the option.
  virtual size_t load_adapter(int id, const GgufFile& f) {
    (void)id; (void)f;
    throw std::runtime_error("load_adapter: the stage was built without lora_adapters");
  }
  virtual void unload_adapter(int id) {
    (void)id;
    throw std::runtime_error("unload_adapter: the stage was built without lora_adapters");
  }
  virtual void set_row_adapters(const std::vector<int>& slots, const std::vector<int>& ids, const std::vector<float>& scales) {
    (void)slots; (void)ids; (void)scales;
    throw std::runtime_error("set_row_adapters: the stage was built without lora_adapters");
  }
  // how often capture_graphs() ran (health(): an admit on a row_sampling engine must not grow it)
  virtual long graph_captures() const { return 0; }

  // Checkpoint / resume (the reference has none beyond re-reading the GGUF):
  // the KV of sequence slot `slot` (= mb * mb_size + row) for positions [0, n_tok) of every layer
  // of this stage as opaque bytes in the backend's own layout (HIP: bf16-class f16 pages, CPU:
  // f32 rows), appended to `out`; kv_import writes the same bytes back.  Called with the stage
  // idle (between decode_steps calls).
  virtual void kv_export(int slot, int n_tok, std::vector<uint8_t>& out) = 0;
  // paged KV (kvpager.h): the block table [n_slots][max_ctx / 64] of page ids (kv_pages = TRASH),
  // installed between engine calls (the stage's stream is idle or synchronised first)
  virtual void set_block_table(const std::vector<int32_t>& table) = 0;
  virtual void kv_import(int slot, int n_tok, const uint8_t* data, size_t bytes) = 0;
  // Context shift, between engine calls: `table` is the block table after KvPager::shift of every
  // record's slot.  Installs it, then, in every layer of this stage, moves each record's entries of
  // positions >= n_keep + n_discard back by n_discard (KvShiftRec, kernels_api.h): V as it is, K
  // rotated by minus n_discard positions; positions < n_keep and every other slot are not touched.
  // Returns with the work done.  Never touches a captured graph.
  virtual void kv_shift(const std::vector<KvShiftRec>& recs, const std::vector<int32_t>& table) = 0;
  virtual size_t kv_state_bytes(int n_tok) const = 0;   // bytes kv_export appends for n_tok
  // sampling step counter (seeds the per-row RNG streams of the sampler)
  virtual uint64_t sample_step() = 0;
  virtual void set_sample_step(uint64_t s) = 0;
  virtual const char* backend_name() const = 0;

 protected:
  float temp_ = 0.f, top_p_ = 1.f, min_p_ = 0.f;
  int top_k_ = 0;
  uint64_t seed_ = 0;
  int pen_last_n_ = 64;
  int n_probs_ = 0;
  float pen_repeat_ = 1.f, pen_freq_ = 0.f, pen_presence_ = 0.f;
  int embed_pool_ = POOL_LAST;
  bool embed_norm_ = true;
};

}  // namespace mp
