// HipStage: one pipeline stage on one MI355X = a contiguous layer range, its packed weights in
// HBM, its share of the paged KV cache, per-micro-batch I/O buffers and one captured hipGraph per
// micro-batch for the decode step (E5/E6/E9 of SURVEY.md §2.2, MI355X-native).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <chrono>
#include <vector>

#include "kernels_api.h"
#include "model.h"
#include "qtypes.h"
#include "stage.h"

namespace mp {

class GgufFile;
class HipHead;
class HipLora;

#define HIP_OK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e_) + \
                                                   " at " + __FILE__ + ":" + std::to_string(__LINE__)); \
  } while (0)

// device allocations with one owner: freed when it goes (the device they were made on is current)
struct DevAllocs {
  std::vector<void*> ptrs;
  DevAllocs() = default;
  DevAllocs(const DevAllocs&) = delete;
  DevAllocs& operator=(const DevAllocs&) = delete;
  ~DevAllocs() { for (void* p : ptrs) (void)hipFree(p); }
  void* get(size_t bytes) {
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, bytes < 256 ? 256 : bytes));
    ptrs.push_back(p);
    return p;
  }
  void* zero(size_t bytes) {
    void* p = get(bytes);
    HIP_OK(hipMemset(p, 0, bytes));
    return p;
  }
};

// ggml types of the 2-D weights when initialising a synthetic model on device
struct SyntheticTypes {
  int embd = T_Q4_K, q = T_Q4_K, k = T_Q4_K, v = T_Q4_K, o = T_Q4_K, gate = T_Q4_K, up = T_Q4_K,
      down = T_Q4_K, out = T_Q6_K;
  static SyntheticTypes from_ftype(const std::string& ftype, int layer, int n_layer);
};

struct PackedMat {
  uint8_t* d = nullptr;
  int ptype = -1;
  PackedDims dims{};
  uint8_t* i8 = nullptr;    // int8_gemm: per-row int8 re-quantized copy (P_I8 chunks) ...
  float* i8_ws = nullptr;   // ... and its row scales
  size_t bytes() const { return dims.bytes; }
};

struct MatSeg {  // one launch of a (possibly merged) projection
  PackedMat m;
  int y_off = 0;  // output column offset
};

struct ExpertW {  // MoE layer weights (Mixtral); experts stored back to back
  PackedMat gateup;            // E interleaved gate/up matrices, stride gateup_stride bytes
  size_t gateup_stride = 0;
  PackedMat down;              // E down matrices
  size_t down_stride = 0;
  PackedMat router;            // [E][d] router (f16 packed)
  f16* router_dense = nullptr;  // the router unpacked to dense f16 [E_pad][nsb*256] (launch_router_logits)
};

struct LayerW {
  float* attn_norm = nullptr;
  float* ffn_norm = nullptr;
  std::vector<MatSeg> qkv;
  float* qkv_bias = nullptr;  // [q | k | v] f32 (Qwen2), q/k rows NEOX-permuted like the weights
  // Qwen3 per-head q / k RMSNorm weights, f32 [head_dim], NEOX-permuted like the q/k rows (null: none)
  float* q_norm = nullptr;
  float* k_norm = nullptr;
  PackedMat wo;
  bool fused_gateup = true;
  PackedMat gateup;           // interleaved (fused SwiGLU)
  PackedMat gate, up;         // unfused fallback
  PackedMat down;
  bool moe = false;
  ExpertW ex;
};

// the GemvParams fields every launch on a packed matrix shares
inline GemvParams gemv_params(const void* W, int ntiles, int nsb, const void* X, int ldx, int M, void* Y, int ldy,
                              void* H, int ldh, int n_valid) {
  GemvParams p{};
  p.W = (const uint8_t*)W; p.X = (const f16*)X; p.ldx = ldx; p.M = M; p.Y = (float*)Y; p.ldy = ldy;
  p.H = (f16*)H; p.ldh = ldh; p.ntiles = ntiles; p.nsb = nsb; p.n_valid = n_valid;
  return p;
}

// how a split-K projection delivers its sum
enum class SplitK {
  ADD,     // into Y within the call
  DEFER,   // Y is the residual: stored partials stay pending for its next RMSNorm (sk_pend_); else as ADD
  INIT     // Y = bias + partials, Y holds no fill: only where the route stores partials (MatRoute::store)
};

// one dense projection call (HipStage::gemv): Y / H [M][n_valid] = epilogue(x W^T)
struct MatCall {
  const PackedMat* m; int epi; int M;
  const f16* X = nullptr; int ldx = 0;                    // input rows as f16, or
  const float* Xf = nullptr; const float* gamma = nullptr;   // the f32 residual rows + gamma: fused RMSNorm
  float* Y = nullptr; int ldy = 0; f16* H = nullptr; int ldh = 0; int n_valid = 0;
  const float* bias = nullptr;                     // [n_valid] added once
  float* zero = nullptr; int64_t zero_n = 0;       // side job: floats cleared after the GEMV
  float* ssq = nullptr;                            // ATOMIC + Xf: per-row sums of squares published here
  QkvAppend qa{};                                  // gemvs STORE + Xf: RoPE + KV append epilogue (qa.pos set)
  bool allow_split = false; SplitK deliver = SplitK::ADD;
  bool small = false;                              // the gemvs family (M <= 4) where its LDS plan fits
  MatCall(const PackedMat& mat, int e, int rows) : m(&mat), epi(e), M(rows) {}
  MatCall& in(const f16* x, int ld) { X = x; ldx = ld; return *this; }
  MatCall& in_norm(const float* x, const float* g) { Xf = x; gamma = g; return *this; }
  MatCall& out(float* y, int ld, int n) { Y = y; ldy = ld; n_valid = n; return *this; }
  MatCall& out_h(f16* h, int ld, int n) { H = h; ldh = ld; n_valid = n; return *this; }
  MatCall& split(SplitK d = SplitK::ADD) { allow_split = true; deliver = d; return *this; }
  MatCall& gemvs(bool on) { small = on; return *this; }
};

// one forward pass over M rows: decode of a micro-batch (row t in slot slot0 + t) or a packed prefill chunk
struct Fwd {
  int M; const int32_t* pos; const int32_t* kvlen; const int32_t* slot; bool decode;
  int slot0; const std::vector<PrefillSeg>* segs; hipStream_t st;
  const int32_t* lora_tab = nullptr; int lora_tiles = 0;   // lora_adapters: the call's tile table and its capacity
};

class HipStage : public Stage {
 public:
  HipStage(const ModelConfig& cfg, const StageSpec& spec, const StageOptions& opt);
  ~HipStage() override;

  bool is_gpu() const override { return true; }
  void load_gguf(const GgufFile& f) override;
  void init_synthetic(const std::string& ftype, uint64_t seed) override;
  void alloc_runtime() override;   // KV cache, buffers, rope tables (after weights)

  const StageSpec& spec() const override { return spec_; }
  const ModelConfig& cfg() const { return cfg_; }
  hipStream_t stream() const override { return stream_; }
  int device() const { return spec_.device; }

  float* act(int mb) override { return act_[mb]; }          // [act_rows][d] f32 residual in/out
  int32_t* tokens(int mb) override { return tok_[mb]; }     // [mb_size] (first: input, last: output)
  int32_t* prompt_buf() override { return prompt_dev_; }
  int act_rows() const { return act_rows_; }
  int slot_of(int mb, int b) const { return mb * opt_.mb_size + b; }

  // positions of micro-batch mb (host values) before decode; kvlen = pos + 1
  void set_positions(int mb, const std::vector<int32_t>& pos) override;

  // packed prefill chunk (see Stage::prefill) and the head over the kept last rows
  void prefill(int mb, const std::vector<PrefillSeg>& segs, hipStream_t st) override;
  void prefill_finish(int mb, hipStream_t st, const std::vector<int>* rows = nullptr) override;
  void copy_verify_tokens(int mb, int32_t* host, int n) override;
  void set_n_probs(int n) override;
  const void* logprob_rec(int mb) const override;
  void set_score_targets(int mb, const int32_t* host, int n, int top_n) override;
  void copy_scores(int mb, int n, float* target_lp, int32_t* top_id, float* top_lp) override;
  void copy_embeddings(const std::vector<int>& slots, float* host) override;
  void copy_token_embeddings(int mb, int n_rows, float* host) override;

  // One decode step for micro-batch mb (graph replay if captured).
  void decode(int mb, hipStream_t st) override;
  void capture_graphs() override;
  void destroy_graphs();
  // sampling parameters are baked into the decode graphs: re-capture when they change
  void set_sampling(float temp, int top_k, float top_p, float min_p, uint64_t seed) override;
  void set_penalties(int last_n, float repeat, float freq, float presence) override;
  void set_history(int mb, const std::vector<std::vector<int32_t>>& seqs) override;
  void set_row_sampling(int mb, int row, const RowSampling& r) override;
  void set_row_draws(int mb, const std::vector<int32_t>& draws) override;
  void set_row_masks(const std::vector<int>& slots, const uint32_t* const* bits) override;
  size_t load_adapter(int id, const GgufFile& f) override;
  void unload_adapter(int id) override;
  void set_row_adapters(const std::vector<int>& slots, const std::vector<int>& ids, const std::vector<float>& scales) override;
  long graph_captures() const override { return graph_captures_; }

  size_t weight_bytes() const override { return weight_bytes_; }
  size_t kv_bytes() const override { return kv_bytes_; }
  void kv_export(int slot, int n_tok, std::vector<uint8_t>& out) override;
  void set_block_table(const std::vector<int32_t>& table) override;
  void kv_import(int slot, int n_tok, const uint8_t* data, size_t bytes) override;
  void kv_shift(const std::vector<KvShiftRec>& recs, const std::vector<int32_t>& table) override;
  size_t kv_state_bytes(int n_tok) const override;
  uint64_t sample_step() override;
  void set_sample_step(uint64_t s) override;
  const char* backend_name() const override { return "hip"; }
  const float* logits_ptr() const override;
  int logits_ld() const override;

  // decode body without graph (captured by capture_graphs)
  void decode_eager(int mb, hipStream_t st);

 private:
  void layer_forward(int li, float* x, const Fwd& f);
  void moe_ffn(const LayerW& L, int M, hipStream_t st, float* x);
  void moe_ffn_rows(const LayerW& L, int r0, int M, hipStream_t st, float* x, bool grouped = false);
  // the dense FFN: gate/up (+ SwiGLU) into h_, down into the residual x.  small: the gemvs family;
  // fused: gate/up norm the f32 residual themselves (otherwise they read xn_)
  void ffn_tail(const LayerW& L, int M, float* x, bool small, bool fused, hipStream_t st, int li = -1,
                const Fwd* f = nullptr);
  bool fuse_norm(int M) const;   // RMSNorm folded into the consuming GEMVs at this row count
  // Qwen3: per-head RMSNorm of the q and k heads of the complete q|k|v rows in qkv_ (no-op without weights)
  void qk_norm(const LayerW& L, int M, hipStream_t st);
  void build_i8_copies();
  int8_t* xq_ = nullptr; float* xqs_ = nullptr; int xq_ld_ = 0;   // int8_gemm: quantized activation rows
  const void* xq_src_ = nullptr; int xq_rows_ = 0;   // the f16 rows xq_ currently holds (set by norm_x / the quant)
  bool attention_o(int li, const Fwd& f, float* x, bool pre = false);
  void attention(int li, const Fwd& f, bool qkv_deferred, bool pre = false);
  DecodeAttnParams decode_attn_params(int li, const Fwd& f, bool qkv_deferred) const;
  bool small_path(int M) const { return opt_.small_gemv && M <= 4; }
  size_t kv_eb() const { return opt_.kv_fp8 ? 1 : 2; }   // bytes per cached K/V element
  // the V page strides of this stage's layout (kernels_api.h): blocked by default (opt_.v_blocked)
  void set_v_strides(int& v_kb, int& v_d) const {
    if (opt_.v_blocked) v_strides_blocked(Dp_, v_kb, v_d);
    else v_strides_or_legacy(v_kb, v_d);
  }
  // one V page between this stage's blocked layout and the state format's V^T (host buffers)
  void v_page_permute(const uint8_t* src, uint8_t* dst, bool to_state) const;
  void flush_sk(hipStream_t st);
  // RMSNorm of the residual x into xn_ (absorbing pending split-K partials of x first)
  void norm_x(float* x, const float* w, int M, float* zero, int64_t zero_n, hipStream_t st, const float* bias = nullptr,
              int bias_n = 0);
  // Everything gemv() acts on for one call: the kernel family.  GEMM4: its launch plan, and whether it
  // stores split-K partials to sk_part_.  GEMV: the split count handed to launch_gemv, and whether the
  // splits store to det_part_ for the fixed-order reduction (deterministic mode).  part_n: floats of
  // stored partials, either way
  enum class GemmRoute { I8, GEMM4, GEMM3, GEMM1, GEMV, GEMVS };
  struct MatRoute {
    GemmRoute family = GemmRoute::GEMV;
    Gemm4Plan g4{}; bool store = false;
    int ns = 1; bool det = false;
    size_t part_n = 0;
  };
  GemmRoute gemm_route(const MatCall& c) const;
  // pure; sk_cap: the floats the GEMM4 partials may take (alloc_runtime sizes sk_part_ with "unbounded")
  MatRoute mat_route(const MatCall& c, size_t sk_cap) const;
  GemvParams params(const MatCall& c) const;
  void gemv(const MatCall& c, hipStream_t st);
  // final RMSNorm + LM head of M rows of x into logits [M][head_->logits_ld()].  small: the gemvs form with
  // the norm fused (the decode head at M <= 4; the chunk heads of prefill keep the standalone norm)
  void lm_head(const float* x, int M, float* logits, bool small, hipStream_t st);
  friend class HipHead;
  friend class HipLora;
  // the last stage's head state and what runs on it (hip_head.h); null on every other stage
  std::unique_ptr<HipHead> head_;
  HipHead& need_head(const char* what) const;   // throws `what` on a stage without one
  // the adapter state (hip_lora.h); null without opt_.lora_adapters
  std::unique_ptr<HipLora> lora_;
  bool lora_on() const { return opt_.lora_adapters > 0; }
  // pinned double-buffered weight staging (load_gguf)
  struct Staging {
    uint8_t* buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    size_t cap = 0, bytes = 0;
    int cur = 0;
    hipStream_t st = nullptr;
    std::chrono::steady_clock::time_point t0;
  } stg_;
  double upload_gbps_ = 0;
  void stage_begin();
  void stage_end();
  void stage_put(uint8_t* dst, size_t bytes, size_t granule, const std::function<void(uint8_t*, size_t, size_t)>& fill);
  PackedMat upload_packed(int ggml_type, int64_t N, int64_t K, const std::function<const uint8_t*(int64_t)>& row);
  // E matrices of N x K packed back to back (MoE experts); row(e, n)
  PackedMat upload_packed_experts(int ggml_type, int E, int64_t N, int64_t K, size_t* stride,
                                  const std::function<const uint8_t*(int, int64_t)>& row);
  PackedMat alloc_packed_random(int ggml_type, int64_t N, int64_t K, uint64_t seed);
  float* upload_f32(const float* h, size_t n);
  void* dmalloc(size_t bytes);

  ModelConfig cfg_;
  StageSpec spec_;
  StageOptions opt_;
  hipStream_t stream_ = nullptr;
  std::vector<void*> allocs_;
  size_t weight_bytes_ = 0, kv_bytes_ = 0;

  // weights
  std::vector<LayerW> layers_;
  uint8_t* embd_raw_ = nullptr; int embd_type_ = 0; size_t embd_row_bytes_ = 0;
  float* out_norm_ = nullptr;
  PackedMat out_;

  // dims
  int Kd_ = 0, Ko_ = 0, Kff_ = 0, qkv_n_ = 0, Dp_ = 0;
  int act_rows_ = 0, scratch_rows_ = 0;

  // scratch (shared by micro-batches: compute is serial on the stage's stream)
  static constexpr int kPrefillMaxSplit = 8;
  float* pf_opart_ = nullptr; float* pf_ml_ = nullptr;   // prefill attention KV-split partials
  float* det_part_ = nullptr; size_t det_part_n_ = 0;   // deterministic split-K partials
  float* moe_yslot_ = nullptr;                           // deterministic MoE per-slot down outputs
  float* ssq_ = nullptr;   // [64] deferred-norm sums of squares, immediately followed by qkv_
  f16* xn_ = nullptr; float* qkv_ = nullptr; f16* q_ = nullptr; f16* attn_ = nullptr; f16* h_ = nullptr;
  float* gu_ = nullptr;   // unfused gate|up f32
  float* sk_part_ = nullptr; size_t sk_part_n_ = 0;   // gemm_splitk_store: per-split GEMM partials
  // split-K partials of the last o / down GEMM not yet added into the residual x: the next RMSNorm
  // of x absorbs them (norm_x), anything else reading x first calls flush_sk
  struct SkPending { float* x = nullptr; int M = 0, n = 0, ldy = 0, ns = 0, ldp = 0; int64_t ss = 0; };
  SkPending sk_pend_;
  float* o_part_ = nullptr; float* ml_part_ = nullptr; int n_split_ = 1;
  int32_t* attn_cnt_ = nullptr;   // fused decode attention: split arrival counters
  // MoE scratch
  float* moe_logits_ = nullptr; int32_t* moe_counts_ = nullptr; int32_t* moe_lists_ = nullptr;
  float* moe_w_ = nullptr; f16* moe_h_ = nullptr;
  int moe_ld_ = 64;              // router logits row stride: round_up(n_expert, 64)
  int32_t* moe_sel_ = nullptr;   // n_expert > 64: expert id per slot (fused router -> bucketing)
  // KV
  std::vector<f16*> kc_, vc_;
  int32_t* block_table_ = nullptr; int max_pages_ = 0; int n_pages_ = 0;   // paged KV (kvpager.h)
  std::vector<int32_t> host_bt_;                                            // host copy of the table
  float2* rope_cs_ = nullptr;
  std::vector<float> rope_ff_;
  // per-mb I/O
  std::vector<float*> act_;
  std::vector<int32_t*> tok_, pos_, kvlen_, slot_;
  int32_t* step_ = nullptr;
  long graph_captures_ = 0;
  // prefill metadata
  int32_t* pf_pos_ = nullptr; int32_t* pf_kvlen_ = nullptr; int32_t* pf_slot_ = nullptr;
  int32_t* prompt_dev_ = nullptr;
  // graphs
  std::vector<hipGraphExec_t> graphs_;
};

// device random init (init.hip)
void launch_init_packed(uint8_t* W, size_t nbytes, int pt, float scale, uint64_t seed, hipStream_t st);
void launch_init_raw(uint8_t* W, int64_t nblocks, int t, float scale, uint64_t seed, hipStream_t st);

}  // namespace mp
