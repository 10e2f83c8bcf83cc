// Engine = model + partition + stage workers + links + the micro-batched piped-ring scheduler.
//
// This replaces, MI355X-first, what the reference assembles from `llama-cli --rpc ... -ngl 99`
// (orchestrator/src/main.rs:35-57): llama.cpp's backend scheduler runs the layer splits of the two
// rpc-servers strictly one after the other (E7).  Here every stage owns a GPU and
// runs concurrently: M micro-batches circulate through the S stages (activations forward,
// sampled token ids from the last stage back to the first: the PDF's "piped-ring", D1), each
// stage overlaps its sends/receives (dedicated comm streams, events) with the compute of the
// other micro-batches.
//
// Modes (config "mode"):
//   "local" : all stages in this process, one host thread each; devices from "devices" (may
//             repeat a device for single-GPU PP emulation); links "local" (D2D) or "rccl".
//   "mp"    : one stage per process (torch.distributed / torchrun launch): config carries
//             "world", "rank" and the RCCL unique ids of the links this rank participates in.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "hip_stage.h"
#include "json.h"
#include "kvpager.h"
#include "model.h"
#include "threadpool.h"
#include "transport.h"

namespace mp {

class GgufFile;

struct Item {
  enum Kind { PREFILL, PREFILL_END, DECODE } kind;
  int mb = 0;
  int T = 0;                      // PREFILL: total rows of the packed chunk
  std::vector<PrefillSeg> segs;   // PREFILL: sequences (segments) packed into the chunk
  int round = 0;
  std::vector<int> rows;          // PREFILL_END of an admission: only these rows get a new token
};

struct StepStats {
  std::vector<double> token_ms;   // inter-token latency samples (per micro-batch per round)
  double wall_ms = 0;
};

// The lifecycle of one per-slot setting (a token mask, an adapter binding).  A slot's setting is off,
// pending (set for the slot's next admission) or live (in use by the running sequence).  A setting
// made for a running slot is live at once; one made for an idle slot, or handed to start() for a slot
// that is still busy with the generation before it, is pending until that admission.  start() ends
// the live ones and keeps the pending, release() ends the slot's, load_state() ends them all.
// One value per slot and setting (Engine::Slot); Engine::drain_settings runs start()'s and load_state()'s
// transition over every slot.
class SlotSetting {
 public:
  bool on() const { return st_ != OFF; }
  // running: the slot holds a running sequence and the setting is not meant for the next start()
  void set(bool value, bool running) { st_ = !value ? OFF : running ? LIVE : PENDING; }
  void clear() { st_ = OFF; }
  void admit() { if (st_ == PENDING) st_ = LIVE; }   // set for this admission: in use from here on
  // start() (all = false): a live setting ends and a pending one becomes live; load_state() (all = true):
  // whatever is on ends.  True when it ended: the caller switches it off on the stages.
  bool drain(bool all) {
    const bool ended = st_ == LIVE || (all && st_ != OFF);
    st_ = ended ? OFF : st_ == PENDING ? LIVE : st_;
    return ended;
  }

 private:
  enum State : char { OFF, PENDING, LIVE } st_ = OFF;
};

class Engine {
 public:
  explicit Engine(const Json& cfg);
  ~Engine();

  Json info() const;
  const ModelConfig& model() const { return cfg_; }
  int n_stages() const { return S_; }
  int n_mb() const { return M_; }
  int mb_size() const { return B_; }
  int max_ctx() const { return max_ctx_; }
  int kv_pages() const { return kv_pages_; }
  // config of a replacement engine after a fault: the failed stage's device dropped, layers
  // re-partitioned over the survivors (see engine.cpp)
  static Json failover_config(const Json& cfg, const Json& health);
  int kv_free_pages() const { return pager_.free_pages(); }
  double load_ms() const { return load_ms_; }
  bool owns_last() const;
  bool owns_first() const;

  // assign prompts to slots (sequence i -> mb i / B, row i % B), prefill them, produce token 0
  void start(const std::vector<std::vector<int32_t>>& prompts);
  // run k decode rounds (every micro-batch once per round); blocks until the GPU work is done
  StepStats decode_steps(int k);
  // generated tokens so far per sequence (valid where the last stage lives)
  std::vector<std::vector<int32_t>> tokens() const;
  // Token log-probabilities (config "n_probs": 0 off, -1 chosen token only, 1..20 plus that many
  // alternatives): log-softmax of the raw logits, one entry per token of tokens()
  struct SeqLogprobs {
    std::vector<float> lp;           // [tokens]
    std::vector<int32_t> top_id;     // [tokens][n_top]
    std::vector<float> top_lp;       // [tokens][n_top]
  };
  int n_probs() const { return n_probs_; }
  int n_top() const { return n_probs_ > 0 ? n_probs_ : 0; }
  std::vector<SeqLogprobs> logprobs() const;
  // the record of last_token(slot): false when none was taken (n_probs = 0, speculative decoding)
  bool last_logprob(int slot, float* lp, std::vector<int32_t>* top_id, std::vector<float>* top_lp) const;
  // Prompt scoring: out[i].lp[t] = log p(prompts[i][t + 1] | prompts[i][:t + 1]), t < len - 1, with
  // the top n_top (id, logprob) pairs per position.  At most n_mb * mb_size prompts; every stage in
  // this process.  Ends any running generation (the slots' KV is overwritten).
  void score(const std::vector<std::vector<int32_t>>& prompts, int n_top, std::vector<SeqLogprobs>* out);

  // Embeddings: prompts[k] runs through the packed-prefill path in the idle slot slots[k]; the last
  // stage norms the rows (output_norm), pools them per prompt and, with `normalize`, scales each
  // vector to unit L2 length (the zero vector stays zero).  pooling: POOL_NONE (one vector per
  // token, n_rows = prompt length), POOL_MEAN, POOL_CLS, POOL_LAST, or -1 for default_pooling().
  // No LM head, no sampler step.  Like admit(), legal before start() and between decode_steps
  // calls, for idle slots only; the other slots keep their state and the used slots are idle again
  // (their KV pages returned, their prefix-cache entry dropped) when the call returns.  Every stage
  // in this process.  Throws naming the cause: a busy slot, an empty prompt, a prompt over max_ctx,
  // a token id out of range, a pooling that is not supported.
  struct EmbedResult { std::vector<float> v; int n_rows = 1; };
  void embed(const std::vector<int>& slots, const std::vector<std::vector<int32_t>>& prompts, int pooling,
             bool normalize, std::vector<EmbedResult>* out);
  // the file's pooling_type when it is mean, cls or last; otherwise last (in a causal model the last
  // row is the only one that has seen the whole prompt)
  int default_pooling() const {
    return cfg_.pooling_type >= POOL_MEAN && cfg_.pooling_type <= POOL_LAST ? cfg_.pooling_type : POOL_LAST;
  }
  // "none" | "mean" | "cls" | "last" | "rank" -> its id, "" -> -1 (the default); throws on any other name
  static int pooling_from_name(const std::string& s) {
    if (s.empty()) return -1;
    for (int p = POOL_NONE; p <= POOL_RANK; ++p)
      if (s == pooling_name(p)) return p;
    throw std::runtime_error("unknown pooling \"" + s + "\" (none, mean, cls, last)");
  }
  // slots embed() may use now, ascending
  std::vector<int> idle_slots() const;

  // Continuous batching: between decode rounds, prefill new sequences into the
  // given sequence slots (slot = mb * mb_size + row) while the other slots keep their state; each
  // admitted slot gets its first token like start().  release() marks a slot idle (its row keeps
  // computing garbage until re-admitted; its position is recycled before it could leave the slot's
  // KV pages).  Every process of a multi-process pipeline must make the same calls.
  void admit(const std::vector<int>& slots, const std::vector<std::vector<int32_t>>& prompts);
  void release(int slot);
  // Per-request sampling (config "row_sampling": true; local mode): the record the next start() /
  // admit() of `slot` uses (kernels_api.h, RowSampling).  Legal before start() and for an idle slot;
  // release() puts the slot back to the engine's values.  Without has_seed the slot gets
  // mix64(engine seed ^ 0x9E3779B97F4A7C15 * (n + 1)), n = admissions since the engine was built;
  // slot_sampling() reports the record with the seed in use.  Throws naming the field on a value
  // out of range.  JSON form (C API, sessions, HTTP): {"temp", "top_k", "top_p", "min_p", "repeat",
  // "freq", "presence", "seed" (number or decimal string), "draw0", "logit_bias": [[id, bias | false], ..]},
  // absent fields = the engine's values.
  bool row_sampling() const { return row_sampling_; }
  // for_start: the record is for a start(), which resets every slot, so a busy slot takes it too
  void set_slot_sampling(int slot, const RowSampling& r, bool has_seed = true, bool for_start = false);
  RowSampling slot_sampling(int slot) const;
  const RowSampling& sampling_defaults() const { return row_default_; }
  RowSampling sampling_from_json(const Json& j, bool* has_seed) const;
  static Json sampling_to_json(const RowSampling& r);
  // Per-slot token masks (config "row_masks": true; needs row_sampling and switches it on when that
  // key is absent; local mode).  bits[i]: ceil(vocab / 32) words for slot slots[i], token t allowed iff
  // bits[i][t >> 5] >> (t & 31) & 1; a null entry clears the slot's mask.  From the slot's next token
  // on, the last stage bans every other token after the bias and the penalties, before the cuts and the
  // draw (logprobs stay those of the raw logits).  Legal before start(), for idle slots before admit()
  // and between decode_steps calls for running slots; never re-captures a graph.  A mask set for an
  // idle slot holds for its next start() / admit(); start() clears the masks of the generation before
  // it, release() the slot's, load_state() all of them.  Throws naming the cause: an engine without the
  // key, a slot out of range, a mask that allows no token < vocab.
  bool row_masks() const { return row_masks_; }
  // for_start: the masks are for the next start(), which clears every mask of the generation before
  // it: they survive it even when their slots are still busy with that generation
  void set_slot_masks(const std::vector<int>& slots, const uint32_t* const* bits, bool for_start = false);
  int mask_words() const { return (cfg_.vocab + 31) / 32; }
  // LoRA adapters (config "lora_adapters": the capacity, 0 = off, <= 8; "lora_max_rank", default 64,
  // <= 128; local mode).  load_adapter reads a llama.cpp adapter GGUF onto every stage (each its own
  // layers) and returns its id, the lowest free one; it throws when all ids are in use or the file is
  // refused (lora.h).  unload_adapter is refused while a slot is bound to the id.  set_slot_adapters
  // binds slot slots[i] to adapter ids[i] (-1: none) at user scale scales[i]; one adapter per slot.
  // Legal before start(), for idle slots before admit() and, for running slots, between decode_steps
  // calls; never re-captures a graph.  A binding set for an idle slot holds for its next start() /
  // admit(); start() clears the bindings of the generation before it, release() the slot's,
  // load_state() all of them.  The prefix cache reuses a slot's KV only under the binding that computed
  // it.  save_state throws while a slot is bound.
  int lora_capacity() const { return lora_cap_; }
  int load_adapter(const std::string& path);
  void unload_adapter(int id);
  Json adapters() const;   // [{"id", "path", "alpha", "rank_min", "rank_max", "bytes"}]
  void set_slot_adapters(const std::vector<int>& slots, const std::vector<int>& ids, const std::vector<float>& scales,
                         bool for_start = false);
  // the slot's binding: id (-1: none) and scale
  int slot_adapter(int slot, float* scale = nullptr) const;
  // Context shift (llama.cpp's answer to a full context; local mode, every stage in this process):
  // for each listed running slot, positions [n_keep, n_keep + n_discard) leave its KV and every later
  // position moves n_discard back -- V as it is, K rotated by minus n_discard positions (Stage::kv_shift),
  // nothing recomputed.  n_discard > 0 and a multiple of 64, n_keep >= 0, n_keep + n_discard <=
  // slot_position(slot).  Between engine calls; the slot's position drops by n_discard, n_discard / 64
  // pages return to the pool, no graph is re-captured.  The sampler state of the slot (penalty window,
  // draws, mask, logprobs) and its adapter binding stay.  A shifted slot's KV is no token prefix any
  // more: it is never a prefix-cache hit until re-admitted, and save_state refuses while one is running.
  // Throws naming the cause: mode "mp" / world > 1 / rpc, an idle slot, a violated precondition, a
  // generation that ran speculative decoding.
  void context_shift(const std::vector<int>& slots, const std::vector<int>& n_keep, const std::vector<int>& n_discard);
  // Automatic shifting (config "context_shift": true; "n_keep": tokens of the prompt that stay, default 0):
  // decode_steps(k) first shifts every running slot with position + k + 1 > max_ctx by llama.cpp's rule,
  // page-aligned: n_keep_eff = min(n_keep, prompt length), n_discard = ((pos - n_keep_eff) / 2) / 64 * 64;
  // it throws "context capacity exhausted" as without the option when that is 0 or not enough for k.
  // set_slot_keep: the slot's own n_keep (-1: the whole prompt) from now on; release() puts the
  // engine's value back.
  bool auto_shift() const { return auto_shift_; }
  void set_slot_keep(int slot, int n_keep);
  long context_shifts() const { return context_shifts_; }
  // shifts of the slot's running sequence
  int slot_shifts(int slot) const { return slot_in_range(slot) ? slots_[slot].n_shifts : 0; }
  // the most rounds the next decode_steps call can take before a running slot's context is full
  // (<= 0: one is full now; with automatic shifting a call of 1 round shifts it)
  int context_room() const;
  // what an automatic shift of `slot` would discard now (0: nothing, the kept prefix fills the context)
  int shift_discard(int slot) const;
  int32_t last_token(int slot) const {
    return slot_in_range(slot) && !slots_[slot].gen.empty() ? slots_[slot].gen.back() : -1;
  }
  int slot_position(int slot) const { return slot_in_range(slot) ? slot_pos((size_t)slot) : 0; }
  bool started() const { return started_; }
  bool slot_active(int slot) const { return slot_in_range(slot) && slots_[slot].active; }

  Json generate(const std::vector<std::vector<int32_t>>& prompts, int n_predict,
                std::vector<std::vector<int32_t>>* out);
  // Speculative decoding by prompt lookup (greedy; every stage in this process): see engine.cpp
  Json spec_generate(const std::vector<std::vector<int32_t>>& prompts, int n_predict, int draft_max, int ngram,
                     std::vector<std::vector<int32_t>>* out);
  Json bench(int prompt_len, int warmup, int steps);
  int copy_logits(int mb, float* out, int rows);
  // Chrome-trace timeline of compute / send / recv spans per stage
  void enable_trace(bool on);
  void write_trace(const std::string& path) const;
  // heartbeat counters + link byte counters per owned stage; "ok" false after a fault
  Json health() const;
  // Checkpoint / resume of a running generation: between decode_steps calls,
  // write every owned stage's KV shard (only the used positions of each sequence), its current
  // input tokens and sampler step to <dir>/stage<k>.bin, and the sequences (prompts, generated
  // tokens, rounds done) to <dir>/session.json (by the owner of the last stage).  load_state on an
  // engine built with the same model / partition / micro-batch shape continues the generation
  // exactly where it stopped (greedy and seeded sampling alike).
  Json save_state(const std::string& dir);
  Json load_state(const std::string& dir);

  // streaming hook: called on the host (from the worker of the last stage) after each round
  // with (sequence index, token) pairs
  std::function<void(int seq, int32_t tok)> on_token;
  // spec_generate: a sequence for which this returns false is finished (e.g. end of generation)
  std::function<bool(int seq)> keep_going;
  const Json& config() const { return jcfg_; }

 private:
  struct Worker {
    std::unique_ptr<Stage> stage;
    Link* in = nullptr;    // activations from s-1 (or ring tokens from S-1 for s = 0)
    Link* out = nullptr;   // activations to s+1 (or ring tokens to 0 for s = S-1)
    hipStream_t send_st = nullptr, recv_st = nullptr;
    std::vector<hipEvent_t> comp_ev, sent_ev, recv_ev;
    std::vector<bool> sent_valid;
    std::vector<uint64_t> sent_seq;   // Link::last_seq() of each micro-batch's last send
    std::vector<hipEvent_t> tok_ev;   // last stage: per (round, mb) timing events
    std::vector<double> tok_t;        // CPU backend: host timestamps of the same
    std::vector<bool> ring_pending;   // CPU backend, first stage: ring token not yet received
    std::atomic<long> progress{0};   // items completed (heartbeat)
    long items_seen = 0, sends_seen = 0;
    struct TraceRecT { std::string name; int tid = 0; hipEvent_t a = nullptr, b = nullptr; double ta = 0, tb = 0; };
    std::vector<TraceRecT> tr;
    hipEvent_t tr_base = nullptr;
    double tr_base_ms = 0;
    int device = 0;
    bool cpu = false;   // CpuStage (backend "cpu", or the host stage of a hybrid -ngl split)
    // act_dtype != f32: per micro-batch device staging of the 2-byte wire format
    std::vector<void*> wire_out, wire_in;
  };

  void build_links(const Json& cfg);
  void run_items(Worker& w, const std::vector<Item>& items);
  void run_items_cpu(Worker& w, const std::vector<Item>& items);
  void span(Worker& w, hipStream_t s, int tid, const std::string& name, const std::function<void()>& body);
  bool fault_hook(Worker& w, const char* what);
  void collect_trace();
  void run_all(const std::vector<Item>& items);
  void post_ring_recv(Worker& w, int mb);
  void sync_all();
  // fn(Worker&) for every owned stage / for the owned last stage, its device current (HIP workers)
  template <class F> void for_each_stage(F fn) {
    for (auto& w : workers_) {
      if (!w->cpu) HIP_OK(hipSetDevice(w->device));
      fn(*w);
    }
  }
  template <class F> void for_each_last_stage(F fn) {
    for (auto& w : workers_) {
      if (!w->stage->spec().last()) continue;
      if (!w->cpu) HIP_OK(hipSetDevice(w->device));
      fn(*w);
    }
  }
  // the owned first / last stage's worker, null when another process owns it
  Worker* first_worker() const;
  Worker* last_worker() const;
  // whether a setting made now for `slot` is in use at once (see SlotSetting)
  bool slot_running(int slot, bool for_start) const { return !for_start && started_ && slot_active(slot); }
  bool slot_in_range(int slot) const { return slot >= 0 && slot < M_ * B_; }
  // slots[i] is in range and none of slots[0 .. i) repeats it; throws "<fn>: slot <s> is out of range" /
  // "<fn>: slot <s> is listed twice<twice_suffix>"
  void check_slot_at(const char* fn, const std::vector<int>& slots, size_t i, const char* twice_suffix = "") const;
  // multi-process pipeline: the last stage's host vector (same length on every rank) reaches every
  // rank over the idle ring (S-1 -> 0 -> 1 -> .. -> S-2); no-op in local mode
  void ring_bcast_from_last(std::vector<int32_t>& v);

  Json jcfg_;
  ModelConfig cfg_;
  std::vector<StageSpec> specs_;
  int S_ = 1, M_ = 1, B_ = 1;
  int max_ctx_ = 2048, chunk_ = 256;
  std::string mode_ = "local";
  int rank_ = 0;
  std::vector<std::unique_ptr<Worker>> workers_;   // owned stages (all in local mode)
  std::vector<std::unique_ptr<Link>> links_;
  std::unique_ptr<GgufFile> gguf_;
  // Everything the engine knows about one sequence slot (slot = mb * mb_size + row).  slots_ holds
  // n_mb * mb_size of them from the constructor on and is never resized; a field whose feature is off
  // keeps its default.  Three transitions move a slot: begin_sequence (admission: start, admit),
  // release (the sequence ends) and reset_slots (every slot: start, score, load_state).
  struct KvTag { uint64_t serial = 0; float scale = 0.f; };
  struct Slot {
    std::vector<int32_t> prompt, gen;   // the sequence: its prompt and the tokens generated so far
    SeqLogprobs lp;                     // n_probs != 0: one record per token of gen
    // prefix cache (config "prefix_cache", default on): the tokens the slot's KV holds; an admission
    // prefills only what follows the common prefix (multi-turn chat re-sends the whole history)
    std::vector<int32_t> kv_toks;
    int base_round = 0;                 // the round at which the sequence was admitted
    bool active = false;                // a sequence is running
    // context shift: the positions the running sequence has discarded and how often; the slot's n_keep
    int shifted = 0, n_shifts = 0, n_keep = 0;
    // the prompt tokens an automatic shift keeps (n_keep -1: the whole prompt)
    int keep() const { return n_keep < 0 ? (int)prompt.size() : std::min(n_keep, (int)prompt.size()); }
    RowSampling rec;                    // row_sampling: set for the next admission / in use
    bool seed_given = false;
    int bind_id = -1;                   // LoRA: the bound adapter (-1: none) and its user scale
    float bind_scale = 0.f;
    // the binding the cached KV was computed under (serial 0: the base model; kMixedTag: rebound
    // mid-generation, never reused)
    KvTag kv_tag;
    SlotSetting mask, bind;             // the lifecycle of the slot's token mask / adapter binding
  };
  std::vector<Slot> slots_;
  // the sequences tokens(), logprobs() and session.json list, slots [0, n_seqs_): the prompt count
  // after start / load_state / spec_generate, every slot from the first admit on, none after score
  size_t n_seqs_ = 0;
  void reset_slots(size_t n_seqs);      // every sequence is over; the slots' settings and n_keep stay
  void begin_sequence(size_t slot, const std::vector<int32_t>& prompt);
  void forget_kv_toks() { for (Slot& s : slots_) s.kv_toks.clear(); }   // KV content unknown: no prefix to reuse
  std::vector<int> drain_settings(SlotSetting Slot::*which, bool all);  // the slots whose setting ended
  // the one writer of the first stage's prompt_buf: n tokens of `slot` from position pos0 on (nothing
  // where another process owns the first stage)
  void upload_tokens(size_t slot, int pos0, const int32_t* toks, size_t n);
  // The chunks of one micro-batch, in order: the rows [p0, p0 + len) of sequence row b, cut into
  // packed chunks of at most chunk_ rows (a chunk may hold several sequences; without packed_prefill
  // every segment is its own chunk).  `flags` gives every segment its score / verify / embed marks.
  struct PackRow { int b, p0, len; };
  std::vector<Item> pack_chunks(int mb, const std::vector<PackRow>& rows, const PrefillSeg& flags) const;
  int32_t* out_host_ = nullptr;                    // pinned [rounds_cap][M*B]
  std::vector<int32_t> out_vec_;                   // CPU backend storage of out_host_
  // n_probs != 0: the rounds' logprob records beside the tokens, [rounds_cap][M] records of
  // lp_words_ 4-byte words (Stage::logprob_rec); take_logprobs collects one into the slot's lp
  int n_probs_ = 0;
  size_t lp_words_ = 0;
  uint32_t* lp_host_ = nullptr;
  std::vector<uint32_t> lp_vec_;
  void take_logprobs(size_t seq, size_t round_slot);
  bool cpu_ = false;          // every stage on the CPU backend
  bool hybrid_ = false;       // gpu_layers (-ngl N) < n_layer: stage 0 on the CPU, the rest on GPUs
  bool stage_cpu(int s) const { return cpu_ || (hybrid_ && s == 0); }
  bool kv_fp8_ = false;      // kv_dtype "fp8" (checkpoint fingerprint: the KV bytes' element type)
  bool trace_ = false, failed_ = false;
  bool packed_prefill_ = true;   // several sequences per prefill chunk (config "packed_prefill")
  int act_dtype_ = 0;            // stage-boundary activation wire format (ActDtype; config "act_dtype")
  std::string link_fallback_;    // why local mode's requested RCCL links became LocalLinks (empty: none)
  double trace_t0_ = 0, watchdog_s_ = 600;
  std::vector<std::string> trace_events_;
  Json fault_;
  int rounds_cap_ = 0, rounds_done_ = 0;
  bool started_ = false;
  bool resumable_ = true;   // false after spec_generate (per-sequence positions)
  int32_t* bcast_dev_ = nullptr;   // ring_bcast_from_last device staging (RCCL / device links)
  size_t bcast_cap_ = 0;
  bool prefix_cache_ = true;   // Slot::kv_toks
  long reused_tokens_ = 0;
  void refresh_slot_cache();
  KvPager pager_;           // paged KV: one logical table, installed on every stage
  int kv_pages_ = 0;         // pool pages per stage
  std::vector<double> device_speed_;   // partitioner weights per stage (given or probed)
  int failed_stage_ = -1;    // stage whose worker raised the fault (health()["failed_stage"])
  void kv_grant(size_t slot, int n_tokens);   // throws when the pool is exhausted
  void kv_sync();            // push a changed table to the stages (between engine calls)
  // the next decode position: prompt + rounds since the admission - discarded positions
  int slot_pos(size_t i) const {
    const Slot& s = slots_[i];
    return (int)s.prompt.size() + rounds_done_ - s.base_round - s.shifted;
  }
  // context shift (Slot::shifted, n_shifts, n_keep)
  bool auto_shift_ = false;
  int n_keep_ = 0;
  long context_shifts_ = 0;
  void check_shift_supported(const char* fn) const;
  // the micro-batch's positions -> every stage; its penalty windows (prompt + accepted tokens of
  // every row) -> the last stage
  void push_positions(int mb);
  void push_history(int mb);
  bool row_sampling_ = false;
  bool row_masks_ = false;
  void clear_masks(bool all);               // start(): those in use; load_state(): all
  RowSampling row_default_;                 // the engine keys as a record (seed: the engine's)
  uint64_t admissions_ = 0;
  void apply_slot_sampling(const std::vector<size_t>& seqs);   // before an admission's prefill
  void push_row_draws(int mb);                                 // after it: draw0 + tokens generated
  std::vector<Item> prefill_items(const std::vector<size_t>& seqs, bool admission);
  // LoRA: the loaded adapters (serial: unique per load, so a reused id never matches an old KV tag);
  // the slots' bindings and KV tags live in their Slot
  struct AdapterRec { bool used = false; std::string path; float alpha = 0.f; int r_min = 0, r_max = 0; size_t bytes = 0; uint64_t serial = 0; };
  static constexpr uint64_t kMixedTag = ~0ull;
  int lora_cap_ = 0, lora_max_rank_ = 64;
  uint64_t lora_serial_ = 0;
  std::vector<AdapterRec> adapters_;
  KvTag bind_tag(size_t slot) const;
  // mark_mixed: a running slot whose binding changes keeps KV of two bindings (never a prefix again)
  void push_bindings(const std::vector<int>& slots, const std::vector<int>& ids, const std::vector<float>& scales,
                     bool mark_mixed);
  void clear_bindings(bool all);            // start(): those in use; load_state(): all
  double load_ms_ = 0;
  // persistent stage-worker threads of run_all (declared last: joined before anything they use
  // is destroyed)
  std::unique_ptr<ThreadPool> pool_;
};

}  // namespace mp
