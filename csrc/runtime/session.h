// Session = engine + tokenizer + the text-level generation loop shared by mi-cli and the
// orchestrator (the role llama-cli's main loop plays for the reference):
// tokenize, prefill, decode token by token, stream UTF-8-safe pieces, stop at end-of-generation
// or n_predict, cancel on request (client disconnect), and the llama.cpp-style perf summary.
#pragma once
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "grammar.h"
#include "tokenizer.h"

namespace mp {

// complete-UTF-8 emitter: push() returns the bytes up to the last whole character, keeps the rest
struct Utf8Acc {
  std::string buf;
  std::string push(const std::string& b);
};
double session_now_ms();

struct GenRequest {
  std::string prompt;
  int n_predict = 200;
  // per-request sampling (engines built with row_sampling): the slot record of this request; without
  // has_seed it gets the engine's next default seed (GenResult::seed reports the one used)
  bool has_sampling = false, has_seed = false;
  RowSampling sampling;
  // constrained output (engines built with row_masks): every token the request generates keeps its
  // text inside the grammar's language; it ends with stop "eog" as soon as nothing can follow
  std::shared_ptr<const Grammar> grammar;
  // LoRA (engines built with lora_adapters): the adapter the request's slot is bound to (-1: the base
  // model) and its user scale; bound in the same guarded call as the sampling record, kept across a failover
  int lora_id = -1;
  float lora_scale = 1.f;
  // context shift (engines built with context_shift): the prompt tokens a shift of this request keeps
  // (-1: the whole prompt); without has_keep the engine's n_keep
  bool has_keep = false;
  int n_keep = 0;
  // receives text pieces (complete UTF-8); return false to cancel this sequence
  std::function<bool(const std::string& piece)> on_piece;
};

// one generated token with its log-probability (log-softmax of the raw logits) and the engine's
// n_probs most likely alternatives at that step (engine config n_probs != 0)
struct TokenProb {
  int32_t id = -1;
  std::string piece;
  float logprob = 0;
  struct Alt { int32_t id; std::string piece; float logprob; };
  std::vector<Alt> top;
};

struct GenResult {
  int n_prompt = 0, n_gen = 0;
  double prefill_ms = 0, decode_ms = 0;
  std::string text;
  std::string stop;   // "eog" | "length" | "cancelled" | "context" (never "context" on a context_shift engine
                      // whose pool holds max_ctx per request)
  int n_shifts = 0;   // context shifts the request went through
  bool context_shift = false;   // it ran on a context_shift engine
  std::vector<int32_t> tokens;
  std::vector<TokenProb> probs;   // one per token of `tokens` when the engine records logprobs
  bool has_seed = false;          // row_sampling engines: the seed of the request's random stream
  uint64_t seed = 0;
};

class Session {
 public:
  // gguf may be empty (synthetic model: byte-level stand-in tokenizer)
  Session(Engine& eng, const std::string& gguf_path);
  ~Session();
  Engine& engine() { return *eng_; }
  int capacity() const { return eng_->n_mb() * eng_->mb_size(); }
  // Failover for serve(): called with the error of a failed engine call; returns a replacement
  // engine (e.g. re-partitioned without the failed stage's GPU, Engine::failover_config) or nullptr
  // to give up.  The running requests are then re-admitted as prompt + tokens generated so far and
  // keep streaming.  At most `max_failovers` per serve() call.
  void set_fault_handler(std::function<Engine*(const std::string& error)> h, int max_failovers = 4) {
    on_fault_ = std::move(h);
    max_failovers_ = max_failovers;
  }
  int failovers() const { return failovers_; }
  std::vector<int32_t> encode(const std::string& text) const;
  // text as a bare token stream (no BOS), and the BOS id the vocabulary puts in front (-1: none)
  std::vector<int32_t> encode_raw(const std::string& text) const;
  // text of an embedding request: encode(), plus EOS when the file sets tokenizer.ggml.add_eos_token
  std::vector<int32_t> encode_embedding(const std::string& text) const;
  int bos() const;
  std::string piece(int32_t id) const;
  bool is_eog(int32_t id) const;

  // runs up to capacity() requests together (one sequence slot each)
  std::vector<GenResult> run(std::vector<GenRequest>& reqs);

  // Continuous batching (single-process pipelines): between decode rounds, `next(free)` is asked
  // for up to `free` new requests (non-blocking), which are admitted into idle sequence slots while
  // the running ones keep decoding; `done(request, result)` fires as each request finishes (EOG,
  // n_predict, cancellation, context).  Returns when nothing runs and next() has nothing.
  // An embedding job (Served::embed set; req / done unused): its prompts are embedded between decode
  // rounds in slots no request holds, as many per round as slots and KV pages are free (it waits
  // while there are none), the running requests untouched.  done fires once, with one result per
  // prompt or with the error that ended the job.
  struct EmbedJob {
    std::vector<std::vector<int32_t>> prompts;
    int pooling = -1;        // POOL_NONE .. POOL_LAST, -1: the model's default (Engine::default_pooling)
    bool normalize = true;
    std::function<void(std::vector<Engine::EmbedResult>& out, const std::string& error)> done;
  };
  struct Served {
    GenRequest req;
    std::function<void(GenResult&)> done;
    std::shared_ptr<EmbedJob> embed;
  };
  void serve(const std::function<std::vector<Served>(int free)>& next);
  // llama.cpp-style summary lines (prompt eval / eval / total)
  static std::string perf_summary(const GenResult& r, double load_ms);

 private:
  void push_prob(GenResult& r, int slot, int32_t t) const;
  // row_sampling engines: the record of `slot` for the admission of req (the engine's values without
  // one).  A request that has already produced res.tokens (failover, resume) keeps its seed and goes on
  // at draw0 + tokens produced, so it continues its own stream.
  void set_slot_record(int slot, const GenRequest& req, const GenResult& res);
  // grammar requests: the state at the start of req's grammar (throws without a tokenizer or on an
  // engine without row_masks), and the masks of the given slots' states in one engine call (a null
  // state clears the slot's mask)
  GrammarState grammar_state(const GenRequest& req);
  // Returns one string per slot: empty, or why that state's mask could not be computed (the grammar's
  // tables are full, a state is too ambiguous); such a slot's mask is cleared and its request is the
  // caller's to end.  An engine error is thrown.
  std::vector<std::string> push_masks(const std::vector<int>& slots, const std::vector<const GrammarState*>& states,
                                      bool for_start);
  std::shared_ptr<const GrammarVocab> gvocab_;
  std::vector<std::vector<uint32_t>> mask_buf_;
  Engine* eng_;
  std::function<Engine*(const std::string&)> on_fault_;
  int max_failovers_ = 0, failovers_ = 0;
  std::unique_ptr<GgufFile> gguf_;
  std::unique_ptr<Tokenizer> tok_;
};

}  // namespace mp
