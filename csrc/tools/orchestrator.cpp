// orchestrator: the HTTP front-end (reference `orchestrator/src/main.rs`, SURVEY.md C1-C10, D5, D7,
// D12), C++ instead of Rust/axum and with the engine IN-PROCESS: the model is loaded once at
// start-up (the reference spawns a fresh llama-cli per request and reloads the GGUF every time,
// `main.rs:35-57`).
//
//   POST /chat        {"prompt": str, "n_predict"?: int} -> text/event-stream of
//                     data: {"msg_type": "log"|"token", "content": str}   (main.rs:23-27,97)
//                     keep-alive comment every 1 s (main.rs:97); generation is cancelled when the
//                     client disconnects (the reference lets the child run on, main.rs:77,91)
//   POST /completion  {"prompt", "n_predict"} -> {"content", "response", "tokens_predicted", ...}
//                     (the PDF's proxy design, p.9-10, llama-server style)
//   POST /embedding   {"content": str | [str], "pooling"?, "embd_normalize"?: 2 | -1} -> [{"index", "embedding"}]
//   POST /v1/embeddings  {"input": str | [str] | [int] | [[int]], "encoding_format"?: "float"} ->
//                     {"object": "list", "data": [{"object": "embedding", "index", "embedding"}], "model",
//                     "usage": {"prompt_tokens", "total_tokens"}}; queued like a completion and run between
//                     decode rounds in idle slots (Engine::embed: output norm + pooling, no LM head)
//   GET  /metrics     Prometheus text (requests, tokens, tok/s, p50/p90/p99 per token, stage
//                     heartbeats, link bytes)
//   GET  /health      engine health JSON
//   GET  /models      registered models ({"data": [{"id", "loaded", "source"}]}); requests pick one
//                     with "model": NAME (--model-alias NAME=PATH|synthetic:NAME, PDF p.7 item 3:
//                     multi-model management), at most --max-models engines resident (LRU)
//   GET  /*           static files (default ./static, index.html at /) (main.rs:104)
//   CORS: Access-Control-Allow-Origin * on every response, OPTIONS preflight (main.rs:105)
//   errors as axum's Json extractor: 415 (not application/json), 400 (bad JSON), 422 (no
//   "prompt" string), 405 (wrong method), 404; optional --api-key (401) and --rate-limit (429)
//
// Concurrency: connection thread per client; one generation thread batches up to
// n_mb * mb_size queued requests for the same model into one engine run (request-level batching,
// SURVEY.md D5).  A failed run whose engine reports a fault (stage exception, link abort, watchdog)
// is answered with an error and the engine is rebuilt from its config (the design report's worker
// auto-restart, PDF p.6-7 / SURVEY.md D6).
#include <arpa/inet.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <signal.h>
#include <sys/socket.h>
#include <poll.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cerrno>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "cli_common.h"
#include "engine.h"
#include "log.h"
#include "session.h"

using namespace mp;

namespace {

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ------------------------------------------------------------------ events / jobs
struct Event {
  std::string type;      // "log" | "token" | "end"
  std::string content;
};

struct Job {
  std::string prompt;
  std::string model;   // "" = the default model
  int n_predict = 200;
  // per-request sampling (--row-sampling): the record built from the request's fields
  bool has_sampling = false, has_seed = false;
  RowSampling sampling;
  std::shared_ptr<const Grammar> grammar;   // constrained output (--row-masks): grammar | json_schema | response_format
  int lora_id = -1;            // LoRA (--lora): the request's adapter (-1: the base model) and scale
  float lora_scale = 1.f;
  bool has_keep = false;       // context shift (--context-shift): the request's own n_keep (-1: its whole prompt)
  int n_keep = 0;
  double enqueued_ms = 0;   // fairness between models (serve_model)
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Event> q;
  bool done = false;
  std::atomic<bool> cancelled{false};
  GenResult result;
  // an embedding request (/embedding, /v1/embeddings): its inputs as texts or token lists, queued like
  // a completion; the vectors (or the error that ended it) when done
  bool is_embed = false;
  std::vector<std::string> embed_texts;
  std::vector<std::vector<int32_t>> embed_tokens;
  int embed_pooling = -1;
  bool embed_normalize = true;
  std::vector<Engine::EmbedResult> embed_out;
  int embed_n_tokens = 0;
  std::string embed_err;
  void push(Event e) {
    {
      std::lock_guard<std::mutex> l(mu);
      q.push_back(std::move(e));
    }
    cv.notify_all();
  }
  void finish() {
    {
      std::lock_guard<std::mutex> l(mu);
      done = true;
    }
    cv.notify_all();
  }
};

struct Metrics {
  std::mutex mu;
  uint64_t requests = 0, completed = 0, cancelled = 0, errors = 0, prompt_tokens = 0, gen_tokens = 0;
  uint64_t embed_requests = 0, embed_tokens = 0;
  uint64_t context_shifts = 0;
  double last_decode_tok_s = 0, last_prefill_tok_s = 0;
  std::vector<double> token_ms;   // recent per-token latencies
  void add_latency(double ms) {
    token_ms.push_back(ms);
    if (token_ms.size() > 4096) token_ms.erase(token_ms.begin(), token_ms.begin() + 2048);
  }
};

double pctl(std::vector<double> v, double p) {
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  return v[std::min(v.size() - 1, (size_t)(p * (v.size() - 1) + 0.5))];
}

// ------------------------------------------------------------------ server state
struct ModelSlot {
  std::string name, source;
  Json cfg;
  std::unique_ptr<Engine> eng;
  std::unique_ptr<Session> sess;
  double last_used = 0;
  int restarts = 0;
};

struct Server {
  Engine* eng = nullptr;     // the default model's engine (models[0])
  std::vector<std::unique_ptr<ModelSlot>> models;
  int max_models = 2;        // resident engines (the default one included)
  std::mutex eng_mu;         // engine swaps (restart / load) vs /health and /metrics readers
  bool ready = false;        // start-up finished (later logs are not replayed to new requests)
  bool mock = false;
  bool continuous = true;    // continuous batching (--no-continuous: one batch per engine run)
  int mock_delay_ms = 2;
  int capacity = 1;
  int default_n = 200;
  std::string static_dir = "static";
  std::string api_key;
  int rate_limit = 0;   // requests per minute per client IP (0 = off)
  std::mutex rl_mu;
  std::map<std::string, std::deque<double>> rl_hist;
  std::vector<std::string> startup_logs;
  std::mutex jobs_mu;
  std::condition_variable jobs_cv;
  std::deque<std::shared_ptr<Job>> pending;
  std::vector<std::shared_ptr<Job>> active;
  std::mutex active_mu;
  Metrics metrics;
  std::atomic<bool> stop{false};
  std::atomic<int> connections{0};
  // a request for another model that has waited this long stops admission into the model being
  // served; its live requests drain and the generation loop switches models (no starvation)
  double switch_after_ms = 2000;
  // --spawn-cli: the reference's process model (main.rs:35-57) -- every request runs a CLI child
  // (mi-cli with the model flags this server was started with); its stdout streams as "token"
  // messages, its stderr lines as "log" messages; a client disconnect kills the child
  std::string spawn_cli;
  std::vector<std::string> cli_args;
  // --lora FILE ...: the default model's adapters in id order (loaded with its engine) and the scale
  // each has by default; at most one is non-zero (one adapter per sequence)
  std::vector<std::string> lora_paths;
  std::vector<float> lora_scale;
  std::mutex lora_mu;
};

Server* g_srv = nullptr;

void broadcast_log(const std::string& line) {
  if (!g_srv) return;
  std::lock_guard<std::mutex> l(g_srv->active_mu);
  for (auto& j : g_srv->active) j->push({"log", line});
}

// mock generation (no model): echoes words for API tests (SURVEY.md T6 "mock engine")
GenResult mock_run(Job& j, int delay_ms) {
  GenResult r;
  r.n_prompt = (int)j.prompt.size();
  std::vector<std::string> words = {" once", " upon", " a", " time", " there", " was", " a", " pipeline", ".",
                                    " \xc3\xa7", "\xc4\x9f", " \xf0\x9f\x9a\x80"};
  const double t0 = now_ms();
  for (int i = 0; i < j.n_predict; ++i) {
    if (j.cancelled) { r.stop = "cancelled"; break; }
    const std::string& w = words[i % words.size()];
    r.text += w;
    r.n_gen++;
    j.push({"token", w});
    std::this_thread::sleep_for(std::chrono::milliseconds(delay_ms));
  }
  if (r.stop.empty()) r.stop = "length";
  r.decode_ms = now_ms() - t0;
  return r;
}

ModelSlot* find_model(Server& S, const std::string& name) {
  if (name.empty()) return S.models.empty() ? nullptr : S.models[0].get();
  for (auto& m : S.models)
    if (m->name == name) return m.get();
  return nullptr;
}

void load_slot(Server& S, ModelSlot& m) {
  const bool dflt = &m == S.models[0].get();
  {
    std::lock_guard<std::mutex> l(S.eng_mu);
    if (dflt) S.eng = nullptr;
    m.sess.reset();
    m.eng.reset();
  }
  std::unique_ptr<Engine> e(new Engine(m.cfg));
  if (dflt && !m.cfg.has("lora_preload"))   // (a failover's replacement takes them over through its config)
    for (size_t i = 0; i < S.lora_paths.size(); ++i)
      if (e->load_adapter(S.lora_paths[i]) != (int)i) throw std::runtime_error("--lora: adapter ids out of order");
  std::unique_ptr<Session> ss(new Session(*e, m.cfg.get_str("gguf", "")));
  std::lock_guard<std::mutex> l(S.eng_mu);
  m.eng = std::move(e);
  m.sess = std::move(ss);
  if (dflt) S.eng = m.eng.get();
}

// generation thread only: the slot of `name`, loaded (evicting the least recently used other
// model when more than max_models engines would be resident)
ModelSlot* acquire_model(Server& S, const std::string& name) {
  ModelSlot* m = find_model(S, name);
  if (!m) throw std::runtime_error("unknown model " + name);
  if (!m->eng) {
    int resident = 0;
    for (auto& x : S.models) resident += x->eng ? 1 : 0;
    while (resident >= S.max_models) {
      ModelSlot* lru = nullptr;
      for (size_t i = 1; i < S.models.size(); ++i)
        if (S.models[i]->eng && (!lru || S.models[i]->last_used < lru->last_used)) lru = S.models[i].get();
      if (!lru) break;
      MP_LOGI("orchestrator: unloading model %s", lru->name.c_str());
      std::lock_guard<std::mutex> l(S.eng_mu);
      lru->sess.reset();
      lru->eng.reset();
      --resident;
    }
    MP_LOGI("orchestrator: loading model %s (%s)", m->name.c_str(), m->source.c_str());
    load_slot(S, *m);
  }
  m->last_used = now_ms();
  return m;
}

// per-request bookkeeping once a generation ends (both scheduling modes)
void record_result(Server& S, Job& j, const GenResult& r, double load_ms) {
  j.result = r;
  const std::string perf = Session::perf_summary(r, load_ms);
  j.push({"log", perf});
  fputs(perf.c_str(), stderr);
  if (r.n_shifts > 0) j.push({"log", "context shifts: " + std::to_string(r.n_shifts) + "\n"});
  std::lock_guard<std::mutex> l(S.metrics.mu);
  S.metrics.completed++;
  S.metrics.context_shifts += (uint64_t)std::max(0, r.n_shifts);
  if (r.stop == "cancelled") S.metrics.cancelled++;
  S.metrics.prompt_tokens += r.n_prompt;
  S.metrics.gen_tokens += r.n_gen;
  if (r.decode_ms > 0 && r.n_gen > 1) {
    S.metrics.last_decode_tok_s = (r.n_gen - 1) * 1e3 / r.decode_ms;
    S.metrics.add_latency(r.decode_ms / (r.n_gen - 1));
  }
  if (r.prefill_ms > 0) S.metrics.last_prefill_tok_s = r.n_prompt * 1e3 / r.prefill_ms;
}

// the engine is poisoned (aborted links, failed stage): rebuild it; injected faults are a one-shot
// test hook and are not re-armed
void restart_if_failed(Server& S, ModelSlot* slot) {
  if (!slot || !slot->eng || slot->eng->health().get_bool("ok", true)) return;
  slot->cfg["fault"] = Json::object();
  try {
    load_slot(S, *slot);
    slot->restarts++;
    MP_LOGW("orchestrator: engine of model %s restarted after a fault (%d restarts)", slot->name.c_str(),
            slot->restarts);
  } catch (const std::exception& e2) {
    MP_LOGE("orchestrator: engine restart failed: %s", e2.what());
  }
}

// the token lists of an embedding job: given as ids, or its texts through the model's tokenizer
// (EOS appended when the file sets tokenizer.ggml.add_eos_token)
std::vector<std::vector<int32_t>> embed_prompts(const Job& j, const Session& sess) {
  std::vector<std::vector<int32_t>> p = j.embed_tokens;
  for (const std::string& t : j.embed_texts) p.push_back(sess.encode_embedding(t));
  return p;
}

void record_embedding(Server& S, Job& j, std::vector<Engine::EmbedResult>& out, const std::string& err, int n_tokens) {
  j.embed_out = std::move(out);
  j.embed_err = err;
  j.embed_n_tokens = n_tokens;
  std::lock_guard<std::mutex> l(S.metrics.mu);
  if (err.empty()) {
    S.metrics.completed++;
    S.metrics.embed_tokens += (uint64_t)n_tokens;
  } else {
    S.metrics.errors++;
  }
}

// Continuous batching (default): requests for `model` are admitted into free sequence slots between
// decode rounds while the running ones keep generating; each finishes (and frees its slot) on its own.
void serve_model(Server& S, ModelSlot* slot, const std::string& model) {
  const double turn_start = now_ms();
  auto next = [&](int free) {
    std::vector<std::shared_ptr<Job>> taken;
    {
      std::lock_guard<std::mutex> l(S.jobs_mu);
      // each model gets a turn of at least switch_after_ms before another model's waiting request
      // can end it (otherwise two busy models would hand the turn back and forth, admitting nothing)
      const double now = now_ms();
      if (now - turn_start > S.switch_after_ms)
        for (auto& pj : S.pending)
          if (pj->model != model && now - pj->enqueued_ms > S.switch_after_ms) return std::vector<Session::Served>{};
      for (auto it = S.pending.begin(); it != S.pending.end() && (int)taken.size() < free;) {
        if ((*it)->model == model) {
          taken.push_back(*it);
          it = S.pending.erase(it);
        } else {
          ++it;
        }
      }
    }
    std::vector<Session::Served> out;
    for (auto& j : taken) {
      {
        std::lock_guard<std::mutex> l(S.active_mu);
        S.active.push_back(j);
      }
      j->push({"log", "orchestrator: request accepted (continuous batching, " + std::to_string(free) + " free slots)\n"});
      for (auto& sl : S.startup_logs) j->push({"log", sl});
      Session::Served sv;
      if (j->is_embed) {
        std::shared_ptr<Job> keep = j;
        sv.embed = std::make_shared<Session::EmbedJob>();
        sv.embed->prompts = embed_prompts(*j, *slot->sess);
        sv.embed->pooling = j->embed_pooling;
        sv.embed->normalize = j->embed_normalize;
        int n_tok = 0;
        for (auto& pr : sv.embed->prompts) n_tok += (int)pr.size();
        sv.embed->done = [&S, keep, n_tok](std::vector<Engine::EmbedResult>& out, const std::string& err) {
          record_embedding(S, *keep, out, err, n_tok);
          {
            std::lock_guard<std::mutex> l(S.active_mu);
            S.active.erase(std::remove(S.active.begin(), S.active.end(), keep), S.active.end());
          }
          keep->finish();
        };
        out.push_back(std::move(sv));
        continue;
      }
      sv.req.prompt = j->prompt;
      sv.req.n_predict = j->n_predict;
      sv.req.has_sampling = j->has_sampling; sv.req.has_seed = j->has_seed; sv.req.sampling = j->sampling;
      sv.req.grammar = j->grammar;
      sv.req.lora_id = j->lora_id; sv.req.lora_scale = j->lora_scale;
      sv.req.has_keep = j->has_keep; sv.req.n_keep = j->n_keep;
      Job* jp = j.get();
      sv.req.on_piece = [jp](const std::string& p) {
        if (jp->cancelled) return false;
        jp->push({"token", p});
        return true;
      };
      std::shared_ptr<Job> keep = j;
      sv.done = [&S, slot, keep](GenResult& r) {
        record_result(S, *keep, r, slot->eng->load_ms());
        {
          std::lock_guard<std::mutex> l(S.active_mu);
          S.active.erase(std::remove(S.active.begin(), S.active.end(), keep), S.active.end());
        }
        keep->finish();
      };
      out.push_back(std::move(sv));
    }
    return out;
  };
  // failover: a stage fault mid-generation rebuilds the engine without the failed stage's GPU
  // (layers re-partitioned over the survivors) and the running requests continue on it
  slot->sess->set_fault_handler([&S, slot](const std::string& err) -> Engine* {
    if (!slot->eng) return nullptr;
    const Json cfg2 = Engine::failover_config(slot->cfg, slot->eng->health());
    MP_LOGW("orchestrator: engine of model %s faulted (%s); failing over", slot->name.c_str(), err.c_str());
    // free the faulted engine's weights and KV on the surviving GPUs BEFORE the replacement sizes
    // and allocates its own there (it carries more layers per GPU and an auto-sized KV pool)
    std::unique_ptr<Engine> old;
    bool dflt = false;
    {
      std::lock_guard<std::mutex> l(S.eng_mu);
      dflt = S.eng == slot->eng.get();
      if (dflt) S.eng = nullptr;
      old = std::move(slot->eng);
    }
    old.reset();
    std::unique_ptr<Engine> e(new Engine(cfg2));
    std::lock_guard<std::mutex> l(S.eng_mu);
    slot->eng = std::move(e);
    slot->cfg = cfg2;
    slot->restarts++;
    if (dflt) S.eng = slot->eng.get();
    return slot->eng.get();
  });
  try {
    slot->sess->serve(next);
  } catch (const std::exception& e) {
    MP_LOGE("generation failed: %s", e.what());
    std::vector<std::shared_ptr<Job>> left;
    {
      std::lock_guard<std::mutex> l(S.active_mu);
      left.swap(S.active);
    }
    {
      std::lock_guard<std::mutex> l(S.metrics.mu);
      S.metrics.errors += left.size();
    }
    for (auto& j : left) {
      j->embed_err = e.what();   // (read by an embedding request; a completion reads the log line)
      j->push({"log", std::string("error: ") + e.what() + "\n"});
      j->finish();
    }
    restart_if_failed(S, slot);
  }
}

void generation_loop(Server& S) {
  std::string last_model;
  bool have_last = false;
  while (!S.stop) {
    std::vector<std::shared_ptr<Job>> batch;
    ModelSlot* slot = nullptr;
    std::string model;
    {
      std::unique_lock<std::mutex> l(S.jobs_mu);
      S.jobs_cv.wait_for(l, std::chrono::milliseconds(200), [&] { return !S.pending.empty() || S.stop; });
      if (S.pending.empty()) continue;
      // the oldest request's model, except that the oldest request of ANOTHER model than the one
      // served last goes first once it has waited switch_after_ms (serve_model stopped for it)
      model = S.pending.front()->model;
      const double now = now_ms();
      if (have_last)
        for (auto& pj : S.pending)
          if (pj->model != last_model && now - pj->enqueued_ms > S.switch_after_ms) {
            model = pj->model;
            break;
          }
    }
    last_model = model;
    have_last = true;
    int cap = S.capacity;
    if (!S.mock) {
      try {
        slot = acquire_model(S, model);
        cap = slot->sess->capacity();
      } catch (const std::exception& e) {
        MP_LOGE("orchestrator: model %s unavailable: %s", model.c_str(), e.what());
        std::shared_ptr<Job> j;
        {
          std::lock_guard<std::mutex> l(S.jobs_mu);
          j = S.pending.front();
          S.pending.pop_front();
        }
        j->embed_err = e.what();   // (read by an embedding request; a completion reads the log line)
        j->push({"log", std::string("error: ") + e.what() + "\n"});
        j->finish();
        continue;
      }
    }
    if (!S.mock && S.continuous && slot->cfg.get_int("draft_max", 0) <= 0) {
      serve_model(S, slot, model);
      continue;
    }
    {
      // the oldest request's model; later requests for other models keep their place in the queue
      std::lock_guard<std::mutex> l(S.jobs_mu);
      for (auto it = S.pending.begin(); it != S.pending.end() && (int)batch.size() < cap;) {
        if ((*it)->model == model) {
          batch.push_back(*it);
          it = S.pending.erase(it);
        } else {
          ++it;
        }
      }
    }
    // embedding requests of the batch run first, on the idle engine (one batch per engine run: nothing
    // is generating between batches)
    for (auto it = batch.begin(); it != batch.end();) {
      if (!(*it)->is_embed) { ++it; continue; }
      Job& j = **it;
      std::vector<Engine::EmbedResult> out;
      std::string err;
      int n_tok = 0;
      try {
        if (S.mock) throw std::runtime_error("the mock engine has no embeddings");
        Engine& e = *slot->eng;
        for (int sl = 0; sl < cap; ++sl) e.release(sl);
        const auto prompts = embed_prompts(j, *slot->sess);
        for (size_t g = 0; g < prompts.size(); g += (size_t)cap) {
          const size_t take = std::min((size_t)cap, prompts.size() - g);
          std::vector<int> sl(take);
          for (size_t k = 0; k < take; ++k) sl[k] = (int)k;
          std::vector<Engine::EmbedResult> r;
          e.embed(sl, std::vector<std::vector<int32_t>>(prompts.begin() + g, prompts.begin() + g + take), j.embed_pooling,
                  j.embed_normalize, &r);
          for (auto& v : r) out.push_back(std::move(v));
        }
        for (auto& pr : prompts) n_tok += (int)pr.size();
      } catch (const std::exception& ex) {
        err = ex.what();
      }
      record_embedding(S, j, out, err, n_tok);
      j.finish();
      it = batch.erase(it);
    }
    if (batch.empty()) continue;
    {
      std::lock_guard<std::mutex> l(S.active_mu);
      S.active = batch;
    }
    for (auto& j : batch) {
      j->push({"log", "orchestrator: request accepted (" + std::to_string(batch.size()) + " in this batch)\n"});
      for (auto& s : S.startup_logs) j->push({"log", s});
    }
    try {
      std::vector<GenResult> res;
      if (S.mock) {
        for (auto& j : batch) res.push_back(mock_run(*j, S.mock_delay_ms));
      } else {
        std::vector<GenRequest> reqs(batch.size());
        for (size_t i = 0; i < batch.size(); ++i) {
          reqs[i].prompt = batch[i]->prompt;
          reqs[i].n_predict = batch[i]->n_predict;
          reqs[i].has_sampling = batch[i]->has_sampling; reqs[i].has_seed = batch[i]->has_seed;
          reqs[i].sampling = batch[i]->sampling;
          reqs[i].lora_id = batch[i]->lora_id; reqs[i].lora_scale = batch[i]->lora_scale;
          reqs[i].has_keep = batch[i]->has_keep; reqs[i].n_keep = batch[i]->n_keep;
          reqs[i].grammar = batch[i]->grammar;
          Job* jp = batch[i].get();
          reqs[i].on_piece = [jp](const std::string& p) {
            if (jp->cancelled) return false;
            jp->push({"token", p});
            return true;
          };
        }
        res = slot->sess->run(reqs);
      }
      for (size_t i = 0; i < batch.size(); ++i) record_result(S, *batch[i], res[i], slot ? slot->eng->load_ms() : 0.0);
    } catch (const std::exception& e) {
      MP_LOGE("generation failed: %s", e.what());
      {
        std::lock_guard<std::mutex> l(S.metrics.mu);
        S.metrics.errors += batch.size();
      }
      for (auto& j : batch) j->push({"log", std::string("error: ") + e.what() + "\n"});
      restart_if_failed(S, slot);
    }
    {
      std::lock_guard<std::mutex> l(S.active_mu);
      S.active.clear();
    }
    for (auto& j : batch) j->finish();
  }
}

// ------------------------------------------------------------------ HTTP
struct Request {
  std::string method, path, query, version;
  std::map<std::string, std::string> headers;   // lower-case keys
  std::string body;
  std::string peer;
  std::string header(const std::string& k) const {
    auto it = headers.find(k);
    return it == headers.end() ? "" : it->second;
  }
};

bool write_all(int fd, const std::string& s) {
  size_t off = 0;
  while (off < s.size()) {
    ssize_t w = ::send(fd, s.data() + off, s.size() - off, MSG_NOSIGNAL);
    if (w <= 0) return false;
    off += (size_t)w;
  }
  return true;
}

std::string lower(std::string s) {
  for (auto& c : s) c = (char)tolower((unsigned char)c);
  return s;
}

const char* status_text(int code) {
  switch (code) {
    case 200: return "OK";
    case 204: return "No Content";
    case 400: return "Bad Request";
    case 401: return "Unauthorized";
    case 404: return "Not Found";
    case 405: return "Method Not Allowed";
    case 413: return "Payload Too Large";
    case 415: return "Unsupported Media Type";
    case 422: return "Unprocessable Entity";
    case 429: return "Too Many Requests";
    case 500: return "Internal Server Error";
    case 503: return "Service Unavailable";
  }
  return "Unknown";
}

const char* kCors =
    "Access-Control-Allow-Origin: *\r\n"
    "Access-Control-Allow-Methods: GET, POST, OPTIONS\r\n"
    "Access-Control-Allow-Headers: *\r\n";

void respond(int fd, int code, const std::string& ctype, const std::string& body, const std::string& extra = "") {
  std::string h = "HTTP/1.1 " + std::to_string(code) + " " + status_text(code) + "\r\n";
  if (!ctype.empty()) h += "Content-Type: " + ctype + "\r\n";
  h += "Content-Length: " + std::to_string(body.size()) + "\r\n";
  h += kCors;
  h += extra;
  h += "Connection: close\r\n\r\n";
  write_all(fd, h + body);
}

void respond_text(int fd, int code, const std::string& msg) { respond(fd, code, "text/plain; charset=utf-8", msg); }

// 1 = request read, 0 = connection closed / oversized, -1 = malformed (answer 400)
int read_request(int fd, Request& r) {
  std::string buf;
  char tmp[8192];
  size_t hdr_end = std::string::npos;
  while ((hdr_end = buf.find("\r\n\r\n")) == std::string::npos) {
    ssize_t n = ::recv(fd, tmp, sizeof(tmp), 0);
    if (n <= 0) return 0;
    buf.append(tmp, (size_t)n);
    if (buf.size() > (1 << 20)) return 0;
  }
  const std::string head = buf.substr(0, hdr_end);
  r.body = buf.substr(hdr_end + 4);
  size_t eol = head.find("\r\n");
  const std::string line = head.substr(0, eol);
  size_t a = line.find(' '), b = line.rfind(' ');
  if (a == std::string::npos || b == a) return 0;
  r.method = line.substr(0, a);
  std::string target = line.substr(a + 1, b - a - 1);
  r.version = line.substr(b + 1);
  const size_t q = target.find('?');
  r.path = target.substr(0, q);
  if (q != std::string::npos) r.query = target.substr(q + 1);
  size_t pos = eol == std::string::npos ? head.size() : eol + 2;
  while (pos < head.size()) {
    size_t e = head.find("\r\n", pos);
    if (e == std::string::npos) e = head.size();
    const std::string h = head.substr(pos, e - pos);
    const size_t c = h.find(':');
    if (c != std::string::npos) {
      std::string v = h.substr(c + 1);
      while (!v.empty() && (v[0] == ' ' || v[0] == '\t')) v.erase(0, 1);
      r.headers[lower(h.substr(0, c))] = v;
    }
    pos = e + 2;
  }
  size_t cl = 0;
  const std::string clh = r.header("content-length");
  if (!clh.empty()) {
    // strict decimal: a malformed or out-of-range value is a 400, never an exception on this thread
    errno = 0;
    char* end = nullptr;
    const unsigned long long v = std::strtoull(clh.c_str(), &end, 10);
    if (clh[0] < '0' || clh[0] > '9' || errno == ERANGE || !end || *end != '\0') return -1;
    if (v > (8ull << 20)) return 0;
    cl = (size_t)v;
  }
  while (r.body.size() < cl) {
    ssize_t n = ::recv(fd, tmp, sizeof(tmp), 0);
    if (n <= 0) return 0;
    r.body.append(tmp, (size_t)n);
  }
  r.body.resize(cl);
  return 1;
}

std::string mime_of(const std::string& p) {
  auto ends = [&](const char* s) { return p.size() >= strlen(s) && p.compare(p.size() - strlen(s), strlen(s), s) == 0; };
  if (ends(".html") || ends(".htm")) return "text/html; charset=utf-8";
  if (ends(".js")) return "application/javascript";
  if (ends(".css")) return "text/css";
  if (ends(".json")) return "application/json";
  if (ends(".png")) return "image/png";
  if (ends(".svg")) return "image/svg+xml";
  if (ends(".ico")) return "image/x-icon";
  return "application/octet-stream";
}

void serve_static(Server& S, int fd, const Request& r) {
  std::string p = r.path == "/" ? "/index.html" : r.path;
  if (p.find("..") != std::string::npos) return respond_text(fd, 404, "Not Found");
  const std::string full = S.static_dir + p;
  struct stat stt;
  if (stat(full.c_str(), &stt) != 0 || !S_ISREG(stt.st_mode)) return respond_text(fd, 404, "Not Found");
  try {
    const std::string body = read_file(full);
    respond(fd, 200, mime_of(full), r.method == "HEAD" ? "" : body);
  } catch (...) {
    respond_text(fd, 404, "Not Found");
  }
}

// axum Json<ChatRequest> extractor semantics (main.rs:18-21)
bool parse_prompt_body(int fd, const Request& r, std::string* prompt, int* n_predict, int def_n,
                       std::string* model = nullptr, Json* body = nullptr) {
  if (lower(r.header("content-type")).find("application/json") == std::string::npos) {
    respond_text(fd, 415, "Expected request with `Content-Type: application/json`");
    return false;
  }
  Json j;
  try {
    j = Json::parse(r.body);
  } catch (const std::exception& e) {
    respond_text(fd, 400, std::string("Failed to parse the request body as JSON: ") + e.what());
    return false;
  }
  if (!j.is_obj() || !j.has("prompt") || !j["prompt"].is_str()) {
    respond_text(fd, 422, "Failed to deserialize the JSON body into the target type: missing field `prompt`");
    return false;
  }
  *prompt = j["prompt"].str();
  *n_predict = j.get_int("n_predict", def_n);
  if (*n_predict < 0) *n_predict = def_n;
  if (model) *model = j.get_str("model", "");
  if (body) *body = j;
  return true;
}

bool authorized(Server& S, int fd, const Request& r) {
  if (!S.api_key.empty()) {
    const std::string a = r.header("authorization"), k = r.header("x-api-key");
    if (a != "Bearer " + S.api_key && k != S.api_key) {
      respond_text(fd, 401, "Unauthorized");
      return false;
    }
  }
  if (S.rate_limit > 0) {
    std::lock_guard<std::mutex> l(S.rl_mu);
    auto& h = S.rl_hist[r.peer];
    const double t = now_ms();
    while (!h.empty() && t - h.front() > 60000) h.pop_front();
    if ((int)h.size() >= S.rate_limit) {
      respond(fd, 429, "text/plain; charset=utf-8", "Too Many Requests", "Retry-After: 60\r\n");
      return false;
    }
    h.push_back(t);
  }
  return true;
}

bool known_model(Server& S, int fd, std::string* model) {
  if (S.mock || model->empty()) return true;
  if (ModelSlot* m = find_model(S, *model)) {
    if (m == S.models[0].get()) model->clear();   // the default model under its own name
    return true;
  }
  respond(fd, 404, "application/json", "{\"error\":\"unknown model\"}");
  return false;
}

// one request = one child process (spawn-cli mode)
void spawn_job(Server& S, std::shared_ptr<Job> job) {
  std::vector<std::string> av{S.spawn_cli};
  av.insert(av.end(), S.cli_args.begin(), S.cli_args.end());
  for (const char* a : {"-p", "", "-n", "", "--no-display-prompt"}) av.push_back(a);
  av[av.size() - 4] = job->prompt;
  av[av.size() - 2] = std::to_string(job->n_predict);
  int out[2], err[2];
  if (pipe(out) != 0 || pipe(err) != 0) {
    job->push({"log", std::string("error: pipe: ") + strerror(errno) + "\n"});
    job->finish();
    return;
  }
  const double t0 = now_ms();
  const pid_t pid = fork();
  if (pid == 0) {   // child: exec before touching anything else (no GPU state in this process)
    dup2(out[1], 1);
    dup2(err[1], 2);
    close(out[0]); close(out[1]); close(err[0]); close(err[1]);
    std::vector<char*> cv;
    for (auto& a : av) cv.push_back(const_cast<char*>(a.c_str()));
    cv.push_back(nullptr);
    execv(cv[0], cv.data());
    fprintf(stderr, "exec %s: %s\n", cv[0], strerror(errno));
    _exit(127);
  }
  close(out[1]);
  close(err[1]);
  if (pid < 0) {
    close(out[0]); close(err[0]);
    job->push({"log", std::string("error: fork: ") + strerror(errno) + "\n"});
    job->finish();
    return;
  }
  Utf8Acc acc;
  std::string line, text;
  pollfd fds[2] = {{out[0], POLLIN, 0}, {err[0], POLLIN, 0}};
  int open_fds = 2;
  bool killed = false;
  char buf[4096];
  while (open_fds > 0) {
    if (job->cancelled && !killed) { kill(pid, SIGTERM); killed = true; }
    if (poll(fds, 2, 100) < 0 && errno != EINTR) break;
    for (int k = 0; k < 2; ++k) {
      if (fds[k].fd < 0 || !(fds[k].revents & (POLLIN | POLLHUP | POLLERR))) continue;
      const ssize_t n = read(fds[k].fd, buf, sizeof(buf));
      if (n <= 0) { close(fds[k].fd); fds[k].fd = -1; --open_fds; continue; }
      if (k == 0) {   // token stream (UTF-8 safe pieces, like the reference's stdout pump)
        const std::string p = acc.push(std::string(buf, (size_t)n));
        if (!p.empty()) { text += p; job->push({"token", p}); }
      } else {        // log lines (stderr), line by line
        line.append(buf, (size_t)n);
        size_t nl;
        while ((nl = line.find('\n')) != std::string::npos) {
          job->push({"log", line.substr(0, nl + 1)});
          line.erase(0, nl + 1);
        }
      }
    }
  }
  if (!acc.buf.empty()) { text += acc.buf; job->push({"token", acc.buf}); }
  if (!line.empty()) job->push({"log", line + "\n"});
  int status = 0;
  waitpid(pid, &status, 0);
  GenResult r;
  r.text = text;
  r.stop = killed ? "cancelled" : (WIFEXITED(status) && WEXITSTATUS(status) == 0 ? "length" : "error");
  r.decode_ms = now_ms() - t0;
  job->result = r;
  {
    std::lock_guard<std::mutex> l(S.metrics.mu);
    if (r.stop == "length") S.metrics.completed++;
    else if (killed) S.metrics.cancelled++;
    else S.metrics.errors++;
  }
  job->finish();
}

// The sampling fields every llama.cpp-server client sends: temperature, top_k, top_p, min_p, seed,
// repeat_penalty, frequency_penalty, presence_penalty, logit_bias ([[id, bias | false], ..] or {"id": bias})
// -> the request's slot record (Engine::sampling_from_json).  They need a server started with
// --row-sampling; repeat_last_n is the server's (a request may only repeat it).  false: a 400 was sent.
struct ReqSampling {
  bool has = false, has_seed = false;
  RowSampling rec;
  std::shared_ptr<const Grammar> grammar;
  int lora_id = -1;
  float lora_scale = 1.f;
  bool has_keep = false;
  int n_keep = 0;
};

// "n_keep": the prompt tokens a context shift of this request keeps (-1: the whole prompt); the field
// is accepted on every server and used by one started with --context-shift
bool parse_keep(int fd, const Json& body, ReqSampling* out) {
  if (!body.has("n_keep") || body["n_keep"].is_null()) return true;
  const Json& v = body["n_keep"];
  if (!v.is_num() || v.num() != std::floor(v.num()) || v.num() < -1 || v.num() > 1e9) {
    respond_text(fd, 400, "n_keep must be an integer >= 0, or -1 for the whole prompt");
    return false;
  }
  out->has_keep = true;
  out->n_keep = (int)v.num();
  return true;
}

// [{"id", "scale"}, ..] -> the one adapter with a non-zero scale (-1: none).  Throws naming the cause.
void parse_lora_list(const Json& a, size_t n_adapters, int* id, float* scale) {
  if (!a.is_arr()) throw std::runtime_error("lora: expected a list of {\"id\", \"scale\"} objects");
  *id = -1;
  *scale = 0.f;
  for (const Json& e : a.arr()) {
    if (!e.is_obj() || !e.has("id") || !e["id"].is_num()) throw std::runtime_error("lora: every entry needs a numeric \"id\"");
    const double idv = e["id"].num();
    if (idv < 0 || idv >= (double)n_adapters || idv != (double)(int)idv)
      throw std::runtime_error("lora: unknown adapter id " + e["id"].dump() + " (" + std::to_string(n_adapters) + " loaded)");
    if (e.has("scale") && !e["scale"].is_num()) throw std::runtime_error("lora: \"scale\" must be a number");
    const double sc = e.has("scale") ? e["scale"].num() : 1.0;
    if (!(sc - sc == 0.0)) throw std::runtime_error("lora: \"scale\" must be finite");
    if (sc == 0.0) continue;
    if (*id >= 0) throw std::runtime_error("lora: more than one adapter with a non-zero scale (one adapter per sequence)");
    *id = (int)idv;
    *scale = (float)sc;
  }
}

// The request's adapter: its "lora" field, else the server's default.  false: a 400 was sent.
bool parse_lora(Server& S, int fd, const Json& body, const std::string& model, ReqSampling* out) {
  const bool has = body.has("lora") && !body["lora"].is_null();
  ModelSlot* dm = S.models.empty() ? nullptr : S.models[0].get();
  const bool dflt_model = model.empty() || (dm && model == dm->name);
  if (has && (S.lora_paths.empty() || !S.spawn_cli.empty() || S.mock)) {
    respond_text(fd, 400, "lora: this server was started without --lora");
    return false;
  }
  if (has && !dflt_model) {
    respond_text(fd, 400, "lora: the adapters belong to the default model");
    return false;
  }
  if (!dflt_model || S.lora_paths.empty()) return true;
  if (!has) {
    std::lock_guard<std::mutex> l(S.lora_mu);
    for (size_t i = 0; i < S.lora_scale.size(); ++i)
      if (S.lora_scale[i] != 0.f) { out->lora_id = (int)i; out->lora_scale = S.lora_scale[i]; }
    return true;
  }
  try {
    parse_lora_list(body["lora"], S.lora_paths.size(), &out->lora_id, &out->lora_scale);
  } catch (const std::exception& ex) {
    respond_text(fd, 400, ex.what());
    return false;
  }
  return true;
}
bool parse_sampling(Server& S, int fd, const Json& body, const std::string& model, ReqSampling* out) {
  static const char* const kFields[][2] = {{"temperature", "temp"}, {"top_k", "top_k"}, {"top_p", "top_p"},
                                           {"min_p", "min_p"}, {"seed", "seed"}, {"repeat_penalty", "repeat"},
                                           {"frequency_penalty", "freq"}, {"presence_penalty", "presence"},
                                           {"logit_bias", "logit_bias"}};
  Json j = Json::object();
  bool any = body.has("repeat_last_n");
  for (auto& f : kFields)
    if (body.has(f[0]) && !body[f[0]].is_null()) {
      any = true;
      // llama.cpp clients send seed -1 (or 2^32 - 1) for "pick one": the same as no seed
      if (std::string(f[0]) == "seed" && body[f[0]].is_num() && (body[f[0]].num() < 0 || body[f[0]].num() == 4294967295.0))
        continue;
      j[f[1]] = body[f[0]];
    }
  if (!any) return true;
  if (!S.spawn_cli.empty()) {
    respond_text(fd, 400, "per-request sampling fields are not supported in --spawn-cli mode");
    return false;
  }
  std::lock_guard<std::mutex> l(S.eng_mu);
  Engine* e = S.eng;
  if (!model.empty())
    if (ModelSlot* m = find_model(S, model)) e = m->eng.get();
  if (!e || !e->row_sampling()) {
    respond_text(fd, 400, "per-request sampling fields (temperature, top_k, top_p, min_p, seed, repeat_penalty, "
                          "frequency_penalty, presence_penalty, logit_bias) need a server started with --row-sampling");
    return false;
  }
  if (body.has("repeat_last_n")) {
    const int have = e->config().get_int("repeat_last_n", 64);
    if (!body["repeat_last_n"].is_num() || body["repeat_last_n"].num() != (double)have) {
      respond_text(fd, 400, "repeat_last_n is the server's (" + std::to_string(have) + "), not a per-request value");
      return false;
    }
  }
  try {
    out->rec = e->sampling_from_json(j, &out->has_seed);
    out->has = true;
  } catch (const std::exception& ex) {
    respond_text(fd, 400, ex.what());
    return false;
  }
  return true;
}

// Constrained output: "grammar" (GBNF text), "json_schema" (a schema object) or "response_format"
// ({"type": "json_object"}, or {"type": "json_schema", "json_schema": {"schema": ..}} / {.., "schema": ..}),
// at most one of them.  They need a server started with --row-masks.  Parsed grammars are kept by
// their text.  false: a 400 was sent.
bool parse_grammar(Server& S, int fd, const Json& body, const std::string& model, ReqSampling* out) {
  int n = 0;
  for (const char* k : {"grammar", "json_schema", "response_format"}) n += body.has(k) && !body[k].is_null() ? 1 : 0;
  if (!n) return true;
  if (n > 1) {
    respond_text(fd, 400, "send one of grammar, json_schema and response_format, not several");
    return false;
  }
  if (!S.spawn_cli.empty()) {
    respond_text(fd, 400, "grammar, json_schema and response_format are not supported in --spawn-cli mode");
    return false;
  }
  {
    std::lock_guard<std::mutex> l(S.eng_mu);
    Engine* e = S.eng;
    if (!model.empty())
      if (ModelSlot* m = find_model(S, model)) e = m->eng.get();
    if (!e || !e->row_masks()) {
      respond_text(fd, 400, "grammar, json_schema and response_format need a server started with --row-masks");
      return false;
    }
  }
  try {
    std::string text;
    if (body.has("grammar") && !body["grammar"].is_null()) {
      if (!body["grammar"].is_str()) throw std::runtime_error("grammar is a string of GBNF text");
      text = body["grammar"].str();
      if (text.empty()) throw std::runtime_error("grammar is empty");
    } else if (body.has("json_schema") && !body["json_schema"].is_null()) {
      text = json_schema_to_gbnf(body["json_schema"]);
    } else {
      const Json& rf = body["response_format"];
      const std::string type = rf.is_obj() ? rf.get_str("type", "") : "";
      if (type == "json_object") {
        Json any = Json::object();
        any["type"] = "json_object";
        text = json_schema_to_gbnf(rf.has("schema") ? rf["schema"] : any);
      } else if (type == "json_schema") {
        if (rf.has("json_schema") && rf["json_schema"].is_obj() && rf["json_schema"].has("schema")) text = json_schema_to_gbnf(rf["json_schema"]["schema"]);
        else if (rf.has("schema")) text = json_schema_to_gbnf(rf["schema"]);
        else throw std::runtime_error("response_format of type json_schema carries no schema");
      } else {
        throw std::runtime_error("response_format.type must be json_object or json_schema");
      }
    }
    static std::mutex mu;
    static std::map<std::string, std::shared_ptr<const Grammar>> cache;
    std::lock_guard<std::mutex> l(mu);
    auto it = cache.find(text);
    if (it != cache.end() && it->second->table_full()) {   // its state tables only grow: start over
      cache.erase(it);
      it = cache.end();
    }
    if (it == cache.end()) {
      if (cache.size() >= 64) cache.clear();
      it = cache.emplace(text, Grammar::parse(text)).first;
    }
    out->grammar = it->second;
  } catch (const std::exception& ex) {
    respond_text(fd, 400, ex.what());
    return false;
  }
  return true;
}

std::shared_ptr<Job> submit(Server& S, const std::string& prompt, int n, const std::string& model = "",
                            const ReqSampling* rs = nullptr) {
  auto job = std::make_shared<Job>();
  if (rs) job->grammar = rs->grammar;
  if (rs) { job->lora_id = rs->lora_id; job->lora_scale = rs->lora_scale; }
  if (rs) { job->has_keep = rs->has_keep; job->n_keep = rs->n_keep; }
  if (rs && rs->has) { job->has_sampling = true; job->has_seed = rs->has_seed; job->sampling = rs->rec; }
  job->prompt = prompt;
  job->n_predict = n;
  job->model = model;
  {
    std::lock_guard<std::mutex> l(S.metrics.mu);
    S.metrics.requests++;
  }
  printf("request: %s\n", prompt.c_str());   // reference main.rs:32 request log
  fflush(stdout);
  if (!S.spawn_cli.empty()) {   // a child process per request, no engine in this process
    std::thread(spawn_job, std::ref(S), job).detach();
    return job;
  }
  {
    std::lock_guard<std::mutex> l(S.jobs_mu);
    job->enqueued_ms = now_ms();
    S.pending.push_back(job);
  }
  S.jobs_cv.notify_all();
  return job;
}

std::string sse_event(const Event& e) {
  Json m = Json::object();
  m["msg_type"] = e.type;
  m["content"] = e.content;
  return "data: " + m.dump() + "\n\n";
}

std::string chunk(const std::string& s) {
  char h[32];
  snprintf(h, sizeof(h), "%zx\r\n", s.size());
  return std::string(h) + s + "\r\n";
}

void handle_chat(Server& S, int fd, const Request& r) {
  std::string prompt;
  int n = S.default_n;
  std::string model;
  Json body;
  if (!parse_prompt_body(fd, r, &prompt, &n, S.default_n, &model, &body) || !known_model(S, fd, &model)) return;
  ReqSampling rs;
  if (!parse_sampling(S, fd, body, model, &rs) || !parse_grammar(S, fd, body, model, &rs) || !parse_lora(S, fd, body, model, &rs) ||
      !parse_keep(fd, body, &rs))
    return;
  auto job = submit(S, prompt, n, model, &rs);
  std::string h = "HTTP/1.1 200 OK\r\nContent-Type: text/event-stream\r\nCache-Control: no-cache\r\n";
  h += kCors;
  h += "Transfer-Encoding: chunked\r\nConnection: close\r\n\r\n";
  if (!write_all(fd, h)) { job->cancelled = true; return; }
  double last = now_ms();
  for (;;) {
    std::vector<Event> evs;
    bool done;
    {
      std::unique_lock<std::mutex> l(job->mu);
      job->cv.wait_for(l, std::chrono::milliseconds(100), [&] { return !job->q.empty() || job->done; });
      while (!job->q.empty()) {
        evs.push_back(std::move(job->q.front()));
        job->q.pop_front();
      }
      done = job->done;
    }
    std::string out;
    for (auto& e : evs) out += sse_event(e);
    if (out.empty() && now_ms() - last >= 1000.0) out = ":\n\n";   // keep-alive (main.rs:97)
    if (!out.empty()) {
      if (!write_all(fd, chunk(out))) {   // client went away: stop generating for it
        job->cancelled = true;
        return;
      }
      last = now_ms();
    }
    if (done && evs.empty()) break;
  }
  write_all(fd, "0\r\n\r\n");
}

void handle_completion(Server& S, int fd, const Request& r) {
  std::string prompt;
  int n = 128;   // PDF p.10: n_predict 128
  std::string model;
  Json body;
  if (!parse_prompt_body(fd, r, &prompt, &n, 128, &model, &body) || !known_model(S, fd, &model)) return;
  // "n_probs": k alternatives per generated token, at most what the engine records (--n-probs)
  const int n_probs = body.get_int("n_probs", 0);
  int have = 0;
  {
    std::lock_guard<std::mutex> l(S.eng_mu);
    if (S.eng) have = std::max(0, S.eng->n_probs());
  }
  if (n_probs < 0) {
    respond_text(fd, 400, "n_probs must not be negative");
    return;
  }
  if (n_probs > have) {
    respond_text(fd, 400, "n_probs " + std::to_string(n_probs) + " exceeds what this server records (--n-probs " +
                              std::to_string(have) + ")");
    return;
  }
  ReqSampling rs;
  if (!parse_sampling(S, fd, body, model, &rs) || !parse_grammar(S, fd, body, model, &rs) || !parse_lora(S, fd, body, model, &rs) ||
      !parse_keep(fd, body, &rs))
    return;
  auto job = submit(S, prompt, n, model, &rs);
  {
    std::unique_lock<std::mutex> l(job->mu);
    job->cv.wait(l, [&] { return job->done; });
  }
  const GenResult& g = job->result;
  Json o = Json::object();
  o["content"] = g.text;
  o["response"] = g.text;
  o["tokens_predicted"] = g.n_gen;
  if (g.has_seed) {   // --row-sampling: the seed of this request's stream (a string above 2^53, which a number cannot hold)
    if (g.seed <= (1ULL << 53)) o["seed"] = (double)g.seed;
    else o["seed"] = std::to_string(g.seed);
  }
  if (n_probs > 0) {   // llama.cpp's field: one entry per generated token, n_probs alternatives each
    Json cp = Json::array();
    for (const TokenProb& tp : g.probs) {
      Json e = Json::object();
      e["id"] = (int)tp.id; e["token"] = tp.piece; e["logprob"] = (double)tp.logprob;
      Json top = Json::array();
      for (size_t k = 0; k < tp.top.size() && (int)k < n_probs; ++k) {
        Json a = Json::object();
        a["id"] = (int)tp.top[k].id; a["token"] = tp.top[k].piece; a["logprob"] = (double)tp.top[k].logprob;
        top.push(a);
      }
      e["top_logprobs"] = top;
      cp.push(e);
    }
    o["completion_probabilities"] = cp;
  }
  o["tokens_evaluated"] = g.n_prompt;
  o["stop_reason"] = g.stop;
  if (g.context_shift) o["context_shifts"] = g.n_shifts;   // --context-shift servers only: every other reply keeps its fields
  Json t = Json::object();
  t["prompt_ms"] = g.prefill_ms;
  t["predicted_ms"] = g.decode_ms;
  t["predicted_per_second"] = g.n_gen > 1 && g.decode_ms > 0 ? (g.n_gen - 1) * 1e3 / g.decode_ms : 0.0;
  o["timings"] = t;
  respond(fd, 200, "application/json", o.dump());
}

// POST /embedding (llama.cpp server: {"content": str | [str]} -> [{"index", "embedding"}]) and
// POST /v1/embeddings (OpenAI: {"input": str | [str] | [int] | [[int]], "encoding_format": "float"} ->
// {"object": "list", "data": [{"object": "embedding", "index", "embedding"}], "model", "usage"}).
// Both take "pooling" (none | mean | cls | last; default: the model's pooling_type, else last) and
// "embd_normalize" (2: unit L2 length, the default; -1: as computed).  The request waits in the same
// queue as completions and runs between decode rounds (Session::serve).
void handle_embedding(Server& S, int fd, const Request& r, bool openai) {
  if (lower(r.header("content-type")).find("application/json") == std::string::npos)
    return respond_text(fd, 415, "Expected request with `Content-Type: application/json`");
  Json body;
  try {
    body = Json::parse(r.body);
  } catch (const std::exception& e) {
    return respond_text(fd, 400, std::string("Failed to parse the request body as JSON: ") + e.what());
  }
  const char* key = openai ? "input" : (body.is_obj() && body.has("content") ? "content" : "input");
  if (!body.is_obj() || !body.has(key))
    return respond_text(fd, 422, std::string("Failed to deserialize the JSON body into the target type: missing field `") +
                                     (openai ? "input" : "content") + "`");
  if (S.mock || !S.spawn_cli.empty()) return respond_text(fd, 501, "embeddings need a model in this process (not --mock / --spawn-cli)");
  auto job = std::make_shared<Job>();
  job->is_embed = true;
  // str | [str] | [int] | [[int]]
  const Json& in = body[key];
  auto ints = [](const Json& a, std::vector<int32_t>* t) {
    for (const Json& x : a.arr()) {
      if (!x.is_num() || x.num() != (double)(int32_t)x.num()) return false;
      t->push_back((int32_t)x.num());
    }
    return true;
  };
  bool ok = true;
  if (in.is_str()) job->embed_texts.push_back(in.str());
  else if (in.is_arr() && !in.arr().empty() && in.arr()[0].is_num()) {
    job->embed_tokens.emplace_back();
    ok = ints(in, &job->embed_tokens.back());
  } else if (in.is_arr() && !in.arr().empty()) {
    for (const Json& e : in.arr()) {
      if (e.is_str() && job->embed_tokens.empty()) job->embed_texts.push_back(e.str());
      else if (e.is_arr() && !e.arr().empty() && job->embed_texts.empty()) {
        job->embed_tokens.emplace_back();
        ok = ok && ints(e, &job->embed_tokens.back());
      } else ok = false;
    }
  } else ok = false;
  for (const std::string& t : job->embed_texts) ok = ok && !t.empty();
  if (!ok)
    return respond_text(fd, 400, std::string("`") + key + "` must be a non-empty string, a list of them, a list of token ids or a "
                                     "list of such lists");
  if (body.has("embd_normalize") && !body["embd_normalize"].is_null()) {
    const Json& n = body["embd_normalize"];
    if (!n.is_num() || (n.num() != 2 && n.num() != -1))
      return respond_text(fd, 422, "embd_normalize must be 2 (unit L2 length) or -1 (none)");
    job->embed_normalize = n.num() == 2;
  }
  if (body.has("pooling") && !body["pooling"].is_null()) {
    try {
      if (!body["pooling"].is_str()) throw std::runtime_error("pooling must be a string (none, mean, cls, last)");
      job->embed_pooling = Engine::pooling_from_name(body["pooling"].str());
    } catch (const std::exception& e) {
      return respond_text(fd, 400, e.what());
    }
    if (job->embed_pooling == POOL_RANK) return respond_text(fd, 400, "pooling \"rank\" (reranking) is not supported");
  }
  if (openai && job->embed_pooling == POOL_NONE)
    return respond_text(fd, 400, "pooling \"none\" is not supported on /v1/embeddings (one vector per input); use /embedding");
  if (openai && body.has("encoding_format") && !body["encoding_format"].is_null() &&
      (!body["encoding_format"].is_str() || body["encoding_format"].str() != "float"))
    return respond_text(fd, 400, "encoding_format must be \"float\" (base64 is not supported)");
  std::string model = body.get_str("model", "");
  const std::string model_name = model;
  if (!known_model(S, fd, &model)) return;
  job->model = model;
  {
    std::lock_guard<std::mutex> l(S.metrics.mu);
    S.metrics.requests++;
    S.metrics.embed_requests++;
  }
  {
    std::lock_guard<std::mutex> l(S.jobs_mu);
    job->enqueued_ms = now_ms();
    S.pending.push_back(job);
  }
  S.jobs_cv.notify_all();
  {
    std::unique_lock<std::mutex> l(job->mu);
    job->cv.wait(l, [&] { return job->done; });
  }
  if (!job->embed_err.empty()) return respond_text(fd, 400, job->embed_err);
  size_t d = 0;
  for (auto& e : job->embed_out) d = e.n_rows > 0 ? e.v.size() / (size_t)e.n_rows : d;
  Json data = Json::array();
  for (size_t i = 0; i < job->embed_out.size(); ++i) {
    const Engine::EmbedResult& e = job->embed_out[i];
    auto row = [&](int t) {
      Json v = Json::array();
      for (size_t c = 0; c < d; ++c) v.push(Json((double)e.v[(size_t)t * d + c]));
      return v;
    };
    Json o = Json::object();
    if (openai) o["object"] = "embedding";
    o["index"] = (int)i;
    if (job->embed_pooling == POOL_NONE) {
      Json rows = Json::array();
      for (int t = 0; t < e.n_rows; ++t) rows.push(row(t));
      o["embedding"] = rows;
    } else {
      o["embedding"] = row(0);
    }
    data.push(o);
  }
  if (!openai) return respond(fd, 200, "application/json", data.dump());
  Json o = Json::object();
  o["object"] = "list";
  o["data"] = data;
  o["model"] = model_name.empty() && !S.models.empty() ? S.models[0]->name : model_name;
  Json u = Json::object();
  u["prompt_tokens"] = job->embed_n_tokens;
  u["total_tokens"] = job->embed_n_tokens;
  o["usage"] = u;
  respond(fd, 200, "application/json", o.dump());
}

void handle_metrics(Server& S, int fd) {
  std::string m;
  char b[512];
  {
    std::lock_guard<std::mutex> l(S.metrics.mu);
    auto& M = S.metrics;
    snprintf(b, sizeof(b),
             "# TYPE mipipe_requests_total counter\nmipipe_requests_total %llu\n"
             "# TYPE mipipe_requests_completed_total counter\nmipipe_requests_completed_total %llu\n"
             "# TYPE mipipe_requests_cancelled_total counter\nmipipe_requests_cancelled_total %llu\n"
             "# TYPE mipipe_request_errors_total counter\nmipipe_request_errors_total %llu\n"
             "# TYPE mipipe_prompt_tokens_total counter\nmipipe_prompt_tokens_total %llu\n"
             "# TYPE mipipe_generated_tokens_total counter\nmipipe_generated_tokens_total %llu\n",
             (unsigned long long)M.requests, (unsigned long long)M.completed, (unsigned long long)M.cancelled,
             (unsigned long long)M.errors, (unsigned long long)M.prompt_tokens, (unsigned long long)M.gen_tokens);
    m += b;
    snprintf(b, sizeof(b),
             "# TYPE mipipe_embedding_requests_total counter\nmipipe_embedding_requests_total %llu\n"
             "# TYPE mipipe_embedding_tokens_total counter\nmipipe_embedding_tokens_total %llu\n",
             (unsigned long long)M.embed_requests, (unsigned long long)M.embed_tokens);
    m += b;
    snprintf(b, sizeof(b), "# TYPE mipipe_context_shifts_total counter\nmipipe_context_shifts_total %llu\n",
             (unsigned long long)M.context_shifts);
    m += b;
    snprintf(b, sizeof(b),
             "# TYPE mipipe_decode_tokens_per_second gauge\nmipipe_decode_tokens_per_second %.3f\n"
             "# TYPE mipipe_prefill_tokens_per_second gauge\nmipipe_prefill_tokens_per_second %.3f\n"
             "# TYPE mipipe_token_latency_ms summary\n"
             "mipipe_token_latency_ms{quantile=\"0.5\"} %.4f\nmipipe_token_latency_ms{quantile=\"0.9\"} %.4f\n"
             "mipipe_token_latency_ms{quantile=\"0.99\"} %.4f\n",
             M.last_decode_tok_s, M.last_prefill_tok_s, pctl(M.token_ms, 0.5), pctl(M.token_ms, 0.9),
             pctl(M.token_ms, 0.99));
    m += b;
  }
  {
    std::lock_guard<std::mutex> l(S.jobs_mu);
    snprintf(b, sizeof(b), "# TYPE mipipe_queue_depth gauge\nmipipe_queue_depth %zu\n", S.pending.size());
    m += b;
  }
  snprintf(b, sizeof(b), "# TYPE mipipe_open_connections gauge\nmipipe_open_connections %d\n", S.connections.load());
  m += b;
  std::unique_lock<std::mutex> el(S.eng_mu);
  if (S.eng) {
    Json h = S.eng->health();
    el.unlock();
    m += "# TYPE mipipe_stage_items_done counter\n";
    for (auto& st : h["stages"].arr()) {
      snprintf(b, sizeof(b), "mipipe_stage_items_done{stage=\"%d\"} %lld\n", (int)st["stage"].num(),
               (long long)st.get_num("items_done", 0));
      m += b;
    }
    m += "# TYPE mipipe_link_bytes_sent counter\n";
    for (auto& st : h["stages"].arr())
      if (st.has("bytes_sent")) {
        snprintf(b, sizeof(b), "mipipe_link_bytes_sent{stage=\"%d\",link=\"%s\"} %lld\n", (int)st["stage"].num(),
                 st.get_str("link", "").c_str(), (long long)st.get_num("bytes_sent", 0));
        m += b;
      }
    snprintf(b, sizeof(b), "# TYPE mipipe_engine_ok gauge\nmipipe_engine_ok %d\n", h.get_bool("ok", false) ? 1 : 0);
    m += b;
  }
  respond(fd, 200, "text/plain; version=0.0.4", m);
}

// GET /lora-adapters: [{"id", "path", "scale"}], scale = the default every request without a "lora" field gets
void handle_lora_get(Server& S, int fd) {
  Json arr = Json::array();
  std::lock_guard<std::mutex> l(S.lora_mu);
  for (size_t i = 0; i < S.lora_paths.size(); ++i) {
    Json o = Json::object();
    o["id"] = (int)i; o["path"] = S.lora_paths[i]; o["scale"] = (double)S.lora_scale[i];
    arr.push(o);
  }
  respond(fd, 200, "application/json", arr.dump());
}

// POST /lora-adapters [{"id", "scale"}]: the new defaults (adapters not listed go to 0)
void handle_lora_post(Server& S, int fd, const Request& r) {
  if (S.lora_paths.empty()) return respond_text(fd, 400, "lora: this server was started without --lora");
  int id = -1;
  float scale = 0.f;
  try {
    parse_lora_list(Json::parse(r.body), S.lora_paths.size(), &id, &scale);
  } catch (const std::exception& e) {
    return respond_text(fd, 400, e.what());
  }
  {
    std::lock_guard<std::mutex> l(S.lora_mu);
    std::fill(S.lora_scale.begin(), S.lora_scale.end(), 0.f);
    if (id >= 0) S.lora_scale[id] = scale;
  }
  handle_lora_get(S, fd);
}

void handle_conn(Server& S, int fd, std::string peer) {
  S.connections++;
  Request r;
  r.peer = peer;
  const int rr = read_request(fd, r);
  if (rr < 0) respond_text(fd, 400, "Bad Request: invalid Content-Length");
  if (rr > 0) {
    try {
      if (r.method == "OPTIONS") {
        respond(fd, 204, "", "");
      } else if (r.path == "/chat") {
        if (r.method != "POST") respond(fd, 405, "text/plain; charset=utf-8", "Method Not Allowed", "Allow: POST\r\n");
        else if (authorized(S, fd, r)) handle_chat(S, fd, r);
      } else if (r.path == "/completion") {
        if (r.method != "POST") respond(fd, 405, "text/plain; charset=utf-8", "Method Not Allowed", "Allow: POST\r\n");
        else if (authorized(S, fd, r)) handle_completion(S, fd, r);
      } else if (r.path == "/embedding" || r.path == "/embeddings" || r.path == "/v1/embeddings") {
        if (r.method != "POST") respond(fd, 405, "text/plain; charset=utf-8", "Method Not Allowed", "Allow: POST\r\n");
        else if (authorized(S, fd, r)) handle_embedding(S, fd, r, r.path == "/v1/embeddings");
      } else if (r.path == "/lora-adapters") {
        if (r.method == "GET") handle_lora_get(S, fd);
        else if (r.method != "POST") respond(fd, 405, "text/plain; charset=utf-8", "Method Not Allowed", "Allow: GET, POST\r\n");
        else if (authorized(S, fd, r)) handle_lora_post(S, fd, r);
      } else if (r.path == "/metrics" && r.method == "GET") {
        handle_metrics(S, fd);
      } else if (r.path == "/health" && r.method == "GET") {
        Json h;
        {
          std::lock_guard<std::mutex> l(S.eng_mu);
          h = S.eng ? S.eng->health() : Json::object();
          if (!S.eng) h["ok"] = S.mock || !S.spawn_cli.empty();
          if (!S.spawn_cli.empty()) h["spawn_cli"] = S.spawn_cli;
          int restarts = 0;
          for (auto& mm : S.models) restarts += mm->restarts;
          h["engine_restarts"] = restarts;
        }
        h["mock"] = S.mock;
        respond(fd, 200, "application/json", h.dump());
      } else if (r.path == "/models" && r.method == "GET") {
        Json arr = Json::array();
        {
          std::lock_guard<std::mutex> l(S.eng_mu);
          for (auto& mm : S.models) {
            Json e = Json::object();
            e["id"] = mm->name;
            e["source"] = mm->source;
            e["loaded"] = (bool)mm->eng;
            e["restarts"] = mm->restarts;
            arr.push(e);
          }
        }
        Json o = Json::object();
        o["object"] = "list";
        o["data"] = arr;
        respond(fd, 200, "application/json", o.dump());
      } else if (r.method == "GET" || r.method == "HEAD") {
        serve_static(S, fd, r);
      } else {
        respond_text(fd, 405, "Method Not Allowed");
      }
    } catch (const std::exception& e) {
      respond_text(fd, 500, e.what());
    }
  }
  ::shutdown(fd, SHUT_RDWR);
  ::close(fd);
  S.connections--;
}

void usage() {
  fprintf(stderr, "usage: orchestrator (-m MODEL.gguf | --synthetic NAME | --mock) [--port 3005] [--host 0.0.0.0]\n"
                  "                    [--static DIR] [--api-key KEY] [--rate-limit N/min] [engine flags]\n"
                  "                    [--alias NAME] [--model-alias NAME=PATH.gguf|synthetic:NAME ...] [--max-models N]\n"
                  "                    [--spawn-cli mi-cli|PATH]  (a CLI child process per request, as the reference)\n");
  print_common_usage(stderr);
}

}  // namespace

int main(int argc, char** argv) {
  signal(SIGPIPE, SIG_IGN);
  Server S;
  g_srv = &S;
  int port = 3005;   // main.rs:107
  std::string host = "0.0.0.0";
  bool mock = false;
  std::string alias, synthetic_name = "model";
  std::vector<std::string> aliases;
  for (int i = 1; i + 1 < argc; ++i)
    if (!strcmp(argv[i], "--synthetic")) synthetic_name = argv[i + 1];
  CliOptions o;
  std::vector<char*> args(argv, argv + argc);
  for (int i = 1; i < argc; ++i)
    if (!strcmp(argv[i], "--mock")) mock = true;
  try {
    auto extra = [&](const std::string& a, const std::function<std::string()>& val) {
      if (a == "--port") port = std::atoi(val().c_str());
      else if (a == "--host") host = val();
      else if (a == "--static") S.static_dir = val();
      else if (a == "--api-key") S.api_key = val();
      else if (a == "--rate-limit") S.rate_limit = std::atoi(val().c_str());
      else if (a == "--mock") {}
      else if (a == "--mock-delay-ms") S.mock_delay_ms = std::atoi(val().c_str());
      else if (a == "--alias") alias = val();
      else if (a == "--model-alias") aliases.push_back(val());
      else if (a == "--max-models") S.max_models = std::max(1, std::atoi(val().c_str()));
      else if (a == "--no-continuous") S.continuous = false;
      else if (a == "--model-switch-ms") S.switch_after_ms = std::atof(val().c_str());
      else if (a == "--spawn-cli") S.spawn_cli = val();
      else if (a == "-h" || a == "--help") { usage(); exit(0); }
      else return false;
      return true;
    };
    if (mock) {
      // model flags optional in mock mode
      std::vector<char*> a2{argv[0], (char*)"--synthetic", (char*)"stories15m"};
      for (int i = 1; i < argc; ++i) a2.push_back(argv[i]);
      o = parse_cli((int)a2.size(), a2.data(), extra);
    } else {
      o = parse_cli(argc, argv, extra);
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "orchestrator: %s\n", e.what());
    usage();
    return 2;
  }
  S.mock = mock;
  S.default_n = o.n_predict;
  // --lora FILE ...: one adapter alone is every request's default (at its scale) unless --lora-init-without-apply
  for (auto& a : o.lora) { S.lora_paths.push_back(a.first); S.lora_scale.push_back(0.f); }
  if (o.lora.size() == 1 && !o.lora_init_without_apply) S.lora_scale[0] = o.lora[0].second;
  if (!S.spawn_cli.empty()) {
    // forward the model / engine flags to every child; the server's own flags stay here
    static const char* own1[] = {"--port", "--host", "--static", "--api-key", "--rate-limit", "--mock-delay-ms",
                                 "--alias", "--model-alias", "--max-models", "--model-switch-ms", "--spawn-cli",
                                 "-p", "--prompt", "-n", "--n-predict"};
    static const char* own0[] = {"--mock", "--no-continuous", "--daemon"};
    for (int i = 1; i < argc; ++i) {
      bool skip = false;
      for (const char* f : own1)
        if (!strcmp(argv[i], f)) { skip = true; ++i; break; }
      for (const char* f : own0)
        if (!strcmp(argv[i], f)) skip = true;
      if (!skip) S.cli_args.push_back(argv[i]);
    }
    if (S.spawn_cli == "mi-cli" || S.spawn_cli == "default") {   // the mi-cli next to this binary
      char exe[4096];
      const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
      if (n > 0) { exe[n] = 0; std::string d(exe); S.spawn_cli = d.substr(0, d.rfind('/')) + "/mi-cli"; }
    }
  }
  {
    struct stat stt;
    if (stat(S.static_dir.c_str(), &stt) != 0) {   // fall back to the package's static/ next to bin/
      char exe[4096];
      const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
      if (n > 0) {
        exe[n] = 0;
        std::string d(exe);
        d = d.substr(0, d.rfind('/'));
        d = d.substr(0, d.rfind('/')) + "/static";
        if (stat(d.c_str(), &stt) == 0) S.static_dir = d;
      }
    }
  }
  // capture start-up logs (placement / offload lines) to replay to every request's log pane
  log_set_callback([&S](const std::string& line) {
    if (!S.ready && !S.mock) S.startup_logs.push_back(line);
    else broadcast_log(line);
  });
  try {
    if (!S.spawn_cli.empty()) {
      S.startup_logs.push_back("spawn-cli mode: every request runs " + S.spawn_cli + " (no engine in this process)\n");
      S.capacity = 1 << 20;
    } else if (!mock) {
      if (!o.eng.has("mb_size")) o.eng["mb_size"] = 4;
      std::unique_ptr<ModelSlot> d(new ModelSlot);
      d->cfg = o.eng;
      d->source = o.eng.has("gguf") ? o.eng.get_str("gguf", "") : "synthetic:" + synthetic_name;
      d->name = !alias.empty() ? alias : d->source.substr(d->source.rfind('/') + 1);
      S.models.push_back(std::move(d));
      for (const std::string& a : aliases) {
        const size_t eq = a.find('=');
        if (eq == std::string::npos || eq == 0) throw std::runtime_error("--model-alias expects NAME=PATH");
        std::unique_ptr<ModelSlot> m(new ModelSlot);
        m->name = a.substr(0, eq);
        m->source = a.substr(eq + 1);
        m->cfg = o.eng;
        if (m->source.rfind("synthetic:", 0) == 0) {
          m->cfg.erase("gguf");
          m->cfg["synthetic"] = synthetic_arch(m->source.substr(10));
        } else {
          m->cfg.erase("synthetic");
          m->cfg["gguf"] = m->source;
        }
        S.models.push_back(std::move(m));
      }
      load_slot(S, *S.models[0]);
      S.models[0]->last_used = now_ms();
      S.capacity = S.models[0]->sess->capacity();
    } else {
      S.startup_logs.push_back("mock engine: stage 0: layers 0-5 offloaded to GPU 0 (mock)\n");
      S.capacity = 4;
    }
  } catch (const std::exception& e) {
    MP_LOGE("orchestrator: engine init failed: %s", e.what());
    return 1;
  }
  S.ready = true;
  int ls = socket(AF_INET, SOCK_STREAM, 0);
  int one = 1;
  setsockopt(ls, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
  sockaddr_in addr{};
  addr.sin_family = AF_INET;
  addr.sin_port = htons((uint16_t)port);
  if (inet_pton(AF_INET, host.c_str(), &addr.sin_addr) != 1) {
    MP_LOGE("bad --host %s", host.c_str());
    return 2;
  }
  if (bind(ls, (sockaddr*)&addr, sizeof(addr)) != 0 || listen(ls, 128) != 0) {
    MP_LOGE("cannot listen on %s:%d: %s", host.c_str(), port, strerror(errno));   // main.rs:109 panics; we exit 1
    return 1;
  }
  std::thread gen(generation_loop, std::ref(S));
  printf("orchestrator ready on http://%s:%d (static: %s, %s)\n", host.c_str(), port, S.static_dir.c_str(),
         mock ? "mock engine" : "engine loaded");
  fflush(stdout);
  while (!S.stop) {
    sockaddr_in peer{};
    socklen_t pl = sizeof(peer);
    int fd = accept(ls, (sockaddr*)&peer, &pl);
    if (fd < 0) continue;
    setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
    char ip[64];
    inet_ntop(AF_INET, &peer.sin_addr, ip, sizeof(ip));
    std::thread(handle_conn, std::ref(S), fd, std::string(ip)).detach();
  }
  gen.join();
  return 0;
}
