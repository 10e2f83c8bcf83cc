// mi-cli: the generation driver (the role of llama-cli in the reference; flags as
// spawned by `orchestrator/src/main.rs:38-53`).  stdout = prompt echo + generated text (streamed,
// UTF-8 safe), stderr = logs incl. the stage placement lines and the perf summary.
//
//   mi-cli -m model.gguf -p "Once upon a time" -n 200 -c 2048 -ngl 99 --stages 2 --verbose
//   mi-cli --synthetic llama3-70b --ftype Q4_K --bench --mb-size 16
//   mi-cli -m m.gguf --world 2 --rank 0 --next 10.0.0.2      (one process per stage, TCP ring)
//   mi-cli -m embed.gguf --embedding -p "a query" --pooling last     (`embedding 0: v0 v1 ...`)
//   mi-cli -m m.gguf --daemon      (JSON-lines server on stdin/stdout for the orchestrator)
//   mi-cli --rpc-server 50052      (long-lived stage worker; a client attaches with --rpc host:port,..)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

#include "cli_common.h"
#include "engine.h"
#include "log.h"
#include "perplexity.h"
#include "rpc.h"
#include "session.h"

using namespace mp;

static void usage() {
  fprintf(stderr, "usage: mi-cli -m MODEL.gguf [-p PROMPT] [-n N] [-c CTX] [-ngl N] [options]\n");
  print_common_usage(stderr);
  fprintf(stderr,
          "mi-cli:\n"
          "  --perplexity -f FILE      prints a running estimate and `Final estimate: PPL = x +/- y`\n"
          "  --bench [--bench-prompt L --bench-warmup W --bench-steps K]   decode throughput of full batches\n"
          "  --daemon                  read {\"prompt\":..,\"n_predict\":..} lines on stdin, answer with JSON lines\n"
          "  --no-display-prompt       do not echo the prompt\n"
          "  --state-save DIR          after generating, checkpoint the KV shards + sequences to DIR\n"
          "  --state-load DIR          resume a checkpoint: continue its sequence for -n more tokens\n"
          "  --rpc-server PORT [-m LOCAL.gguf] [--device D] [--rpc-jobs N]\n"
          "                            stage worker (llama.cpp rpc-server role): serve --rpc clients, N jobs (0 = forever)\n");
}

// --perplexity -f FILE: llama.cpp's default procedure (perplexity.h) on the engine's prompt scoring;
// the windows go through Engine::score capacity() at a time
static int run_perplexity(Engine& eng, Session& s, const std::string& text) {
  const int c = eng.max_ctx();
  const std::vector<int32_t> toks = s.encode_raw(text);
  if (!ppl_enough_tokens(toks.size(), c)) {
    fprintf(stderr, "mi-cli: --perplexity needs at least %d tokens (2 x the context of %d), the file has %zu\n", 2 * c, c,
            toks.size());
    return 1;
  }
  const long n_win = ppl_n_windows(toks.size(), c);
  const int bos = s.bos();
  MP_LOGI("perplexity: %zu tokens, %ld windows of %d, %d at a time", toks.size(), n_win, c, s.capacity());
  PplEstimate est;
  const double t0 = session_now_ms();
  for (long w0 = 0; w0 < n_win; w0 += s.capacity()) {
    std::vector<std::vector<int32_t>> wins;
    for (long w = w0; w < std::min(n_win, w0 + (long)s.capacity()); ++w) wins.push_back(ppl_window(toks, w, c, bos));
    std::vector<Engine::SeqLogprobs> sc;
    eng.score(wins, 0, &sc);
    for (size_t i = 0; i < wins.size(); ++i) {
      est.add_window(sc[i].lp.data(), c);
      printf("[%ld]%.4lf,", w0 + (long)i + 1, est.ppl());
    }
    fflush(stdout);
  }
  printf("\n");
  MP_LOGI("perplexity: %.1f ms, %ld positions counted", session_now_ms() - t0, est.count);
  printf("Final estimate: PPL = %.4lf +/- %.5lf\n", est.ppl(), est.err());
  fflush(stdout);
  return 0;
}

// --embedding: one prompt per line of the -p / -f text; `embedding N: v0 v1 ...` per vector (with
// --pooling none one per token, numbered through), values as %.9g so that they read back exactly
static int run_embedding(Engine& eng, Session& s, const CliOptions& o) {
  std::vector<std::vector<int32_t>> prompts;
  std::stringstream ss(o.prompt);
  for (std::string line; std::getline(ss, line);) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (!line.empty()) prompts.push_back(s.encode_embedding(line));
  }
  if (prompts.empty()) throw std::runtime_error("--embedding: no prompt (-p TEXT, or -f FILE with one prompt per line)");
  const int pooling = Engine::pooling_from_name(o.pooling);
  const size_t d = (size_t)eng.model().d_model;
  const double t0 = session_now_ms();
  size_t n_tok = 0;
  int n = 0;
  for (size_t g = 0; g < prompts.size();) {
    const std::vector<int> idle = eng.idle_slots();
    const size_t take = std::min(idle.size(), prompts.size() - g);
    if (take == 0) throw std::runtime_error("--embedding: no idle slot");
    std::vector<Engine::EmbedResult> res;
    eng.embed(std::vector<int>(idle.begin(), idle.begin() + take),
              std::vector<std::vector<int32_t>>(prompts.begin() + g, prompts.begin() + g + take), pooling, o.embd_normalize == 2,
              &res);
    if (eng.owns_last())
      for (const auto& r : res)
        for (int row = 0; row < r.n_rows; ++row) {
          printf("embedding %d:", n++);
          for (size_t i = 0; i < d; ++i) printf(" %.9g", (double)r.v[(size_t)row * d + i]);
          printf("\n");
        }
    for (size_t k = g; k < g + take; ++k) n_tok += prompts[k].size();
    g += take;
  }
  fflush(stdout);
  MP_LOGI("embedding: %zu prompts, %zu tokens, pooling %s, %.1f ms", prompts.size(), n_tok,
          pooling_name(pooling < 0 ? eng.default_pooling() : pooling), session_now_ms() - t0);
  return 0;
}

static int run_daemon(Session& s) {
  // one JSON request per line -> {"piece": ...} lines then {"done": true, stats}
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    Json rq;
    try {
      rq = Json::parse(line);
    } catch (const std::exception& e) {
      Json err = Json::object();
      err["error"] = e.what();
      printf("%s\n", err.dump().c_str());
      fflush(stdout);
      continue;
    }
    std::vector<GenRequest> reqs(1);
    reqs[0].prompt = rq.get_str("prompt", "");
    reqs[0].n_predict = rq.get_int("n_predict", 200);
    if (rq.has("n_keep")) { reqs[0].has_keep = true; reqs[0].n_keep = rq.get_int("n_keep", 0); }
    reqs[0].on_piece = [](const std::string& p) {
      Json o = Json::object();
      o["piece"] = p;
      printf("%s\n", o.dump().c_str());
      fflush(stdout);
      return true;
    };
    auto r = s.run(reqs)[0];
    Json d = Json::object();
    d["done"] = true;
    d["n_prompt"] = r.n_prompt;
    d["n_gen"] = r.n_gen;
    d["prefill_ms"] = r.prefill_ms;
    d["decode_ms"] = r.decode_ms;
    d["stop"] = r.stop;
    d["n_shifts"] = r.n_shifts;
    printf("%s\n", d.dump().c_str());
    fflush(stdout);
  }
  return 0;
}

// mi-cli --rpc-server PORT [-m LOCAL.gguf] [--device D] [--rpc-jobs N] [--verbose]
static int rpc_server_main(int argc, char** argv) {
  int port = 0, device = -1, jobs = 0;
  std::string gguf;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&]() -> std::string {
      if (i + 1 >= argc) throw std::runtime_error("missing value for " + a);
      return argv[++i];
    };
    if (a == "--rpc-server") port = std::atoi(val().c_str());
    else if (a == "-m" || a == "--model") gguf = val();
    else if (a == "--device") device = std::atoi(val().c_str());
    else if (a == "--rpc-jobs") jobs = std::atoi(val().c_str());
    else if (a == "--verbose") log_set_level(LOG_DEBUG);
    else throw std::runtime_error("--rpc-server: unknown flag " + a);
  }
  if (port <= 0) throw std::runtime_error("--rpc-server needs a port");
  return run_rpc_server(port, gguf, device, jobs);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (std::strcmp(argv[i], "--rpc-server") == 0) {
      try {
        return rpc_server_main(argc, argv);
      } catch (const std::exception& e) {
        MP_LOGE("mi-cli: %s", e.what());
        return 2;
      }
    }
  bool daemon = false;
  std::string state_save, state_load;
  CliOptions o;
  try {
    o = parse_cli(argc, argv, [&](const std::string& a, const std::function<std::string()>& val) {
      if (a == "--daemon") { daemon = true; return true; }
      if (a == "--state-save") { state_save = val(); return true; }
      if (a == "--state-load") { state_load = val(); return true; }
      if (a == "-h" || a == "--help") { usage(); exit(0); }
      return false;
    });
  } catch (const std::exception& e) {
    fprintf(stderr, "mi-cli: %s\n", e.what());
    usage();
    return 2;
  }
  try {
    if (!o.grammar.empty() && (daemon || !state_load.empty()))
      throw std::runtime_error("a grammar cannot be combined with --daemon or --state-load");
    if (o.lora.size() > 1)
      throw std::runtime_error("--lora / --lora-scaled: exactly one adapter may be given (stacking adapters on a sequence is not supported)");
    if (!o.lora.empty() && (daemon || !state_load.empty() || !state_save.empty() || o.bench))
      throw std::runtime_error("--lora cannot be combined with --daemon, --state-load, --state-save or --bench");
    if (o.bench) {
      if (!o.eng.has("mb_size")) o.eng["mb_size"] = 16;
      const int need = o.bench_prompt + o.bench_warmup + o.bench_steps + 8;
      if (o.eng.get_int("max_ctx", 2048) < need) o.eng["max_ctx"] = need;
    }
    RpcClient rpc;
    const bool attached = !o.bench && !daemon && state_load.empty() && !o.rpc.empty() &&
                          rpc_attach(o.rpc, o.eng, o.prompt, o.n_predict, o.master.empty() ? "127.0.0.1" : o.master, rpc);
    Engine eng(o.eng);
    if (!o.trace.empty()) eng.enable_trace(true);
    if (o.bench) {
      Json r = eng.bench(o.bench_prompt, o.bench_warmup, o.bench_steps);
      r["info"] = eng.info();
      printf("%s\n", r.dump().c_str());
      if (!o.trace.empty()) eng.write_trace(o.trace);
      return 0;
    }
    // --lora: the one adapter, bound to every sequence slot (the prompt-scoring and embedding chunks of
    // --perplexity / --embedding take the binding like any prefill chunk)
    int lora_id = -1;
    if (!o.lora.empty()) {
      lora_id = eng.load_adapter(o.lora[0].first);
      const int ns = eng.n_mb() * eng.mb_size();
      std::vector<int> slots(ns), ids(ns, lora_id);
      for (int i = 0; i < ns; ++i) slots[i] = i;
      eng.set_slot_adapters(slots, ids, std::vector<float>(ns, o.lora[0].second));
    }
    Session s(eng, o.eng.get_str("gguf", ""));
    if (daemon) return run_daemon(s);
    if (o.perplexity) return run_perplexity(eng, s, o.prompt);
    if (o.embedding) return run_embedding(eng, s, o);
    if (!state_load.empty()) {
      // resume: continue sequence 0 of the checkpoint token by token
      eng.load_state(state_load);
      const bool solo = eng.owns_first() && eng.owns_last();
      Utf8Acc acc;
      int n = 0;
      const double t0 = session_now_ms();
      for (; n < o.n_predict; ++n) {
        eng.decode_steps(1);
        if (!eng.owns_last()) continue;
        const int32_t t = eng.tokens()[0].back();
        if (s.is_eog(t) && solo) break;
        const std::string p = acc.push(s.piece(t));
        fwrite(p.data(), 1, p.size(), stdout);
        fflush(stdout);
      }
      if (eng.owns_last()) {
        fputs((acc.buf + "\n").c_str(), stdout);
        MP_LOGI("resumed %s: %d tokens in %.1f ms", state_load.c_str(), n, session_now_ms() - t0);
      }
      if (!state_save.empty()) eng.save_state(state_save);
      return 0;
    }
    if (o.echo_prompt && eng.owns_last()) {
      fputs(o.prompt.c_str(), stdout);
      fflush(stdout);
    }
    std::vector<GenRequest> reqs(1);
    reqs[0].prompt = o.prompt;
    reqs[0].n_predict = o.n_predict;
    if (!o.grammar.empty()) reqs[0].grammar = Grammar::parse(o.grammar);
    if (lora_id >= 0) { reqs[0].lora_id = lora_id; reqs[0].lora_scale = o.lora[0].second; }
    reqs[0].on_piece = [](const std::string& p) {
      fwrite(p.data(), 1, p.size(), stdout);
      fflush(stdout);
      return true;
    };
    auto r = s.run(reqs)[0];
    if (eng.owns_last()) {
      fputs("\n", stdout);
      fflush(stdout);
      MP_LOGI("\n%s", Session::perf_summary(r, eng.load_ms()).c_str());
      if (eng.auto_shift()) MP_LOGI("stop: %s after %d tokens, %d context shifts", r.stop.c_str(), r.n_gen, r.n_shifts);
    }
    if (!state_save.empty()) eng.save_state(state_save);
    if (!o.trace.empty()) eng.write_trace(o.trace);
    if (attached) rpc_collect(rpc);
  } catch (const std::exception& e) {
    MP_LOGE("mi-cli: error: %s", e.what());
    return 1;
  }
  return 0;
}
