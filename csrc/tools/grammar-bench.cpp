// grammar-bench: host time of GrammarState::mask for the JSON-object grammar, at the start of the
// document, inside a string and between two members, first computation and cached.
//   grammar-bench -m MODEL.gguf      the model's own vocabulary
//   grammar-bench [--vocab N]        a synthetic vocabulary: the 256 bytes, then N - 257 random pieces of
//                                    2..8 characters over letters, digits, blanks and JSON punctuation, one EOG
// Host code only.  The same file is the stand-alone program for a sanitizer run of the grammar engine:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc/runtime \
//       csrc/tools/grammar-bench.cpp csrc/runtime/{grammar,json,tokenizer,gguf,model,log}.cpp -o grammar_bench_asan
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "gguf.h"
#include "grammar.h"
#include "tokenizer.h"

using namespace mp;

int main(int argc, char** argv) {
  std::string gguf;
  int n_vocab = 128256, reps = 5;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if ((a == "-m" || a == "--model") && i + 1 < argc) gguf = argv[++i];
    else if (a == "--vocab" && i + 1 < argc) n_vocab = std::atoi(argv[++i]);
    else if (a == "--reps" && i + 1 < argc) reps = std::atoi(argv[++i]);
    else { fprintf(stderr, "usage: grammar-bench [-m MODEL.gguf | --vocab N] [--reps R]\n"); return 2; }
  }
  try {
    std::shared_ptr<const GrammarVocab> v;
    if (!gguf.empty()) {
      GgufFile f(gguf);
      v = std::make_shared<GrammarVocab>(Tokenizer::from_gguf(f));
    } else {
      if (n_vocab < 300) throw std::runtime_error("--vocab must be at least 300");
      std::vector<std::string> pieces;
      uint64_t x = 88172645463325252ULL;
      auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
      for (int i = 0; i < 256; ++i) pieces.push_back(std::string(1, (char)i));
      const char al[] = "abcdefghijklmnopqrstuvwxyz ABCDEFGH0123456789{}[]\",:.-_\n\t\\";
      const size_t n_al = sizeof(al) - 1;
      while ((int)pieces.size() < n_vocab - 1) {
        std::string s;
        const int n = 2 + (int)(rnd() % 7);
        for (int k = 0; k < n; ++k) s += al[rnd() % n_al];
        pieces.push_back(s);
      }
      pieces.push_back("");
      v = std::make_shared<GrammarVocab>(pieces, std::vector<int32_t>{n_vocab - 1});
    }
    Json any = Json::object();
    any["type"] = "json_object";
    const std::string gbnf = json_schema_to_gbnf(any);
    std::vector<uint32_t> bits(v->mask_words());
    printf("vocabulary: %d tokens\n", v->n_vocab());
    for (const char* pre : {"", "{\"key\": \"some te", "{\"key\": \"v\","}) {
      double first = 1e30, cached = 1e30;
      int allowed = 0;
      for (int r = 0; r < reps; ++r) {
        auto g = Grammar::parse(gbnf);   // a fresh grammar: nothing cached
        GrammarState st(g, v);
        if (!st.accept_text(pre)) throw std::runtime_error(std::string("the prefix is not JSON: ") + pre);
        const auto t0 = std::chrono::steady_clock::now();
        st.mask(bits.data());
        const auto t1 = std::chrono::steady_clock::now();
        st.mask(bits.data());
        const auto t2 = std::chrono::steady_clock::now();
        first = std::min(first, std::chrono::duration<double, std::milli>(t1 - t0).count());
        cached = std::min(cached, std::chrono::duration<double, std::milli>(t2 - t1).count());
        allowed = 0;
        for (uint32_t w : bits) allowed += __builtin_popcount(w);
      }
      printf("after '%s': %d tokens allowed, first mask %.3f ms, the same state again %.4f ms (best of %d)\n", pre, allowed,
             first, cached, reps);
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "grammar-bench: %s\n", e.what());
    return 1;
  }
  return 0;
}
