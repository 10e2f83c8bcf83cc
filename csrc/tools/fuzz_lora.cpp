// Host-side robustness driver for the LoRA adapter reader (csrc/runtime/lora.cpp), for sanitizer
// builds (make sanitize-lora: -fsanitize=address,undefined, no GPU code, a plain executable).  Adapter
// files come from users: every input must end as "ok" or as a clean rejection (exception), never as
// a sanitizer report.
//
//   fuzz_lora BASE.gguf ADAPTER.gguf...    exit 0; prints "ok ..." / "rejected: <reason>" per adapter
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "gguf.h"
#include "lora.h"
#include "model.h"

using namespace mp;

static void check_adapter(const ModelConfig& cfg, const char* path) {
  GgufFile f(path);
  const LoraFile lf = lora_read(f, cfg, kLoraMaxRank, 0, cfg.n_layer);
  size_t words = 0;
  std::vector<uint16_t> a, b;
  for (const LoraPair& p : lf.pairs) {
    lora_pack_f16(p, cfg.rope_neox && p.target <= LORA_K ? cfg.head_dim : 0, &a, &b);
    words += a.size() + b.size();
  }
  // the tile builder over a small row -> adapter map
  const int32_t ids[20] = {0, -1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
  std::vector<float> sc(20, 0.5f);
  const int mt = lora_max_tiles(20, 2);
  std::vector<int32_t> tab(lora_table_words(mt));
  const int nt = lora_build_tiles(ids, sc.data(), 20, 2, mt, tab.data());
  std::printf("ok %d pairs, ranks %d..%d, alpha %g, %zu f16 words, %d tiles\n", lf.n_pairs, lf.r_min, lf.r_max, (double)lf.alpha,
              words, nt);
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: fuzz_lora BASE.gguf ADAPTER.gguf...\n");
    return 2;
  }
  ModelConfig cfg;
  try {
    GgufFile base(argv[1]);
    cfg = ModelConfig::from_gguf(base);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fuzz_lora: base model: %s\n", e.what());
    return 2;
  }
  for (int i = 2; i < argc; ++i) {
    try {
      check_adapter(cfg, argv[i]);
    } catch (const std::exception& e) {
      std::printf("rejected: %.160s\n", e.what());
    }
  }
  return 0;
}
