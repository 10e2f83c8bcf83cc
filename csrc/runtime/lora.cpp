#include "lora.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>

#include "gguf.h"
#include "pack.h"

namespace mp {

static const char* kTargetNames[LORA_N_TARGETS] = {"attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down"};

const char* lora_target_name(int t) { return t >= 0 && t < LORA_N_TARGETS ? kTargetNames[t] : "?"; }

void lora_target_dims(const ModelConfig& c, int target, int* K, int* N) {
  switch (target) {
    case LORA_Q: *K = c.d_model; *N = c.q_dim(); break;
    case LORA_K: case LORA_V: *K = c.d_model; *N = c.kv_dim(); break;
    case LORA_O: *K = c.q_dim(); *N = c.d_model; break;
    case LORA_GATE: case LORA_UP: *K = c.d_model; *N = c.d_ff; break;
    case LORA_DOWN: *K = c.d_ff; *N = c.d_model; break;
    default: throw std::runtime_error("lora: bad target");
  }
}

static bool ends_with(const std::string& s, const char* suf) {
  const size_t n = std::strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// "blk.<layer>.<target>.weight" -> (layer, target); false for any other name
static bool parse_base_name(const std::string& base, int n_layer, int* layer, int* target) {
  if (base.compare(0, 4, "blk.") != 0) return false;
  size_t p = 4;
  if (p >= base.size() || base[p] < '0' || base[p] > '9') return false;
  long li = 0;
  while (p < base.size() && base[p] >= '0' && base[p] <= '9' && li < (1 << 24)) li = li * 10 + (base[p++] - '0');
  if (p >= base.size() || base[p] != '.' || li >= n_layer) return false;
  const std::string rest = base.substr(p + 1);
  for (int t = 0; t < LORA_N_TARGETS; ++t)
    if (rest == std::string(kTargetNames[t]) + ".weight") { *layer = (int)li; *target = t; return true; }
  return false;
}

static std::vector<float> matrix_f32(const GgufTensor& t) {
  const int64_t K = t.ne[0], R = t.ne[1];
  const int be = block_elems(t.type);
  if (be <= 0) throw std::runtime_error("lora: " + t.name + ": unsupported element type " + std::to_string(t.type));
  if (K % be) throw std::runtime_error("lora: " + t.name + ": row is not a block multiple of " + type_name(t.type));
  const size_t rb = row_bytes(t.type, K);
  if (rb * (size_t)R > t.nbytes) throw std::runtime_error("lora: " + t.name + ": data is shorter than its shape");
  std::vector<float> v((size_t)K * R);
  for (int64_t r = 0; r < R; ++r) dequant_row(t.type, t.data + r * rb, v.data() + r * K, K);
  return v;
}

LoraFile lora_read(const GgufFile& f, const ModelConfig& cfg, int max_rank, int layer_begin, int layer_end) {
  LoraFile out;
  out.path = f.path();
  auto field = [&](const char* key, const std::string& want) {
    const GgufValue* v = f.get(key);
    const std::string got = v && v->type == GV_STRING ? v->s : std::string();
    if (got != want)
      throw std::runtime_error(std::string("lora: ") + key + " is \"" + got + "\", expected \"" + want + "\" (" + f.path() + ")");
  };
  field("general.type", "adapter");
  field("adapter.type", "lora");
  field("general.architecture", cfg.arch);
  {
    const GgufValue* a = f.get("adapter.lora.alpha");
    if (!a || a->type == GV_STRING || a->type == GV_ARRAY) throw std::runtime_error("lora: adapter.lora.alpha is missing (" + f.path() + ")");
    out.alpha = (float)(a->type == GV_F32 || a->type == GV_F64 ? a->f : (double)a->i);
    if (!(out.alpha == out.alpha) || out.alpha - out.alpha != 0.f) throw std::runtime_error("lora: adapter.lora.alpha is not finite");
  }
  if (max_rank < 1 || max_rank > kLoraMaxRank) throw std::runtime_error("lora: lora_max_rank must be 1.." + std::to_string(kLoraMaxRank));

  struct Ab { const GgufTensor* a = nullptr; const GgufTensor* b = nullptr; };
  std::map<std::pair<int, int>, Ab> found;
  for (const GgufTensor& t : f.tensors()) {
    const bool is_a = ends_with(t.name, ".lora_a"), is_b = ends_with(t.name, ".lora_b");
    if (!is_a && !is_b) continue;
    const std::string base = t.name.substr(0, t.name.size() - 7);
    int li = 0, tg = 0;
    if (!parse_base_name(base, cfg.n_layer, &li, &tg))
      throw std::runtime_error("lora: " + t.name + ": adapters on this tensor are not supported (attn_q, attn_k, attn_v, "
                               "attn_output, ffn_gate, ffn_up, ffn_down of the model's layers only)");
    if (cfg.n_expert && tg >= LORA_GATE)
      throw std::runtime_error("lora: " + t.name + ": a mixture-of-experts model takes adapters on the attention projections only");
    if (t.ne.size() != 2) throw std::runtime_error("lora: " + t.name + ": expected a 2-D tensor");
    Ab& e = found[{li, tg}];
    if ((is_a ? e.a : e.b)) throw std::runtime_error("lora: " + t.name + ": listed twice");
    (is_a ? e.a : e.b) = &t;
  }
  bool first = true;
  for (auto& kv : found) {
    const int li = kv.first.first, tg = kv.first.second;
    const std::string base = "blk." + std::to_string(li) + "." + kTargetNames[tg] + ".weight";
    const Ab& e = kv.second;
    if (!e.a) throw std::runtime_error("lora: " + base + ".lora_b has no " + base + ".lora_a");
    if (!e.b) throw std::runtime_error("lora: " + base + ".lora_a has no " + base + ".lora_b");
    int K = 0, N = 0;
    lora_target_dims(cfg, tg, &K, &N);
    if (e.a->ne[0] != K)
      throw std::runtime_error("lora: " + e.a->name + ": K is " + std::to_string(e.a->ne[0]) + ", the base tensor's is " + std::to_string(K));
    if (e.b->ne[1] != N)
      throw std::runtime_error("lora: " + e.b->name + ": N is " + std::to_string(e.b->ne[1]) + ", the base tensor's is " + std::to_string(N));
    const int64_t r = e.a->ne[1];
    if (e.b->ne[0] != r)
      throw std::runtime_error("lora: " + e.b->name + ": rank " + std::to_string(e.b->ne[0]) + " differs from " + e.a->name + "'s " +
                               std::to_string(r));
    if (r < 1) throw std::runtime_error("lora: " + e.a->name + ": rank 0");
    if (r > max_rank)
      throw std::runtime_error("lora: " + e.a->name + ": rank " + std::to_string(r) + " exceeds lora_max_rank " + std::to_string(max_rank));
    out.r_min = first ? (int)r : std::min(out.r_min, (int)r);
    out.r_max = first ? (int)r : std::max(out.r_max, (int)r);
    first = false;
    ++out.n_pairs;
    if (li < layer_begin || li >= layer_end) continue;
    LoraPair p;
    p.layer = li; p.target = tg; p.r = (int)r; p.K = K; p.N = N;
    p.A = matrix_f32(*e.a);
    p.B = matrix_f32(*e.b);
    if (out.alpha != 0.f) {
      const float s = out.alpha / (float)r;
      for (float& v : p.B) v *= s;
    }
    out.pairs.push_back(std::move(p));
  }
  if (!out.n_pairs) throw std::runtime_error("lora: " + f.path() + " holds no .lora_a / .lora_b tensor pair");
  return out;
}

void lora_pack_f16(const LoraPair& p, int neox_hd, std::vector<uint16_t>* A16, std::vector<uint16_t>* B16) {
  const int rp = lora_rank_pad(p.r);
  A16->assign((size_t)rp * p.K, 0);
  B16->assign((size_t)p.N * rp, 0);
  for (int j = 0; j < p.r; ++j)
    for (int k = 0; k < p.K; ++k) (*A16)[(size_t)j * p.K + k] = f32_to_f16(p.A[(size_t)j * p.K + k]);
  for (int n = 0; n < p.N; ++n) {
    const long src = neox_hd > 0 ? neox_src_row(n, neox_hd) : n;
    for (int j = 0; j < p.r; ++j) (*B16)[(size_t)n * rp + j] = f32_to_f16(p.B[(size_t)src * p.r + j]);
  }
}

int lora_build_tiles(const int32_t* ids, const float* scales, int M, int n_adapters, int max_tiles, int32_t* out) {
  if (M < 0 || n_adapters < 0 || max_tiles < 0 || !out) throw std::runtime_error("lora tiles: bad arguments");
  std::memset(out, 0, lora_table_words(max_tiles) * 4);
  LoraTile* tiles = reinterpret_cast<LoraTile*>(out + kLoraTabHeader);
  int nt = 0;
  for (int a = 0; a < n_adapters; ++a) {
    int fill = kLoraTileRows;   // rows in the open tile (full: none open)
    for (int m = 0; m < M; ++m) {
      if (ids[m] != a) continue;
      if (fill == kLoraTileRows) {
        if (nt == max_tiles) throw std::runtime_error("lora tiles: more tiles than the table holds");
        LoraTile& t = tiles[nt++];
        t.adapter = a;
        for (int i = 0; i < kLoraTileRows; ++i) { t.rows[i] = -1; t.scale[i] = 0.f; }
        fill = 0;
      }
      LoraTile& t = tiles[nt - 1];
      t.rows[fill] = m;
      t.scale[fill] = scales ? scales[m] : 1.f;
      ++fill;
    }
  }
  for (int m = 0; m < M; ++m)
    if (ids[m] >= n_adapters || ids[m] < -1) throw std::runtime_error("lora tiles: adapter id " + std::to_string(ids[m]) + " is out of range");
  out[0] = nt;
  return nt;
}

}  // namespace mp
