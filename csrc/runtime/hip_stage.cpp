#include "hip_stage.h"
#include "hip_head.h"
#include "hip_lora.h"

#include <functional>
#include "tuning.h"

#include <chrono>
#include <cstring>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <stdexcept>

#include "gguf.h"
#include "log.h"
#include "pack.h"

namespace mp {

void launch_prefill_meta(int32_t* pos, int32_t* kvlen, int32_t* slot, int p0, int T, int s, hipStream_t st);

SyntheticTypes SyntheticTypes::from_ftype(const std::string& ftype_in, int layer, int n_layer) {
  std::string f = ftype_in;
  for (auto& c : f) c = (char)toupper(c);
  SyntheticTypes t;
  auto all = [&](int ty) { t.embd = t.q = t.k = t.v = t.o = t.gate = t.up = t.down = t.out = ty; };
  auto more_bits = [&](int i, int n) { return i < n / 8 || i >= 7 * n / 8 || (i - n / 8) % 3 == 2; };
  if (f == "F16") all(T_F16);
  else if (f == "BF16") all(T_BF16);
  else if (f == "F32") all(T_F32);
  else if (f == "Q8_0") all(T_Q8_0);
  else if (f == "Q6_K") all(T_Q6_K);
  else if (f == "Q5_K" || f == "Q5_K_M") { all(T_Q5_K); t.out = T_Q6_K; }
  else if (f == "Q4_0") all(T_Q4_0);
  else if (f == "Q4_K" || f == "Q4_K_S") { all(T_Q4_K); t.out = T_Q6_K; }
  else if (f == "Q4_K_M") {
    all(T_Q4_K);
    t.out = T_Q6_K;
    if (more_bits(layer, n_layer)) { t.v = T_Q6_K; t.down = T_Q6_K; }
  } else if (f == "Q3_K" || f == "Q3_K_S") { all(T_Q3_K); t.out = T_Q6_K; }
  else if (f == "Q3_K_M" || f == "Q3_K_L") {   // the mixes of models/config.py tensor_type
    const bool large = f == "Q3_K_L";
    all(T_Q3_K);
    t.out = T_Q6_K;
    t.v = large || layer < 2 ? T_Q5_K : T_Q4_K;
    t.o = large ? T_Q5_K : T_Q4_K;
    t.down = large || layer < n_layer / 16 ? T_Q5_K : T_Q4_K;
  } else if (f == "Q2_K") {
    all(T_Q2_K);
    t.out = T_Q6_K;
    t.v = t.o = t.down = T_Q3_K;
  } else if (f == "Q5_0") all(T_Q5_0);
  else if (f == "Q5_1") all(T_Q5_1);
  else if (f == "IQ4_NL") all(T_IQ4_NL);
  else if (f == "IQ4_XS") {   // the mix of models/config.py tensor_type
    all(T_IQ4_XS);
    t.out = T_Q6_K;
    t.v = T_Q5_K;
    if (layer < n_layer / 8) t.down = T_Q5_K;
  } else throw std::runtime_error("unknown synthetic ftype " + ftype_in);
  if (f == "Q5_K_M" && more_bits(layer, n_layer)) { t.v = T_Q6_K; t.down = T_Q6_K; }
  return t;
}

HipStage::HipStage(const ModelConfig& cfg, const StageSpec& spec, const StageOptions& opt)
    : cfg_(cfg), spec_(spec), opt_(opt) {
  HIP_OK(hipSetDevice(spec_.device));
  HIP_OK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  if (opt_.max_ctx % 64) opt_.max_ctx = (int)round_up(opt_.max_ctx, 64);
  if (opt_.prefill_chunk < 1) opt_.prefill_chunk = 1;
  layers_.resize(spec_.layer_end - spec_.layer_begin);
  Dp_ = cfg_.padded_head_dim();
  Kd_ = (int)round_up(cfg_.d_model, 256);
  Ko_ = (int)round_up(cfg_.q_dim(), 256);
  Kff_ = (int)round_up(cfg_.d_ff, 256);
  qkv_n_ = cfg_.q_dim() + 2 * cfg_.kv_dim();
}

HipStage::~HipStage() {
  (void)hipSetDevice(spec_.device);
  destroy_graphs();
  head_.reset();
  lora_.reset();
  for (void* p : allocs_) (void)hipFree(p);
  if (stream_) (void)hipStreamDestroy(stream_);
}

void* HipStage::dmalloc(size_t bytes) {
  void* p = nullptr;
  HIP_OK(hipMalloc(&p, std::max<size_t>(bytes, 256)));
  allocs_.push_back(p);
  return p;
}

float* HipStage::upload_f32(const float* h, size_t n) {
  float* d = (float*)dmalloc(n * sizeof(float));
  HIP_OK(hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice));
  weight_bytes_ += n * sizeof(float);
  return d;
}

// ---- weight upload (load_gguf): T16 packing on host threads into pinned double-buffered staging,
// hipMemcpyAsync on a dedicated stream, so packing piece i+1 overlaps the DMA of piece i (v1
// packed into pageable memory and then blocked in a synchronous hipMemcpy per tensor)
void HipStage::stage_begin() {
  if (stg_.buf[0]) return;
  stg_.cap = (size_t)256 << 20;
  for (int b = 0; b < 2; ++b) {
    HIP_OK(hipHostMalloc((void**)&stg_.buf[b], stg_.cap, hipHostMallocDefault));
    HIP_OK(hipEventCreateWithFlags(&stg_.ev[b], hipEventDisableTiming));
    stg_.busy[b] = false;
  }
  HIP_OK(hipStreamCreateWithFlags(&stg_.st, hipStreamNonBlocking));
  stg_.cur = 0;
  stg_.bytes = 0;
  stg_.t0 = std::chrono::steady_clock::now();
}

void HipStage::stage_end() {
  if (!stg_.buf[0]) return;
  HIP_OK(hipStreamSynchronize(stg_.st));
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - stg_.t0).count();
  upload_gbps_ = s > 0 ? stg_.bytes / s / 1e9 : 0.0;
  MP_LOGI("stage %d: uploaded %.2f GiB of packed weights in %.2f s (%.2f GB/s incl. packing)", spec_.stage,
          stg_.bytes / 1073741824.0, s, upload_gbps_);
  for (int b = 0; b < 2; ++b) {
    HIP_OK(hipEventDestroy(stg_.ev[b]));
    HIP_OK(hipHostFree(stg_.buf[b]));
    stg_.buf[b] = nullptr;
  }
  HIP_OK(hipStreamDestroy(stg_.st));
  stg_.st = nullptr;
}

// dst[0, bytes) <- fill(host, off, n) piece by piece through the staging buffers
void HipStage::stage_put(uint8_t* dst, size_t bytes, size_t granule,
                         const std::function<void(uint8_t*, size_t, size_t)>& fill) {
  const bool own = !stg_.buf[0];
  if (own) stage_begin();
  const size_t piece = std::max(granule, stg_.cap / granule * granule);
  if (piece > stg_.cap) throw std::runtime_error("stage_put: granule larger than the staging buffer");
  for (size_t off = 0; off < bytes; off += piece) {
    const size_t n = std::min(piece, bytes - off);
    const int b = stg_.cur;
    if (stg_.busy[b]) HIP_OK(hipEventSynchronize(stg_.ev[b]));   // its previous DMA has drained
    fill(stg_.buf[b], off, n);
    HIP_OK(hipMemcpyAsync(dst + off, stg_.buf[b], n, hipMemcpyHostToDevice, stg_.st));
    HIP_OK(hipEventRecord(stg_.ev[b], stg_.st));
    stg_.busy[b] = true;
    stg_.cur ^= 1;
    stg_.bytes += n;
  }
  if (own) stage_end();
}

PackedMat HipStage::upload_packed(int t, int64_t N, int64_t K, const std::function<const uint8_t*(int64_t)>& row) {
  PackedMat m;
  m.ptype = pack_type_of(t);
  if (m.ptype < 0) throw std::runtime_error(std::string("unsupported weight type ") + type_name(t));
  m.dims = packed_dims(m.ptype, N, K);
  m.d = (uint8_t*)dmalloc(m.dims.bytes);
  const size_t tile_b = (size_t)m.dims.nsb * chunk_bytes(m.ptype);
  stage_put(m.d, m.dims.bytes, tile_b, [&](uint8_t* h, size_t off, size_t n) {
    pack_t16_tiles(t, N, K, row, h, (int64_t)(off / tile_b), (int64_t)((off + n) / tile_b));
  });
  weight_bytes_ += m.dims.bytes;
  return m;
}

PackedMat HipStage::upload_packed_experts(int t, int E, int64_t N, int64_t K, size_t* stride,
                                          const std::function<const uint8_t*(int, int64_t)>& row) {
  PackedMat m;
  m.ptype = pack_type_of(t);
  if (m.ptype < 0) throw std::runtime_error(std::string("unsupported expert type ") + type_name(t));
  m.dims = packed_dims(m.ptype, N, K);
  *stride = m.dims.bytes;
  m.d = (uint8_t*)dmalloc(m.dims.bytes * E);
  const size_t tile_b = (size_t)m.dims.nsb * chunk_bytes(m.ptype);
  for (int e = 0; e < E; ++e)
    stage_put(m.d + (size_t)e * m.dims.bytes, m.dims.bytes, tile_b, [&](uint8_t* h, size_t off, size_t n) {
      pack_t16_tiles(t, N, K, [&](int64_t r) { return row(e, r); }, h, (int64_t)(off / tile_b),
                     (int64_t)((off + n) / tile_b));
    });
  weight_bytes_ += m.dims.bytes * E;
  return m;
}

PackedMat HipStage::alloc_packed_random(int t, int64_t N, int64_t K, uint64_t seed) {
  PackedMat m;
  m.ptype = pack_type_of(t);
  m.dims = packed_dims(m.ptype, N, K);
  m.d = (uint8_t*)dmalloc(m.dims.bytes);
  launch_init_packed(m.d, m.dims.bytes, m.ptype, 1.0f / std::sqrt((float)K), seed, stream_);
  weight_bytes_ += m.dims.bytes;
  return m;
}

static std::vector<float> tensor_f32(const GgufTensor& t) {
  std::vector<float> v(t.nelem());
  const int64_t K = t.ne[0];
  const size_t rb = row_bytes(t.type, K);
  for (int64_t r = 0; r < t.nelem() / K; ++r) dequant_row(t.type, t.data + r * rb, v.data() + r * K, K);
  return v;
}

void HipStage::load_gguf(const GgufFile& f) {
  HIP_OK(hipSetDevice(spec_.device));
  stage_begin();
  auto need = [&](const std::string& n) -> const GgufTensor& {
    const GgufTensor* t = f.tensor(n);
    if (!t) throw std::runtime_error("missing tensor " + n);
    return *t;
  };
  auto rows_of = [](const GgufTensor& t) {
    const size_t rb = row_bytes(t.type, t.ne[0]);
    return [&t, rb](int64_t n) -> const uint8_t* { return t.data + n * rb; };
  };
  auto pack_mat = [&](const GgufTensor& t) { return upload_packed(t.type, t.ne[1], t.ne[0], rows_of(t)); };

  for (int li = spec_.layer_begin; li < spec_.layer_end; ++li) {
    LayerW& L = layers_[li - spec_.layer_begin];
    const std::string p = "blk." + std::to_string(li) + ".";
    {
      auto v = tensor_f32(need(p + "attn_norm.weight"));
      L.attn_norm = upload_f32(v.data(), v.size());
      auto w = tensor_f32(need(p + "ffn_norm.weight"));
      L.ffn_norm = upload_f32(w.data(), w.size());
    }
    const GgufTensor& tq = need(p + "attn_q.weight");
    const GgufTensor& tk = need(p + "attn_k.weight");
    const GgufTensor& tv = need(p + "attn_v.weight");
    // merge same-type q/k/v into one launch (tile-major layout concatenates)
    const GgufTensor* qkv[3] = {&tq, &tk, &tv};
    int off = 0;
    for (int i = 0; i < 3;) {
      int j = i + 1;
      while (j < 3 && pack_type_of(qkv[j]->type) == pack_type_of(qkv[i]->type) && qkv[j - 1]->ne[1] % 16 == 0 &&
             qkv[j]->type == qkv[i]->type)
        ++j;
      int64_t N = 0;
      std::vector<std::pair<const GgufTensor*, int64_t>> parts;
      for (int k = i; k < j; ++k) { parts.push_back({qkv[k], N}); N += qkv[k]->ne[1]; }
      const bool neox = cfg_.rope_neox;
      const int hd = cfg_.head_dim;
      auto rowfn = [&parts, &tq, &tk, neox, hd](int64_t n) -> const uint8_t* {
        for (auto it = parts.rbegin(); it != parts.rend(); ++it)
          if (n >= it->second) {
            const GgufTensor* t = it->first;
            int64_t r = n - it->second;
            if (neox && (t == &tq || t == &tk)) r = neox_src_row(r, hd);
            return t->data + r * row_bytes(t->type, t->ne[0]);
          }
        return nullptr;
      };
      MatSeg s;
      s.m = upload_packed(qkv[i]->type, N, qkv[i]->ne[0], rowfn);
      s.y_off = off;
      off += (int)N;
      L.qkv.push_back(s);
      i = j;
    }
    if (cfg_.qkv_bias) {
      std::vector<float> b(qkv_n_, 0.f);
      const char* nm[3] = {"attn_q.bias", "attn_k.bias", "attn_v.bias"};
      const int o[3] = {0, cfg_.q_dim(), cfg_.q_dim() + cfg_.kv_dim()};
      for (int i = 0; i < 3; ++i) {
        const std::vector<float> v = tensor_f32(need(p + nm[i]));
        for (size_t r = 0; r < v.size(); ++r)
          b[o[i] + r] = v[i < 2 && cfg_.rope_neox ? neox_src_row((long)r, cfg_.head_dim) : r];
      }
      L.qkv_bias = upload_f32(b.data(), b.size());
    }
    if (cfg_.qk_norm) {
      // the sum of squares is invariant under the per-head NEOX row permutation; the weight is not
      const int hd = cfg_.head_dim;
      float** dst[2] = {&L.q_norm, &L.k_norm};
      const char* nm[2] = {"attn_q_norm.weight", "attn_k_norm.weight"};
      for (int i = 0; i < 2; ++i) {
        const std::vector<float> v = tensor_f32(need(p + nm[i]));
        if ((int)v.size() != hd) throw std::runtime_error(p + nm[i] + ": expected head_dim weights");
        std::vector<float> w(hd);
        for (int r = 0; r < hd; ++r) w[r] = v[cfg_.rope_neox ? neox_src_row(r, hd) : r];
        *dst[i] = upload_f32(w.data(), w.size());
      }
    }
    L.wo = pack_mat(need(p + "attn_output.weight"));
    if (cfg_.n_expert) {
      // Mixtral: router [E][d] + stacked experts (ffn_*_exps [E][F][d]) or legacy per-expert tensors
      L.moe = true;
      const int E = cfg_.n_expert;
      L.ex.router = pack_mat(need(p + "ffn_gate_inp.weight"));
      std::vector<const GgufTensor*> g(E), u(E), dn(E);
      const GgufTensor* sg = f.tensor(p + "ffn_gate_exps.weight");
      for (int e = 0; e < E; ++e) {
        if (sg) {
          g[e] = sg;
          u[e] = &need(p + "ffn_up_exps.weight");
          dn[e] = &need(p + "ffn_down_exps.weight");
        } else {
          const std::string s = "." + std::to_string(e) + ".weight";
          g[e] = &need(p + "ffn_gate" + s);
          u[e] = &need(p + "ffn_up" + s);
          dn[e] = &need(p + "ffn_down" + s);
        }
      }
      if (g[0]->type != u[0]->type) throw std::runtime_error("MoE gate/up types differ");
      const int64_t F = cfg_.d_ff, D = cfg_.d_model;
      // row n of expert e of a (possibly stacked) tensor
      auto erow = [&](const GgufTensor* t, int e, int64_t n, int64_t rows) -> const uint8_t* {
        const size_t rb = row_bytes(t->type, t->ne[0]);
        return t->data + ((sg ? (size_t)e * rows : 0) + n) * rb;
      };
      L.ex.gateup = upload_packed_experts(g[0]->type, E, 2 * F, D, &L.ex.gateup_stride,
                                          [&](int e, int64_t n) -> const uint8_t* {
                                            bool up;
                                            const int64_t r = gateup_src_row(n, &up);
                                            if (r >= F) return nullptr;
                                            return erow(up ? u[e] : g[e], e, r, F);
                                          });
      L.ex.down = upload_packed_experts(dn[0]->type, E, D, F, &L.ex.down_stride,
                                        [&](int e, int64_t n) { return erow(dn[e], e, n, D); });
      continue;
    }
    const GgufTensor& tg = need(p + "ffn_gate.weight");
    const GgufTensor& tu = need(p + "ffn_up.weight");
    // (a lora_adapters stage needs gate and up as f32 before the SwiGLU: never fused)
    if (tg.type == tu.type && cfg_.d_ff % 8 == 0 && !lora_on()) {
      L.fused_gateup = true;
      const size_t rb = row_bytes(tg.type, tg.ne[0]);
      const int64_t F = tg.ne[1];
      L.gateup = upload_packed(tg.type, 2 * F, tg.ne[0], [&](int64_t n) -> const uint8_t* {
        bool up;
        const int64_t r = gateup_src_row(n, &up);
        if (r >= F) return nullptr;
        return (up ? tu.data : tg.data) + r * rb;
      });
    } else {
      L.fused_gateup = false;
      L.gate = pack_mat(tg);
      L.up = pack_mat(tu);
    }
    L.down = pack_mat(need(p + "ffn_down.weight"));
  }
  const GgufTensor& te = need("token_embd.weight");
  if (spec_.first()) {
    embd_type_ = te.type;
    embd_row_bytes_ = row_bytes(te.type, te.ne[0]);
    embd_raw_ = (uint8_t*)dmalloc(te.nbytes);
    stage_put(embd_raw_, te.nbytes, 1, [&](uint8_t* h, size_t off, size_t n) { std::memcpy(h, te.data + off, n); });
    weight_bytes_ += te.nbytes;
  }
  if (spec_.last()) {
    auto v = tensor_f32(need("output_norm.weight"));
    out_norm_ = upload_f32(v.data(), v.size());
    const GgufTensor* to = f.tensor("output.weight");
    out_ = pack_mat(to ? *to : te);
  }
  rope_ff_.clear();
  if (const GgufTensor* rf = f.tensor("rope_freqs.weight")) rope_ff_ = tensor_f32(*rf);
  stage_end();
  HIP_OK(hipDeviceSynchronize());
}

void HipStage::init_synthetic(const std::string& ftype, uint64_t seed) {
  HIP_OK(hipSetDevice(spec_.device));
  const int d = cfg_.d_model, qd = cfg_.q_dim(), kvd = cfg_.kv_dim(), F = cfg_.d_ff;
  std::vector<float> ones(std::max({d, cfg_.head_dim, 1}), 1.0f);
  for (int li = spec_.layer_begin; li < spec_.layer_end; ++li) {
    LayerW& L = layers_[li - spec_.layer_begin];
    const SyntheticTypes t = SyntheticTypes::from_ftype(ftype, li, cfg_.n_layer);
    const uint64_t s = seed * 1000003ULL + (uint64_t)li * 97;
    L.attn_norm = upload_f32(ones.data(), d);
    L.ffn_norm = upload_f32(ones.data(), d);
    int off = 0;
    if (t.q == t.k && t.k == t.v) {
      L.qkv.push_back({alloc_packed_random(t.q, qd + 2 * kvd, d, s + 1), 0});
    } else if (t.q == t.k) {
      L.qkv.push_back({alloc_packed_random(t.q, qd + kvd, d, s + 1), 0});
      L.qkv.push_back({alloc_packed_random(t.v, kvd, d, s + 2), qd + kvd});
    } else {
      L.qkv.push_back({alloc_packed_random(t.q, qd, d, s + 1), off});
      L.qkv.push_back({alloc_packed_random(t.k, kvd, d, s + 2), qd});
      L.qkv.push_back({alloc_packed_random(t.v, kvd, d, s + 3), qd + kvd});
    }
    if (cfg_.qk_norm) {
      L.q_norm = upload_f32(ones.data(), cfg_.head_dim);
      L.k_norm = upload_f32(ones.data(), cfg_.head_dim);
    }
    L.wo = alloc_packed_random(t.o, d, qd, s + 4);
    if (cfg_.n_expert) {
      const int E = cfg_.n_expert;
      L.moe = true;
      L.ex.router = alloc_packed_random(T_F16, E, d, s + 7);
      auto experts = [&](int ty, int64_t N, int64_t K, size_t* stride, uint64_t sd) {
        PackedMat m;
        m.ptype = pack_type_of(ty);
        m.dims = packed_dims(m.ptype, N, K);
        *stride = m.dims.bytes;
        m.d = (uint8_t*)dmalloc(m.dims.bytes * E);
        launch_init_packed(m.d, m.dims.bytes * E, m.ptype, 1.0f / std::sqrt((float)K), sd, stream_);
        weight_bytes_ += m.dims.bytes * E;
        return m;
      };
      L.ex.gateup = experts(t.gate, 2 * F, d, &L.ex.gateup_stride, s + 5);
      L.ex.down = experts(t.down, d, F, &L.ex.down_stride, s + 6);
      continue;
    }
    L.fused_gateup = !lora_on();
    if (L.fused_gateup) {
      L.gateup = alloc_packed_random(t.gate, 2 * F, d, s + 5);
    } else {
      L.gate = alloc_packed_random(t.gate, F, d, s + 5);
      L.up = alloc_packed_random(t.up, F, d, s + 8);
    }
    L.down = alloc_packed_random(t.down, d, F, s + 6);
  }
  const SyntheticTypes t0 = SyntheticTypes::from_ftype(ftype, 0, cfg_.n_layer);
  if (spec_.first()) {
    embd_type_ = t0.embd;
    embd_row_bytes_ = row_bytes(embd_type_, d);
    const size_t nb = embd_row_bytes_ * (size_t)cfg_.vocab;
    embd_raw_ = (uint8_t*)dmalloc(nb);
    launch_init_raw(embd_raw_, (int64_t)(nb / block_bytes(embd_type_)), embd_type_, 1.0f, seed ^ 0xE3BD, stream_);
    weight_bytes_ += nb;
  }
  if (spec_.last()) {
    out_norm_ = upload_f32(ones.data(), d);
    out_ = alloc_packed_random(t0.out, cfg_.vocab, d, seed ^ 0x0F7);
  }
  HIP_OK(hipStreamSynchronize(stream_));
}

// int8_gemm: an int8 copy of every quantized projection (K15; the wide GEMMs then run gemm3<P_I8>):
// each matrix is unpacked to dense f16 in a temporary buffer and re-quantized per row
void HipStage::build_i8_copies() {
  auto each = [&](const std::function<void(PackedMat&)>& f) {
    for (LayerW& L : layers_) {
      if (L.moe) continue;
      for (MatSeg& sg : L.qkv) f(sg.m);
      f(L.wo);
      if (L.fused_gateup) f(L.gateup);
      else { f(L.gate); f(L.up); }
      f(L.down);
    }
  };
  size_t maxe = 0;
  each([&](PackedMat& m) {
    if (m.d && !is16(m.ptype)) maxe = std::max(maxe, (size_t)m.dims.ntiles * 16 * m.dims.nsb * 256);
  });
  if (!maxe) return;
  f16* tmp = nullptr;
  HIP_OK(hipMalloc(&tmp, maxe * 2));
  size_t bytes = 0;
  each([&](PackedMat& m) {
    if (!m.d || is16(m.ptype)) return;
    const int nt = (int)m.dims.ntiles, nsb = (int)m.dims.nsb;
    launch_unpack(m.ptype, m.d, nt, nsb, tmp, nsb * 256, stream_);
    m.i8 = (uint8_t*)dmalloc((size_t)nt * nsb * 4096);
    m.i8_ws = (float*)dmalloc((size_t)nt * 16 * 4);
    launch_requant_i8(tmp, nsb * 256, (int)m.dims.N, nt * 16, nsb, m.i8, m.i8_ws, stream_);
    bytes += (size_t)nt * nsb * 4096;
  });
  HIP_OK(hipStreamSynchronize(stream_));
  HIP_OK(hipFree(tmp));
  weight_bytes_ += bytes;
  MP_LOGI("stage %d: int8_gemm: %.2f GiB of per-row int8 weight copies", spec_.stage, bytes / 1073741824.0);
}

void HipStage::alloc_runtime() {
  HIP_OK(hipSetDevice(spec_.device));
  if (opt_.int8_gemm && opt_.prefill_gemm) build_i8_copies();
  // MoE routers as dense f16 (E x d x 2 B per layer: 64 KB at Mixtral): the router-logits kernel
  // reads them row-major, one launch of M / 4 workgroups for any micro-batch width
  for (LayerW& L : layers_) {
    if (!L.moe || !L.ex.router.d) continue;
    const PackedMat& r = L.ex.router;
    const size_t bytes = (size_t)r.dims.ntiles * 16 * r.dims.nsb * 256 * 2;
    L.ex.router_dense = (f16*)dmalloc(bytes);
    launch_unpack(r.ptype, r.d, (int)r.dims.ntiles, (int)r.dims.nsb, L.ex.router_dense, (int)r.dims.nsb * 256, stream_);
    weight_bytes_ += bytes;
  }
  HIP_OK(hipStreamSynchronize(stream_));
  const int B = opt_.mb_size, NM = opt_.n_mb;
  const int d = cfg_.d_model, Hq = cfg_.n_head, Hkv = cfg_.n_head_kv;
  scratch_rows_ = std::max(B, opt_.prefill_chunk);
  act_rows_ = scratch_rows_;
  auto zalloc = [&](size_t bytes) {
    void* p = dmalloc(bytes);
    HIP_OK(hipMemset(p, 0, bytes));
    return p;
  };
  xn_ = (f16*)zalloc((size_t)scratch_rows_ * Kd_ * 2);
  if (opt_.int8_gemm && opt_.prefill_gemm && std::max(B, opt_.prefill_chunk) > 64) {
    xq_ld_ = std::max({Kd_, Ko_, Kff_});
    xq_ = (int8_t*)zalloc((size_t)scratch_rows_ * xq_ld_);
    xqs_ = (float*)zalloc((size_t)scratch_rows_ * 4);
  }
  attn_ = (f16*)zalloc((size_t)scratch_rows_ * Ko_ * 2);
  h_ = (f16*)zalloc((size_t)scratch_rows_ * Kff_ * 2);
  // [64 floats: per-row sum of squares of the deferred qkv RMSNorm][rows][q|k|v] f32 split-K
  // accumulator; one contiguous range so the o-proj's zero side job clears both
  ssq_ = (float*)zalloc((64 + (size_t)scratch_rows_ * qkv_n_) * 4);
  qkv_ = ssq_ + 64;
  q_ = (f16*)zalloc((size_t)scratch_rows_ * Hq * Dp_ * 2);
  bool any_unfused = false;
  for (auto& L : layers_) any_unfused |= !L.fused_gateup;
  if (any_unfused) gu_ = (float*)zalloc((size_t)scratch_rows_ * 2 * cfg_.d_ff * 4);
  if (cfg_.n_expert) {
    if (cfg_.n_expert > 128 || cfg_.n_expert_used > 8 || cfg_.n_expert_used < 1 || cfg_.n_expert_used > cfg_.n_expert)
      throw std::runtime_error("MoE: need n_expert <= 128 and 1 <= n_expert_used <= min(8, n_expert)");
    const int k = cfg_.n_expert_used;
    // logits row stride: 64 up to 64 experts (moe_route_kernel), 128 above (moe_router_kernel)
    moe_ld_ = (int)round_up(cfg_.n_expert, 64);
    moe_logits_ = (float*)zalloc((size_t)scratch_rows_ * moe_ld_ * 4);
    moe_counts_ = (int32_t*)zalloc((size_t)moe_ld_ * 4);
    if (cfg_.n_expert > 64) moe_sel_ = (int32_t*)zalloc((size_t)scratch_rows_ * k * 4);
    moe_lists_ = (int32_t*)zalloc((size_t)cfg_.n_expert * scratch_rows_ * k * 4);
    moe_w_ = (float*)zalloc((size_t)scratch_rows_ * k * 4);
    moe_h_ = (f16*)zalloc((size_t)scratch_rows_ * k * Kff_ * 2);
    if (opt_.deterministic) moe_yslot_ = (float*)zalloc((size_t)std::min(scratch_rows_, 64) * k * cfg_.d_model * 4);
  }
  int split = opt_.attn_split_len;
  if (split <= 0) {
    // auto: enough (sequence, kv head, split) workgroups to cover the CUs, but >= 256 keys per
    // split (a split merge costs a publish/acquire round trip; short contexts use one split)
    const int target = knob(KNOB_ATTN_WG_TARGET);
    const int pairs = std::max(1, B * Hkv);
    const int want = std::max(1, std::min((target + pairs - 1) / pairs, (opt_.max_ctx + 255) / 256));
    split = (opt_.max_ctx + want - 1) / want;
  }
  split = std::max(128, (int)round_up(split, 128));
  // the fused decode attention merges at most 128 splits per (token, kv head) in LDS
  split = std::max(split, (int)round_up((opt_.max_ctx + 127) / 128, 128));
  opt_.attn_split_len = split;
  n_split_ = (int)((opt_.max_ctx + split - 1) / split);
  if (n_split_ > 1) {
    o_part_ = (float*)zalloc((size_t)n_split_ * B * Hq * Dp_ * 4);
    ml_part_ = (float*)zalloc((size_t)n_split_ * B * Hq * 2 * 4);
  }
  attn_cnt_ = (int32_t*)zalloc((size_t)std::max(B, 16) * Hkv * 4);
  if (opt_.prefill_flash && opt_.max_ctx > 256) {   // prefill KV-split partials (attn_prefill.hip)
    pf_opart_ = (float*)zalloc((size_t)kPrefillMaxSplit * opt_.prefill_chunk * Hq * Dp_ * 4);
    pf_ml_ = (float*)zalloc((size_t)kPrefillMaxSplit * opt_.prefill_chunk * Hq * 2 * 4);
  }
  {
    // stored split-K partials, the largest any ATOMIC projection's route asks for (mat_route): sk_part_
    // for the M > 64 GEMMs (decode micro-batches and prompt chunks wider than 64 rows; a chunk of
    // another width that needs more runs split-K with atomics), det_part_ for the fixed-order GEMV
    // splits of the deterministic mode (<= 64 rows per call)
    auto acc = [&](const PackedMat& m) {
      if (!m.d) return;
      for (int M = 1; M <= std::max(opt_.mb_size, opt_.prefill_chunk); ++M) {
        if (M > 64 && M != opt_.mb_size && M != opt_.prefill_chunk) continue;
        const MatRoute r = mat_route(MatCall(m, EPI_ATOMIC, M).in(xn_, Kd_).split(), SIZE_MAX);
        size_t& need = r.family == GemmRoute::GEMM4 ? sk_part_n_ : det_part_n_;
        need = std::max(need, r.part_n);
      }
    };
    for (const LayerW& L : layers_) {
      for (const MatSeg& sg : L.qkv) acc(sg.m);
      acc(L.wo);
      acc(L.down);
      if (L.moe) acc(L.ex.router);
    }
    if (sk_part_n_) sk_part_ = (float*)dmalloc(sk_part_n_ * 4);
    if (det_part_n_) det_part_ = (float*)zalloc(det_part_n_ * 4);
  }
  // KV cache: a pool of kv_pages 64-token pages per layer + one TRASH page (id kv_pages) that
  // unmapped block-table entries point at (idle rows of a micro-batch still append K/V); the engine's
  // KvPager installs the table (set_block_table)
  const int n_slots = NM * B;
  max_pages_ = opt_.max_ctx / 64;
  n_pages_ = opt_.kv_pages > 0 ? opt_.kv_pages : n_slots * max_pages_;
  const size_t per = (size_t)(n_pages_ + 1) * Hkv * 64 * Dp_ * kv_eb();
  for (size_t i = 0; i < layers_.size(); ++i) {
    kc_.push_back((f16*)zalloc(per));
    vc_.push_back((f16*)zalloc(per));
    kv_bytes_ += 2 * per;
  }
  host_bt_.assign((size_t)n_slots * max_pages_, n_pages_);
  block_table_ = (int32_t*)dmalloc(host_bt_.size() * 4);
  HIP_OK(hipMemcpy(block_table_, host_bt_.data(), host_bt_.size() * 4, hipMemcpyHostToDevice));
  // RoPE table (NORM mode), Llama-3.1 frequency factors if present
  const int hd2 = cfg_.head_dim / 2;
  std::vector<float2> cs((size_t)opt_.max_ctx * hd2);
  for (int i = 0; i < hd2; ++i) {
    double inv = std::pow((double)cfg_.rope_base, -2.0 * i / cfg_.head_dim);
    if (!rope_ff_.empty()) inv /= rope_ff_[i];
    for (int p = 0; p < opt_.max_ctx; ++p) {
      const double a = p * inv;
      cs[(size_t)p * hd2 + i] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
  }
  rope_cs_ = (float2*)dmalloc(cs.size() * sizeof(float2));
  HIP_OK(hipMemcpy(rope_cs_, cs.data(), cs.size() * sizeof(float2), hipMemcpyHostToDevice));
  // per micro-batch I/O
  for (int mb = 0; mb < NM; ++mb) {
    act_.push_back((float*)zalloc((size_t)act_rows_ * d * 4));
    tok_.push_back((int32_t*)zalloc(std::max(B, 16) * 4));
    pos_.push_back((int32_t*)zalloc(std::max(B, 16) * 4));
    kvlen_.push_back((int32_t*)zalloc(std::max(B, 16) * 4));
    std::vector<int32_t> sl(std::max(B, 16), 0);
    for (int b = 0; b < B; ++b) sl[b] = slot_of(mb, b);
    int32_t* sd = (int32_t*)dmalloc(sl.size() * 4);
    HIP_OK(hipMemcpy(sd, sl.data(), sl.size() * 4, hipMemcpyHostToDevice));
    slot_.push_back(sd);
  }
  step_ = (int32_t*)zalloc(16);
  pf_pos_ = (int32_t*)zalloc((size_t)opt_.prefill_chunk * 4);
  pf_kvlen_ = (int32_t*)zalloc((size_t)opt_.prefill_chunk * 4);
  pf_slot_ = (int32_t*)zalloc((size_t)opt_.prefill_chunk * 4);
  prompt_dev_ = (int32_t*)zalloc((size_t)n_slots * opt_.max_ctx * 4);
  if (opt_.row_masks && !opt_.row_sampling) throw std::runtime_error("row_masks needs row_sampling");
  if (spec_.last()) head_ = std::make_unique<HipHead>(*this);
  if (lora_on()) lora_ = std::make_unique<HipLora>(*this, (int)layers_.size(), scratch_rows_);
  HIP_OK(hipDeviceSynchronize());
  MP_LOGI("stage %d: layers %d-%d offloaded to GPU %d (%s), weights %.2f GiB, KV %.2f GiB (%d pages of 64 tokens; "
          "%d slots x <= %d ctx)",
          spec_.stage, spec_.layer_begin, spec_.layer_end - 1, spec_.device,
          spec_.first() && spec_.last() ? "embd+head" : spec_.first() ? "embd" : spec_.last() ? "head" : "mid",
          weight_bytes_ / 1073741824.0, kv_bytes_ / 1073741824.0, n_pages_, n_slots, opt_.max_ctx);
}

void HipStage::set_positions(int mb, const std::vector<int32_t>& pos) {
  HIP_OK(hipSetDevice(spec_.device));
  std::vector<int32_t> p(std::max(opt_.mb_size, 16), 0), k(std::max(opt_.mb_size, 16), 1);
  for (size_t i = 0; i < pos.size() && i < p.size(); ++i) { p[i] = pos[i]; k[i] = pos[i] + 1; }
  HIP_OK(hipMemcpyAsync(pos_[mb], p.data(), p.size() * 4, hipMemcpyHostToDevice, stream_));
  HIP_OK(hipMemcpyAsync(kvlen_[mb], k.data(), k.size() * 4, hipMemcpyHostToDevice, stream_));
  HIP_OK(hipStreamSynchronize(stream_));
}

void HipStage::set_block_table(const std::vector<int32_t>& t) {
  if (t.size() != host_bt_.size()) throw std::runtime_error("set_block_table: size mismatch");
  for (int32_t e : t)
    if (e < 0 || e > n_pages_) throw std::runtime_error("set_block_table: page id out of range");
  HIP_OK(hipSetDevice(spec_.device));
  HIP_OK(hipStreamSynchronize(stream_));   // no launch may still read the old table
  host_bt_ = t;
  HIP_OK(hipMemcpy(block_table_, host_bt_.data(), host_bt_.size() * 4, hipMemcpyHostToDevice));
}

// Context shift: the new table, then one launch_kv_shift per layer (and per kKvShiftMaxRec records)
// on the stage's stream.  Plain launches outside the captured decode graphs, which read the table
// and the positions from device memory: nothing is re-captured.
void HipStage::kv_shift(const std::vector<KvShiftRec>& recs, const std::vector<int32_t>& table) {
  set_block_table(table);   // synchronises the stream first
  KvShiftParams p{};
  p.block_table = block_table_; p.max_pages = max_pages_; p.n_slots = opt_.n_mb * opt_.mb_size; p.n_pages = n_pages_;
  p.Hkv = cfg_.n_head_kv; p.hd = cfg_.head_dim; p.Dp = Dp_; p.kv_fp8 = opt_.kv_fp8 ? 1 : 0;
  set_v_strides(p.v_kb, p.v_d);
  p.rope_cs = rope_cs_; p.rope_rows = opt_.max_ctx;
  for (size_t r0 = 0; r0 < recs.size(); r0 += kKvShiftMaxRec) {
    p.n_rec = (int)std::min(recs.size() - r0, (size_t)kKvShiftMaxRec);
    std::copy(recs.begin() + r0, recs.begin() + r0 + p.n_rec, p.rec);
    for (size_t li = 0; li < layers_.size(); ++li) {
      p.k_cache = kc_[li]; p.v_cache = vc_[li];
      launch_kv_shift(p, stream_);
    }
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(stream_));
}

// KV of one slot: per layer the first ceil(n_tok / 64) pages of K, then of V, each page
// [Hkv][64][Dp] (K) / [Hkv][Dp][64] (V) f16 (or e4m3 bytes), located through the slot's block-table row.
// The state holds V pages as V^T [Dp][64] whatever the stage's layout: a v_blocked stage permutes
// them on the host ([8][Dp][8] <-> [Dp][8][8], 8-key runs moved whole), so state moves between builds
// and layouts.
void HipStage::v_page_permute(const uint8_t* src, uint8_t* dst, bool to_state) const {
  const size_t run = 8 * kv_eb();   // 8 consecutive keys of one dim
  for (int h = 0; h < cfg_.n_head_kv; ++h) {
    const size_t hb = (size_t)h * Dp_ * 64 * kv_eb();
    for (int kb = 0; kb < 8; ++kb)
      for (int d = 0; d < Dp_; ++d) {
        const size_t blocked = hb + ((size_t)kb * Dp_ + d) * run, state = hb + ((size_t)d * 8 + kb) * run;
        if (to_state) memcpy(dst + state, src + blocked, run);
        else memcpy(dst + blocked, src + state, run);
      }
  }
}

size_t HipStage::kv_state_bytes(int n_tok) const {
  const size_t page = (size_t)cfg_.n_head_kv * 64 * Dp_ * kv_eb();
  return kc_.size() * 2 * (size_t)((n_tok + 63) / 64) * page;
}

void HipStage::kv_export(int slot, int n_tok, std::vector<uint8_t>& out) {
  HIP_OK(hipSetDevice(spec_.device));
  const size_t page = (size_t)cfg_.n_head_kv * 64 * Dp_ * kv_eb();
  const int np = (n_tok + 63) / 64;
  const size_t base = out.size();
  out.resize(base + kv_state_bytes(n_tok));
  uint8_t* dst = out.data() + base;
  std::vector<uint8_t> tmp(opt_.v_blocked ? page : 0);
  HIP_OK(hipStreamSynchronize(stream_));
  for (size_t li = 0; li < kc_.size(); ++li)
    for (f16* c : {kc_[li], vc_[li]})
      for (int k = 0; k < np; ++k) {
        const int32_t pg = host_bt_[(size_t)slot * max_pages_ + k];
        if (pg >= n_pages_) throw std::runtime_error("kv_export: slot has no page for its tokens");
        const uint8_t* src = reinterpret_cast<const uint8_t*>(c) + (size_t)pg * page;
        if (opt_.v_blocked && c == vc_[li]) {
          HIP_OK(hipMemcpy(tmp.data(), src, page, hipMemcpyDeviceToHost));
          v_page_permute(tmp.data(), dst, true);
        } else {
          HIP_OK(hipMemcpy(dst, src, page, hipMemcpyDeviceToHost));
        }
        dst += page;
      }
}

void HipStage::kv_import(int slot, int n_tok, const uint8_t* data, size_t bytes) {
  if (bytes != kv_state_bytes(n_tok)) throw std::runtime_error("kv_import: size mismatch");
  HIP_OK(hipSetDevice(spec_.device));
  const size_t page = (size_t)cfg_.n_head_kv * 64 * Dp_ * kv_eb();
  const int np = (n_tok + 63) / 64;
  std::vector<uint8_t> tmp(opt_.v_blocked ? page : 0);
  HIP_OK(hipStreamSynchronize(stream_));
  for (size_t li = 0; li < kc_.size(); ++li)
    for (f16* c : {kc_[li], vc_[li]})
      for (int k = 0; k < np; ++k) {
        const int32_t pg = host_bt_[(size_t)slot * max_pages_ + k];
        if (pg >= n_pages_) throw std::runtime_error("kv_import: slot has no page for its tokens");
        uint8_t* dstp = reinterpret_cast<uint8_t*>(c) + (size_t)pg * page;
        if (opt_.v_blocked && c == vc_[li]) {
          v_page_permute(data, tmp.data(), false);
          HIP_OK(hipMemcpy(dstp, tmp.data(), page, hipMemcpyHostToDevice));
        } else {
          HIP_OK(hipMemcpy(dstp, data, page, hipMemcpyHostToDevice));
        }
        data += page;
      }
}

uint64_t HipStage::sample_step() {
  HIP_OK(hipSetDevice(spec_.device));
  HIP_OK(hipStreamSynchronize(stream_));
  int32_t v = 0;
  HIP_OK(hipMemcpy(&v, step_, 4, hipMemcpyDeviceToHost));
  return (uint64_t)(uint32_t)v;
}

void HipStage::set_sample_step(uint64_t s) {
  HIP_OK(hipSetDevice(spec_.device));
  const int32_t v = (int32_t)s;
  HIP_OK(hipMemcpy(step_, &v, 4, hipMemcpyHostToDevice));
}

void HipStage::set_sampling(float temp, int top_k, float top_p, float min_p, uint64_t seed) {
  const bool changed = temp != temp_ || top_k != top_k_ || top_p != top_p_ || min_p != min_p_ || seed != seed_;
  Stage::set_sampling(temp, top_k, top_p, min_p, seed);
  if (changed && !graphs_.empty() && head_) capture_graphs();
}

void HipStage::set_penalties(int last_n, float repeat, float freq, float presence) {
  const bool changed = last_n != pen_last_n_ || repeat != pen_repeat_ || freq != pen_freq_ || presence != pen_presence_;
  Stage::set_penalties(last_n, repeat, freq, presence);
  if (!head_) return;
  head_->ensure_hist();
  head_->ensure_logprob();
  if (changed && !graphs_.empty()) capture_graphs();
}

void HipStage::set_n_probs(int n) {
  if (n < -1 || n > kMaxProbs) throw std::runtime_error("n_probs must be -1 (chosen token only) or 0.." + std::to_string(kMaxProbs));
  const bool changed = n != n_probs_;
  n_probs_ = n;
  if (!head_) return;
  head_->ensure_logprob();
  if (changed && !graphs_.empty()) capture_graphs();
}

// ---- the head's state (hip_head.h): setters are no-ops on a stage without one, reads throw
HipHead& HipStage::need_head(const char* what) const {
  if (!head_) throw std::runtime_error(what);
  return *head_;
}
const float* HipStage::logits_ptr() const { return head_ ? head_->logits() : nullptr; }
int HipStage::logits_ld() const { return head_ ? head_->logits_ld() : 0; }
const void* HipStage::logprob_rec(int mb) const { return head_ ? head_->logprob_rec(mb) : nullptr; }
void HipStage::set_history(int mb, const std::vector<std::vector<int32_t>>& seqs) { if (head_) head_->set_history(mb, seqs); }
void HipStage::set_row_sampling(int mb, int row, const RowSampling& r) { if (head_) head_->set_row_sampling(mb, row, r); }
void HipStage::set_row_draws(int mb, const std::vector<int32_t>& draws) { if (head_) head_->set_row_draws(mb, draws); }
void HipStage::set_row_masks(const std::vector<int>& slots, const uint32_t* const* bits) { if (head_) head_->set_row_masks(slots, bits); }
void HipStage::set_score_targets(int mb, const int32_t* host, int n, int top_n) { if (head_) head_->set_score_targets(mb, host, n, top_n); }
void HipStage::copy_scores(int mb, int n, float* target_lp, int32_t* top_id, float* top_lp) {
  need_head("no scores").copy_scores(mb, n, target_lp, top_id, top_lp);
}
void HipStage::copy_verify_tokens(int mb, int32_t* host, int n) { need_head("no verify tokens").copy_verify_tokens(mb, host, n); }
void HipStage::copy_embeddings(const std::vector<int>& slots, float* host) { need_head("no embeddings").copy_embeddings(slots, host); }
void HipStage::copy_token_embeddings(int mb, int n_rows, float* host) {
  need_head("no token embeddings").copy_token_embeddings(mb, n_rows, host);
}

// ---- LoRA adapters (hip_lora.h); without opt_.lora_adapters the Stage defaults throw
size_t HipStage::load_adapter(int id, const GgufFile& f) {
  if (!lora_) return Stage::load_adapter(id, f);
  const size_t bytes = lora_->load_adapter(id, f);
  weight_bytes_ += bytes;
  return bytes;
}
void HipStage::unload_adapter(int id) {
  if (!lora_) return Stage::unload_adapter(id);
  weight_bytes_ -= lora_->unload_adapter(id);
}
void HipStage::set_row_adapters(const std::vector<int>& slots, const std::vector<int>& ids, const std::vector<float>& scales) {
  if (!lora_) return Stage::set_row_adapters(slots, ids, scales);
  lora_->set_row_adapters(slots, ids, scales);
}

// The kernel family of a projection call.  c.small (M <= 4): gemvs, unless its LDS plan overflows:
// deterministic mode cannot split K over grid.y, so a wide K (70B down: 28672) with M >= 3 rows
// overflows LDS and takes the v2 GEMV with its fixed-order split-K reduction instead.
// Up to 64 rows (decode micro-batches, short prompt chunks): the dequant GEMV.  Above: gemm4 for the
// types it takes, gemm3 for 16-bit weights, the 64 x 64 GEMM for the rest (Q4_0) -- except its wide
// gate/up (>= 192 workgroups of 16 tiles), which the two-tile GEMV beats per 64 rows
// (profiles/r1g_prefill_gemm_vs_gemv.txt).  How the selection got here: docs/PERFORMANCE.md, 3.1.
HipStage::GemmRoute HipStage::gemm_route(const MatCall& c) const {
  const PackedMat& m = *c.m;
  if (c.small) {
    const GemvsPlan pl = plan_gemvs((int)m.dims.ntiles, (int)m.dims.nsb, c.M, c.epi, false, opt_.deterministic);
    if (c.Xf || pl.lds + (size_t)pl.sb_per_split * 64 <= 150 * 1024) return GemmRoute::GEMVS;   // (+ the single-row form's table)
  }
  if (c.M <= 64 || !opt_.prefill_gemm) return GemmRoute::GEMV;
  if (m.i8 && xq_ && c.X) return GemmRoute::I8;
  const int gv = opt_.prefill_gemm_v == 2 ? 4 : opt_.prefill_gemm_v != 0 ? opt_.prefill_gemm_v : is16(m.ptype) ? 3 : 4;
  if (gv == 4 && gemm4_supported(m.ptype)) return GemmRoute::GEMM4;
  if (gv == 3) return GemmRoute::GEMM3;
  const bool wide_swiglu = c.epi == EPI_SWIGLU && m.dims.ntiles / 16 >= 192;
  return wide_swiglu ? GemmRoute::GEMV : GemmRoute::GEMM1;
}

HipStage::MatRoute HipStage::mat_route(const MatCall& c, size_t sk_cap) const {
  const int nt = (int)c.m->dims.ntiles, nsb = (int)c.m->dims.nsb;
  MatRoute r;
  r.family = gemm_route(c);
  if (r.family == GemmRoute::GEMM4) {
    // split-K shapes store per-split partials while they fit sk_cap floats; the rest run whole-K or,
    // outside the deterministic mode, split with atomics
    const bool want = opt_.gemm_splitk_store && c.epi == EPI_ATOMIC && c.allow_split;
    auto plan = [&](bool store) {
      return plan_gemm4(c.m->ptype, c.epi, c.M, nt, nsb, store || (c.allow_split && !opt_.deterministic), store);
    };
    r.g4 = plan(want);
    r.part_n = want && r.g4.ok ? (size_t)r.g4.nsplit * c.M * nt * 16 : 0;
    r.store = r.part_n && r.part_n <= sk_cap;
    if (!r.store) r.part_n = 0;
    if (want && !r.store) r.g4 = plan(false);
  } else if (r.family == GemmRoute::GEMV && c.M <= 64) {   // (wider calls run as 64-row slices, each routed)
    r.ns = c.allow_split ? gemv_auto_split(nt, nsb, c.M, c.epi) : 1;
    if (opt_.deterministic && c.epi == EPI_ATOMIC && c.allow_split) {
      // fixed order: the split count launch_gemv will actually use (its rounding reproduced)
      const int per = (nsb + std::max(1, r.ns) - 1) / std::max(1, r.ns), ns = (nsb + per - 1) / per;
      r.det = ns > 1;
      if (r.det) { r.ns = ns; r.part_n = (size_t)ns * c.M * nt * 16; }
    }
  }
  return r;
}

GemvParams HipStage::params(const MatCall& c) const {
  const PackedMat& m = *c.m;
  GemvParams p = gemv_params(m.d, (int)m.dims.ntiles, (int)m.dims.nsb, c.X, c.ldx, c.M, c.Y, c.ldy, c.H, c.ldh, c.n_valid);
  if (c.Xf) { p.Xf = c.Xf; p.ldxf = cfg_.d_model; p.gamma = c.gamma; p.eps = cfg_.eps; p.d_norm = cfg_.d_model; }
  p.bias = c.bias; p.zero = c.zero; p.zero_n = c.zero_n; p.ssq = c.ssq; p.qa = c.qa;
  return p;
}

void HipStage::gemv(const MatCall& c, hipStream_t st) {
  const PackedMat& m = *c.m;
  const MatRoute r = mat_route(c, sk_part_n_);
  const bool init = c.deliver == SplitK::INIT, defer = c.deliver == SplitK::DEFER;
  const bool vec = r.family == GemmRoute::GEMV || r.family == GemmRoute::GEMVS;   // the families with fusions
  // a field the route's kernels do not take is an error, never dropped
  if ((!vec && (c.Xf || c.zero || c.ssq || (c.bias && !(init && r.store)))) || (init && !r.store) ||
      (c.qa.pos && r.family != GemmRoute::GEMVS) || (r.family == GemmRoute::GEMVS && (c.zero || c.ssq)) ||
      (r.family == GemmRoute::GEMV && c.M > 64 && (c.Xf || c.zero)))
    throw std::runtime_error("gemv: the call sets a field its route cannot honour");
  GemvParams p = params(c);
  const bool atomics = c.allow_split && !opt_.deterministic;
  switch (r.family) {
    case GemmRoute::I8: {
      // int8_gemm: x rows quantized per row, int8 MFMA against the re-quantized copy (gemm3<P_I8>)
      if (c.X != xq_src_ || c.M != xq_rows_) {   // not already quantized by norm_x / the previous GEMM on X
        launch_quant_rows_i8(c.X, c.ldx, c.M, p.nsb * 256, xq_, xq_ld_, xqs_, st);
        xq_src_ = c.X;
        xq_rows_ = c.M;
      }
      p.X = reinterpret_cast<const f16*>(xq_); p.ldx = xq_ld_;
      p.W = m.i8; p.xscale = xqs_; p.wscale = m.i8_ws;
      launch_gemm3(P_I8, c.epi, p, st, atomics);
      return;
    }
    case GemmRoute::GEMM4:
      if (!r.g4.ok) throw std::runtime_error("gemv: no gemm4 launch plan for this projection");
      if (!r.store) return run_gemm4(m.ptype, r.g4, c.epi, p, st);
      flush_sk(st);   // sk_part_ is about to be rewritten
      run_gemm4_splitk(m.ptype, r.g4, p, sk_part_, st, !defer, init);
      // (into the residual x: absorbed by the next RMSNorm)
      if (defer) sk_pend_ = SkPending{c.Y, c.M, c.n_valid, c.ldy, r.g4.nsplit, p.ntiles * 16, (int64_t)c.M * p.ntiles * 16};
      return;
    case GemmRoute::GEMM3: return launch_gemm3(m.ptype, c.epi, p, st, atomics);
    case GemmRoute::GEMM1: return launch_gemm(m.ptype, c.epi, p, st);
    case GemmRoute::GEMVS: return launch_gemvs(m.ptype, c.epi, p, opt_.deterministic, st);
    case GemmRoute::GEMV: break;
  }
  if (c.M > 64) {
    for (int r0 = 0; r0 < c.M; r0 += 64) {
      MatCall s = c;
      s.M = std::min(64, c.M - r0);
      s.X = c.X + (size_t)r0 * c.ldx;
      if (c.Y) s.Y = c.Y + (size_t)r0 * c.ldy;
      if (c.H) s.H = c.H + (size_t)r0 * c.ldh;
      gemv(s, st);
    }
    return;
  }
  if (!r.det) return launch_gemv(m.ptype, c.epi, p, r.ns, st);
  // split s stores its partial to det_part_[s]; then one fixed-order reduction adds them into Y
  const int ldp = p.ntiles * 16;
  if (r.part_n > det_part_n_) throw std::runtime_error("deterministic split-K scratch too small");
  GemvParams q = p;
  q.Y = det_part_; q.ldy = ldp; q.split_stride = (int64_t)c.M * ldp;
  launch_gemv(m.ptype, EPI_STORE, q, r.ns, st);
  launch_splitk_reduce(det_part_, r.ns, q.split_stride, ldp, c.M, c.n_valid, c.Y, c.ldy, st);
}

void HipStage::flush_sk(hipStream_t st) {
  if (!sk_pend_.x) return;
  launch_splitk_reduce(sk_part_, sk_pend_.ns, sk_pend_.ss, sk_pend_.ldp, sk_pend_.M, sk_pend_.n, sk_pend_.x, sk_pend_.ldy, st);
  sk_pend_ = SkPending{};
}

void HipStage::norm_x(float* x, const float* w, int M, float* zero, int64_t zero_n, hipStream_t st, const float* bias,
                      int bias_n) {
  const int d = cfg_.d_model;
  const bool pend = sk_pend_.x == x && sk_pend_.M == M && sk_pend_.n == d && sk_pend_.ldy == d;
  // int8_gemm: the wide GEMMs reading xn_ take its int8 rows from this launch (no separate quant)
  const bool q8 = xq_ && M > 64 && M <= scratch_rows_;
  if ((pend || q8) && d <= 8192 && (d & 3) == 0) {
    launch_rmsnorm_acc(x, d, w, d, cfg_.eps, xn_, Kd_, M, zero, zero_n, pend ? sk_part_ : nullptr, sk_pend_.ns,
                       sk_pend_.ss, sk_pend_.ldp, st, bias, bias_n, q8 ? xq_ : nullptr, xq_ld_, q8 ? xqs_ : nullptr);
    if (pend) sk_pend_ = SkPending{};
    xq_src_ = q8 ? (const void*)xn_ : nullptr;
    xq_rows_ = M;
    return;
  }
  flush_sk(st);
  launch_rmsnorm(x, d, w, d, cfg_.eps, xn_, Kd_, M, zero, zero_n, st, bias, bias_n);
  xq_src_ = nullptr;
}

void HipStage::moe_ffn(const LayerW& L, int M, hipStream_t st, float* x) {
  // > 64 tokens (wide decode micro-batches, prompt chunks): ONE grouped GEMM per projection over
  // every routed expert (gemm4.hip MoE mode: each expert's weights read once per call, its rows
  // gathered into 128/256-row MFMA tiles).  The deterministic mode keeps the slices (its per-slot
  // combine buffer holds 64 tokens).
  if (M > 64 && opt_.prefill_gemm && opt_.moe_gemm && !opt_.deterministic && gemm4_supported(L.ex.gateup.ptype) &&
      gemm4_supported(L.ex.down.ptype))
    return moe_ffn_rows(L, 0, M, st, x, true);
  // otherwise slices of <= 64 tokens, so every slice takes the workgroup-shared MoE GEMV (weights
  // streamed once per 64 tokens, not once per 16 routed rows as in v1)
  const bool v1 = knob(KNOB_MOE_V) == 1;
  const int step = v1 ? M : 64;
  for (int r0 = 0; r0 < M; r0 += step) moe_ffn_rows(L, r0, std::min(step, M - r0), st, x);
}

void HipStage::moe_ffn_rows(const LayerW& L, int r0, int M, hipStream_t st, float* x, bool grouped) {
  const int E = cfg_.n_expert, k = cfg_.n_expert_used, d = cfg_.d_model, F = cfg_.d_ff;
  const f16* xn = xn_ + (size_t)r0 * Kd_;
  float* logits = moe_logits_ + (size_t)r0 * moe_ld_;
  MoeRouteParams rp{};
  rp.logits = logits; rp.ld = moe_ld_; rp.M = M; rp.E = E; rp.k = k;
  rp.counts = moe_counts_; rp.lists = moe_lists_; rp.list_cap = scratch_rows_ * k; rp.weights = moe_w_;
  const int Kr = (int)L.ex.router.dims.nsb * 256;
  if (E > 64) {
    // Qwen3-MoE: logits, top-k and lists from the fused router (16 token rows share each router slice)
    if (!L.ex.router_dense || Kd_ < Kr) throw std::runtime_error("moe_ffn: the fused router needs the dense f16 router");
    rp.sel = moe_sel_;
    launch_moe_router(xn, Kd_, L.ex.router_dense, Kr, logits, rp, st);
  } else {
    // router logits [M][E]: one 16-row tile, so split-K over the super-blocks (atomics into the
    // buffer the ffn RMSNorm cleared) instead of one serial workgroup (28.5 us -> a few us per layer)
    if (L.ex.router_dense && Kd_ >= Kr)
      launch_router_logits(xn, Kd_, L.ex.router_dense, Kr, E, M, logits, moe_ld_, st);
    else
      gemv(MatCall(L.ex.router, EPI_ATOMIC, M).in(xn, Kd_).out(logits, moe_ld_, E).split(), st);
    launch_moe_route(rp, st);
  }
  MoeGemvParams gp{};
  gp.W = L.ex.gateup.d; gp.estride = L.ex.gateup_stride;
  gp.ntiles = (int)L.ex.gateup.dims.ntiles; gp.nsb = (int)L.ex.gateup.dims.nsb;
  gp.X = xn; gp.ldx = Kd_; gp.x_per_slot = 0; gp.k = k;
  gp.counts = moe_counts_; gp.lists = moe_lists_; gp.list_cap = rp.list_cap; gp.E = E;
  gp.H = moe_h_; gp.ldh = Kff_; gp.n_valid = F; gp.M = M;
  MoeGemvParams dp = gp;
  dp.W = L.ex.down.d; dp.estride = L.ex.down_stride;
  dp.ntiles = (int)L.ex.down.dims.ntiles; dp.nsb = (int)L.ex.down.dims.nsb;
  dp.X = moe_h_; dp.ldx = Kff_; dp.x_per_slot = 1; dp.H = nullptr; dp.ldh = 0;
  dp.Y = x + (size_t)r0 * d; dp.ldy = d; dp.weights = moe_w_; dp.n_valid = d;
  if (grouped) {
    if (!launch_moe_gemm4(L.ex.gateup.ptype, EPI_SWIGLU, gp, st) || !launch_moe_gemm4(L.ex.down.ptype, EPI_ATOMIC, dp, st))
      throw std::runtime_error("moe_ffn: grouped GEMM does not support the expert weight type");
    return;
  }
  launch_moe_gemv(L.ex.gateup.ptype, EPI_SWIGLU, gp, 1, st);
  if (opt_.deterministic) dp.Yslot = moe_yslot_;   // per-slot outputs, combined in expert-rank order below
  // only ~k/E of the expert grid is busy: size the split for the active experts
  const int active = std::min(E, M * k);
  // v1 (M > 64): one tile per 1-wave workgroup, ~4096 of them; v2: 8-tile workgroups, ~1024 of
  // them across the active experts
  const int nsplit = M <= 64 ? std::max(1, std::min(dp.nsb / 4, 1024 / std::max(1, (dp.ntiles + 7) / 8 * active)))
                             : std::max(1, std::min(dp.nsb / 4, 4096 / std::max(1, dp.ntiles * active)));
  launch_moe_gemv(L.ex.down.ptype, EPI_ATOMIC, dp, nsplit, st);
  if (opt_.deterministic) launch_moe_combine(moe_yslot_, d, k, M, d, x + (size_t)r0 * d, d, st);
}

void HipStage::ffn_tail(const LayerW& L, int M, float* x, bool small, bool fused, hipStream_t st, int li, const Fwd* f) {
  const int d = cfg_.d_model, F = cfg_.d_ff;
  auto up = [&](const PackedMat& m, int epi) {
    MatCall c = MatCall(m, epi, M).gemvs(small);
    return fused ? c.in_norm(x, L.ffn_norm) : c.in(xn_, Kd_);
  };
  if (L.fused_gateup) {
    gemv(up(L.gateup, EPI_SWIGLU).out_h(h_, Kff_, F), st);
  } else {
    gemv(up(L.gate, EPI_STORE).out(gu_, 2 * F, F), st);
    gemv(up(L.up, EPI_STORE).out(gu_ + F, 2 * F, F), st);
    if (lora_on() && f) {   // gate and up are complete f32 rows here, before the SwiGLU consumes them
      const int tg[2] = {LORA_GATE, LORA_UP}, n[2] = {F, F}, off[2] = {0, F};
      lora_->group(li, *f, 2, tg, n, off, xn_, Kd_, d, gu_, 2 * F);
    }
    launch_swiglu(gu_, 2 * F, F, M, h_, Kff_, st);
  }
  // stored partials: absorbed by the next layer's attention norm (or flushed after the last layer)
  gemv(MatCall(L.down, EPI_ATOMIC, M).in(h_, Kff_).out(x, d, d).split(SplitK::DEFER).gemvs(small), st);
  if (lora_on() && f) {   // (pending split-K partials of down and this delta are both plain adds into x, in stream order)
    const int tg[1] = {LORA_DOWN}, n[1] = {d}, off[1] = {0};
    lora_->group(li, *f, 1, tg, n, off, h_, Kff_, F, x, d);
  }
}

void HipStage::layer_forward(int li, float* x, const Fwd& f) {
  const LayerW& L = layers_[li];
  const int d = cfg_.d_model, M = f.M;
  hipStream_t st = f.st;
  // q|k|v segment s from the f16 rows xn_, or (norm) from the residual with the attention norm fused
  auto qkv_seg = [&](const MatSeg& s, int epi, bool norm) {
    MatCall c = MatCall(s.m, epi, M).out(qkv_ + s.y_off, qkv_n_, (int)s.m.dims.N);
    return norm ? c.in_norm(x, L.attn_norm) : c.in(xn_, Kd_);
  };
  const MatCall wo = MatCall(L.wo, EPI_ATOMIC, M).in(attn_, Ko_).out(x, d, d);
  const bool lora = lora_on();
  // LoRA deltas of a group whose base projections have delivered (one shrink + one expand launch)
  auto lora_qkv = [&] {
    const int tg[3] = {LORA_Q, LORA_K, LORA_V}, n[3] = {cfg_.q_dim(), cfg_.kv_dim(), cfg_.kv_dim()};
    const int off[3] = {0, cfg_.q_dim(), cfg_.q_dim() + cfg_.kv_dim()};
    lora_->group(li, f, 3, tg, n, off, xn_, Kd_, d, qkv_, qkv_n_);
  };
  auto lora_o = [&] {
    const int tg[1] = {LORA_O}, n[1] = {d}, off[1] = {0};
    lora_->group(li, f, 1, tg, n, off, attn_, Ko_, cfg_.q_dim(), x, d);
  };
  if (lora && small_path(M)) {
    // the gemvs family on a lora_adapters stage: the adapters read the normed f16 rows, so the norms run
    // standalone into xn_; q|k|v stay complete and un-rotated until the delta is in (no RoPE + append
    // epilogue, no fused attention + o), gate and up unfused (ffn_tail)
    norm_x(x, L.attn_norm, M, nullptr, 0, st);
    for (const MatSeg& s : L.qkv) {
      MatCall c = qkv_seg(s, EPI_STORE, false).gemvs(true);
      c.bias = L.qkv_bias ? L.qkv_bias + s.y_off : nullptr;
      gemv(c, st);
    }
    lora_qkv();
    qk_norm(L, M, st);
    attention(li, f, false, false);
    gemv(MatCall(wo).split().gemvs(true), st);
    lora_o();
    if (L.moe) {
      launch_rmsnorm(x, d, L.ffn_norm, d, cfg_.eps, xn_, Kd_, M, moe_logits_, (int64_t)M * moe_ld_, st);
      xq_src_ = nullptr;
      moe_ffn(L, M, st, x);
    } else {
      norm_x(x, L.ffn_norm, M, nullptr, 0, st);
      ffn_tail(L, M, x, true, false, st, li, &f);
    }
    return;
  }
  if (small_path(M)) {
    // gemvs: RMSNorms fused into the qkv / gate-up GEMVs, complete outputs per workgroup (q|k|v
    // stored with its bias, o / down added into the residual by their single owner)
    const bool two = knob(KNOB_GEMVS2) != 0;
    // decode: RoPE and the KV append in the qkv GEMV's epilogue (QkvAppend), so the attention starts
    // from rotated q and a complete cache (no dependent position -> page -> append chain of its own)
    // (a q/k-normed layer needs the complete projection before the rotation: no QkvAppend)
    const bool pre = f.decode && opt_.fused_attn && knob(KNOB_ATTN_PRE) && !opt_.deterministic && !L.q_norm &&
                     attn_decode_pre_ok(decode_attn_params(li, f, false));
    auto seg = [&](const MatSeg& s) {
      MatCall c = qkv_seg(s, EPI_STORE, true).gemvs(true);
      c.bias = L.qkv_bias ? L.qkv_bias + s.y_off : nullptr;
      if (pre) {
        c.qa.pos = f.pos; c.qa.slot0 = f.slot0; c.qa.block_table = block_table_; c.qa.max_pages = max_pages_;
        c.qa.rope_cs = rope_cs_; c.qa.k_cache = kc_[li]; c.qa.v_cache = vc_[li]; c.qa.col0 = (int)s.y_off;
        c.qa.Hq = cfg_.n_head; c.qa.Hkv = cfg_.n_head_kv; c.qa.hd = cfg_.head_dim; c.qa.Dp = Dp_; c.qa.kv_fp8 = opt_.kv_fp8;
        set_v_strides(c.qa.v_kb, c.qa.v_d);
      }
      return c;
    };
    const int first = L.qkv.size() == 2 && gemvs2_supported(L.qkv[1].m.ptype, L.qkv[0].m.ptype) ? 1 : 0;
    if (two && L.qkv.size() == 2 && gemvs2_supported(L.qkv[first].m.ptype, L.qkv[1 - first].m.ptype) &&
        L.qkv[0].m.dims.nsb == L.qkv[1].m.dims.nsb) {
      // mixed-type q+k | v (Q4_K_M's Q6_K attn_v): both segments in one launch
      launch_gemvs2(L.qkv[first].m.ptype, L.qkv[1 - first].m.ptype, params(seg(L.qkv[first])),
                    params(seg(L.qkv[1 - first])), st);
    } else {
      for (const MatSeg& s : L.qkv) gemv(seg(s), st);
    }
    qk_norm(L, M, st);
    if (!(f.decode && attention_o(li, f, x, pre))) {
      attention(li, f, false, pre);
      gemv(MatCall(wo).split().gemvs(true), st);
    }
    if (L.moe) {
      launch_rmsnorm(x, d, L.ffn_norm, d, cfg_.eps, xn_, Kd_, M, moe_logits_, (int64_t)M * moe_ld_, st);
      xq_src_ = nullptr;
      moe_ffn(L, M, st, x);
    } else {
      ffn_tail(L, M, x, true, true, st);
    }
    return;
  }
  // M <= 4 (fuse_norm): the RMSNorms are folded into the consuming GEMVs (gemv2.hip deferred
  // norm).  qkv: the split-K GEMV publishes per-row sums of squares to ssq_ and the fused decode
  // attention applies rsqrt and the bias when it reads q|k|v.  The o-proj then clears ssq_ + the
  // q|k|v accumulator (invariant: zero outside [qkv GEMV, o-proj]; unfused forwards clear it after
  // their last layer).
  const bool small = fuse_norm(M) && !lora;   // (the deferred norm leaves no normed rows for the adapters)
  // (a q/k-normed layer normalises final q|k|v values: it takes the standalone attn_norm; the o-proj's
  // zero side job below still clears the range, so the invariant holds for the next layer)
  const bool qkv_deferred = small && f.decode && opt_.fused_attn && !L.q_norm;
  if (qkv_deferred) {
    for (const MatSeg& s : L.qkv) {
      MatCall c = qkv_seg(s, EPI_ATOMIC, true).split();
      c.ssq = &s == &L.qkv[0] ? ssq_ : nullptr;   // the sums of squares once per row
      gemv(c, st);
    }
  } else {
    // When every qkv segment stores split-K partials, their reductions write q|k|v = bias + partials
    // and the norm launch fills nothing; any other route accumulates onto the zero / bias fill
    int covered = 0;
    bool init = !L.qkv.empty();
    for (const MatSeg& s : L.qkv) {
      init = init && s.y_off == covered && mat_route(qkv_seg(s, EPI_ATOMIC, false).split(), sk_part_n_).store;
      covered += (int)s.m.dims.N;
    }
    init = init && covered == qkv_n_;
    if (init) norm_x(x, L.attn_norm, M, nullptr, 0, st);
    else norm_x(x, L.attn_norm, M, qkv_, (int64_t)M * qkv_n_, st, L.qkv_bias, qkv_n_);
    for (const MatSeg& s : L.qkv) {
      MatCall c = qkv_seg(s, EPI_ATOMIC, false).split(init ? SplitK::INIT : SplitK::ADD);
      if (init && L.qkv_bias) c.bias = L.qkv_bias + s.y_off;
      gemv(c, st);
    }
  }
  if (lora) lora_qkv();   // before the q / k norm and the rotation
  qk_norm(L, M, st);
  attention(li, f, qkv_deferred);
  if (small) {
    MatCall c = MatCall(wo).split();
    c.zero = ssq_; c.zero_n = 64 + (int64_t)M * qkv_n_;
    gemv(c, st);
  } else {
    gemv(MatCall(wo).split(SplitK::DEFER), st);
    if (lora) lora_o();
    if (opt_.fused_norm && li + 1 == (int)layers_.size())
      HIP_OK(hipMemsetAsync(ssq_, 0, (64 + (size_t)M * qkv_n_) * 4, st));
  }
  const bool ffn_fused = small && !L.moe;
  // MoE: the same launch clears the router logits, which the router GEMV then accumulates split-K
  if (!ffn_fused) norm_x(x, L.ffn_norm, M, L.moe ? moe_logits_ : nullptr, L.moe ? (int64_t)M * moe_ld_ : 0, st);
  if (L.moe) moe_ffn(L, M, st, x);
  else ffn_tail(L, M, x, false, ffn_fused, st, li, &f);
}

void HipStage::qk_norm(const LayerW& L, int M, hipStream_t st) {
  if (!L.q_norm) return;
  QkNormParams p{};
  p.qkv = qkv_; p.ldqkv = qkv_n_; p.M = M; p.Hq = cfg_.n_head; p.Hkv = cfg_.n_head_kv; p.hd = cfg_.head_dim;
  p.wq = L.q_norm; p.wk = L.k_norm; p.eps = cfg_.eps;
  launch_qk_norm(p, st);
}

// single-stream decode: attention + o-projection in one launch (attention.hip attn_o_kernel) while
// the context is short enough for every workgroup of a kv head to compute that head's attention
// itself; false: the caller runs the two-kernel path
bool HipStage::attention_o(int li, const Fwd& f, float* x, bool pre) {
  const LayerW& L = layers_[li];
  if (!opt_.fused_attn || opt_.deterministic || opt_.attn_o_max_ctx <= 0 || opt_.max_ctx > opt_.attn_o_max_ctx)
    return false;
  // one split over the whole context (every workgroup of a kv head runs that head's attention)
  DecodeAttnParams dp = decode_attn_params(li, f, false);
  dp.split_len = (int)round_up(opt_.max_ctx, 128); dp.n_split = 1;
  dp.pre = pre;   // q rotated and K / V appended by the qkv GEMV
  AttnOParams op{};
  op.W = L.wo.d; op.ptype = L.wo.ptype; op.ntiles = (int)L.wo.dims.ntiles; op.nsb = (int)L.wo.dims.nsb;
  op.Y = x; op.ldy = cfg_.d_model; op.n_valid = cfg_.d_model;
  if (!attn_o_supported(dp, op)) return false;
  launch_attn_o(dp, op, f.st);
  return true;
}

// the fused decode attention's parameters for layer li (decode rows: slots f.slot0 + t)
DecodeAttnParams HipStage::decode_attn_params(int li, const Fwd& f, bool qkv_deferred) const {
  const LayerW& L = layers_[li];
  DecodeAttnParams dp{};
  dp.qkv = qkv_; dp.ldqkv = qkv_n_; dp.pos = f.pos; dp.slot = f.slot; dp.block_table = block_table_;
  dp.slot0 = f.slot0;
  dp.max_pages = max_pages_; dp.rope_cs = rope_cs_; dp.q_scale = 1.0f / std::sqrt((float)cfg_.head_dim);
  dp.k_cache = kc_[li]; dp.v_cache = vc_[li]; dp.M = f.M; dp.Hq = cfg_.n_head; dp.Hkv = cfg_.n_head_kv;
  dp.kv_fp8 = opt_.kv_fp8;
  set_v_strides(dp.v_kb, dp.v_d);
  dp.hd = cfg_.head_dim; dp.Dp = Dp_; dp.split_len = opt_.attn_split_len; dp.n_split = n_split_;
  dp.o_part = o_part_; dp.ml_part = ml_part_; dp.counters = attn_cnt_; dp.out = attn_; dp.ldo = Ko_;
  if (qkv_deferred) { dp.ssq = ssq_; dp.eps = cfg_.eps; dp.d_model = cfg_.d_model; dp.bias = L.qkv_bias; }
  return dp;
}

void HipStage::attention(int li, const Fwd& f, bool qkv_deferred, bool pre) {
  const int M = f.M;
  const int32_t *pos = f.pos, *kvlen = f.kvlen, *slot = f.slot;
  const bool decode = f.decode;
  const std::vector<PrefillSeg>* segs = f.segs;
  hipStream_t st = f.st;
  if (decode && opt_.fused_attn) {
    DecodeAttnParams dp = decode_attn_params(li, f, qkv_deferred);
    dp.pre = pre;
#ifdef MIPIPE_TIMING_PROBES
    dp.probe = knob(KNOB_ATTN_PROBE);
#endif
    launch_attn_decode(dp, st);
  } else {
    RopeKvParams rp{};
    rp.qkv = qkv_; rp.ldqkv = qkv_n_; rp.M = M; rp.Hq = cfg_.n_head; rp.Hkv = cfg_.n_head_kv;
    rp.hd = cfg_.head_dim; rp.Dp = Dp_; rp.pos = pos; rp.slot = slot; rp.block_table = block_table_;
    rp.max_pages = max_pages_; rp.rope_cs = rope_cs_; rp.q_scale = 1.0f / std::sqrt((float)cfg_.head_dim);
    rp.q_out = q_; rp.k_cache = kc_[li]; rp.v_cache = vc_[li]; rp.kv_fp8 = opt_.kv_fp8;
    set_v_strides(rp.v_kb, rp.v_d);
    launch_rope_kv(rp, st);
    if (!decode && opt_.prefill_flash) {
      PrefillAttnParams pa{};
      pa.q = q_; pa.pos = pos; pa.slot = slot; pa.block_table = block_table_; pa.max_pages = max_pages_;
      pa.k_cache = kc_[li]; pa.v_cache = vc_[li]; pa.Hq = cfg_.n_head; pa.Hkv = cfg_.n_head_kv;
      pa.kv_fp8 = opt_.kv_fp8;
      set_v_strides(pa.v_kb, pa.v_d);
      pa.hd = cfg_.head_dim; pa.Dp = Dp_; pa.out = attn_; pa.ldo = Ko_;
      const int bt = prefill_attn_rows_per_tile(cfg_.n_head / cfg_.n_head_kv);
      auto add_rows = [&](int row0, int T) {
        for (int r = 0; r < T; r += bt) {
          if (pa.n_tiles == kPrefillAttnMaxTiles) { launch_attn_prefill(pa, st); pa.n_tiles = 0; }
          pa.tiles[pa.n_tiles++] = (uint32_t)(row0 + r) | ((uint32_t)std::min(bt, T - r) << 16);
        }
      };
      int pages_needed = 0, n_tiles = 0;
      if (segs && !segs->empty()) {
        for (const PrefillSeg& sg : *segs) {
          pages_needed = std::max(pages_needed, (sg.p0 + sg.T - 1) / 64 + 1);
          n_tiles += (sg.T + bt - 1) / bt;
        }
      }
      // long contexts: split every tile's pages over grid.z so the chunk fills the CUs; the LSE
      // merge runs in the same launcher (one workgroup list per launch, so only when it fits one)
      pa.M = M;
      if (pf_opart_ && n_tiles > 0 && n_tiles <= kPrefillAttnMaxTiles) {
        pa.n_split = prefill_attn_splits(n_tiles, cfg_.n_head_kv, pages_needed, kPrefillMaxSplit, &pa.split_pages);
        pa.o_part = pf_opart_; pa.ml_part = pf_ml_;
      }
      if (segs && !segs->empty()) {
        int row = 0;
        for (const PrefillSeg& sg : *segs) { add_rows(row, sg.T); row += sg.T; }
      } else {
        add_rows(0, M);
      }
      launch_attn_prefill(pa, st);
    } else {
    AttnParams ap{};
    ap.q = q_; ap.kvlen = kvlen; ap.slot = slot; ap.block_table = block_table_; ap.max_pages = max_pages_;
    if (opt_.kv_fp8) throw std::runtime_error("kv_dtype fp8: the unfused attention path reads f16 pages");
    ap.k_cache = kc_[li]; ap.v_cache = vc_[li]; ap.M = M; ap.Hq = cfg_.n_head; ap.Hkv = cfg_.n_head_kv;
    ap.hd = cfg_.head_dim; ap.Dp = Dp_; ap.max_kv = opt_.max_ctx; ap.out = attn_; ap.ldo = Ko_;
    set_v_strides(ap.v_kb, ap.v_d);
    if (decode) {
      ap.tq = 1;
      ap.split_len = opt_.attn_split_len;
      ap.n_split = n_split_;
      ap.o_part = o_part_; ap.ml_part = ml_part_;
    } else {
      const int G = cfg_.n_head / cfg_.n_head_kv;
      ap.tq = std::max(1, 16 / G);
      ap.split_len = (int)round_up(opt_.max_ctx, 128);
      ap.n_split = 1;
    }
    if (!decode && segs && segs->size() > 1) {
      // packed prefill: a row group of the attention kernel must belong to one sequence
      int row = 0;
      for (const PrefillSeg& s : *segs) {
        AttnParams a = ap;
        a.q = q_ + (size_t)row * cfg_.n_head * Dp_;
        a.kvlen = kvlen + row; a.slot = slot + row; a.M = s.T;
        a.out = attn_ + (size_t)row * Ko_;
        launch_attention(a, st);
        row += s.T;
      }
    } else {
      launch_attention(ap, st);
    }
    }
  }
}

bool HipStage::fuse_norm(int M) const { return opt_.fused_norm && M <= 4; }

void HipStage::lm_head(const float* x, int M, float* logits, bool small, hipStream_t st) {
  const int d = cfg_.d_model;
  const MatCall c = MatCall(out_, EPI_STORE, M).out(logits, head_->logits_ld(), cfg_.vocab);
  if (small) return gemv(MatCall(c).in_norm(x, out_norm_).gemvs(true), st);
  // (the LM head keeps the standalone norm: the deferred-norm GEMV variant needs ~50 more VGPRs,
  // which halves the head's occupancy: 90.5 vs 72.7 + 4.6 us at 8B, profiles/r2h_prof_8b_mb1.txt)
  launch_rmsnorm(x, d, out_norm_, d, cfg_.eps, xn_, Kd_, M, nullptr, 0, st);
  xq_src_ = nullptr;
  gemv(MatCall(c).in(xn_, Kd_), st);
}

void HipStage::prefill(int mb, const std::vector<PrefillSeg>& segs, hipStream_t st) {
  const int d = cfg_.d_model;
  float* x = act_[mb];
  int T = 0;
  for (const PrefillSeg& s : segs) {
    if (s.p0 + s.T > opt_.max_ctx) throw std::runtime_error("prompt exceeds context");
    const int sl = slot_of(mb, s.b);
    launch_prefill_meta(pf_pos_ + T, pf_kvlen_ + T, pf_slot_ + T, s.p0, s.T, sl, st);
    if (spec_.first())
      launch_embed(embd_type_, embd_raw_, (int64_t)embd_row_bytes_, d, prompt_dev_ + (size_t)sl * opt_.max_ctx + s.p0,
                   s.T, x + (size_t)T * d, d, st);
    T += s.T;
  }
  if (T > opt_.prefill_chunk) throw std::runtime_error("prefill chunk too large");
  Fwd f{T, pf_pos_, pf_kvlen_, pf_slot_, false, -1, &segs, st};
  if (lora_) lora_->bind_prefill(mb, segs, T, f);
  for (size_t li = 0; li < layers_.size(); ++li) layer_forward((int)li, x, f);
  flush_sk(st);
  if (head_) head_->prefill_chunk(mb, segs, x, T, st);
}

void HipStage::prefill_finish(int mb, hipStream_t st, const std::vector<int>* rows) {
  if (head_) head_->prefill_finish(mb, tok_[mb], st, rows);
}

void HipStage::decode_eager(int mb, hipStream_t st) {
  const int B = opt_.mb_size;
  float* x = act_[mb];
  if (spec_.first())
    launch_embed(embd_type_, embd_raw_, (int64_t)embd_row_bytes_, cfg_.d_model, tok_[mb], B, x, cfg_.d_model, st);
  Fwd f{B, pos_[mb], kvlen_[mb], slot_[mb], true, slot_of(mb, 0), nullptr, st};   // slot_[mb][b] = slot0 + b
  if (lora_) lora_->bind_decode(mb, f);
  for (size_t li = 0; li < layers_.size(); ++li) layer_forward((int)li, x, f);
  flush_sk(st);
  if (head_) head_->run(mb, B, x, tok_[mb], (uint64_t)mb + 1, st, true);
  launch_advance(pos_[mb], kvlen_[mb], B, mb == 0 ? step_ : nullptr, st);
}

void HipStage::capture_graphs() {
  HIP_OK(hipSetDevice(spec_.device));
  destroy_graphs();
  ++graph_captures_;
  if (!opt_.use_graphs) return;
  for (int mb = 0; mb < opt_.n_mb; ++mb) {
    hipGraph_t g;
    HIP_OK(hipStreamBeginCapture(stream_, hipStreamCaptureModeRelaxed));
    decode_eager(mb, stream_);
    HIP_OK(hipStreamEndCapture(stream_, &g));
    hipGraphExec_t ex;
    HIP_OK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    HIP_OK(hipGraphDestroy(g));
    graphs_.push_back(ex);
  }
}

void HipStage::destroy_graphs() {
  for (auto g : graphs_) (void)hipGraphExecDestroy(g);
  graphs_.clear();
}

void HipStage::decode(int mb, hipStream_t st) {
  if (!graphs_.empty()) HIP_OK(hipGraphLaunch(graphs_[mb], st));
  else decode_eager(mb, st);
}

}  // namespace mp
