#include "hip_lora.h"

#include <algorithm>
#include <cstring>

#include "gguf.h"

namespace mp {

HipLora::HipLora(HipStage& stage, int n_layers, int scratch_rows)
    : s_(stage), cfg_(stage.cfg_), opt_(stage.opt_), n_layers_(n_layers) {
  if (opt_.lora_adapters > kLoraMaxAdapters) throw std::runtime_error("lora_adapters: at most " + std::to_string(kLoraMaxAdapters));
  if (opt_.lora_max_rank < 1 || opt_.lora_max_rank > kLoraMaxRank)
    throw std::runtime_error("lora_max_rank must be 1.." + std::to_string(kLoraMaxRank));
  if (cfg_.d_model % 8 || cfg_.q_dim() % 8 || cfg_.d_ff % 8)
    throw std::runtime_error("lora_adapters: d_model, n_head * head_dim and d_ff must be multiples of 8");
  const int cap = opt_.lora_adapters, B = opt_.mb_size, NM = opt_.n_mb;
  ad_.resize(cap);
  rcap_ = lora_rank_pad(opt_.lora_max_rank);
  tgt_host_.assign((size_t)cap * n_layers_ * LORA_N_TARGETS, LoraTargetRec{});
  tgt_ = (LoraTargetRec*)mem_.zero(std::max<size_t>(tgt_host_.size(), 1) * sizeof(LoraTargetRec));
  tiles_dec_ = lora_max_tiles(B, cap);
  const size_t words = lora_table_words(tiles_dec_);
  for (int mb = 0; mb < NM; ++mb) tab_.push_back((int32_t*)mem_.zero(words * 4));
  HIP_OK(hipHostMalloc((void**)&tab_host_, (size_t)NM * words * 4, hipHostMallocDefault));
  std::memset(tab_host_, 0, (size_t)NM * words * 4);
  const int pf_tiles = lora_max_tiles(scratch_rows, cap);
  tab_pf_ = (int32_t*)mem_.zero(lora_table_words(pf_tiles) * 4);
  // the largest group: q|k|v and gate|up read d_model, o reads q_dim, down reads d_ff
  const int mt = std::max(pf_tiles, tiles_dec_);
  part_n_ = std::max({lora_part_floats(mt, cfg_.d_model, 3, rcap_), lora_part_floats(mt, cfg_.q_dim(), 1, rcap_),
                      lora_part_floats(mt, cfg_.d_ff, 1, rcap_)});
  part_ = (float*)mem_.get(part_n_ * 4);
  row_ad_.assign((size_t)NM * B, -1);
  row_sc_.assign((size_t)NM * B, 0.f);
}

HipLora::~HipLora() {
  (void)hipSetDevice(s_.device());
  if (tab_host_) (void)hipHostFree(tab_host_);
  for (LoraDev& a : ad_)
    for (void* p : a.bufs) (void)hipFree(p);
}

size_t HipLora::load_adapter(int id, const GgufFile& f) {
  if (id < 0 || id >= (int)ad_.size() || ad_[id].used) throw std::runtime_error("load_adapter: adapter id " + std::to_string(id) + " is not free");
  const StageSpec& spec = s_.spec();
  const LoraFile lf = lora_read(f, cfg_, opt_.lora_max_rank, spec.layer_begin, spec.layer_end);
  HIP_OK(hipSetDevice(s_.device()));
  LoraDev a;
  std::vector<LoraTargetRec> recs((size_t)n_layers_ * LORA_N_TARGETS);
  try {
    std::vector<uint16_t> A16, B16;
    for (const LoraPair& p : lf.pairs) {
      // the rows of B_q / B_k follow the base q / k rows' NEOX permutation; A reads the un-permuted input
      const bool perm = cfg_.rope_neox && (p.target == LORA_Q || p.target == LORA_K);
      lora_pack_f16(p, perm ? cfg_.head_dim : 0, &A16, &B16);
      void* d[2] = {nullptr, nullptr};
      const std::vector<uint16_t>* h[2] = {&A16, &B16};
      for (int i = 0; i < 2; ++i) {
        HIP_OK(hipMalloc(&d[i], std::max<size_t>(h[i]->size() * 2, 256)));
        a.bufs.push_back(d[i]);
        HIP_OK(hipMemcpy(d[i], h[i]->data(), h[i]->size() * 2, hipMemcpyHostToDevice));
        a.bytes += h[i]->size() * 2;
      }
      LoraTargetRec& r = recs[(size_t)(p.layer - spec.layer_begin) * LORA_N_TARGETS + p.target];
      r.A = d[0]; r.B = d[1]; r.r_pad = lora_rank_pad(p.r);
    }
    HIP_OK(hipStreamSynchronize(s_.stream_));   // no launch may read the table while it changes
    std::copy(recs.begin(), recs.end(), tgt_host_.begin() + (size_t)id * recs.size());
    HIP_OK(hipMemcpy(tgt_ + (size_t)id * recs.size(), recs.data(), recs.size() * sizeof(LoraTargetRec), hipMemcpyHostToDevice));
  } catch (...) {
    for (void* p : a.bufs) (void)hipFree(p);
    throw;
  }
  a.used = true;
  ad_[id] = std::move(a);
  return ad_[id].bytes;
}

size_t HipLora::unload_adapter(int id) {
  if (id < 0 || id >= (int)ad_.size() || !ad_[id].used) throw std::runtime_error("unload_adapter: adapter id " + std::to_string(id) + " is not loaded");
  for (int32_t a : row_ad_)
    if (a == id) throw std::runtime_error("unload_adapter: adapter " + std::to_string(id) + " is bound to a slot");
  HIP_OK(hipSetDevice(s_.device()));
  HIP_OK(hipStreamSynchronize(s_.stream_));
  const size_t n = (size_t)n_layers_ * LORA_N_TARGETS;
  std::fill(tgt_host_.begin() + (size_t)id * n, tgt_host_.begin() + (size_t)(id + 1) * n, LoraTargetRec{});
  HIP_OK(hipMemcpy(tgt_ + (size_t)id * n, tgt_host_.data() + (size_t)id * n, n * sizeof(LoraTargetRec), hipMemcpyHostToDevice));
  for (void* p : ad_[id].bufs) HIP_OK(hipFree(p));
  const size_t bytes = ad_[id].bytes;
  ad_[id] = LoraDev{};
  return bytes;
}

// The tile tables of the micro-batches whose slots changed are rebuilt in the pinned mirror and copied
// on the stage's stream; one synchronisation after the last copy (as HipHead::set_row_masks).
void HipLora::set_row_adapters(const std::vector<int>& slots, const std::vector<int>& ids, const std::vector<float>& scales) {
  if (ids.size() != slots.size() || scales.size() != slots.size()) throw std::runtime_error("set_row_adapters: one id and one scale per slot");
  const int B = opt_.mb_size;
  for (size_t i = 0; i < slots.size(); ++i) {
    if (slots[i] < 0 || slots[i] >= (int)row_ad_.size()) throw std::runtime_error("set_row_adapters: bad slot");
    if (ids[i] < -1 || ids[i] >= (int)ad_.size() || (ids[i] >= 0 && !ad_[ids[i]].used))
      throw std::runtime_error("set_row_adapters: adapter id " + std::to_string(ids[i]) + " is not loaded");
    if (ids[i] >= 0 && !(scales[i] == scales[i] && scales[i] - scales[i] == 0.f)) throw std::runtime_error("set_row_adapters: scale is not finite");
  }
  if (slots.empty()) return;
  std::vector<char> touched(opt_.n_mb, 0);
  for (size_t i = 0; i < slots.size(); ++i) {
    row_ad_[slots[i]] = ids[i];
    row_sc_[slots[i]] = ids[i] >= 0 ? scales[i] : 0.f;
    touched[slots[i] / B] = 1;
  }
  HIP_OK(hipSetDevice(s_.device()));
  HIP_OK(hipStreamSynchronize(s_.stream_));   // the mirror rows about to be rewritten are not in flight
  const size_t words = lora_table_words(tiles_dec_);
  for (int mb = 0; mb < opt_.n_mb; ++mb) {
    if (!touched[mb]) continue;
    int32_t* h = tab_host_ + (size_t)mb * words;
    lora_build_tiles(row_ad_.data() + (size_t)mb * B, row_sc_.data() + (size_t)mb * B, B, opt_.lora_adapters, tiles_dec_, h);
    HIP_OK(hipMemcpyAsync(tab_[mb], h, words * 4, hipMemcpyHostToDevice, s_.stream_));
  }
  HIP_OK(hipStreamSynchronize(s_.stream_));
}

// the chunk's rows grouped by their slots' adapters; the table travels in kernel arguments, in stream
// order with the chunk's other metadata
void HipLora::bind_prefill(int mb, const std::vector<PrefillSeg>& segs, int T, Fwd& f) {
  std::vector<int32_t> ids;
  std::vector<float> sc;
  for (const PrefillSeg& s : segs) {
    const size_t sl = (size_t)s_.slot_of(mb, s.b);
    ids.insert(ids.end(), s.T, row_ad_[sl]);
    sc.insert(sc.end(), s.T, row_sc_[sl]);
  }
  const int mt = lora_max_tiles(T, opt_.lora_adapters);
  std::vector<int32_t> tab(lora_table_words(mt));
  lora_build_tiles(ids.data(), sc.data(), T, opt_.lora_adapters, mt, tab.data());
  launch_lora_table(tab_pf_, tab.data(), mt, f.st);
  f.lora_tab = tab_pf_; f.lora_tiles = std::max(mt, 1);
}

void HipLora::group(int li, const Fwd& f, int n_t, const int* tgt, const int* N, const int* yoff, const f16* X, int ldx,
                    int K, float* Y, int ldy) {
  if (!f.lora_tab) throw std::runtime_error("lora: the forward pass carries no tile table");
  LoraGroupParams p{};
  p.tiles = f.lora_tab; p.max_tiles = f.lora_tiles; p.targets = tgt_;
  p.n_adapters = opt_.lora_adapters; p.n_layers = n_layers_; p.layer = li; p.n_t = n_t;
  for (int i = 0; i < n_t; ++i) { p.tgt[i] = tgt[i]; p.N[i] = N[i]; p.yoff[i] = yoff[i]; }
  p.X = X; p.ldx = ldx; p.K = K; p.Y = Y; p.ldy = ldy;
  p.part = part_; p.part_floats = part_n_; p.rcap = rcap_;
  launch_lora_shrink(p, f.st);
  launch_lora_expand(p, f.st);
}

}  // namespace mp
