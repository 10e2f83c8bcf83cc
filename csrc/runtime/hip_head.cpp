#include "hip_head.h"

#include <algorithm>
#include <cstring>

namespace mp {

HipHead::HipHead(HipStage& stage) : s_(stage), cfg_(stage.cfg_), opt_(stage.opt_) {
  const int B = opt_.mb_size, NM = opt_.n_mb, n_slots = NM * B;
  logits_ld_ = (int)round_up(cfg_.vocab, 16);
  logits_ = (float*)mem_.zero((size_t)B * logits_ld_ * 4);
  am_.rows = std::max(B, opt_.prefill_chunk);
  am_.part = (float*)mem_.zero((size_t)am_.rows * kArgmaxChunks * 2 * 4);
  am_.counters = (int32_t*)mem_.zero((size_t)am_.rows * 4);
  for (int mb = 0; mb < NM; ++mb) last_h_.push_back((float*)mem_.zero((size_t)B * cfg_.d_model * 4));
  if (opt_.row_sampling) {   // every slot starts greedy and neutral, draw index 0
    row_host_.assign((size_t)n_slots, RowSampling{});
    row_tab_ = (RowSampling*)mem_.get(row_host_.size() * sizeof(RowSampling));
    HIP_OK(hipMemcpy(row_tab_, row_host_.data(), row_host_.size() * sizeof(RowSampling), hipMemcpyHostToDevice));
    row_draw_ = (int32_t*)mem_.zero((size_t)n_slots * 4);
  }
  if (opt_.row_masks) {   // every slot starts unconstrained
    mask_ldw_ = (cfg_.vocab + 31) / 32;
    const size_t words = (size_t)n_slots * mask_ldw_;
    mask_tab_ = (uint32_t*)mem_.zero(words * 4);
    mask_on_ = (int32_t*)mem_.zero((size_t)n_slots * 4);
    HIP_OK(hipHostMalloc((void**)&mask_host_, words * 4, hipHostMallocDefault));
    HIP_OK(hipHostMalloc((void**)&mask_on_host_, (size_t)n_slots * 4, hipHostMallocDefault));
    std::memset(mask_host_, 0, words * 4);
    std::memset(mask_on_host_, 0, (size_t)n_slots * 4);
  }
}

HipHead::~HipHead() {
  (void)hipSetDevice(s_.device());
  if (mask_host_) (void)hipHostFree(mask_host_);
  if (mask_on_host_) (void)hipHostFree(mask_on_host_);
}

void HipHead::ensure_hist() {
  // (row_sampling: the windows exist whatever the engine's penalties are, a request may bring its own)
  if (!(s_.penalties_on() || rows_on()) || (hist_ && hist_n_ == s_.pen_last_n_)) return;
  const size_t rows = (size_t)opt_.n_mb * opt_.mb_size;
  hist_ld_ = s_.pen_last_n_ + (rows_on() ? kMaxLogitBias : 0);
  hist_ = (int32_t*)mem_.get(rows * hist_ld_ * 4);
  HIP_OK(hipMemset(hist_, 0xFF, rows * hist_ld_ * 4));   // -1: empty
  if (!hist_cnt_) hist_cnt_ = (int32_t*)mem_.get(rows * 4);
  HIP_OK(hipMemset(hist_cnt_, 0, rows * 4));
  hist_n_ = s_.pen_last_n_;
  if (rows_on())   // the bias ids the slots already have
    for (size_t r = 0; r < rows; ++r) {
      int32_t ids[kMaxLogitBias];
      for (int i = 0; i < kMaxLogitBias; ++i) ids[i] = i < row_host_[r].n_bias ? row_host_[r].bias_id[i] : -1;
      HIP_OK(hipMemcpy(hist_ + r * hist_ld_ + hist_n_, ids, sizeof(ids), hipMemcpyHostToDevice));
    }
}

void HipHead::set_row_sampling(int mb, int row, const RowSampling& r) {
  if (!rows_on()) throw std::runtime_error("set_row_sampling: the stage was built without row_sampling");
  if (mb < 0 || mb >= opt_.n_mb || row < 0 || row >= opt_.mb_size) throw std::runtime_error("set_row_sampling: bad row");
  check_row_sampling(r, cfg_.vocab);
  ensure_hist();
  ensure_logprob();
  const size_t s = (size_t)s_.slot_of(mb, row);
  row_host_[s] = r;
  int32_t ids[kMaxLogitBias];
  for (int i = 0; i < kMaxLogitBias; ++i) ids[i] = i < r.n_bias ? r.bias_id[i] : -1;
  HIP_OK(hipSetDevice(s_.device()));
  HIP_OK(hipStreamSynchronize(s_.stream_));   // no launch may still read the old record
  HIP_OK(hipMemcpy(row_tab_ + s, &r, sizeof(RowSampling), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(row_draw_ + s, &r.draw0, 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(hist_ + s * hist_ld_ + hist_n_, ids, sizeof(ids), hipMemcpyHostToDevice));
}

void HipHead::set_row_draws(int mb, const std::vector<int32_t>& draws) {
  if (!rows_on()) return;
  if (mb < 0 || mb >= opt_.n_mb || (int)draws.size() != opt_.mb_size) throw std::runtime_error("set_row_draws: bad size");
  HIP_OK(hipSetDevice(s_.device()));
  HIP_OK(hipStreamSynchronize(s_.stream_));
  HIP_OK(hipMemcpy(row_draw_ + (size_t)s_.slot_of(mb, 0), draws.data(), draws.size() * 4, hipMemcpyHostToDevice));
}

// The changed rows go to the pinned mirror, then to the device on the stage's stream with the on
// flags behind them; one synchronisation, after the last copy, so the mirror is free again and no
// head can run between a row and its flag.
void HipHead::set_row_masks(const std::vector<int>& slots, const uint32_t* const* bits) {
  if (!mask_tab_) throw std::runtime_error("set_row_masks: the stage was built without row_masks");
  const int n_slots = opt_.n_mb * opt_.mb_size;
  for (size_t i = 0; i < slots.size(); ++i) {
    if (slots[i] < 0 || slots[i] >= n_slots) throw std::runtime_error("set_row_masks: bad slot");
    for (size_t k = 0; k < i; ++k)   // a second copy into the same mirror row would race the first one's stream copy
      if (slots[k] == slots[i]) throw std::runtime_error("set_row_masks: a slot is listed twice");
  }
  if (slots.empty()) return;
  HIP_OK(hipSetDevice(s_.device()));
  const size_t row_bytes = (size_t)mask_ldw_ * 4;
  for (size_t i = 0; i < slots.size(); ++i) {
    const size_t s = (size_t)slots[i];
    mask_on_host_[s] = bits[i] ? 1 : 0;
    if (!bits[i]) continue;
    std::memcpy(mask_host_ + s * mask_ldw_, bits[i], row_bytes);
    HIP_OK(hipMemcpyAsync(mask_tab_ + s * mask_ldw_, mask_host_ + s * mask_ldw_, row_bytes, hipMemcpyHostToDevice, s_.stream_));
  }
  HIP_OK(hipMemcpyAsync(mask_on_, mask_on_host_, (size_t)n_slots * 4, hipMemcpyHostToDevice, s_.stream_));
  HIP_OK(hipStreamSynchronize(s_.stream_));
}

// token logprob buffers (n_probs != 0): allocated when recording is switched on and when the penalty
// window changes size; nothing exists, and run() enqueues nothing more, with n_probs 0
void HipHead::ensure_logprob() {
  if (s_.n_probs_ == 0) return;
  const int B = opt_.mb_size;
  if (lp_rec_.empty()) {
    HIP_OK(hipSetDevice(s_.device()));
    for (int mb = 0; mb < opt_.n_mb; ++mb) {
      lp_rec_.push_back((float*)mem_.get(Stage::logprob_rec_words(B) * 4));
      HIP_OK(hipMemset(lp_rec_.back(), 0xFF, Stage::logprob_rec_words(B) * 4));
    }
    lp_lse_ = (float*)mem_.get((size_t)B * 4);
  }
  if (hist_ && lp_hist_n_ != hist_ld_) {
    lp_hist_raw_ = (float*)mem_.get((size_t)B * hist_ld_ * 4);
    lp_hist_n_ = hist_ld_;
  }
}

// the buffers of a chunk whose every row goes through the LM head (speculative verify chunks and
// score chunks share them): the chunk's logits and, per micro-batch, the greedy token after each row
void HipHead::ensure_chunk_head() {
  if (!vlogits_) vlogits_ = (float*)mem_.get((size_t)opt_.prefill_chunk * logits_ld_ * 4);
  if (!vtok_) vtok_ = (int32_t*)mem_.get((size_t)opt_.n_mb * opt_.prefill_chunk * 4);
}

void HipHead::set_score_targets(int mb, const int32_t* host, int n, int top_n) {
  if (n > opt_.prefill_chunk || top_n < 0 || top_n > Stage::kMaxProbs) throw std::runtime_error("set_score_targets: bad size");
  HIP_OK(hipSetDevice(s_.device()));
  const size_t rows = (size_t)opt_.n_mb * opt_.prefill_chunk;
  if (!sc_tgt_) {
    sc_tgt_ = (int32_t*)mem_.get(rows * 4);
    sc_lp_ = (float*)mem_.get(rows * 4);
    sc_lse_ = (float*)mem_.get(rows * 4);
  }
  if (top_n > 0 && !sc_top_id_) {
    sc_top_id_ = (int32_t*)mem_.get(rows * Stage::kMaxProbs * 4);
    sc_top_lp_ = (float*)mem_.get(rows * Stage::kMaxProbs * 4);
  }
  ensure_chunk_head();
  sc_top_n_ = top_n;
  HIP_OK(hipMemcpy(sc_tgt_ + (size_t)mb * opt_.prefill_chunk, host, (size_t)n * 4, hipMemcpyHostToDevice));
}

void HipHead::copy_scores(int mb, int n, float* target_lp, int32_t* top_id, float* top_lp) {
  constexpr int kMaxProbs = Stage::kMaxProbs;
  if (!sc_lp_ || n > opt_.prefill_chunk) throw std::runtime_error("no scores");
  HIP_OK(hipSetDevice(s_.device()));
  HIP_OK(hipStreamSynchronize(s_.stream_));
  const size_t off = (size_t)mb * opt_.prefill_chunk;
  HIP_OK(hipMemcpy(target_lp, sc_lp_ + off, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (sc_top_n_ > 0 && top_id && top_lp) {
    HIP_OK(hipMemcpy2D(top_id, (size_t)sc_top_n_ * 4, sc_top_id_ + off * kMaxProbs, (size_t)kMaxProbs * 4,
                       (size_t)sc_top_n_ * 4, n, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy2D(top_lp, (size_t)sc_top_n_ * 4, sc_top_lp_ + off * kMaxProbs, (size_t)kMaxProbs * 4,
                       (size_t)sc_top_n_ * 4, n, hipMemcpyDeviceToHost));
  }
}

void HipHead::copy_verify_tokens(int mb, int32_t* host, int n) {
  if (!vtok_ || n > opt_.prefill_chunk) throw std::runtime_error("no verify tokens");
  HIP_OK(hipSetDevice(s_.device()));
  HIP_OK(hipMemcpy(host, vtok_ + (size_t)mb * opt_.prefill_chunk, (size_t)n * 4, hipMemcpyDeviceToHost));
}

void HipHead::ensure_pool(int mb) {
  const size_t d = (size_t)cfg_.d_model, ns = (size_t)opt_.n_mb * opt_.mb_size;
  if (!pool_tab_) {
    pool_tab_cap_ = opt_.mb_size;   // a chunk holds at most one segment per sequence of its micro-batch
    pool_tab_ = (PoolSeg*)mem_.get((size_t)pool_tab_cap_ * sizeof(PoolSeg));
    pool_emb_ = (float*)mem_.get(ns * d * 4);
  }
  if (s_.embed_pool_ == POOL_MEAN && !pool_acc_) {
    pool_acc_ = (float*)mem_.get(ns * d * 4);
    // every segment's last block may be short: ceil(T / rows) summed is at most chunk / rows + segments
    pool_part_cap_ = opt_.prefill_chunk / kPoolBlockRows + opt_.mb_size + 1;
    pool_part_ = (float*)mem_.get((size_t)pool_part_cap_ * d * 4);
  }
  if (s_.embed_pool_ == POOL_MEAN || s_.embed_pool_ == POOL_NONE) {
    if (pool_h_.empty()) pool_h_.assign(opt_.n_mb, nullptr);
    if (!pool_h_[mb]) pool_h_[mb] = (float*)mem_.get((size_t)opt_.prefill_chunk * d * 4);
  }
}

// embed chunk: x [T][d] -> the slots' vectors (pool.hip)
void HipHead::pool_chunk(int mb, const std::vector<PrefillSeg>& segs, const float* x, int T, hipStream_t st) {
  ensure_pool(mb);
  std::vector<PoolSeg> tab;
  int row = 0;
  for (const PrefillSeg& s : segs) {
    if (!s.embed) throw std::runtime_error("embed chunk: a segment of another kind");
    // an embed prompt is prefilled whole (no prefix reuse), so the segment that ends it tells its length
    tab.push_back(PoolSeg{row, s.T, s_.slot_of(mb, s.b), s.p0, s.p0 + s.T, s.last ? 1 : 0});
    row += s.T;
  }
  PoolParams p{};
  p.x = x; p.ldx = cfg_.d_model; p.w = s_.out_norm_; p.d = cfg_.d_model; p.eps = cfg_.eps;
  p.segs = tab.data(); p.n_seg = (int)tab.size(); p.seg_tab = pool_tab_; p.seg_cap = pool_tab_cap_;
  p.T = T; p.pooling = s_.embed_pool_; p.normalize = s_.embed_norm_ ? 1 : 0; p.n_slots = opt_.n_mb * opt_.mb_size;
  p.h = pool_h_.empty() ? nullptr : pool_h_[mb];
  p.part = pool_part_; p.part_cap = pool_part_cap_; p.pool_acc = pool_acc_; p.emb = pool_emb_;
  launch_pool_embed(p, st);
}

void HipHead::copy_embeddings(const std::vector<int>& slots, float* host) {
  if (!pool_emb_) throw std::runtime_error("no embeddings");
  HIP_OK(hipSetDevice(s_.device()));
  HIP_OK(hipStreamSynchronize(s_.stream_));
  const size_t d = (size_t)cfg_.d_model;
  for (size_t k = 0; k < slots.size(); ++k) {
    if (slots[k] < 0 || slots[k] >= opt_.n_mb * opt_.mb_size) throw std::runtime_error("copy_embeddings: bad slot");
    HIP_OK(hipMemcpy(host + k * d, pool_emb_ + (size_t)slots[k] * d, d * 4, hipMemcpyDeviceToHost));
  }
}

void HipHead::copy_token_embeddings(int mb, int n_rows, float* host) {
  if ((size_t)mb >= pool_h_.size() || !pool_h_[mb] || n_rows > opt_.prefill_chunk) throw std::runtime_error("no token embeddings");
  HIP_OK(hipSetDevice(s_.device()));
  HIP_OK(hipStreamSynchronize(s_.stream_));
  HIP_OK(hipMemcpy(host, pool_h_[mb], (size_t)n_rows * cfg_.d_model * 4, hipMemcpyDeviceToHost));
}

void HipHead::set_history(int mb, const std::vector<std::vector<int32_t>>& seqs) {
  if (!(s_.penalties_on() || rows_on())) return;
  ensure_hist();
  ensure_logprob();
  const int B = opt_.mb_size, n = hist_n_, ld = hist_ld_;
  std::vector<int32_t> h((size_t)B * ld, -1), cnt(B, 0);
  for (int b = 0; b < B; ++b) {
    if (b < (int)seqs.size()) {
      const auto& q = seqs[b];
      const int take = std::min<int>(n, (int)q.size());
      for (int i = 0; i < take; ++i) h[(size_t)b * ld + i] = q[q.size() - take + i];
      cnt[b] = take;
    }
    if (rows_on()) {   // the row's bias ids stay behind its window
      const RowSampling& r = row_host_[(size_t)s_.slot_of(mb, b)];
      for (int i = 0; i < r.n_bias; ++i) h[(size_t)b * ld + n + i] = r.bias_id[i];
    }
  }
  HIP_OK(hipSetDevice(s_.device()));
  HIP_OK(hipMemcpy(hist_ + (size_t)mb * B * ld, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(hist_cnt_ + (size_t)mb * B, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice));
}

// Every step is written once; where the row form (row_sampling: fixed arguments, the rows' records,
// draw indices and windows read from device memory, so the decode graphs are captured once) and the
// engine-wide form (the stage's sampling values baked into the launch) differ, they are the branches
// of that step.  The windows have one stride for both: without row_sampling hist_ld_ == hist_n_.
void HipHead::run(int mb, int M, const float* x, int32_t* tok_out, uint64_t salt, hipStream_t st, bool advance) {
  const int B = opt_.mb_size, V = cfg_.vocab;
  const size_t r0 = (size_t)mb * B;
  s_.lm_head(x, M, logits_, s_.small_path(M), st);
  const bool rows = rows_on();
  if (rows && !hist_) throw std::runtime_error("row_sampling: the windows were not allocated (set_penalties)");
  // the micro-batch's windows: every row has one with row_sampling, else they follow the engine's penalties
  const bool win = rows || (s_.penalties_on() && hist_);
  int32_t* hist = win ? hist_ + r0 * hist_ld_ : nullptr;
  // token logprobs are those of the RAW logits: the statistics (and the raw logits of the ids the
  // adjustment is about to rewrite: the window, then with row_sampling the bias ids) are taken here,
  // the chosen token's value after the sampler
  const bool lp = s_.n_probs_ != 0 && !lp_rec_.empty();
  float* rec = lp ? lp_rec_[mb] : nullptr;
  if (lp) {
    LogprobParams q{};
    q.logits = logits_; q.ld = logits_ld_; q.n = V; q.M = M;
    q.top_n = std::max(s_.n_probs_, 0); q.lse = lp_lse_;
    q.top_id = (int32_t*)(rec + B); q.top_lp = rec + B + (size_t)B * Stage::kMaxProbs; q.ld_top = Stage::kMaxProbs;
    if (win) { q.hist = hist; q.last_n = hist_ld_; q.hist_raw = lp_hist_raw_; }
    launch_logprob(q, st);
  }
  // adjust: bias + penalties per row, or the engine's penalties
  if (rows) {
    RowAdjustParams ra{};
    ra.logits = logits_; ra.ld = logits_ld_; ra.n = V; ra.M = M;
    ra.rows = row_tab_ + r0; ra.hist = hist; ra.hist_ld = hist_ld_; ra.last_n = hist_n_;
    launch_row_adjust(ra, st);
  } else if (win) {
    PenaltyParams pp{};
    pp.logits = logits_; pp.ld = logits_ld_; pp.n = V; pp.M = M;
    pp.hist = hist; pp.last_n = hist_n_; pp.repeat = s_.pen_repeat_; pp.freq = s_.pen_freq_; pp.presence = s_.pen_presence_;
    launch_penalize(pp, st);
  }
  // mask: the slots' masks (row_masks needs row_sampling), after the bias and the penalties: the cuts
  // and the draw see -inf
  if (mask_tab_) {
    RowMaskParams rm{};
    rm.logits = logits_; rm.ld = logits_ld_; rm.n = V; rm.M = M;
    rm.bits = mask_tab_ + r0 * mask_ldw_; rm.ldw = mask_ldw_; rm.on = mask_on_ + r0;
    launch_row_mask(rm, st);
  }
  // choose: arg-max of every row and the sampled rows' draws over it, or the engine's sampler / arg-max
  if (rows) {
    launch_argmax(logits_, logits_ld_, V, M, tok_out, st, &am_);
    SampleRowsParams sp{};
    sp.logits = logits_; sp.ld = logits_ld_; sp.n = V; sp.M = M;
    sp.rows = row_tab_ + r0; sp.draw = row_draw_ + r0; sp.advance = advance ? 1 : 0; sp.tokens = tok_out;
    launch_sample_rows(sp, st);
  } else if (s_.temp_ > 0.f) {
    SampleParams sp{};
    sp.logits = logits_; sp.ld = logits_ld_; sp.n = V; sp.M = M;
    sp.temp = s_.temp_; sp.top_k = s_.top_k_; sp.top_p = s_.top_p_; sp.min_p = s_.min_p_;
    sp.seed = s_.seed_ ^ (salt * 0x9E3779B97F4A7C15ULL); sp.step = s_.step_; sp.tokens = tok_out;
    launch_sample(sp, st);
  } else {
    launch_argmax(logits_, logits_ld_, V, M, tok_out, st, &am_);
  }
  if (lp) {
    LogprobChosenParams c{};
    c.logits = logits_; c.ld = logits_ld_; c.n = V; c.M = M; c.tokens = tok_out; c.lse = lp_lse_;
    if (win) { c.hist = hist; c.last_n = hist_ld_; c.hist_raw = lp_hist_raw_; }
    c.chosen_lp = rec;
    launch_logprob_chosen(c, st);
  }
  if (win) launch_hist_push_ld(hist, hist_ld_, hist_cnt_ + r0, hist_n_, tok_out, M, st);
}

void HipHead::prefill_chunk(int mb, const std::vector<PrefillSeg>& segs, const float* x, int T, hipStream_t st) {
  const int d = cfg_.d_model;
  if (!segs.empty() && segs[0].verify) {
    // speculative verification: LM head over every row of the chunk, greedy next token per row
    ensure_chunk_head();
    s_.lm_head(x, T, vlogits_, false, st);
    launch_argmax(vlogits_, logits_ld_, cfg_.vocab, T, vtok_ + (size_t)mb * opt_.prefill_chunk, st, &am_);
  } else if (!segs.empty() && segs[0].score) {
    // prompt scoring: LM head over every row of the chunk, then each row's target logprob
    if (!sc_tgt_ || !vlogits_) throw std::runtime_error("score chunk without targets");
    s_.lm_head(x, T, vlogits_, false, st);
    const size_t off = (size_t)mb * opt_.prefill_chunk;
    LogprobParams q{};
    q.logits = vlogits_; q.ld = logits_ld_; q.n = cfg_.vocab; q.M = T;
    q.target = sc_tgt_ + off; q.top_n = sc_top_n_; q.lse = sc_lse_ + off; q.target_lp = sc_lp_ + off;
    if (sc_top_n_ > 0) { q.top_id = sc_top_id_ + off * Stage::kMaxProbs; q.top_lp = sc_top_lp_ + off * Stage::kMaxProbs; }
    q.ld_top = Stage::kMaxProbs;
    launch_logprob(q, st);
  } else if (!segs.empty() && segs[0].embed) {
    // embeddings: output norm + pooling of the rows; no LM head, nothing kept for prefill_finish
    pool_chunk(mb, segs, x, T, st);
  } else {
    int row = 0;
    for (const PrefillSeg& s : segs) {
      row += s.T;
      if (s.last)
        HIP_OK(hipMemcpyAsync(last_h_[mb] + (size_t)s.b * d, x + (size_t)(row - 1) * d, (size_t)d * 4,
                              hipMemcpyDeviceToDevice, st));
    }
  }
}

void HipHead::prefill_finish(int mb, int32_t* tok, hipStream_t st, const std::vector<int>* rows) {
  if (!rows) return run(mb, opt_.mb_size, last_h_[mb], tok, 1000003ULL + (uint64_t)mb, st);
  if (!tok_tmp_) tok_tmp_ = (int32_t*)mem_.get((size_t)std::max(opt_.mb_size, 16) * 4);
  run(mb, opt_.mb_size, last_h_[mb], tok_tmp_, 1000003ULL + (uint64_t)mb, st);
  for (int b : *rows) HIP_OK(hipMemcpyAsync(tok + b, tok_tmp_ + b, 4, hipMemcpyDeviceToDevice, st));
}

}  // namespace mp
