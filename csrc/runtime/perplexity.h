// llama.cpp's default perplexity procedure (llama-perplexity without --ppl-stride), so numbers are
// comparable with published ones: the token stream is cut into consecutive windows of n_ctx
// tokens (BOS in the first slot where the vocabulary adds one), every window is scored, and only
// the second half of a window counts: positions [n_ctx / 2, n_ctx - 1), where position j stands for
// -log p(window[j + 1] | window[:j + 1]).  The +- is the standard error of the mean NLL pushed
// through exp.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace mp {

inline long ppl_n_windows(size_t n_tokens, int n_ctx) { return n_ctx > 1 ? (long)(n_tokens / (size_t)n_ctx) : 0; }
// the procedure needs two windows at least (llama.cpp's rule)
inline bool ppl_enough_tokens(size_t n_tokens, int n_ctx) { return n_ctx > 1 && n_tokens >= 2 * (size_t)n_ctx; }

inline std::vector<int32_t> ppl_window(const std::vector<int32_t>& tokens, long w, int n_ctx, int bos) {
  std::vector<int32_t> o(tokens.begin() + (size_t)w * n_ctx, tokens.begin() + (size_t)(w + 1) * n_ctx);
  if (bos >= 0) o[0] = bos;
  return o;
}

struct PplEstimate {
  double nll = 0, nll2 = 0;
  long count = 0;
  // lp: the window's n_ctx - 1 scores, lp[j] = log p(window[j + 1] | window[:j + 1])
  void add_window(const float* lp, int n_ctx) {
    for (int j = n_ctx / 2; j < n_ctx - 1; ++j) {
      const double v = -(double)lp[j];
      nll += v;
      nll2 += v * v;
      ++count;
    }
  }
  double mean_nll() const { return count ? nll / count : 0.0; }
  double ppl() const { return std::exp(mean_nll()); }
  double err() const {   // standard error of the mean NLL, times the PPL
    if (count < 2) return 0.0;
    const double m = mean_nll();
    const double var = nll2 / count - m * m;
    return var > 0 ? std::sqrt(var / (count - 1)) * ppl() : 0.0;
  }
};

}  // namespace mp
