"""Model shapes for the Llama-family configs named in BASELINE.json / SURVEY.md §2.8.

The reference runs `baronllm-llama3.1-v1-q6_k.gguf` (Llama-3.1-8B, `orchestrator/src/main.rs:40`)
and its UI is titled "Stories-15M" (`orchestrator/static/index.html:36`); BASELINE.json adds
TinyLlama-1.1B, Llama-3-70B and Mixtral-8x7B.  Dims are from the public model cards
(SURVEY.md §2.8 table).
"""
from __future__ import annotations

from dataclasses import dataclass, asdict, replace

from ..utils import quants as Q


@dataclass(frozen=True)
class LlamaConfig:
    name: str
    n_layer: int
    d_model: int
    n_head: int
    n_head_kv: int
    d_ff: int
    vocab: int
    rope_base: float = 10000.0
    eps: float = 1e-5
    n_ctx_train: int = 2048
    n_expert: int = 0
    n_expert_used: int = 0
    head_dim: int = 0           # 0 -> d_model // n_head
    tokenizer: str = "llama"    # "gpt2" (byte-level BPE) or "llama" (SPM)
    rope_freq_factors: bool = False   # Llama-3.1 rope_freqs.weight
    arch: str = "llama"         # GGUF general.architecture: "llama", "qwen2", "qwen3" or "qwen3moe"
    qkv_bias: bool = False      # Qwen2: attn_{q,k,v}.bias
    qk_norm: bool = False       # Qwen3: per-head RMSNorm of q and k before RoPE (attn_{q,k}_norm.weight)
    tied_output: bool = False   # no output.weight (LM head = token_embd)
    # standard deviation of the synthetic router weights.  With 0.5 and unit-RMS inputs the router
    # logits have a standard deviation of 0.5 sqrt(d_model) (11 at d_model 512): a softmax over many
    # experts then puts nearly all weight on one of them, and a wrong 2nd .. k-th expert would barely
    # move the output.  1 / sqrt(d_model) gives logits of about unit standard deviation.
    router_std: float = 0.5
    # <arch>.pooling_type of an embedding model (llama.cpp's ids: 0 none, 1 mean, 2 cls, 3 last, 4 rank);
    # -1 = the key is not written.  Engine.embed pools by it when it is 1..3, by `last` otherwise.
    pooling_type: int = -1
    add_eos: bool = False       # tokenizer.ggml.add_eos_token (Qwen3-Embedding files set it)

    @property
    def hd(self) -> int:
        return self.head_dim or self.d_model // self.n_head

    def as_dict(self):
        return asdict(self)

    def scaled(self, **kw) -> "LlamaConfig":
        return replace(self, **kw)


CONFIGS = {
    "stories15m": LlamaConfig("stories15m", 6, 288, 6, 6, 768, 32000, 10000.0, 1e-5, 256),
    "tinyllama": LlamaConfig("tinyllama", 22, 2048, 32, 4, 5632, 32000, 10000.0, 1e-5, 2048),
    "llama3-8b": LlamaConfig("llama3-8b", 32, 4096, 32, 8, 14336, 128256, 500000.0, 1e-5, 8192,
                             tokenizer="gpt2", rope_freq_factors=True),
    "llama3-70b": LlamaConfig("llama3-70b", 80, 8192, 64, 8, 28672, 128256, 500000.0, 1e-5, 8192,
                              tokenizer="gpt2", rope_freq_factors=True),
    "mixtral-8x7b": LlamaConfig("mixtral-8x7b", 32, 4096, 32, 8, 14336, 32000, 1e6, 1e-5, 32768,
                                n_expert=8, n_expert_used=2),
    "qwen2-7b": LlamaConfig("qwen2-7b", 28, 3584, 28, 4, 18944, 152064, 1e6, 1e-6, 32768,
                            tokenizer="gpt2", arch="qwen2", qkv_bias=True),
    "qwen3-8b": LlamaConfig("qwen3-8b", 36, 4096, 32, 8, 12288, 151936, 1e6, 1e-6, 40960, head_dim=128,
                            tokenizer="gpt2", arch="qwen3", qk_norm=True),
    # Qwen3-30B-A3B: d_ff is the width of ONE expert (expert_feed_forward_length), every layer sparse
    "qwen3-30b-a3b": LlamaConfig("qwen3-30b-a3b", 48, 2048, 32, 4, 768, 151936, 1e6, 1e-6, 40960, head_dim=128,
                                 n_expert=128, n_expert_used=8, tokenizer="gpt2", arch="qwen3moe", qk_norm=True),
    # small test shapes (same code paths, fast to generate)
    "tiny-gqa": LlamaConfig("tiny-gqa", 4, 512, 8, 2, 1024, 2048, 10000.0, 1e-5, 1024),
    "tiny-moe": LlamaConfig("tiny-moe", 3, 512, 8, 2, 768, 2048, 10000.0, 1e-5, 1024,
                            n_expert=4, n_expert_used=2),
    "tiny-qwen2": LlamaConfig("tiny-qwen2", 4, 512, 8, 2, 1024, 4096, 1e6, 1e-6, 1024,
                              tokenizer="gpt2", arch="qwen2", qkv_bias=True, tied_output=True),
    # head_dim decoupled from d_model / n_head (q_dim 1024 != d_model 512), as in Qwen3-0.6B / 4B / 32B
    "tiny-qwen3": LlamaConfig("tiny-qwen3", 4, 512, 8, 2, 1024, 4096, 1e6, 1e-6, 1024, head_dim=128,
                              tokenizer="gpt2", arch="qwen3", qk_norm=True, tied_output=True),
    "tiny-qwen3-hd64": LlamaConfig("tiny-qwen3-hd64", 4, 512, 8, 2, 1024, 4096, 1e6, 1e-6, 1024, head_dim=64,
                                   tokenizer="gpt2", arch="qwen3", qk_norm=True, tied_output=True),
    # 128 experts, 8 per token, one-super-block experts; router logits of about unit standard deviation
    "tiny-qwen3moe": LlamaConfig("tiny-qwen3moe", 2, 256, 4, 2, 256, 4096, 1e6, 1e-6, 1024, head_dim=128,
                                 n_expert=128, n_expert_used=8, tokenizer="gpt2", arch="qwen3moe", qk_norm=True,
                                 tied_output=True, router_std=1.0 / 16.0),
    # d_model = one full super-block and a half one: every projection but ffn_down has K = 384, so
    # the K-quant file types fall to the 32-weight-block types there
    "tiny-k384": LlamaConfig("tiny-k384", 3, 384, 6, 2, 1024, 2048, 10000.0, 1e-5, 1024, head_dim=64),
    "tiny-l3": LlamaConfig("tiny-l3", 4, 1024, 8, 2, 2048, 4096, 500000.0, 1e-5, 1024,
                           tokenizer="gpt2", rope_freq_factors=True),
}


def use_more_bits(i: int, n: int) -> bool:
    """llama.cpp's Q4_K_M layer-promotion rule (upstream; not in mount)."""
    return i < n // 8 or i >= 7 * n // 8 or (i - n // 8) % 3 == 2


def tensor_type(ftype: str, name: str, layer: int, n_layer: int, k_dim: int) -> int:
    """ggml type of a 2-D weight under a named file type (mix)."""
    ftype = ftype.upper()
    plain = {"F32": Q.F32, "F16": Q.F16, "BF16": Q.BF16, "Q8_0": Q.Q8_0, "Q6_K": Q.Q6_K,
             "Q5_K": Q.Q5_K, "Q4_0": Q.Q4_0, "Q5_0": Q.Q5_0, "Q5_1": Q.Q5_1, "IQ4_NL": Q.IQ4_NL}
    kq = k_dim % 256 == 0
    if ftype in plain:
        t = plain[ftype]
        if t in (Q.Q6_K, Q.Q5_K) and not kq:
            return Q.Q8_0
        return t
    if ftype in ("Q4_K", "Q4_K_S"):
        if not kq:
            return Q.Q8_0
        return Q.Q6_K if name == "output" else Q.Q4_K
    if ftype == "Q4_K_M":
        if not kq:
            return Q.Q8_0
        if name == "output":
            return Q.Q6_K
        if name in ("attn_v", "ffn_down") and use_more_bits(layer, n_layer):
            return Q.Q6_K
        return Q.Q4_K
    if ftype == "Q5_K_M":
        if not kq:
            return Q.Q8_0
        if name == "output":
            return Q.Q6_K
        if name in ("attn_v", "ffn_down") and use_more_bits(layer, n_layer):
            return Q.Q6_K
        return Q.Q5_K
    if ftype in ("Q3_K", "Q3_K_S", "Q3_K_M", "Q3_K_L", "Q2_K"):
        # the low-bit K-quant mixes (as recalled from upstream): the base type beside Q4_K / Q5_K / Q6_K
        if name == "output":
            t = Q.Q6_K
        elif ftype == "Q2_K":
            t = Q.Q3_K if name in ("attn_v", "attn_output", "ffn_down") else Q.Q2_K
        elif ftype in ("Q3_K", "Q3_K_S"):
            t = Q.Q3_K
        else:
            large = ftype == "Q3_K_L"
            if name == "attn_v":
                t = Q.Q5_K if large or layer < 2 else Q.Q4_K
            elif name == "attn_output":
                t = Q.Q5_K if large else Q.Q4_K
            elif name == "ffn_down":
                t = Q.Q5_K if large or layer < n_layer // 16 else Q.Q4_K
            else:
                t = Q.Q3_K
        if not kq:   # upstream's rule for the two low-bit types; the others as above
            return Q.Q4_0 if t in (Q.Q2_K, Q.Q3_K) else Q.Q8_0
        return t
    if ftype == "IQ4_XS":
        # (as recalled from upstream) the base type beside a Q6_K output, Q5_K attn_v and early ffn_down;
        # rows that are no multiple of 256 fall to the 32-weight-block type of the same width
        if name == "output":
            t = Q.Q6_K
        elif name == "attn_v" or (name == "ffn_down" and layer < n_layer // 8):
            t = Q.Q5_K
        else:
            t = Q.IQ4_XS
        if not kq:
            return {Q.IQ4_XS: Q.IQ4_NL, Q.Q5_K: Q.Q5_1, Q.Q6_K: Q.Q8_0}[t]
        return t
    raise ValueError(ftype)
