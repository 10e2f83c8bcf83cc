"""LoRA adapter files (llama.cpp's adapter GGUF) for tests, tools and the fp32 oracle.

An adapter GGUF carries general.type = "adapter", adapter.type = "lora", general.architecture (the base
model's), adapter.lora.alpha (f32) and tensor pairs `<base tensor name>.lora_a` (ggml ne = [K, r]) and
`<base tensor name>.lora_b` (ne = [r, N]).  Applied at user scale s, a pair adds
s * (alpha / r if alpha != 0 else 1) * B (A x) to the output of its base projection, r the rank of
that pair (llama.cpp's rule; ranks may differ between tensors).  The engine takes pairs on attn_q,
attn_k, attn_v, attn_output, ffn_gate, ffn_up and ffn_down of any layer (Engine.load_adapter).
"""
from __future__ import annotations

import numpy as np

from .utils import quants as Q
from .utils.gguf import F32T, GGUFReader, GGUFWriter

TARGETS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")


def write_adapter_gguf(path: str, arch: str, alpha: float, pairs: dict, dtype: int = Q.F32,
                       general_type: str = "adapter", adapter_type: str = "lora") -> str:
    """pairs: {base tensor name (e.g. "blk.0.attn_q.weight"): (A [r][K], B [N][r])} as float arrays; a
    value of (A, None) or (None, B) writes only that half (for loader tests).  dtype: the ggml type of
    the stored tensors (F32, F16, BF16 or a block type whose block divides K and r)."""
    w = GGUFWriter(path)
    w.add("general.architecture", arch)
    w.add("general.type", general_type)
    w.add("adapter.type", adapter_type)
    w.add("adapter.lora.alpha", float(alpha), F32T)
    for name, (A, B) in pairs.items():
        for suffix, m in ((".lora_a", A), (".lora_b", B)):
            if m is None:
                continue
            m = np.ascontiguousarray(m, np.float32)
            assert m.ndim == 2, name
            w.add_tensor(name + suffix, Q.quantize(m, dtype), dtype, (m.shape[1], m.shape[0]))
    w.write()
    return path


def read_adapter(path: str) -> dict:
    """{"arch", "alpha", "pairs": {base tensor name: (A [r][K], B [N][r])}} with the tensors as f32."""
    r = GGUFReader(path)
    if r.kv.get("general.type") != "adapter" or r.kv.get("adapter.type") != "lora":
        raise ValueError(f"{path}: not a LoRA adapter (general.type / adapter.type)")
    pairs: dict = {}
    for name in r.tensors:
        for suffix, k in ((".lora_a", 0), (".lora_b", 1)):
            if name.endswith(suffix):
                pairs.setdefault(name[:-len(suffix)], [None, None])[k] = r.tensor_f32(name)
    for base, (A, B) in pairs.items():
        if A is None or B is None:
            raise ValueError(f"{path}: {base} has only one of .lora_a / .lora_b")
    return {"arch": r.kv.get("general.architecture"), "alpha": float(r.kv.get("adapter.lora.alpha", 0.0)),
            "pairs": {k: (v[0], v[1]) for k, v in pairs.items()}}


def merged_tensors(base_tensors: dict, adapter: dict, scale: float = 1.0) -> dict:
    """The base model's tensors with the adapter merged at user scale `scale`:
    W + scale * (alpha / r if alpha != 0 else 1) * B A per target (for RefLlama, the fp32 oracle)."""
    out = dict(base_tensors)
    alpha = adapter["alpha"]
    for base, (A, B) in adapter["pairs"].items():
        r = A.shape[0]
        s = scale * (alpha / r if alpha != 0 else 1.0)
        W = np.asarray(base_tensors[base], np.float64)
        out[base] = (W + s * (np.asarray(B, np.float64) @ np.asarray(A, np.float64))).astype(np.float32)
    return out
