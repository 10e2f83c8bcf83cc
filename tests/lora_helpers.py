"""Shared by the LoRA tests: a fixed-seed adapter generator and the merged fp32 oracles."""
import os

import numpy as np

TARGETS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")
ATTN_TARGETS = TARGETS[:4]


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


def make_pairs(base_tensors, n_layer, seed, targets=TARGETS, ranks=(8, 3), alpha=4.0, rel=0.5):
    """One (A, B) pair per (layer, target), ranks alternating between `ranks`.  B is scaled so that
    the merged delta alpha / r * B A has `rel` times the standard deviation of the base tensor: large
    enough that an engine ignoring the adapter misses the oracle by far more than the test bound."""
    rng = np.random.default_rng(seed)
    pairs = {}
    i = 0
    for li in range(n_layer):
        for t in targets:
            name = f"blk.{li}.{t}.weight"
            W = np.asarray(base_tensors[name])
            N, K = W.shape
            r = ranks[i % len(ranks)]
            i += 1
            A = (rng.standard_normal((r, K)) / np.sqrt(K)).astype(np.float32)
            s = alpha / r if alpha != 0 else 1.0
            b = rel * float(W.std()) / (s * np.sqrt(r) * (1.0 / np.sqrt(K)))
            B = (rng.standard_normal((N, r)) * b).astype(np.float32)
            pairs[name] = (A, B)
    return pairs


def make_adapter(model_dir, base_path, cfg, seed, targets=TARGETS, ranks=(8, 3), alpha=4.0, rel=0.5, dtype=None):
    """Writes an adapter for the base model at base_path (cached per argument set); returns
    (path, adapter dict of mipipe.lora.read_adapter)."""
    from mipipe import lora
    from mipipe.utils import quants as Q
    from mipipe.utils.gguf import GGUFReader
    tag = f"{os.path.basename(base_path)}-lora{seed}-{len(targets)}-{'_'.join(map(str, ranks))}-{alpha}-{rel}-{dtype}"
    path = os.path.join(str(model_dir), tag + ".gguf")
    if not os.path.exists(path):
        r = GGUFReader(base_path)
        need = {f"blk.{li}.{t}.weight" for li in range(cfg.n_layer) for t in targets}
        base = {n: r.tensor_f32(n) for n in need}
        pairs = make_pairs(base, cfg.n_layer, seed, targets, ranks, alpha, rel)
        lora.write_adapter_gguf(path, cfg.arch, alpha, pairs, Q.F32 if dtype is None else dtype)
    return path, lora.read_adapter(path)


def merged_ref(ref, adapter, scale):
    """A RefLlama over the base oracle's tensors with the adapter merged at user scale `scale`."""
    from mipipe import lora
    from mipipe.models.reference import RefLlama
    base = {k: v.cpu().numpy() for k, v in ref.t.items()}
    return RefLlama(lora.merged_tensors(base, adapter, scale), ref.hp, ref.dtype, ref.device)


def follow(ref, prompt, toks):
    """The oracle's last-row logits after the prompt and after each of `toks` fed in turn."""
    ref.reset()
    out = [ref.forward(prompt, 0)[-1].float().cpu().numpy()]
    pos = len(prompt)
    for t in toks:
        out.append(ref.forward([int(t)], pos)[-1].float().cpu().numpy())
        pos += 1
    return out
