"""Qwen3 family without a GPU: the CPU engine against the torch fp32 oracle, the oracle against an
independent numpy evaluation of the per-head Q/K RMSNorm + NEOX RoPE, config parsing and rejections,
and the stability of the synthetic writer for the existing configs."""
import hashlib

import numpy as np
import pytest

from conftest import make_model


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


@pytest.mark.parametrize("name,ftype", [("tiny-qwen3", "Q4_K_M"), ("tiny-qwen3-hd64", "Q8_0")])
@pytest.mark.parametrize("act", ["f32", "q8"])
def test_cpu_engine_matches_reference_qwen3(native, model_dir, name, ftype, act):
    """Body and tolerances of test_cpu_engine_matches_reference (1e-8 for cpu_act f32, 2e-3 for q8)."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, name, ftype)
    ref = RefLlama.from_gguf(path)
    assert ref.hd == cfg.hd and ref.hp["rope_neox"]
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(3, cfg.vocab, 21)]
    tol = 1e-8 if act == "f32" else 2e-3
    with Engine(gguf=path, backend="cpu", max_ctx=128, prefill_chunk=16, threads=4, cpu_act=act) as eng:
        eng.start([prompt])
        lg = eng.logits()[0]
        ref.reset()
        rl = ref.forward(prompt, 0)[-1].numpy()
        assert nmse(lg, rl) < tol, nmse(lg, rl)
        pos = len(prompt)
        for step in range(4):
            tok = eng.tokens()[0][-1]
            top2 = np.sort(rl)[-2:]
            if act == "f32" or top2[1] - top2[0] > 0.05 * (abs(top2).max() + 1):
                assert tok == int(rl.argmax()), step
            eng.decode(1)
            lg = eng.logits()[0]
            rl = ref.forward([tok], pos)[-1].numpy()
            pos += 1
            assert nmse(lg, rl) < tol, (step, nmse(lg, rl))


def _rms(x, w, eps):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w


def _neox(x, pos, base):
    hd = x.shape[-1]
    inv = base ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)
    ang = np.outer(np.asarray(pos, np.float64), inv)[:, None, :]
    c, s = np.cos(ang), np.sin(ang)
    x0, x1 = x[..., : hd // 2], x[..., hd // 2:]
    return np.concatenate([x0 * c - x1 * s, x0 * s + x1 * c], -1)


def test_oracle_matches_independent_numpy(model_dir):
    """Layer 0 of tiny-qwen3 F32, one 5-token prompt: k (and q) after the norm and NEOX RoPE computed
    in plain numpy fp64 from the dequantised tensors equal what RefLlama caches; RoPE-then-norm does
    not, so the synthetic norm weights tell the two orders apart."""
    import torch
    from mipipe.models.reference import RefLlama
    from mipipe.utils.gguf import GGUFReader
    path, cfg = make_model(model_dir, "tiny-qwen3", "F32")
    r = GGUFReader(path)
    t = {n: np.asarray(r.tensor_f32(n), np.float64) for n in r.tensors if n.startswith("blk.0.") or n == "token_embd.weight"}
    prompt = [11, 300, 7, 4000, 42]
    T, hd, Hq, Hk, eps = len(prompt), cfg.hd, cfg.n_head, cfg.n_head_kv, cfg.eps
    assert hd == 128 and Hq * hd != cfg.d_model
    assert t["blk.0.attn_q_norm.weight"].shape == (hd,) and t["blk.0.attn_k_norm.weight"].shape == (hd,)
    x = t["token_embd.weight"][prompt]
    h = _rms(x, t["blk.0.attn_norm.weight"], eps)
    q = (h @ t["blk.0.attn_q.weight"].T).reshape(T, Hq, hd)
    k = (h @ t["blk.0.attn_k.weight"].T).reshape(T, Hk, hd)
    pos = list(range(T))
    wq, wk = t["blk.0.attn_q_norm.weight"], t["blk.0.attn_k_norm.weight"]
    k_good = _neox(_rms(k, wk, eps), pos, cfg.rope_base)
    k_swapped = _rms(_neox(k, pos, cfg.rope_base), wk, eps)
    q_good = _neox(_rms(q, wq, eps), pos, cfg.rope_base)

    ref = RefLlama.from_gguf(path, dtype=torch.float64)
    seen = {}
    rope = ref.rope

    def spy(x, p):   # the oracle's rotation outputs: q first, then k
        out = rope(x, p)
        seen.setdefault("q" if x.shape[1] == Hq else "k", out.numpy().copy())
        return out
    ref.rope = spy
    ref.forward(prompt, 0, layers=(0, 1), want_logits=False)
    ck = ref.cache_k[0].numpy()
    np.testing.assert_allclose(ck, k_good, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(seen["q"], q_good, rtol=1e-5, atol=1e-9)
    assert not np.allclose(ck, k_swapped, rtol=1e-2, atol=1e-3)
    # ... and not by a hair: the two orders differ by a sizeable fraction of the signal
    assert nmse(k_swapped, k_good) > 1e-2


def test_qwen3_config_parsing(native, model_dir):
    """A written tiny-qwen3 GGUF loads with head_dim 128 (from attention.key_length; d_model / n_head
    is 64), the Q/K norm and NEOX RoPE, as the engine's info() and describe() report them."""
    import json
    from mipipe import _native as N
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-qwen3", "Q8_0")
    mc = json.loads(N.lib().mp_model_config_json(N.cstr(path)).decode())
    assert mc["arch"] == "qwen3" and mc["head_dim"] == 128 and mc["qk_norm"] and mc["rope_neox"]
    assert not mc["qkv_bias"] and mc["tied_output"]
    with Engine(gguf=path, backend="cpu", max_ctx=64, threads=2) as eng:
        m = eng.info["model"]
        assert m["head_dim"] == 128 and m["qk_norm"] is True and m["rope_neox"] is True and m["arch"] == "qwen3"
        assert m["n_head"] * m["head_dim"] == 2 * m["d_model"]
        d = m["describe"]
        assert "arch=qwen3" in d and "head_dim=128" in d and " qk_norm" in d and "rope=neox" in d
    # the other families report no Q/K norm
    path2, _ = make_model(model_dir, "tiny-qwen2", "Q8_0")
    mc2 = json.loads(N.lib().mp_model_config_json(N.cstr(path2)).decode())
    assert mc2["qk_norm"] is False and mc2["head_dim"] == 64


def test_qwen3moe_rejected(native, model_dir):
    from mipipe.engine import Engine
    path, _ = make_model(model_dir, "tiny-qwen3", "Q8_0", arch="qwen3moe")
    with pytest.raises(RuntimeError, match="unsupported architecture: qwen3moe"):
        Engine(gguf=path, backend="cpu", max_ctx=64, threads=2)


def test_qwen3_without_q_norm_rejected(native, model_dir):
    from mipipe.engine import Engine
    path, _ = make_model(model_dir, "tiny-qwen3", "Q8_0", qk_norm=False)
    with pytest.raises(RuntimeError, match=r"missing tensor blk\.0\.attn_q_norm\.weight"):
        Engine(gguf=path, backend="cpu", max_ctx=64, threads=2)


def test_qwen3_value_length_and_partial_rotary_rejected(native, model_dir, tmp_path):
    """attention.value_length != key_length and rope.dimension_count != head_dim are refused."""
    from mipipe.engine import Engine
    from mipipe.models import synthetic as S
    from mipipe.models.config import CONFIGS
    cfg = CONFIGS["tiny-qwen3"].scaled(n_layer=1)

    class W(S.GGUFWriter):
        override = {}

        def add(self, key, value, *a, **kw):
            return super().add(key, self.override.get(key, value), *a, **kw)

    for key, msg in (("qwen3.attention.value_length", "value_length"), ("qwen3.rope.dimension_count", "partial rotary")):
        W.override = {key: 64}
        orig, S.GGUFWriter = S.GGUFWriter, W
        try:
            path = S.write_synthetic_gguf(str(tmp_path / (msg.split()[0] + ".gguf")), cfg, "Q8_0", fast_random_blocks=False)
        finally:
            S.GGUFWriter = orig
        with pytest.raises(RuntimeError, match=msg):
            Engine(gguf=path, backend="cpu", max_ctx=64, threads=2)


# sha256 of write_synthetic_gguf(tiny-gqa, Q8_0, seed 0, fast_random_blocks=False, wscale=1.0) as the
# commit before the Qwen3 tensors were added wrote it: the new tensors are yielded only under
# cfg.qk_norm, so the rng draw sequence of every existing config is unchanged
TINY_GQA_Q8_0_SHA256 = "3367e713e0540ee8b1cdfdf10672214afba395070080ae40cdd0be8f032d2874"


def test_synthetic_writer_unchanged_for_existing_configs(tmp_path):
    from mipipe.models.config import CONFIGS
    from mipipe.models.synthetic import write_synthetic_gguf
    p = write_synthetic_gguf(str(tmp_path / "tiny-gqa.gguf"), CONFIGS["tiny-gqa"], "Q8_0", seed=0,
                             fast_random_blocks=False, wscale=1.0)
    with open(p, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == TINY_GQA_Q8_0_SHA256
