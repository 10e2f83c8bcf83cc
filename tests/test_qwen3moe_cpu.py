"""Qwen3-MoE family without a GPU: the CPU engine on tiny-qwen3moe (128 experts, 8 per token, expert
FFN width 256 from expert_feed_forward_length) against the torch fp32 oracle, what info() reports,
the load-time rejections, and the oracle's tie rule and router-margin record."""
import json

import numpy as np
import pytest

from conftest import make_model


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


@pytest.mark.parametrize("act", ["f32", "q8"])
def test_cpu_engine_matches_reference_qwen3moe(native, model_dir, act):
    """Body and tolerances of test_cpu_engine_matches_reference_qwen3 (1e-8 for cpu_act f32, 2e-3 for q8)."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-qwen3moe", "Q8_0")
    ref = RefLlama.from_gguf(path)
    assert ref.hd == cfg.hd == 128 and ref.hp["rope_neox"] and ref.hp["n_expert"] == 128
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(3, cfg.vocab, 21)]
    tol = 1e-8 if act == "f32" else 2e-3
    with Engine(gguf=path, backend="cpu", max_ctx=128, prefill_chunk=16, threads=4, cpu_act=act) as eng:
        m = eng.info["model"]
        assert m["arch"] == "qwen3moe" and m["n_expert"] == 128 and m["n_expert_used"] == 8 and m["qk_norm"] is True
        assert m["d_ff"] == 256 and m["d_ff_kind"] == "expert" and m["expert_d_ff"] == 256
        assert "expert_d_ff=256" in m["describe"] and "n_expert=128" in m["describe"]
        eng.start([prompt])
        lg = eng.logits()[0]
        ref.reset()
        rl = ref.forward(prompt, 0)[-1].numpy()
        assert len(ref.router_margins) == cfg.n_layer and ref.router_margins[0][2].shape == (len(prompt),)
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


def test_qwen3moe_config_parsing(native, model_dir):
    from mipipe import _native as N
    path, cfg = make_model(model_dir, "tiny-qwen3moe", "Q8_0")
    mc = json.loads(N.lib().mp_model_config_json(N.cstr(path)).decode())
    assert mc["arch"] == "qwen3moe" and mc["n_expert"] == 128 and mc["n_expert_used"] == 8
    assert mc["qk_norm"] and mc["rope_neox"] and not mc["qkv_bias"] and mc["expert_ff"] and mc["head_dim"] == 128


def _write_with(tmp_path, name, override=None, drop=()):
    """tiny-qwen3moe (1 layer) with some metadata keys overridden or left out."""
    from mipipe.models import synthetic as S
    from mipipe.models.config import CONFIGS
    cfg = CONFIGS["tiny-qwen3moe"].scaled(n_layer=1)

    class W(S.GGUFWriter):
        def add(self, key, value, *a, **kw):
            if key in drop:
                return None
            return super().add(key, (override or {}).get(key, value), *a, **kw)

    orig, S.GGUFWriter = S.GGUFWriter, W
    try:
        return S.write_synthetic_gguf(str(tmp_path / (name + ".gguf")), cfg, "Q8_0", fast_random_blocks=True)
    finally:
        S.GGUFWriter = orig


@pytest.mark.parametrize("key,value,msg", [
    ("qwen3moe.expert_count", 129, r"qwen3moe\.expert_count = 129"),
    ("qwen3moe.expert_used_count", 9, r"qwen3moe\.expert_used_count = 9"),
    ("qwen3moe.expert_feed_forward_length", 512, r"qwen3moe\.expert_feed_forward_length = 512 disagrees"),
])
def test_qwen3moe_load_errors(native, tmp_path, key, value, msg):
    from mipipe.engine import Engine
    path = _write_with(tmp_path, "bad", {key: value})
    with pytest.raises(RuntimeError, match=msg):
        Engine(gguf=path, backend="cpu", max_ctx=64, threads=2)


def test_qwen3moe_expert_width_from_tensor_shape(native, tmp_path):
    """Without expert_feed_forward_length the width is ne[1] of blk.0.ffn_gate_exps.weight, whatever
    feed_forward_length says."""
    from mipipe.engine import Engine
    path = _write_with(tmp_path, "nokey", {"qwen3moe.feed_forward_length": 6144}, drop=("qwen3moe.expert_feed_forward_length",))
    with Engine(gguf=path, backend="cpu", max_ctx=64, threads=2) as eng:
        assert eng.info["model"]["expert_d_ff"] == 256
        out, _ = eng.generate([[5, 6, 7]], 2)
        assert len(out[0]) == 2


def test_reference_moe_ties_and_margins():
    """RefLlama._moe resolves equal router logits to the lower expert index and records
    l_(k) - l_(k+1) and the row RMS."""
    import torch
    from mipipe.models.reference import RefLlama
    E, k, d, F = 6, 2, 4, 3
    hp = dict(n_layer=1, d_model=d, n_head=1, n_head_kv=1, head_dim=4, d_ff=F, rope_base=1e4, eps=1e-6, n_expert=E,
              n_expert_used=k)
    router = np.zeros((E, d), np.float32)
    router[:, 0] = [1, 3, 3, 3, 0, 2]          # x = e0 -> logits 1 3 3 3 0 2: top-2 must be experts 1, 2
    rng = np.random.default_rng(0)
    t = {"token_embd.weight": np.zeros((2, d), np.float32), "blk.0.ffn_gate_inp.weight": router,
         "blk.0.ffn_gate_exps.weight": rng.standard_normal((E, F, d)).astype(np.float32),
         "blk.0.ffn_up_exps.weight": rng.standard_normal((E, F, d)).astype(np.float32),
         "blk.0.ffn_down_exps.weight": rng.standard_normal((E, d, F)).astype(np.float32)}
    ref = RefLlama(t, hp)
    h = torch.tensor([[1.0, 0, 0, 0]])
    out = ref._moe(h, "blk.0.", 0, 0)[0].numpy()

    def expert(e):
        g, u = t["blk.0.ffn_gate_exps.weight"][e] @ h[0].numpy(), t["blk.0.ffn_up_exps.weight"][e] @ h[0].numpy()
        return t["blk.0.ffn_down_exps.weight"][e] @ (g / (1 + np.exp(-g)) * u)
    np.testing.assert_allclose(out, 0.5 * expert(1) + 0.5 * expert(2), rtol=1e-5, atol=1e-6)
    (layer, pos, margin, rms), = ref.router_margins
    assert (layer, pos) == (0, 0) and margin[0] == 0.0   # l_(2) = l_(3) = 3
    assert rms[0] == pytest.approx(np.sqrt((1 + 9 + 9 + 9 + 0 + 4) / 6))
    ref.reset()
    assert ref.router_margins == []
