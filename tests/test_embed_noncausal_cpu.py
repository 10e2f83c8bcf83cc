"""Engine.embed on a model written with <arch>.attention.causal = false (tiny-qwen2), CPU backend,
against the torch fp32 oracle run with causal=False.  Bound: NMSE < 1e-8, as test_embed_cpu.py
(cpu_act="f32": the oracle's f32 arithmetic; only the key bound of the attention differs here)."""
import functools

import numpy as np
import pytest

from conftest import make_model
from test_embed_cpu import BOUND, nmse, pool, prompts_for

LENS = (37, 21, 5)   # prefill_chunk 48: 37 alone, then 21 + 5 packed; none is split
MODEL = ("tiny-qwen2", "Q4_K_M")


@functools.lru_cache(maxsize=None)
def setup(model_dir):   # (path, cfg, prompts, oracle rows [len][d] of each prompt), computed once
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, *MODEL, causal=False)
    ref = RefLlama.from_gguf(path)
    prompts = prompts_for(cfg, LENS)
    return path, cfg, prompts, [ref.rmsnorm(ref.forward(p, 0, want_logits=False, causal=False),
                                            ref.t["output_norm.weight"]).double().numpy() for p in prompts]


def cpu_engine(path, **kw):
    from mipipe.engine import Engine
    return Engine(**dict(dict(gguf=path, backend="cpu", cpu_act="f32", max_ctx=128, prefill_chunk=48, mb_size=4,
                              threads=4), **kw))


def cls_moves_with_the_last_token(eng, prompts, vocab):
    """Under the causal mask row 0 has seen one token: only a non-causal row 0 can change."""
    other = prompts[0][:-1] + [(prompts[0][-1] + 1) % vocab]
    return nmse(*eng.embed([prompts[0], other], pooling="cls"))


def check_engine(eng, cfg, prompts, rows, bound, chunk):
    assert eng.info["model"]["causal_attn"] is False and eng.info["embed_attention"] == "non-causal"
    for pooling in ("mean", "cls", "last"):
        for p, g, h in zip(prompts, eng.embed(prompts, pooling=pooling), rows):
            e = nmse(g, pool(h, pooling))
            print(f"{pooling} len {len(p)}: measured {e:.3g}")
            assert np.isfinite(g).all() and e <= bound, (pooling, len(p), e)
    assert cls_moves_with_the_last_token(eng, prompts, cfg.vocab) > 1e-4
    with pytest.raises(RuntimeError, match=f"prompt 0 has {chunk + 1} tokens, more than prefill_chunk = {chunk}"):
        eng.embed([[5] * (chunk + 1)])
    assert len(eng.embed([[5] * chunk])) == 1 and eng.idle_slots() == [0, 1, 2, 3]


def test_noncausal_embed_matches_reference(native, model_dir):
    path, cfg, prompts, rows = setup(model_dir)
    with cpu_engine(path) as eng:
        check_engine(eng, cfg, prompts, rows, BOUND, 48)


def test_embed_attention_causal_reproduces_the_causal_model(native, model_dir):
    """embed_attention="causal" on the non-causal file: bit for bit the vectors of the same weights in a
    file without the key (chunks of 16 split the prompts), and row 0 blind to the last token again."""
    path, cfg, prompts, _ = setup(model_dir)
    plain, _ = make_model(model_dir, *MODEL)
    with cpu_engine(plain, prefill_chunk=16) as eng:
        assert eng.info["model"]["causal_attn"] is True and eng.info["embed_attention"] == "causal"
        want = {pl: eng.embed(prompts, pooling=pl) for pl in ("mean", "cls", "last")}
    with cpu_engine(path, prefill_chunk=16, embed_attention="causal") as eng:
        for pl, w in want.items():
            assert all(np.array_equal(g, v) for g, v in zip(eng.embed(prompts, pooling=pl), w)), pl
        assert cls_moves_with_the_last_token(eng, prompts, cfg.vocab) == 0.0
    with pytest.raises(RuntimeError, match="embed_attention"):
        cpu_engine(path, embed_attention="bidirectional")
