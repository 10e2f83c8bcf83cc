"""Engine.embed on a file with <arch>.attention.causal = false through the HIP engine
(HipStage::attention_encode, attn_encode.hip) against the torch oracle run with causal=False.  Bound:
BOUND_F16 of test_embed_engine_gpu.py (the layers' f16-MFMA error, which the key bound does not change)."""
import numpy as np
import pytest

from test_embed_engine_gpu import BOUND_F16
from test_embed_noncausal_cpu import check_engine, prompts_for, setup

pytestmark = pytest.mark.gpu


def gpu_engine(path, **kw):
    from mipipe.engine import Engine
    return Engine(**dict(dict(gguf=path, max_ctx=256, prefill_chunk=48, mb_size=4), **kw))


@pytest.mark.parametrize("kw", [dict(), dict(stages=2, devices=[0, 0], v_blocked=False)], ids=["pp1", "pp2-vt"])
def test_noncausal_embed_matches_reference(cuda, native, model_dir, kw):
    path, cfg, prompts, rows = setup(model_dir)
    with gpu_engine(path, **kw) as eng:
        check_engine(eng, cfg, prompts, rows, BOUND_F16, 48)
        assert eng.kv_stats()["kv_free_pages"] == eng.kv_stats()["kv_pages"]


def test_noncausal_embed_leaves_a_running_generation_alone(cuda, native, model_dir):
    """A greedy sequence in slot 0 (causal, captured decode graphs) keeps its tokens with embeds between rounds."""
    path, cfg, prompts, rows = setup(model_dir)
    gen_prompt = prompts_for(cfg, (11,), seed=5)[0]

    def run(with_embed):
        with gpu_engine(path, deterministic=True) as eng:
            caps = lambda: eng.health()["stages"][-1]["graph_captures"]
            eng.start([gen_prompt])
            c0 = caps()
            for r in range(4):
                eng.decode(2)
                if with_embed:
                    assert all(np.isfinite(x).all() for x in eng.embed(prompts[r % 2:r % 2 + 2], pooling="mean"))
            assert caps() == c0 and eng.idle_slots() == [1, 2, 3]
            return eng.tokens()[0]
    assert run(False) == run(True)
