"""The later stages of the sampler chain through the engine: slots of one micro-batch that mix them
with a greedy row, the sampling dict's round trip, a checkpoint, and the refused values (on the CPU
backend, whose host chain follows the same definitions)."""
import numpy as np
import pytest

from conftest import make_model

# one prompt in four slots: greedy; only the maximum survives (temperature and seed do not matter);
# the top token of two always removed; several stages on at once
RECS = [dict(temp=0.0), dict(temp=1.5, top_n_sigma=1e-4, seed=7),
        dict(temp=1.0, xtc_probability=1.0, xtc_threshold=0.0, top_k=2, seed=7),
        dict(temp=1.0, typical_p=0.7, top_p=0.95, dynatemp_range=0.5, dynatemp_exponent=2.0, seed=9)]
NEW = ("top_n_sigma", "typical_p", "xtc_probability", "xtc_threshold", "dynatemp_range", "dynatemp_exponent")

def _engine(path, **kw):
    from mipipe.engine import Engine
    return Engine(**{**dict(gguf=path, max_ctx=128, prefill_chunk=16, n_mb=1, mb_size=4, row_sampling=True), **kw})

def _mixed_slots(eng, cfg, steps):
    """Every step: slot 1's token is slot 0's; slot 2 draws the second largest logit of its own row."""
    eng.start([[int(t) for t in np.random.default_rng(21).integers(3, cfg.vocab, 13)]] * 4, sampling=RECS)
    for _ in range(steps):
        lg, toks = eng.logits(rows=4), eng.tokens()
        assert toks[1][-1] == toks[0][-1]
        assert toks[2][-1] == np.argsort(-lg[2].astype(np.float64), kind="stable")[1]
        eng.decode(1)
    return eng.tokens()

@pytest.mark.gpu
def test_mixed_slots_round_trip_and_checkpoint(cuda, native, model_dir, tmp_path):
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    with _engine(path, deterministic=True) as eng:
        _mixed_slots(eng, cfg, 6)
        got = [eng.slot_sampling(i) for i in range(4)]
        assert not any(k in got[0] for k in NEW)
        assert [{k: g[k] for k in NEW if k in g} for g in got[1:]] == [
            dict(top_n_sigma=float(np.float32(1e-4))), dict(xtc_probability=1.0, xtc_threshold=0.0),
            dict(typical_p=float(np.float32(0.7)), dynatemp_range=0.5, dynatemp_exponent=2.0)]
        eng.save_state(str(tmp_path / "ck"))
        eng.decode(6)
        want = eng.tokens()
    with _engine(path, deterministic=True) as eng:
        eng.load_state(str(tmp_path / "ck"))
        assert [eng.slot_sampling(i) for i in range(4)] == got
        eng.decode(6)
        assert eng.tokens() == want
    assert len(set(want[3])) > 3 and want[3] != want[0]

def test_cpu_engine_same_requests_and_refusals(native, model_dir):
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    with _engine(path, backend="cpu", cpu_act="f32", threads=4) as eng:
        assert len(set(_mixed_slots(eng, cfg, 4)[3])) > 1
        eng.release(0)
        for field, v in (("typical_p", 0), ("xtc_probability", 1.5), ("dynatemp_exponent", 0)):
            with pytest.raises(RuntimeError, match=field):
                eng.set_slot_sampling(0, temp=1.0, **{field: v})
        eng.set_slot_sampling(0, temp=1.0, top_n_sigma=-1.0, typical_p=1.0)   # what llama.cpp's clients send for "off"
        assert not any(k in eng.slot_sampling(0) for k in NEW)
