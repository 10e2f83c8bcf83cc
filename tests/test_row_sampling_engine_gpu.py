"""Per-request sampling through the HIP engine (row_sampling): the last stage's table, the order of
head() and the draw-index rule, checked against the logits the sampler itself saw.  eng.logits()
returns them as head() left them (bias and penalties applied in place), so each row's token is
compared with the float64 oracle of test_sampler_oracle_gpu for the row's own record and draw
index; that is robust to the order of the split-K atomics, which moves the logits, not the rule."""
import numpy as np
import pytest

from conftest import make_model
from test_sampler_oracle_gpu import TOL, draw_cdf, interval_distance, kept_set, uniform

pytestmark = pytest.mark.gpu


def near_tie(row, a, b):
    """The near-tie rule of test_engine_matches_reference."""
    return abs(row[a] - row[b]) < 1e-2 * (np.abs(np.sort(row)[-2:]).max() + 1)


def _prompts(cfg):
    rng = np.random.default_rng(11)
    return [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (19, 7, 33, 12)]


def _engine(path, **kw):
    from mipipe.engine import Engine
    cfg = dict(gguf=path, max_ctx=256, prefill_chunk=16, n_mb=1, mb_size=4, row_sampling=True)
    cfg.update(kw)
    return Engine(**cfg)


def _check(row, rec, d, tok):
    """One token against the logits its row's sampler saw."""
    if rec.get("temp", 0.0) <= 0:
        am = int(np.argmax(row))
        assert tok == am or near_tie(row, tok, am), (tok, am)
        return 0.0
    keep = kept_set(row, rec.get("top_k", 0), rec.get("top_p", 1.0), rec.get("min_p", 0.0))
    cdf = draw_cdf(row, keep, rec["temp"])
    dist = float(interval_distance(cdf, np.array([tok]), np.array([uniform(rec["seed"], d, 0)]))[0])
    assert dist <= TOL, (rec, d, tok, dist)
    return dist


@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("graphs", [True, False])
def test_rows_follow_their_own_records(cuda, native, model_dir, stages, graphs):
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    ps = _prompts(cfg)
    with _engine(path, row_sampling=False, mb_size=1) as eng:     # what slot 2 would say first without its ban
        eng.start([ps[2]])
        banned = eng.tokens()[0][0]
    recs = [dict(temp=0.0),
            dict(temp=0.9, top_k=40, repeat=1.3, freq=0.2, presence=0.1, seed=77),
            dict(temp=0.0, logit_bias=[[banned, False]]),
            dict(temp=1.1, top_p=0.9, seed=(1 << 63) + 5, logit_bias=[[banned, False], [3, 2.5]])]
    worst = 0.0
    with _engine(path, stages=stages, devices=[0] * stages, graphs=graphs) as eng:
        caps = lambda: eng.health()["stages"][-1]["graph_captures"]

        def step(live, fresh=()):
            """rows `live` produced a token in the last engine call (after an admit only the admitted rows did)"""
            nonlocal worst
            lg, toks = eng.logits(rows=4), eng.tokens()
            for i in (fresh or live):
                d = len(toks[i]) - 1
                worst = max(worst, _check(lg[i].astype(np.float64), recs[i], d, toks[i][-1]))

        eng.start(ps[:2], sampling=recs[:2])
        c0 = caps()
        assert c0 >= 1
        step([0, 1])
        for _ in range(2):
            eng.decode(1)
            step([0, 1])
        eng.admit([2], [ps[2]], sampling=[recs[2]])
        step([0, 1, 2], fresh=[2])
        eng.decode(1)
        step([0, 1, 2])
        eng.admit([3], [ps[3]], sampling=[recs[3]])
        step([0, 1, 2, 3], fresh=[3])
        for _ in range(4):
            eng.decode(1)
            step([0, 1, 2, 3])
        assert caps() == c0, "an admit must not re-capture the decode graphs"
        toks = eng.tokens()
        assert eng.slot_sampling(3)["seed"] == (1 << 63) + 5
    assert [len(t) for t in toks] == [8, 8, 6, 5]
    assert banned not in toks[2] and banned not in toks[3]
    assert toks[2][0] != banned
    print(f"row_sampling engine stages={stages} graphs={graphs}: worst {worst:.3e}")


def test_checkpoint(cuda, native, model_dir, tmp_path):
    """save_state / load_state, PP = 1, deterministic: the uninterrupted tokens."""
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    ps = _prompts(cfg)
    samp = [dict(temp=0.9, seed=11), dict(temp=0.0, logit_bias=[[17, False]]),
            dict(temp=1.2, top_k=30, repeat=1.3, seed=12), dict(temp=1.0)]
    with _engine(path, deterministic=True) as eng:
        eng.start(ps, sampling=samp)
        eng.decode(5)
        eng.save_state(str(tmp_path / "ck"))
        eng.decode(7)
        want = eng.tokens()
    with _engine(path, deterministic=True) as eng:
        eng.load_state(str(tmp_path / "ck"))
        eng.decode(7)
        got = eng.tokens()
    assert got == want and len(set(want[0])) > 3


def test_default_off(cuda, native, model_dir):
    """All slots at the defaults and greedy: the tokens of an engine without the key (deterministic, so
    the two runs see the same logits); without the key set_slot_sampling raises."""
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    ps = _prompts(cfg)
    with _engine(path, row_sampling=False, deterministic=True) as eng:
        ref, _ = eng.generate(ps, 12)
        with pytest.raises(RuntimeError, match="row_sampling"):
            eng.set_slot_sampling(0, temp=1.0)
    with _engine(path, deterministic=True) as eng:
        out, _ = eng.generate(ps, 12)
    assert out == ref
