"""Per-request sampling (engine key row_sampling) on the CPU backend: a request's tokens depend on
its own record (cuts, penalties, bias, seed, draw index) and on nothing else -- not on its slot, its
micro-batch, the round it was admitted in or what the other rows do."""
import numpy as np
import pytest

from conftest import make_model

N_TOK = 24
R = dict(temp=0.9, top_k=40, seed=1234)


def _model(model_dir):
    return make_model(model_dir, "tiny-gqa", "Q8_0")


def _engine(path, **kw):
    from mipipe.engine import Engine
    cfg = dict(gguf=path, backend="cpu", max_ctx=128, n_mb=2, mb_size=4, prefill_chunk=16, threads=4, row_sampling=True)
    cfg.update(kw)
    return Engine(**cfg)


def _prompts(cfg):
    rng = np.random.default_rng(5)
    return [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (7, 12, 3, 9)]


@pytest.fixture(scope="module")
def run_a(native, model_dir):
    """Request R alone in slot 0 of an otherwise idle engine: (prompt, its 24 tokens)."""
    path, cfg = _model(model_dir)
    P = _prompts(cfg)[0]
    with _engine(path) as eng:
        eng.start([P], sampling=[R])
        eng.decode(N_TOK - 1)
        toks = eng.tokens()[0]
        assert eng.slot_sampling(0)["seed"] == 1234
    assert len(toks) == N_TOK and len(set(toks)) > 4
    return P, toks


def test_slot_and_time_independence(native, model_dir, run_a):
    """R admitted alone into slot 5 at round 6, beside three other requests with other settings."""
    path, cfg = _model(model_dir)
    P, want = run_a
    others = _prompts(cfg)[1:]
    with _engine(path) as eng:
        eng.start(others, sampling=[dict(temp=1.3, seed=1), dict(temp=0.0), dict(temp=0.7, top_p=0.8, seed=77)])
        eng.decode(6)
        before = eng.health()["stages"][-1]["graph_captures"]
        eng.admit([5], [P], sampling=[R])
        eng.decode(N_TOK - 1)
        got = eng.tokens()[5]
        assert eng.health()["stages"][-1]["graph_captures"] == before
    assert got == want


def test_greedy_beside_sampled(native, model_dir):
    """A greedy row beside three sampled rows gives the text of an all-greedy engine without row_sampling."""
    path, cfg = _model(model_dir)
    ps = _prompts(cfg)
    with _engine(path, row_sampling=False) as eng:
        ref, _ = eng.generate([ps[2]], 16)
    with _engine(path) as eng:
        eng.start(ps, sampling=[dict(temp=1.1, seed=3), dict(temp=0.8, top_k=20, seed=4), dict(temp=0.0),
                                dict(temp=1.5, min_p=0.05, seed=5)])
        eng.decode(15)
        toks = eng.tokens()
    assert toks[2] == ref[0]
    assert toks[0] != toks[2] and toks[1] != toks[2]


def test_draw0_continues_the_stream(native, model_dir, run_a):
    """P + the first 10 tokens with draw0 = 10 continues with tokens 11..24 of run A."""
    path, cfg = _model(model_dir)
    P, want = run_a
    with _engine(path) as eng:
        eng.start([[3, 4, 5]])
        eng.decode(2)
        eng.admit([6], [P + want[:10]], sampling=[dict(R, draw0=10)])
        eng.decode(N_TOK - 11)
        got = eng.tokens()[6]
    assert got == want[10:]


def test_default_seeds(native, model_dir):
    """Two requests without a seed get different reported seeds; a reported seed reproduces the text."""
    path, cfg = _model(model_dir)
    P = _prompts(cfg)[1]
    with _engine(path) as eng:
        eng.start([P, P], sampling=[dict(temp=1.0), dict(temp=1.0)])
        s0, s1 = eng.slot_sampling(0)["seed"], eng.slot_sampling(1)["seed"]
        eng.decode(15)
        t = eng.tokens()
    assert s0 != s1 and t[0] != t[1]
    with _engine(path) as eng:
        eng.start([[9, 9]], sampling=[dict(temp=0.5, seed=2)])
        eng.admit([3], [P], sampling=[dict(temp=1.0, seed=s1)])
        eng.decode(15)
        assert eng.tokens()[3] == t[1]
        assert eng.slot_sampling(3)["seed"] == s1


def test_checkpoint(native, model_dir, tmp_path):
    """save_state after 8 rounds, load_state in a fresh engine: the uninterrupted tokens."""
    path, cfg = _model(model_dir)
    ps = _prompts(cfg)
    samp = [dict(temp=0.9, seed=11), dict(temp=0.0, logit_bias=[[17, False]]), dict(temp=1.2, top_k=30, repeat=1.3, seed=12),
            dict(temp=1.0)]
    with _engine(path) as eng:
        eng.start(ps, sampling=samp)
        eng.decode(8)
        eng.save_state(str(tmp_path / "ck"))
        recs = [eng.slot_sampling(i) for i in range(4)]
        eng.decode(10)
        want = eng.tokens()
    with _engine(path) as eng:
        eng.load_state(str(tmp_path / "ck"))
        assert [eng.slot_sampling(i) for i in range(4)] == recs
        eng.decode(10)
        got = eng.tokens()
    assert got == want


def test_refusals(native, model_dir):
    path, cfg = _model(model_dir)
    with _engine(path, row_sampling=False) as eng:
        with pytest.raises(RuntimeError, match="row_sampling"):
            eng.set_slot_sampling(0, temp=1.0)
    with _engine(path) as eng:
        eng.set_slot_sampling(1, temp=1.0, logit_bias=[[i, 1.0] for i in range(32)])
        with pytest.raises(RuntimeError, match="n_bias"):
            eng.set_slot_sampling(1, logit_bias=[[i, 1.0] for i in range(33)])
        for bad, field in ((dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(min_p=-0.1), "min_p"),
                           (dict(repeat=0.0), "repeat"), (dict(logit_bias=[[cfg.vocab, 1.0]]), "logit_bias id"),
                           (dict(temp=float("nan")), "temp")):
            with pytest.raises(RuntimeError, match=field):
                eng.set_slot_sampling(1, **bad)
        eng.start([[5, 6, 7]])
        with pytest.raises(RuntimeError, match="busy"):
            eng.set_slot_sampling(0, temp=1.0)
        eng.set_slot_sampling(1, temp=1.0)      # an idle slot takes a record while the engine runs
        eng.release(0)
        eng.set_slot_sampling(0, temp=1.0)
        with pytest.raises(RuntimeError, match="row_sampling"):
            eng.spec_generate([[5, 6, 7]], 4)


def test_logprobs_stay_raw_under_bias(native, model_dir):
    """n_probs = -1: a greedy row with +100 on token X emits X every step, and its recorded logprobs
    are those of the RAW logits: equal to Engine.score(P + generated) at those positions (both sides
    are computed in double from the same logits)."""
    path, cfg = _model(model_dir)
    P = _prompts(cfg)[3]
    X = 321
    with _engine(path, n_probs=-1) as eng:
        eng.start([[4, 5, 6], P], sampling=[dict(temp=1.0, seed=1), dict(temp=0.0, logit_bias={str(X): 100.0})])
        eng.decode(7)
        toks = eng.tokens()[1]
        lp = np.asarray(eng.logprobs()[1][0], np.float64)
        assert toks == [X] * 8
        ref = np.asarray(eng.score([P + toks])[0], np.float64)[len(P) - 1:]
    assert lp.shape == ref.shape == (8,)
    assert (lp < -1.0).any()            # X is not what the raw distribution favours
    assert np.abs(lp - ref).max() <= 1e-5, np.abs(lp - ref).max()
