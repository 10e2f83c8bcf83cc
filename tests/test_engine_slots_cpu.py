"""The engine's per-slot bookkeeping on the CPU backend (no GPU): a session that load_state() rejects
leaves a running engine as it was, and the number of sequences the engine reports follows its calls."""
import json

import numpy as np
import pytest

from conftest import make_model

KW = dict(backend="cpu", n_mb=2, mb_size=2, max_ctx=64, prefill_chunk=16)
PROMPTS = [[5, 6, 7, 8, 9], [10, 11, 12], [13, 14, 15, 16], [17, 18]]


@pytest.fixture(scope="module")
def gqa(native, model_dir):
    return make_model(model_dir, "tiny-gqa", "Q8_0")


def run_until_saved(eng, d):
    eng.start(PROMPTS[:2])
    eng.decode(2)
    eng.save_state(str(d))


@pytest.fixture(scope="module")
def uninterrupted(gqa, tmp_path_factory):
    """The same calls without a failed load: start, 2 rounds, save, 3 rounds."""
    from mipipe.engine import Engine
    with Engine(gguf=gqa[0], **KW) as eng:
        run_until_saved(eng, tmp_path_factory.mktemp("twin"))
        eng.decode(3)
        return eng.tokens()


def too_long(j, vocab):
    j["prompts"][0] = list(range(3, 3 + 70))            # longer than max_ctx


def bad_id(j, vocab):
    j["generated"][1][0] = vocab + 5                    # a token id out of range


def future_round(j, vocab):
    j["base_round"] = [0, j["rounds_done"] + 3]         # admitted in the future


@pytest.mark.parametrize("corrupt", [too_long, bad_id, future_round], ids=lambda f: f.__name__)
def test_rejected_load_state_leaves_running_engine(gqa, uninterrupted, tmp_path, corrupt):
    """load_state() validates session.json before it touches the engine: after the rejected load the
    running generation goes on as if the call had not been made."""
    from mipipe.engine import Engine
    path, cfg = gqa
    with Engine(gguf=path, **KW) as eng:
        run_until_saved(eng, tmp_path)
        before = (eng.tokens(), [eng.slot_position(s) for s in range(4)], eng.idle_slots())
        j = json.loads((tmp_path / "session.json").read_text())
        corrupt(j, cfg.vocab)
        (tmp_path / "session.json").write_text(json.dumps(j))
        with pytest.raises(RuntimeError, match="load_state"):
            eng.load_state(str(tmp_path))
        assert (eng.tokens(), [eng.slot_position(s) for s in range(4)], eng.idle_slots()) == before
        eng.decode(3)
        assert eng.tokens() == uninterrupted


def listed(eng):
    """The sequences the engine itself lists (mp_engine_tokens writes one row per sequence, whatever
    the caller's count; the Python wrapper keeps a count of its own, which score() does not change)."""
    from mipipe import _native as N
    cap = max(N.check(N.lib().mp_engine_tokens_longest(eng._h), "tokens"), 1)
    out = np.full((eng.n_seq_cap, cap), -2, np.int32)
    N.check(N.lib().mp_engine_tokens(eng._h, out.ctypes.data, eng.n_seq_cap, cap), "tokens")
    return [[t for t in row if t >= 0] for row in out.tolist() if row[0] != -2]


def test_sequence_count_contract(gqa):
    """How many sequences tokens() lists after each call, each with one token per round since its
    admission (released slots included: their rows keep computing)."""
    from mipipe.engine import Engine
    path, cfg = gqa
    with Engine(gguf=path, **KW) as eng:
        def check(*lens):
            got = listed(eng)
            assert [len(t) for t in got] == list(lens)
            assert all(0 <= t < cfg.vocab for seq in got for t in seq)
            return got

        eng.start(PROMPTS[:3])
        assert check(1, 1, 1) == eng.tokens()              # the short list before an admit
        eng.decode(2)
        check(3, 3, 3)
        eng.release(1)
        check(3, 3, 3)
        eng.admit([3], [PROMPTS[3]])
        assert check(3, 3, 3, 1) == eng.tokens()           # every slot from the first admit on
        eng.decode(2)
        check(5, 5, 5, 3)
        eng.score(PROMPTS[:2])
        check()                                            # scoring ends the generation: none listed
        eng.start(PROMPTS[:1])
        assert check(1) == eng.tokens()
        eng.embed([PROMPTS[1]], slots=[2])
        check(1)                                           # an embedding in an idle slot is no sequence
