"""The lifecycle of per-slot settings on the CPU backend (no GPU): token masks and adapter bindings
share one three-state lifecycle in the engine (off, set for the next admission, in use), and one
table of scenarios is run for both through the public Python API.

A mask that allows the single token id FORCED forces that token; a binding shows in eng.logits():
the logits differ from the base model's.  "Off" is only ever asserted where the slot's KV holds
nothing computed under the setting (after a prefill, or after load_state()), so it means equality
with an engine that never saw the setting: the same tokens, bit-identical logits.

n_mb=2, mb_size=2: eng.logits() holds the rows of the last micro-batch whose head ran, so the slots
observed are 2 and 3 (micro-batch 1) while slots 0 and 1 keep generating beside them."""
import numpy as np
import pytest

from conftest import make_model
from lora_helpers import make_adapter, nmse
from test_lora_cpu import MIN_EFFECT, cpu_engine

FORCED = 7     # the one token a mask allows (the base model generates it at none of the observed points)
SCALE = 1.0


@pytest.fixture(scope="module")
def world(native, model_dir):
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    pa, _ = make_adapter(model_dir, path, cfg, seed=11)
    rng = np.random.default_rng(8)
    prompts = [[int(t) for t in rng.integers(8, cfg.vocab, n)] for n in (6, 9, 7, 11)]
    return dict(path=path, cfg=cfg, pa=pa, prompts=prompts)


def engine(world):
    eng = cpu_engine(world["path"], n_mb=2, mb_size=2, row_masks=True, lora_adapters=2)
    assert eng.load_adapter(world["pa"]) == 0
    return eng


def snap(eng):
    """What the observed slots (2, 3) show now: their last tokens and their logits rows."""
    toks = eng.tokens()
    return [toks[s][-1] if s < len(toks) and toks[s] else None for s in (2, 3)], eng.logits(rows=2).copy()


class Masks:
    kw = "masks"

    def __init__(self, world):
        m = np.zeros((world["cfg"].vocab + 31) // 32, np.uint32)
        m[FORCED >> 5] = 1 << (FORCED & 31)
        self.value = m

    def set(self, eng, slots):
        eng.set_slot_masks(slots, [self.value] * len(slots))

    def is_on(self, got, base, row):
        assert base[0][row] != FORCED          # the precondition: the mask matters
        return got[0][row] == FORCED

    def is_off(self, got, base, row):
        return got[0][row] == base[0][row] != FORCED


class Bindings:
    kw = "adapters"

    def __init__(self, world):
        self.value = (0, SCALE)

    def set(self, eng, slots):
        eng.set_slot_adapters(slots, [0] * len(slots), [SCALE] * len(slots))

    def is_on(self, got, base, row):           # (the precondition and the observation are one: the adapter matters)
        return nmse(got[1][row], base[1][row]) >= MIN_EFFECT

    def is_off(self, got, base, row):
        return np.array_equal(got[1][row], base[1][row])


# Every scenario is a generator run twice over the same calls: once with feat=None on an engine that
# never sees the setting (the base), once with the feature.  It yields (label, expected) after each
# call to observe, expected = per observed slot (2, 3) True: on, False: off, None: not looked at.
def idle_set_holds_for_start(eng, feat, w, tmp):
    P = w["prompts"]
    if feat: feat.set(eng, [3])
    eng.start(P)
    yield "start", (False, True)
    eng.decode(1)
    yield "decode", (None, True)


def idle_set_holds_for_admit(eng, feat, w, tmp):
    P = w["prompts"]
    eng.start(P[:3])
    eng.decode(1)
    if feat: feat.set(eng, [3])
    eng.admit([3], [P[3]])
    yield "admit", (None, True)
    eng.decode(1)
    yield "decode", (None, True)
    eng.release(2)
    eng.admit([2], [P[2]])
    yield "neighbour re-admitted", (False, None)


def passed_to_start_for_busy_slot(eng, feat, w, tmp):
    P = w["prompts"]
    eng.start(P)
    eng.decode(1)                              # slot 3 is never released: still busy with this generation
    eng.start(P, **({feat.kw: [None, None, None, feat.value]} if feat else {}))
    yield "start", (False, True)
    eng.decode(1)
    yield "decode", (None, True)


def set_while_running_gone_after_start(eng, feat, w, tmp):
    P = w["prompts"]
    eng.start(P)
    eng.decode(1)
    if feat: feat.set(eng, [3])
    eng.decode(1)
    yield "decode", (None, True)
    eng.start(P)
    yield "start", (False, False)


def release_clears_only_that_slot(eng, feat, w, tmp):
    P = w["prompts"]
    eng.start(P, **({feat.kw: [None, None, feat.value, feat.value]} if feat else {}))
    yield "start", (True, True)
    eng.release(2)
    eng.admit([2], [P[2]])
    yield "admit", (False, None)
    eng.decode(1)
    yield "decode", (None, True)


def load_state_clears_all(eng, feat, w, tmp):
    P = w["prompts"]
    eng.start(P[:3])
    eng.decode(1)
    eng.save_state(str(tmp))
    if feat: feat.set(eng, [2, 3])             # slot 2 runs: in use at once; slot 3 is idle: set for its admission
    eng.load_state(str(tmp))
    eng.decode(1)
    yield "decode", (False, None)              # (nothing was computed under the setting: equal to the base)
    eng.admit([3], [P[3]])
    yield "admit", (None, False)


SCENARIOS = [idle_set_holds_for_start, idle_set_holds_for_admit, passed_to_start_for_busy_slot,
             set_while_running_gone_after_start, release_clears_only_that_slot, load_state_clears_all]


@pytest.fixture(scope="module")
def base_runs(world, tmp_path_factory):
    """Each scenario once without any setting: the snapshots the feature runs are compared against."""
    out = {}
    for sc in SCENARIOS:
        with engine(world) as eng:
            out[sc.__name__] = [snap(eng) for _ in sc(eng, None, world, tmp_path_factory.mktemp("base"))]
    return out


@pytest.mark.parametrize("feature", [Masks, Bindings], ids=["masks", "bindings"])
@pytest.mark.parametrize("scenario", SCENARIOS, ids=[s.__name__ for s in SCENARIOS])
def test_lifecycle(world, base_runs, tmp_path, scenario, feature):
    feat = feature(world)
    base = base_runs[scenario.__name__]
    with engine(world) as eng:
        n = 0
        for k, (label, expected) in enumerate(scenario(eng, feat, world, tmp_path)):
            got = snap(eng)
            for row, want in enumerate(expected):
                if want is None:
                    continue
                ok = feat.is_on(got, base[k], row) if want else feat.is_off(got, base[k], row)
                assert ok, (scenario.__name__, feat.kw, label, "slot %d" % (2 + row), "on" if want else "off",
                            got[0], base[k][0])
            n += 1
        assert n == len(base)
