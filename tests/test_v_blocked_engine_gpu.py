"""Engine option v_blocked (blocked V pages, the default) against v_blocked=false (V^T pages): the
layout only changes addresses, so logits are bitwise equal, and saved state (always V^T pages) moves
between the two layouts.  The engines run deterministic: the default mode's split-K float atomics
are not bitwise repeatable from run to run whatever the layout."""
import numpy as np
import pytest

from conftest import make_model

pytestmark = pytest.mark.gpu

LENS = (37, 70, 5, 63)   # prefill chunks of 16 cross 8-key blocks and a page; decode crosses 63 -> 64


def _prompts(cfg, n):
    rng = np.random.default_rng(21)
    return [[int(t) for t in rng.integers(3, cfg.vocab, m)] for m in LENS[:n]]


def _engine(path, v_blocked, kv, mb):
    from mipipe.engine import Engine
    return Engine(gguf=path, max_ctx=256, mb_size=mb, prefill_chunk=16, kv_dtype=kv, deterministic=True,
                  v_blocked=v_blocked)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("kv", ["f16", "fp8"])
@pytest.mark.parametrize("mb", [1, 4])
def test_logits_bitwise_equal_between_layouts(cuda, native, model_dir, mb, kv):
    """Prefill and 4 decode steps: single stream (the q|k|v GEMV's append epilogue, the prefetch
    forms) and a micro-batch of 4."""
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    ps = _prompts(cfg, mb)
    runs = []
    for vb in (True, False):
        with _engine(path, vb, kv, mb) as eng:
            eng.start(ps)
            lgs = [eng.logits(rows=mb)]
            for _ in range(4):
                eng.decode(1)
                lgs.append(eng.logits(rows=mb))
            runs.append((lgs, eng.tokens()))
    assert runs[0][1] == runs[1][1]
    for step, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
        assert np.isfinite(np.asarray(a)).all()
        assert _same(a, b), f"logits differ at step {step}"


@pytest.mark.parametrize("kv", ["f16", "fp8"])
@pytest.mark.parametrize("saved_blocked", [True, False], ids=["blocked-to-vt", "vt-to-blocked"])
def test_state_moves_between_layouts(cuda, native, model_dir, tmp_path, saved_blocked, kv):
    """save_state under one layout, load_state under the other: the next step's logits are those
    of the uninterrupted run, bitwise."""
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    mb = 4
    ps = _prompts(cfg, mb)
    with _engine(path, saved_blocked, kv, mb) as eng:
        eng.start(ps)
        eng.decode(2)
        eng.save_state(str(tmp_path / "ck"))
        eng.decode(1)
        want, want_tok = eng.logits(rows=mb), eng.tokens()
    with _engine(path, not saved_blocked, kv, mb) as eng:
        eng.load_state(str(tmp_path / "ck"))
        eng.decode(1)
        got, got_tok = eng.logits(rows=mb), eng.tokens()
    assert got_tok == want_tok
    assert _same(got, want)
