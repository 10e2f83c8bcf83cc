"""Context shift on the host: KvPager::shift, the CPU backend's kv_shift, the engine's bookkeeping,
automatic shifting ("context_shift": true), the refusals, and the command-line surface.

The definition under test (engine.h, Engine::context_shift): positions [n_keep, n_keep + n_discard) of
a slot leave its KV, every later entry moves n_discard back with V unchanged and K rotated by minus
n_discard positions.  With ONE layer a token's K / V depend on the token and its position only, so the
shifted cache must be the cache of the spliced token list, and the next logits must match a fresh
engine started on tokens[:n_keep] + tokens[n_keep + n_discard:] (f32 throughout: cpu_act "f32"; the only
difference is rotating by p and then by -n_discard instead of by p - n_discard once).
Measured nmse of that comparison over the eight cases: 5.5e-14 .. 1.7e-13 (bound 1e-6).
"""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, make_model

TRASH = 12   # n_pages of the pager cases below


def _pager(native, tokens, slot, n_keep, n_discard, n_slots=3, max_pages=8, n_pages=TRASH):
    tok = np.asarray(tokens, np.int32)
    table = np.zeros((n_slots, max_pages), np.int32)
    free = np.full(n_pages, -1, np.int32)
    n_free = np.zeros(1, np.int32)
    merge = np.zeros(1, np.int32)
    owned = native.mp_kvpager_shift(n_slots, max_pages, n_pages, tok.ctypes.data, slot, n_keep, n_discard,
                                    table.ctypes.data, free.ctypes.data, n_free.ctypes.data, merge.ctypes.data)
    if owned < 0:
        raise RuntimeError(native.mp_last_error().decode())
    return owned, table, free[:n_free[0]].tolist(), int(merge[0])


def test_pager_shift_aligned(native):
    # slot 0: pages 0..1, slot 1: pages 2..6 (300 tokens), slot 2: page 7; free 8..11
    owned, table, free, merge = _pager(native, [100, 300, 10], 1, 64, 128)
    assert merge == -1 and owned == 3
    assert table[1].tolist() == [2, 5, 6] + [TRASH] * 5          # entries 1, 2 (pages 3, 4) left the row
    assert table[0].tolist() == [0, 1] + [TRASH] * 6 and table[2].tolist() == [7] + [TRASH] * 7
    assert free == [3, 4, 8, 9, 10, 11]                           # the next grants take 3, then 4


def test_pager_shift_merge(native):
    owned, table, free, merge = _pager(native, [100, 300, 10], 1, 5, 64)
    assert merge == 3 and owned == 4                              # old page n_keep/64 + n_discard/64 = entry 1
    assert table[1].tolist() == [2, 4, 5, 6] + [TRASH] * 4        # page 2 keeps rows < 5, takes page 3's rows >= 5
    assert free == [3, 8, 9, 10, 11]
    owned, table, free, merge = _pager(native, [0, 448, 0], 1, 70, 192)
    assert merge == 4 and owned == 4                              # pages 0..6: entry 1 stays, 2..4 leave
    assert table[1].tolist() == [0, 1, 5, 6] + [TRASH] * 4
    assert free == [2, 3, 4, 7, 8, 9, 10, 11]


def test_pager_shift_preconditions(native):
    for args, msg in [((1, 0, 0), "n_discard must be > 0"), ((1, 0, 32), "not a multiple of 64"),
                      ((1, -1, 64), "n_keep < 0"), ((1, 300, 64), "exceeds"), ((1, 1, 320), "exceeds"),
                      ((5, 0, 64), "bad slot")]:
        with pytest.raises(RuntimeError, match=msg):
            _pager(native, [100, 300, 10], *args)


def _nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / (b ** 2).sum())


def splice_nmse(path, n_keep, n_discard, L=200, **cfg):
    """nmse of the logits after context_shift(n_keep, n_discard) at position L against a fresh engine
    started on the spliced token list (both feed the same token at position L - n_discard)."""
    from mipipe.engine import Engine
    rng = np.random.default_rng(1234)
    with Engine(gguf=path, max_ctx=256, **cfg) as eng:
        toks = rng.integers(1, eng.info["model"]["vocab"], L).tolist()
        eng.start([toks])
        g0 = eng.tokens()[0][0]
        free0 = eng.kv_stats()["kv_free_pages"]
        eng.context_shift([0], [n_keep], [n_discard])
        assert eng.slot_position(0) == L - n_discard and eng.slot_shifts(0) == 1
        assert eng.kv_stats()["kv_free_pages"] == free0 + n_discard // 64
        eng.decode(1)
        got = eng.logits()[0].copy()
    with Engine(gguf=path, max_ctx=256, **cfg) as ref:
        ref.start([toks[:n_keep] + toks[n_keep + n_discard:] + [g0]])
        want = ref.logits()[0].copy()
    return _nmse(got, want)


@pytest.mark.parametrize("n_discard", [64, 128])
@pytest.mark.parametrize("n_keep", [0, 5, 64, 70])
def test_cpu_splice_equivalence(native, model_dir, n_keep, n_discard):
    path, _ = make_model(model_dir, "tiny-gqa", "Q8_0", n_layer=1)
    e = splice_nmse(path, n_keep, n_discard, backend="cpu", cpu_act="f32")
    print(f"n_keep {n_keep} n_discard {n_discard}: nmse {e:.3g}")
    assert e <= 1e-6


def _prompts(vocab):
    rng = np.random.default_rng(7)
    return [rng.integers(1, vocab, 100).tolist(), rng.integers(1, vocab, 30).tolist()]


def test_cpu_endless_generation(native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    prompts = _prompts(cfg.vocab)
    kw = dict(gguf=path, backend="cpu", max_ctx=256, n_mb=1, mb_size=2)
    with Engine(context_shift=True, n_keep=4, **kw) as eng:
        out, stats = eng.generate(prompts, 400)
        assert [len(o) for o in out] == [400, 400] and min(min(o) for o in out) >= 0
        assert eng.slot_shifts(0) in (3, 4) and eng.slot_shifts(1) >= 1
        assert eng.health()["context_shifts"] == eng.slot_shifts(0) + eng.slot_shifts(1) == stats["context_shifts"]
        # the same run step by step: the pool is never over-drawn, every shift returns its page
        eng.start(prompts)
        pool = eng.kv_stats()["kv_pages"]
        left = 399
        while left > 0:
            room = min(256 - eng.slot_position(s) - 1 for s in (0, 1))
            k = min(left, max(1, room))
            eng.decode(k)
            st = eng.kv_stats()
            assert 0 <= st["kv_free_pages"] <= pool == st["kv_pages"]
            assert all(eng.slot_position(s) < 256 for s in (0, 1))
            left -= k
        assert eng.tokens(cap=512) == out
        for s in (0, 1):
            eng.release(s)
        assert eng.kv_stats()["kv_free_pages"] == pool
    # shifting slot 0 does not disturb slot 1: its tokens up to its own first shift are those of an
    # engine without the option (slot 0 there holds a one-token prompt, so both fit 225 tokens)
    n = 256 - 30 - 1
    with Engine(**kw) as base:
        ref, _ = base.generate([[prompts[0][0]], prompts[1]], n)
        assert out[1][:n] == ref[1]
        # (200 tokens: one call's rounds are capped at max_ctx, and 100 + 199 + 1 > 256 already)
        with pytest.raises(RuntimeError, match="context capacity exhausted"):
            base.generate(prompts, 200)
        assert base.health()["context_shifts"] == 0


def test_cpu_shift_refusals(native, model_dir, tmp_path):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    prompts = _prompts(cfg.vocab)
    with Engine(gguf=path, backend="cpu", max_ctx=256, n_mb=1, mb_size=4) as eng:
        eng.start(prompts)
        eng.decode(3)
        for args, msg in [(([2], [0], [64]), "slot 2 is idle"), (([0], [0], [32]), "not a multiple of 64"),
                          (([0], [0], [0]), "n_discard must be > 0"), (([0], [-1], [64]), "n_keep < 0"),
                          (([0], [64], [64]), "exceeds its 103 cached positions"), (([9], [0], [64]), "out of range"),
                          (([0, 0], [0, 0], [64, 64]), "listed twice"), (([1], [0], [64]), "exceeds its 33")]:
            with pytest.raises(RuntimeError, match=msg):
                eng.context_shift(*args)
        assert eng.health()["context_shifts"] == 0 and eng.slot_position(0) == 103
        eng.save_state(str(tmp_path / "before"))
        eng.context_shift([0], [4], [64])
        assert eng.slot_position(0) == 39 and eng.slot_position(1) == 33
        with pytest.raises(RuntimeError, match="not supported after a context shift"):
            eng.save_state(str(tmp_path / "after"))
        eng.release(0)
        eng.save_state(str(tmp_path / "after"))   # the shifted sequence is gone
        eng.spec_generate(prompts, 8, draft_max=4)
        with pytest.raises(RuntimeError, match="not supported after speculative decoding"):
            eng.context_shift([0], [0], [64])
    with Engine(gguf=path, backend="cpu", max_ctx=256, context_shift=True) as eng:
        with pytest.raises(RuntimeError, match="draft_max > 0"):
            eng.spec_generate(prompts[:1], 8, draft_max=4)
    with pytest.raises(RuntimeError, match='mode "mp" is not supported'):
        Engine(gguf=path, backend="cpu", max_ctx=256, context_shift=True, mode="mp", world=1, rank=0)


def test_cpu_shifted_slot_is_no_prefix(native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    p = _prompts(cfg.vocab)[0]
    with Engine(gguf=path, backend="cpu", max_ctx=256) as eng:
        eng.start([p])
        eng.decode(2)
        r0 = eng.health()["prefix_reused_tokens"]
        eng.start([p])                                   # the control: an unshifted slot is a hit
        r1 = eng.health()["prefix_reused_tokens"]
        assert r1 == r0 + len(p) - 1
        eng.decode(2)
        eng.context_shift([0], [4], [64])
        eng.decode(2)                                    # refresh_slot_cache must not refill the entry
        eng.start([p])
        assert eng.health()["prefix_reused_tokens"] == r1
        first = eng.tokens()[0]
        eng.start([p])                                   # re-admitted: a prefix again
        assert eng.health()["prefix_reused_tokens"] == r1 + len(p) - 1 and eng.tokens()[0] == first


# ---------------------------------------------------------------- command line and server
BIN = os.path.join(REPO, "distributed-llm-pipeline_amd", "bin")
PROMPT = "The pipeline sends activations"


def _daemon(path, *flags, **req):
    p = subprocess.run([os.path.join(BIN, "mi-cli"), "-m", path, "-ngl", "0", "-c", "256", "--daemon", *flags],
                       input=json.dumps(dict(dict(prompt=PROMPT, n_predict=400), **req)) + "\n", capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = [json.loads(l) for l in p.stdout.splitlines()]
    return lines[-1], "".join(l["piece"] for l in lines[:-1])


def test_cli_context_shift(native, model_dir):
    path, _ = make_model(model_dir, "tiny-gqa", "Q8_0")
    on, text_on = _daemon(path, "--context-shift", "--keep", "4")
    assert on["done"] and on["n_gen"] == 400 and on["stop"] == "length" and on["n_shifts"] >= 2
    off, text_off = _daemon(path)                       # the default: the context ends the request
    assert off["stop"] == "context" and off["n_gen"] == 256 - off["n_prompt"] - 1 and off["n_shifts"] == 0
    no, text_no = _daemon(path, "--context-shift", "--no-context-shift")   # the last flag counts
    assert (no["stop"], no["n_gen"], text_no) == ("context", off["n_gen"], text_off)
    assert text_on.startswith(text_off) and len(text_on) > len(text_off)   # the same text up to the first shift
    whole, _ = _daemon(path, "--context-shift", "--keep", "-1")            # llama-cli's -1: the whole prompt stays
    req, _ = _daemon(path, "--context-shift", n_keep=-1)                   # the same through the request field
    assert whole["n_gen"] == req["n_gen"] == 400 and whole["n_shifts"] == req["n_shifts"] >= 2
    # the plain form
    p = subprocess.run([os.path.join(BIN, "mi-cli"), "-m", path, "-ngl", "0", "-c", "256", "-n", "400", "-p", PROMPT,
                        "--no-display-prompt", "--context-shift", "--keep", "4"], capture_output=True, timeout=300)
    assert p.returncode == 0 and len(p.stdout) > len(text_off), p.stderr
    assert f"stop: length after 400 tokens, {on['n_shifts']} context shifts".encode() in p.stderr
    for bad, msg in [(["--context-shift", "--draft-max", "4"], "--draft-max"), (["--context-shift", "--keep", "-2"], "--keep"),
                     (["--context-shift", "--world", "2", "--rank", "0"], "--world")]:
        p = subprocess.run([os.path.join(BIN, "mi-cli"), "-m", path, "-ngl", "0", "-p", "x", *bad], capture_output=True,
                           text=True, timeout=60)
        assert p.returncode == 2 and msg in p.stderr, p.stderr


def test_orchestrator_reports_context_shifts(native, model_dir):
    import httpx
    from test_api import Orchestrator
    path, _ = make_model(model_dir, "tiny-gqa", "Q8_0")
    s = Orchestrator("-m", path, "-ngl", "0", "-c", "256", "--mb-size", "2", "--context-shift", "--keep", "4")
    try:
        r = httpx.post(s.url + "/completion", json={"prompt": PROMPT, "n_predict": 300}, timeout=300).json()
        assert r["tokens_predicted"] == 300 and r["stop_reason"] == "length" and r["context_shifts"] >= 1
        k = httpx.post(s.url + "/completion", json={"prompt": PROMPT, "n_predict": 300, "n_keep": -1}, timeout=300).json()
        assert k["tokens_predicted"] == 300 and k["context_shifts"] >= 1 and k["content"] != r["content"]
        assert httpx.post(s.url + "/completion", json={"prompt": PROMPT, "n_keep": -2}, timeout=30).status_code == 400
        assert httpx.post(s.url + "/chat", json={"prompt": PROMPT, "n_keep": "x"}, timeout=30).status_code == 400
        total = r["context_shifts"] + k["context_shifts"]
        assert f"mipipe_context_shifts_total {total}\n" in httpx.get(s.url + "/metrics", timeout=30).text
        assert httpx.get(s.url + "/health", timeout=30).json()["context_shifts"] == total
    finally:
        s.close()
    s = Orchestrator("-m", path, "-ngl", "0", "-c", "256")          # the default: unchanged
    try:
        r = httpx.post(s.url + "/completion", json={"prompt": PROMPT, "n_predict": 300, "n_keep": 4}, timeout=300).json()
        assert r["stop_reason"] == "context" and "context_shifts" not in r and r["tokens_predicted"] < 256
    finally:
        s.close()


def test_failed_auto_shift_changes_nothing(native, model_dir):
    """Both slots fill in the same round; slot 1 keeps its whole prompt and has nothing to discard: the
    call throws before slot 0 is shifted."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    rng = np.random.default_rng(5)
    prompts = [rng.integers(1, cfg.vocab, 200).tolist() for _ in range(2)]
    with Engine(gguf=path, backend="cpu", max_ctx=256, n_mb=1, mb_size=2, context_shift=True, n_keep=4) as eng:
        eng.set_slot_keep(1, -1)
        eng.start(prompts)
        eng.decode(55)
        assert [eng.slot_position(s) for s in (0, 1)] == [255, 255]
        free = eng.kv_stats()["kv_free_pages"]
        with pytest.raises(RuntimeError, match="context capacity exhausted.*slot 1 can discard 0"):
            eng.decode(1)
        assert [eng.slot_position(s) for s in (0, 1)] == [255, 255] and eng.health()["context_shifts"] == 0
        assert eng.kv_stats()["kv_free_pages"] == free and eng.slot_shifts(0) == 0
        eng.release(1)
        eng.decode(1)                                     # slot 0 alone: shifted and goes on
        assert eng.slot_shifts(0) == 1 and eng.slot_position(0) == 255 - 64 + 1


def test_logprobs_and_stats_past_the_context(native, model_dir):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    prompts = _prompts(cfg.vocab)
    with Engine(gguf=path, backend="cpu", max_ctx=256, n_mb=1, mb_size=2, context_shift=True, n_probs=2) as eng:
        out, st1 = eng.generate(prompts, 300)
        assert [len(t) for t in eng.tokens()] == [300, 300] and eng.tokens() == out
        for (lp, tid, tlp), toks in zip(eng.logprobs(), out):
            assert lp.shape == (300,) and tid.shape == tlp.shape == (300, 2) and np.isfinite(lp).all()
            assert tid[:, 0].tolist() == toks and np.allclose(lp, tlp[:, 0])     # greedy: the chosen token leads
        _, st2 = eng.generate(prompts, 300)               # the counter of a call, not of the engine
        assert st1["context_shifts"] == st2["context_shifts"] >= 2
        assert eng.health()["context_shifts"] == 2 * st1["context_shifts"]


def test_cli_kept_prefix_fills_the_context(native, model_dir):
    """A prompt cut to ctx / 2 that is kept whole leaves a shift fewer than 128 positions: nothing to
    discard.  The request ends with stop "context" like without the option; mi-cli does not fail."""
    path, _ = make_model(model_dir, "tiny-gqa", "Q8_0")
    long = " ".join([PROMPT] * 60)
    r, _ = _daemon(path, "--context-shift", "--keep", "-1", prompt=long)
    assert r["n_prompt"] == 128 and r["stop"] == "context" and r["n_shifts"] == 0
    assert r["n_gen"] == 256 - 128   # every position of the context is used (one more than without the option)
    r, _ = _daemon(path, "--context-shift", "--keep", "4", prompt=long)    # the same prompt with room to discard
    assert r["stop"] in ("length", "eog") and r["n_gen"] > 256 - 128 and r["n_shifts"] >= 1, r
