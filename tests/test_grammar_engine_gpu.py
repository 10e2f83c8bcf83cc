"""Grammar-constrained decoding through the HIP engine (row_masks): mipipe.grammar states driven from
Python set one mask per constrained slot per round.  Half of the slots are constrained (a finite
grammar and the JSON-object grammar in each micro-batch), half are free; one release and one admit
happen mid-run.  The engine is deterministic, so the free slots can be compared id for id with a run
of the same engine in which no mask is ever set."""
import json

import numpy as np
import pytest

from conftest import make_model

pytestmark = pytest.mark.gpu

FINITE = 'root ::= ("yes" | "no" | "maybe") " " [0-9]{2}'
MEMBERS = {f"{w} {d:02d}" for w in ("yes", "no", "maybe") for d in range(100)}
ROUNDS = 24
SWAP_AT = 8                    # after this round slot 0 is released and admitted again
CONSTRAINED = {0: "finite", 1: "json", 4: "finite", 5: "json"}
FREE = (2, 3, 6, 7)


def _prompts(cfg, n=9):
    rng = np.random.default_rng(23)
    return [[int(t) for t in rng.integers(3, cfg.vocab - 300, 5 + 3 * i)] for i in range(n)]


def _engine(path, stages, **kw):
    from mipipe.engine import Engine
    cfg = dict(gguf=path, max_ctx=256, prefill_chunk=16, n_mb=2, mb_size=4, graphs=True, deterministic=True,
               stages=stages, devices=[0] * stages, row_masks=True)
    cfg.update(kw)
    return Engine(**cfg)


class Slot:
    def __init__(self, kind, grammars):
        self.kind, self.state = kind, grammars[kind].state()
        self.text, self.done, self.mask = b"", False, None


def _run(path, cfg, tok, stages, masked):
    """24 rounds with the swap; masked: drive the constrained slots, else never set a mask.
    Returns (tokens per slot, texts of the finished constrained requests, captures before / after)."""
    from mipipe.grammar import Grammar
    grammars = {"finite": Grammar(gbnf=FINITE, tokenizer=tok), "json": Grammar(json_schema={"type": "json_object"}, tokenizer=tok)}
    ps = _prompts(cfg)
    eog = {t for t in (tok.eos, tok.eot) if t >= 0}
    finished = []
    slots = {s: Slot(k, grammars) for s, k in CONSTRAINED.items()} if masked else {}
    checked_logits = False
    with _engine(path, stages) as eng:
        assert eng.info["model"]["vocab"] == cfg.vocab
        caps = lambda: eng.health()["stages"][-1]["graph_captures"]

        def push(only=None):
            sl = [s for s in slots if only is None or s in only]
            for s in sl:
                slots[s].mask = None if slots[s].done else slots[s].state.mask(cfg.vocab)
            if sl:
                eng.set_slot_masks(sl, [slots[s].mask for s in sl])

        def consume(only=None):
            toks = eng.tokens()
            for s, c in slots.items():
                if c.done or (only is not None and s not in only):
                    continue
                t = toks[s][-1]
                assert (int(c.mask[t >> 5]) >> (t & 31)) & 1, f"slot {s}: token {t} was banned by the mask set for this round"
                if t in eog:
                    assert c.state.can_end
                    c.done = True
                else:
                    assert c.state.accept(t), (s, t)
                    c.text += tok.piece(t)
                    c.done = c.state.only_end
                if c.done:
                    finished.append((c.kind, c.text))

        push()
        eng.start(ps[:8])
        c0 = caps()
        consume()
        for rnd in range(1, ROUNDS + 1):
            push()
            live = [s for s in (4, 5) if masked and not slots[s].done]
            eng.decode(1)
            if live and not checked_logits:
                # the logits head() left are micro-batch 1's (slots 4..7): -inf exactly at the ids the mask
                # set for this round bans, in the constrained row; the free rows 6 and 7 are untouched
                s = live[0]
                lg = eng.logits(rows=4)
                ids = np.arange(cfg.vocab)
                banned = ((slots[s].mask[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1) == 0
                assert banned.any() and not banned.all()
                assert np.array_equal(np.isneginf(lg[s - 4]), banned)
                assert np.isfinite(lg[2]).all() and np.isfinite(lg[3]).all()
                assert int(np.argmax(lg[s - 4])) == eng.tokens()[s][-1]
                checked_logits = True
            consume()
            if rnd == SWAP_AT:
                eng.release(0)
                if masked:
                    assert slots[0].done, "the finite grammar ends within a few tokens"
                    slots[0] = Slot("finite", grammars)
                    push(only=[0])
                eng.admit([0], [ps[8]])
                consume(only=[0])
        c1 = caps()
        toks = eng.tokens()
    assert not masked or checked_logits
    return toks, finished, (c0, c1)


@pytest.mark.parametrize("stages", [1, 2])
def test_constrained_and_free_slots(cuda, native, model_dir, stages):
    from mipipe.tokenizer import Tokenizer
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    tok = Tokenizer(path)
    toks, finished, (c0, c1) = _run(path, cfg, tok, stages, masked=True)
    ref, _, _ = _run(path, cfg, tok, stages, masked=False)
    assert c0 >= 1 and c1 == c0, "setting, changing and clearing masks must not re-capture the decode graphs"
    kinds = [k for k, _ in finished]
    assert kinds.count("finite") >= 3, finished          # slots 0 and 4, and slot 0 again after the swap
    for kind, text in finished:
        if kind == "finite":
            assert text.decode() in MEMBERS, text
        else:
            assert isinstance(json.loads(text.decode()), dict), text
    for s in FREE:
        assert toks[s] == ref[s], f"free slot {s} differs from the run without masks"
        assert len(toks[s]) == ROUNDS + 1
    assert any(toks[s] != ref[s] for s in CONSTRAINED), "the masks changed nothing: the test is vacuous"


def test_needs_the_key(cuda, native, model_dir):
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    from mipipe.engine import Engine
    with Engine(gguf=path, max_ctx=128, n_mb=1, mb_size=2, row_sampling=True) as eng:
        with pytest.raises(RuntimeError, match="row_masks"):
            eng.set_slot_masks([0], [np.full((cfg.vocab + 31) // 32, 0xFFFFFFFF, np.uint32)])
    with pytest.raises(RuntimeError, match="row_sampling"):
        Engine(gguf=path, max_ctx=128, row_masks=True, row_sampling=False)
    with Engine(gguf=path, max_ctx=128, n_mb=1, mb_size=2, row_masks=True) as eng:
        nw = (cfg.vocab + 31) // 32
        with pytest.raises(RuntimeError, match="allows no token"):
            eng.set_slot_masks([1], [np.zeros(nw, np.uint32)])
        with pytest.raises(RuntimeError, match="out of range"):
            eng.set_slot_masks([2], [np.full(nw, 0xFFFFFFFF, np.uint32)])


def test_second_generation_on_the_same_engine(cuda, native, model_dir):
    """start(..., masks=) twice without a release(): the second generation's masks hold although its
    slots are still busy with the first, the captured graphs are reused, and a third start() without
    masks runs free (the tokens of an engine on which no mask was ever set; prefix_cache off, so every
    start() prefills its prompts in full, as the fresh engine does)."""
    from mipipe.grammar import Grammar
    from mipipe.tokenizer import Tokenizer
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    tok = Tokenizer(path)
    g = Grammar(gbnf=FINITE, tokenizer=tok)
    ps = _prompts(cfg)[:8]
    with _engine(path, 1, prefix_cache=False) as eng:
        eng.start(ps)
        eng.decode(6)
        free = eng.tokens()
    with _engine(path, 1, prefix_cache=False) as eng:
        caps = lambda: eng.health()["stages"][-1]["graph_captures"]
        c0 = None
        for gen in range(2):
            states = {s: g.state() for s in (1, 6)}
            eng.start(ps, masks=[states[s].mask(cfg.vocab) if s in states else None for s in range(8)])
            c0 = c0 or caps()
            texts = {s: b"" for s in states}
            live = set(states)
            for _ in range(12):
                toks = eng.tokens()
                for s in sorted(live):
                    assert states[s].accept(toks[s][-1]), (gen, s, toks[s])
                    texts[s] += tok.piece(toks[s][-1])
                    if states[s].only_end:
                        live.discard(s)
                if not live:
                    break
                eng.set_slot_masks(sorted(states), [None if s not in live else states[s].mask(cfg.vocab) for s in sorted(states)])
                eng.decode(1)
            assert not live and all(t.decode() in MEMBERS for t in texts.values()), (gen, texts)
        eng.start(ps)
        eng.decode(6)
        assert eng.tokens() == free
        assert caps() == c0
        with pytest.raises(RuntimeError, match="listed twice"):
            eng.set_slot_masks([3, 3], [None, None])
