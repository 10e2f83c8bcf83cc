"""Engine(shared_prefix=True): prompts that begin alike share whole KV pages (KvPager::share), are
prefilled from the first private page on, and decode through attn_shared + the suffix kernel.
Logits against the fp32 oracle at the project's NMSE bound for this path (2e-4, test_engine_gpu.py);
prompt scores at the bound test_logprobs_engine_gpu.py sets for this model and f16 pages."""
import numpy as np
import pytest

from conftest import make_model
from test_engine_gpu import nmse
from test_logprobs_engine_gpu import SCORE_BOUND, log_softmax64

pytestmark = pytest.mark.gpu


def _prompts(vocab):
    rng = np.random.default_rng(11)
    toks = lambda n: [int(t) for t in rng.integers(3, vocab, n)]
    pre = toks(130)   # two whole pages + 2 tokens
    # 4 share the prefix with distinct tails, 1 unrelated, 1 equals the prefix (one token left to prefill)
    return [pre + toks(5), toks(70), pre + toks(9), pre + toks(40), pre, pre + toks(1)]


@pytest.mark.parametrize("chunk", [dict(prefill_chunk=64), {}], ids=["chunk64", "one-chunk"])
def test_shared_prefix_matches_reference(cuda, native, model_dir, chunk):
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    ref = RefLlama.from_gguf(path)
    prompts = _prompts(cfg.vocab)
    # (the default chunk holds the whole batch: the donor and its sharers prefill in one launch)
    kw = dict(gguf=path, max_ctx=256, n_mb=1, mb_size=8, **chunk)

    def rows_of(seq):   # the oracle replays a whole sequence (one cache): logits of every position
        ref.reset()
        return ref.forward(seq, 0).numpy()

    def check(eng, want, what):   # want: row -> sequence whose last position the engine just computed
        lg = eng.logits(rows=8)
        for r, seq in want.items():
            e = nmse(lg[r], rows_of(seq)[-1])
            assert e < 2e-4, (what, r, e)

    with Engine(**kw) as plain:
        plain.start(prompts)
        free_plain = plain.kv_stats()["kv_free_pages"]
    with Engine(**kw, shared_prefix=True) as eng:
        assert eng.info["shared_prefix"] is True
        eng.start(prompts)
        st = eng.kv_stats()
        assert st["kv_shared_pages"] == 2
        assert st["kv_free_pages"] == free_plain + 2 * 4   # rows 2, 3, 4, 5 read row 0's two pages
        assert st["shared_prefix_skipped_tokens"] == 128 * 4
        check(eng, dict(enumerate(prompts)), "prompt")
        for step in range(3):
            if step == 2:
                eng.release(0)   # the donor leaves; its shared pages live on through the counts
            toks = eng.tokens()
            eng.decode(1)
            check(eng, {r: prompts[r] + [int(t) for t in toks[r][:step + 1]] for r in range(int(step == 2), 6)}, f"decode {step}")
        assert eng.kv_stats()["kv_shared_pages"] == 2
        # a later request with the same prefix while the others decode: a running row is its donor
        late = prompts[4] + [7, 5, 3]
        eng.admit([0], [late])
        st = eng.kv_stats()
        assert st["kv_shared_pages"] == 2 and st["shared_prefix_skipped_tokens"] == 128 * 5
        check(eng, {0: late}, "admit")
        first = int(eng.tokens()[0][0])
        eng.decode(1)
        check(eng, {0: late + [first]}, "decode after admit")
        # scoring rewrites slots 0 and 2, which name the same two pages, from position 0 with
        # different tokens: they must give the shared pages back first
        sc = [prompts[1], prompts[0], prompts[1][::-1]]
        got = eng.score(sc)
        assert eng.kv_stats()["kv_shared_pages"] == 0
        for p, g in zip(sc, got):
            ls = log_softmax64(rows_of(p))
            err = float(np.abs(g - np.array([ls[t, p[t + 1]] for t in range(len(p) - 1)])).max())
            assert err <= SCORE_BOUND, err


@pytest.mark.parametrize("other,kw", [("context_shift", dict(context_shift=True)), ("CPU stage", dict(backend="cpu"))])
def test_refused_combinations_name_both_options(cuda, native, model_dir, other, kw):
    from mipipe.engine import Engine
    path, _ = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    with pytest.raises(RuntimeError, match=f"shared_prefix.*{other}"):
        Engine(gguf=path, max_ctx=256, mb_size=4, shared_prefix=True, **kw)
