"""Engine.embed on the CPU backend (no GPU) against the torch fp32 oracle.

The oracle of a prompt p: RefLlama.forward(p, 0, want_logits=False), the output RMSNorm over every
row, then pooling and L2 normalisation in float64.  With cpu_act="f32" the CpuStage computes the same
f32 arithmetic as the oracle (dequantized weights, f32 dots), which tests/test_engine_cpu.py bounds at
NMSE < 1e-8 on the logits of that configuration; the vectors here come out of the same forward with
one matrix product less (no LM head) and are held to the same 1e-8."""
import numpy as np
import pytest

from conftest import make_model

BOUND = 1e-8   # test_engine_cpu.py::test_cpu_engine_matches_reference, cpu_act f32
LENS = (37, 21, 1)
CASES = [("tiny-gqa", "Q8_0"), ("tiny-qwen3", "Q4_K_M")]


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


def prompts_for(cfg, lens=LENS, seed=0):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in lens]


def oracle_rows(ref, prompt):
    """[len][d] float64: the normed hidden rows of one prompt."""
    ref.reset()
    x = ref.forward(prompt, 0, want_logits=False)
    return ref.rmsnorm(x, ref.t["output_norm.weight"]).double().numpy()


def pool(h, pooling, normalize=True):
    v = {"mean": h.mean(0), "cls": h[0], "last": h[-1], "none": h}[pooling]
    if not normalize:
        return v
    s = np.sqrt((v * v).sum(-1, keepdims=True))
    return np.where(s > 0, v / np.where(s > 0, s, 1), 0.0)


_cache = {}


def setup(model_dir, name, ftype, **kw):
    key = (name, ftype, tuple(sorted(kw.items())))
    if key not in _cache:
        from mipipe.models.reference import RefLlama
        path, cfg = make_model(model_dir, name, ftype, **kw)
        ref = RefLlama.from_gguf(path)
        prompts = prompts_for(cfg)
        _cache[key] = (path, cfg, prompts, [oracle_rows(ref, p) for p in prompts])
    return _cache[key]


def cpu_engine(path, **kw):
    from mipipe.engine import Engine
    cfg = dict(gguf=path, backend="cpu", cpu_act="f32", max_ctx=128, prefill_chunk=16, mb_size=4, threads=4)
    cfg.update(kw)
    return Engine(**cfg)


@pytest.mark.parametrize("name,ftype", CASES)
@pytest.mark.parametrize("stages", [1, 2])
def test_embed_matches_reference(native, model_dir, name, ftype, stages):
    """Every pooling, normalised and not: prompts of 37 (three chunks of 16), 21 and 1 tokens packed
    into shared chunks."""
    path, cfg, prompts, rows = setup(model_dir, name, ftype)
    with cpu_engine(path, stages=stages) as eng:
        for pooling in ("last", "mean", "cls", "none"):
            for normalize in (True, False):
                got = eng.embed(prompts, pooling=pooling, normalize=normalize)
                assert len(got) == len(prompts)
                for p, g, h in zip(prompts, got, rows):
                    want = pool(h, pooling, normalize)
                    assert g.dtype == np.float32 and g.shape == want.shape, (pooling, g.shape)
                    e = nmse(g, want)
                    assert e < BOUND, (pooling, normalize, len(p), e)
                    if normalize:
                        assert np.allclose(np.linalg.norm(g.astype(np.float64), axis=-1), 1.0, atol=1e-5)
        assert eng.idle_slots() == [0, 1, 2, 3]
        assert eng.kv_stats()["kv_free_pages"] == eng.kv_stats()["kv_pages"]


def test_none_returns_one_row_per_token(native, model_dir):
    path, cfg, prompts, rows = setup(model_dir, *CASES[0])
    with cpu_engine(path) as eng:
        got = eng.embed(prompts, pooling="none", normalize=False)
    assert [g.shape for g in got] == [(len(p), cfg.d_model) for p in prompts]


def test_default_pooling_follows_the_file(native, model_dir):
    """pooling=None: a file with pooling_type = 1 gives the mean vector, one without the key (and one
    whose pooling_type is 0, none) the last row's."""
    from mipipe import _native as N
    import json
    for pt, want, shown in ((1, "mean", "mean"), (-1, "last", "last"), (0, "last", "last"), (2, "cls", "cls")):
        kw = {} if pt < 0 else {"pooling_type": pt}
        path, cfg, prompts, rows = setup(model_dir, "tiny-qwen3", "Q4_K_M", **kw)
        mc = json.loads(N.lib().mp_model_config_json(N.cstr(path)).decode())
        assert mc["pooling_type"] == pt
        with cpu_engine(path) as eng:
            assert eng.info["model"]["pooling_type"] == pt and eng.info["pooling"] == shown
            assert ("pooling_type=%d" % pt in eng.info["model"]["describe"]) == (pt >= 0)
            got = eng.embed(prompts)
        for g, h in zip(got, rows):
            assert nmse(g, pool(h, want)) < BOUND, (pt, nmse(g, pool(h, want)))
    # the two poolings are far apart, so the check above tells them apart
    h = rows[0]
    assert nmse(pool(h, "mean"), pool(h, "last")) > 1e-2


def test_more_prompts_than_slots(native, model_dir):
    path, cfg, prompts, rows = setup(model_dir, *CASES[0])
    many = prompts + prompts[::-1] + prompts[:1]          # 7 prompts, 2 slots
    want = rows + rows[::-1] + rows[:1]
    with cpu_engine(path, mb_size=2) as eng:
        got = eng.embed(many, pooling="mean")
    assert len(got) == 7
    for g, h in zip(got, want):
        assert nmse(g, pool(h, "mean")) < BOUND


@pytest.mark.parametrize("name,ftype", CASES)
@pytest.mark.parametrize("stages", [1, 2])
def test_embed_between_decode_rounds_leaves_the_other_slot_alone(native, model_dir, name, ftype, stages):
    """A greedy sequence in slot 0; embeddings into slot 1 between its decode rounds: the sequence's
    tokens equal those of a run without the embeddings, and the vectors equal the oracle's."""
    path, cfg, prompts, rows = setup(model_dir, name, ftype)
    gen_prompt = prompts_for(cfg, (11,), seed=5)[0]
    with cpu_engine(path, mb_size=2, stages=stages) as eng:
        eng.start([gen_prompt])
        eng.decode(6)
        plain = eng.tokens()[0]
    with cpu_engine(path, mb_size=2, stages=stages) as eng:
        before = eng.embed(prompts[:1], pooling="mean")[0]     # legal before start()
        eng.start([gen_prompt])
        assert eng.idle_slots() == [1]
        eng.decode(1)
        a = eng.embed([prompts[0]], pooling="mean", slots=[1])[0]
        eng.decode(1)
        b = eng.embed([prompts[1]], pooling="last")[0]
        eng.decode(4)
        assert eng.tokens()[0] == plain
        assert eng.idle_slots() == [1]
    assert nmse(before, pool(rows[0], "mean")) < BOUND
    assert nmse(a, pool(rows[0], "mean")) < BOUND
    assert nmse(b, pool(rows[1], "last")) < BOUND


def test_embed_errors_name_the_cause(native, model_dir):
    import json
    from mipipe import _native as N
    path, cfg, prompts, rows = setup(model_dir, *CASES[0])
    with cpu_engine(path, mb_size=2) as eng:
        eng.start([prompts[1]])
        with pytest.raises(RuntimeError, match="slot 0 is busy"):
            eng.embed([prompts[2]], slots=[0])
        # the C call takes what it is given at once: two prompts, one idle slot
        out = np.zeros(2 * cfg.d_model, np.float32)
        rq = json.dumps({"prompts": [prompts[2], prompts[2]]})
        assert N.lib().mp_engine_embed(eng._h, N.cstr(rq), out.ctypes.data, out.size) == -1
        assert b"2 prompts but 1 idle slots" in N.lib().mp_last_error()
        with pytest.raises(RuntimeError, match="is empty"):
            eng.embed([[]])
        with pytest.raises(RuntimeError, match="more than max_ctx = 128"):
            eng.embed([[5] * 129])
        with pytest.raises(RuntimeError, match="token id %d out of range" % cfg.vocab):
            eng.embed([[3, cfg.vocab]])
        with pytest.raises(RuntimeError, match="token id -1 out of range"):
            eng.embed([[-1]])
        with pytest.raises(RuntimeError, match="rank"):
            eng.embed([prompts[2]], pooling="rank")
        with pytest.raises(RuntimeError, match="unknown pooling \"max\""):
            eng.embed([prompts[2]], pooling="max")
        with pytest.raises(RuntimeError, match="bad slot 7"):
            eng.embed([prompts[2]], slots=[7])
        # none of the refused calls disturbed the engine
        eng.decode(2)
        got = eng.embed([prompts[2]])[0]
        assert nmse(got, pool(rows[2], "last")) < BOUND
        assert eng.idle_slots() == [1]
