"""Engine.embed through the HIP engine (HipStage, pool.hip) against the torch fp32 oracle.

Oracle of a prompt p: RefLlama.forward(p, 0, want_logits=False), the output RMSNorm over every row,
then pooling and L2 normalisation in float64 (fp8 KV: with the oracle's kv_round).  Metric: NMSE of
each vector (for "none": of the [len][d] block) against the oracle's.

The error is the engine's f16-MFMA error through the layers and cannot be derived per vector; the
project's only figure for it is NMSE < 2e-4 on logits (test_engine_gpu.py), which is the expectation
here, not the assertion.  Each case prints its `measured` value; the asserted bound is 3x the largest
value measured on the MI355X per KV type (the factor covers split-K order and box spread, as in
test_logprobs_engine_gpu.py).  Measured (largest over the poolings and prompts, PP = 1 / stages = 2):
    f16 KV:  tiny-gqa Q4_K_M 2.75e-6 / 2.75e-6, tiny-l3 Q6_K 7.21e-7 / 7.23e-7, tiny-qwen3 Q4_K_M 5.16e-6 / 5.16e-6,
             tiny-moe Q8_0 4.38e-6 / 4.38e-6
    fp8 KV:  tiny-gqa Q4_K_M 5.05e-4 (PP = 1, against the fp8-rounding oracle; the same over three runs)

Discrimination: the oracle vector of the wrong pooling (mean for last and the reverse) and the oracle
of the prompt without its first token must each miss the engine's vector by more than 10x the
asserted bound; the oracle's own mean-vs-last distance is checked against that on the CPU first.
Measured misses: 0.033 .. 0.14 with f16 KV (10x the bound: 1.5e-4), 0.058 with fp8 KV (1.5e-2)."""
import numpy as np
import pytest
import torch

from conftest import make_model

pytestmark = pytest.mark.gpu

BOUND_F16 = 3 * 5.16e-6   # 3 x the largest measured f16-KV value (docstring)
BOUND_FP8 = 3 * 5.05e-4    # 3 x the measured fp8-KV value
MODELS = [("tiny-gqa", "Q4_K_M"), ("tiny-l3", "Q6_K"), ("tiny-qwen3", "Q4_K_M"), ("tiny-moe", "Q8_0")]
LENS = (37, 21, 1)
POOLINGS = ("last", "mean", "cls", "none")


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


def prompts_for(cfg, lens=LENS, seed=0):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in lens]


def pool(h, pooling):
    v = {"mean": h.mean(0), "cls": h[0], "last": h[-1], "none": h}[pooling]
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


_oracle = {}


def oracle(model_dir, name, ftype, kv_dtype):
    """(path, cfg, prompts, rows, rows of each prompt without its first token), computed once"""
    key = (name, ftype, kv_dtype)
    if key not in _oracle:
        from mipipe.models.reference import RefLlama
        path, cfg = make_model(model_dir, name, ftype)
        ref = RefLlama.from_gguf(path)
        if kv_dtype == "fp8":
            ref.kv_round = lambda t: t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(t.dtype)

        def rows(p):
            ref.reset()
            x = ref.forward(p, 0, want_logits=False)
            return ref.rmsnorm(x, ref.t["output_norm.weight"]).double().numpy()
        prompts = prompts_for(cfg)
        _oracle[key] = (path, cfg, prompts, [rows(p) for p in prompts], [rows(p[1:]) if len(p) > 1 else None for p in prompts])
    return _oracle[key]


def gpu_engine(path, **kw):
    from mipipe.engine import Engine
    cfg = dict(gguf=path, max_ctx=256, prefill_chunk=16, mb_size=2)
    cfg.update(kw)
    if "stages" in cfg:
        cfg["devices"] = [0] * cfg["stages"]
    return Engine(**cfg)


def _case(model_dir, name, ftype, stages, kv_dtype, bound):
    path, cfg, prompts, rows, shifted = oracle(model_dir, name, ftype, kv_dtype)
    # the oracle tells its own poolings and prompts apart by more than the rule asks (CPU only)
    for h, hs in zip(rows, shifted):
        if hs is not None:
            assert nmse(pool(h, "mean"), pool(h, "last")) > 10 * bound
            assert nmse(pool(hs, "last"), pool(h, "last")) > 10 * bound
    with gpu_engine(path, stages=stages, kv_dtype=kv_dtype) as eng:
        got = {pl: eng.embed(prompts, pooling=pl) for pl in POOLINGS}     # 3 prompts, 2 slots: two groups
        assert eng.idle_slots() == [0, 1]
        assert eng.kv_stats()["kv_free_pages"] == eng.kv_stats()["kv_pages"]
    worst, miss = 0.0, np.inf
    for i, (p, h, hs) in enumerate(zip(prompts, rows, shifted)):
        for pl in POOLINGS:
            g, want = got[pl][i], pool(h, pl)
            assert g.shape == want.shape and np.isfinite(g).all(), (pl, g.shape)
            worst = max(worst, nmse(g, want))
        if hs is None:
            continue
        miss = min(miss, nmse(got["last"][i], pool(h, "mean")), nmse(got["mean"][i], pool(h, "last")),
                   nmse(got["last"][i], pool(hs, "last")), nmse(got["mean"][i], pool(hs, "mean")))
    print(f"{name} {ftype} stages={stages} kv={kv_dtype}: measured {worst:.3g} (wrong pooling / shifted prompt miss by {miss:.3g})")
    assert worst <= bound, worst
    assert miss > 10 * bound, miss


@pytest.mark.parametrize("name,ftype", MODELS)
@pytest.mark.parametrize("stages", [1, 2])
def test_embed_matches_reference(cuda, native, model_dir, name, ftype, stages):
    _case(model_dir, name, ftype, stages, "f16", BOUND_F16)


def test_embed_fp8_kv_matches_rounding_oracle(cuda, native, model_dir):
    _case(model_dir, "tiny-gqa", "Q4_K_M", 1, "fp8", BOUND_FP8)


@pytest.mark.parametrize("stages", [1, 2])
def test_embed_between_rounds_leaves_the_other_slot_alone(cuda, native, model_dir, stages):
    """deterministic engine: a greedy sequence in slot 0, embeddings into slot 1 between its decode
    rounds; its tokens equal a run without them, and the vectors are the same bits every time."""
    path, cfg, prompts, rows, _ = oracle(model_dir, "tiny-gqa", "Q4_K_M", "f16")
    gen_prompt = prompts_for(cfg, (11,), seed=5)[0]
    with gpu_engine(path, deterministic=True, stages=stages) as eng:
        eng.start([gen_prompt])
        eng.decode(6)
        plain = eng.tokens()[0]
    with gpu_engine(path, deterministic=True, stages=stages) as eng:
        before = eng.embed([prompts[0]], pooling="mean")[0]
        eng.start([gen_prompt])
        eng.decode(1)
        a = eng.embed([prompts[0]], pooling="mean", slots=[1])[0]
        eng.decode(1)
        b = eng.embed([prompts[1]], pooling="last")[0]
        eng.decode(4)
        assert eng.tokens()[0] == plain
        assert eng.idle_slots() == [1]
    assert np.array_equal(a, before)
    assert nmse(a, pool(rows[0], "mean")) <= BOUND_F16 and nmse(b, pool(rows[1], "last")) <= BOUND_F16


@pytest.mark.parametrize("extra", [dict(n_probs=5), dict(row_sampling=True), dict(n_probs=5, row_sampling=True)])
def test_embed_touches_no_sampler_state(cuda, native, model_dir, extra):
    """Engines that record logprobs / sample per row: an embed between rounds captures no graph and
    changes neither the other slot's tokens nor its logprob records (the embed path runs no head)."""
    path, cfg, prompts, rows, _ = oracle(model_dir, "tiny-gqa", "Q4_K_M", "f16")
    gen_prompt = prompts_for(cfg, (11,), seed=5)[0]
    sampling = [dict(temp=0.8, top_k=40, seed=11)] if extra.get("row_sampling") else None

    def run(with_embed):
        with gpu_engine(path, deterministic=True, **extra) as eng:
            caps = lambda: eng.health()["stages"][-1]["graph_captures"]
            eng.start([gen_prompt], sampling=sampling)
            c0 = caps()
            vecs = []
            for r in range(4):
                eng.decode(1)
                if with_embed:
                    vecs.append(eng.embed([prompts[r % 2]], pooling=POOLINGS[r])[0])
            assert caps() == c0, "an embed must not re-capture the decode graphs"
            rec = eng.logprobs()[0] if extra.get("n_probs") else None
            return eng.tokens()[0], rec, vecs
    t0, r0, _ = run(False)
    t1, r1, vecs = run(True)
    assert t0 == t1
    if r0 is not None:
        assert all(np.array_equal(x, y) for x, y in zip(r0, r1))
    for r, v in enumerate(vecs):
        assert nmse(v, pool(rows[r % 2], POOLINGS[r])) <= BOUND_F16
