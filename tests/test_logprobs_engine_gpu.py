"""Token log-probabilities through the HIP engine: the generation record against the engine's own
logits (sharp, derived bound), prompt scoring against the fp32 oracle (measured bound), and that
recording does not perturb sampling.

Sharp check, TOL = 1e-4 (the kernel's derived bound, test_logprob_kernel_gpu.py): the record of a step
(chosen logprob, top-5 ids and logprobs) against the float64 log-softmax of eng.logits() of that step.

score() against RefLlama: the error is the engine's f16-MFMA logit error, which cannot be derived per
logprob (the existing tests bound it as NMSE < 2e-4 only).  Measured max |delta| on the MI355X over
both prompts, PP = 1 and stages = 2 (printed by each case as `measured`):
    f16 KV:  tiny-gqa Q4_K_M 2.92e-3 / 2.92e-3, tiny-l3 Q6_K 2.15e-3 / 2.90e-3, tiny-moe Q8_0 3.08e-3 / 3.08e-3
             (PP = 1 / stages = 2; tiny-l3 moved between 2.15e-3 and 2.90e-3 over three runs)
    fp8 KV:  tiny-gqa Q4_K_M 4.83e-2, tiny-l3 Q6_K 3.02e-2 (PP = 1, against the fp8-rounding oracle)
The asserted bound is 3x the largest measured value per KV type (the factor covers split-K atomics
order and box spread): 9.24e-3 and 1.45e-1.  The oracle with targets shifted by one position is
asserted to miss by more than 10x that bound (measured misses: 2.4 .. 4.0)."""
import numpy as np
import pytest
import torch

from conftest import make_model

pytestmark = pytest.mark.gpu

TOL = 1e-4
SCORE_BOUND = 3 * 3.08e-3
SCORE_BOUND_FP8 = 3 * 4.83e-2
MODELS = [("tiny-gqa", "Q4_K_M"), ("tiny-l3", "Q6_K"), ("tiny-moe", "Q8_0")]
LENS = (37, 21)


def log_softmax64(rows):
    x = np.asarray(rows, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def prompts_for(cfg, seed=0):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in LENS]


def near_tie(row, a, b):
    """The near-tie rule of test_engine_matches_reference."""
    return abs(row[a] - row[b]) < 1e-2 * (np.abs(np.sort(row)[-2:]).max() + 1)


@pytest.mark.parametrize("name,ftype", MODELS)
@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("graphs", [True, False])
def test_generation_record_matches_own_logits(cuda, native, model_dir, name, ftype, stages, graphs):
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, name, ftype)
    prompts = prompts_for(cfg)
    with Engine(gguf=path, stages=stages, devices=[0] * stages, max_ctx=256, prefill_chunk=16, mb_size=2,
                graphs=graphs, n_probs=5) as eng:
        eng.start(prompts)
        rows = [eng.logits(rows=2)]
        for _ in range(4):
            eng.decode(1)
            rows.append(eng.logits(rows=2))
        toks, rec = eng.tokens(), eng.logprobs()
    worst = 0.0
    for i in range(2):
        lp, ids, lps = rec[i]
        assert lp.shape == (5,) and ids.shape == (5, 5) and lps.shape == (5, 5)
        for s in range(5):
            row = rows[s][i]
            ls = log_softmax64(row)
            t = toks[i][s]
            order = np.argsort(-row.astype(np.float64), kind="stable")[:5]
            assert t == ids[s, 0]                                   # greedy: the chosen token leads the list
            worst = max(worst, abs(lp[s] - ls[t]), float(np.abs(lps[s] - ls[ids[s]]).max()))
            for k in range(5):
                assert ids[s, k] == order[k] or near_tie(row, ids[s, k], order[k]), (i, s, k)
    print(f"{name} {ftype} stages={stages} graphs={graphs}: worst {worst:.3g}")
    assert worst <= TOL, worst


def _score_case(model_dir, name, ftype, stages, kv_dtype, bound):
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, name, ftype)
    ref = RefLlama.from_gguf(path)
    if kv_dtype == "fp8":
        ref.kv_round = lambda t: t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(t.dtype)
    prompts = prompts_for(cfg, seed=3)
    with Engine(gguf=path, stages=stages, devices=[0] * stages, max_ctx=256, prefill_chunk=16, mb_size=2,
                kv_dtype=kv_dtype) as eng:
        got = eng.score(prompts)
        got3 = eng.score(prompts, n_probs=3)
    worst, miss = 0.0, np.inf
    for p, g, (g3, ids, lps) in zip(prompts, got, got3):
        ref.reset()
        ls = log_softmax64(ref.forward(p, 0).numpy())
        want = np.array([ls[t, p[t + 1]] for t in range(len(p) - 1)])
        assert g.shape == want.shape
        worst = max(worst, float(np.abs(g - want).max()))
        shifted = np.array([ls[t, p[t]] for t in range(len(p) - 1)])
        miss = min(miss, float(np.abs(g - shifted).max()))
        # the alternatives are sorted and contain no duplicate; asking for them changes nothing
        assert (np.diff(lps, axis=1) <= 0).all() and all(len(set(r)) == 3 for r in ids.tolist())
        assert np.abs(g3 - g).max() <= bound        # (two runs: split-K atomics may order differently)
    print(f"{name} {ftype} stages={stages} kv={kv_dtype}: measured {worst:.3g} (shifted targets miss by {miss:.3g})")
    assert worst <= bound, worst
    assert miss > 10 * bound, miss


@pytest.mark.parametrize("name,ftype", MODELS)
@pytest.mark.parametrize("stages", [1, 2])
def test_score_matches_reference(cuda, native, model_dir, name, ftype, stages):
    _score_case(model_dir, name, ftype, stages, "f16", SCORE_BOUND)


@pytest.mark.parametrize("name,ftype", [("tiny-gqa", "Q4_K_M"), ("tiny-l3", "Q6_K")])
def test_score_fp8_kv_matches_rounding_oracle(cuda, native, model_dir, name, ftype):
    _score_case(model_dir, name, ftype, 1, "fp8", SCORE_BOUND_FP8)


def test_score_hybrid_split_and_second_micro_batch(cuda, native, model_dir):
    """The hybrid split (first layers on a CPU stage, the rest and the head on the GPU) with three
    prompts over two micro-batches.  With cpu_act="f32" the CPU stage's layers are closer to the
    oracle than the GPU's, so the all-GPU bound holds (measured 3.1e-3; the default int8 activation
    blocks of the CPU stage measured 2.5e-2, their own rounding, and are not what this case is about)."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    ref = RefLlama.from_gguf(path)
    rng = np.random.default_rng(5)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (37, 21, 9)]
    with Engine(gguf=path, max_ctx=128, n_mb=2, mb_size=2, prefill_chunk=16, gpu_layers=2, stages=1, devices=[0],
                split="even", cpu_act="f32") as eng:
        assert eng.info["backend"] == "hybrid"
        got = eng.score(prompts)
    worst = 0.0
    for p, g in zip(prompts, got):
        ref.reset()
        ls = log_softmax64(ref.forward(p, 0).numpy())
        worst = max(worst, float(np.abs(g - np.array([ls[t, p[t + 1]] for t in range(len(p) - 1)])).max()))
    print(f"hybrid: measured {worst:.3g}")
    assert worst <= SCORE_BOUND, worst


@pytest.mark.parametrize("first", ["score", "spec"])
def test_score_and_speculative_decoding_share_one_engine(cuda, native, model_dir, first):
    """Score chunks and speculative verify chunks share the last stage's chunk-logits buffer; the
    verify chunks also need their per-row token buffer.  Either order on one engine gives what fresh
    engines give (deterministic=true: bitwise)."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    rng = np.random.default_rng(1)
    motif = [int(t) for t in rng.integers(3, cfg.vocab, 6)]
    prompts = [motif * 4, [int(t) for t in rng.integers(3, cfg.vocab, 11)]]
    kw = dict(gguf=path, max_ctx=128, mb_size=2, prefill_chunk=32, deterministic=True)
    with Engine(**kw) as eng:
        want_spec, _ = eng.spec_generate(prompts, 16, draft_max=5, ngram=3)
    with Engine(**kw) as eng:
        want_score = eng.score(prompts, n_probs=2)
    with Engine(**kw) as eng:
        if first == "score":
            got_score = eng.score(prompts, n_probs=2)
            got_spec, st = eng.spec_generate(prompts, 16, draft_max=5, ngram=3)
        else:
            got_spec, st = eng.spec_generate(prompts, 16, draft_max=5, ngram=3)
            got_score = eng.score(prompts, n_probs=2)
    assert st["verify_rounds"] >= 1
    assert got_spec == want_spec
    for (a, ai, al), (b, bi, bl) in zip(got_score, want_score):
        assert np.array_equal(a, b) and np.array_equal(ai, bi) and np.array_equal(al, bl)


def test_recording_does_not_perturb_sampling(cuda, native, model_dir):
    """deterministic=true: tokens of an n_probs = 0 engine equal those of the same engine with
    n_probs = 5 (seeded sampling with a repeat penalty), and the n_probs = 0 engine has no record."""
    from mipipe.engine import Engine
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    prompts = prompts_for(cfg, seed=7)
    outs = {}
    for k in (0, 5, -1):
        with Engine(gguf=path, max_ctx=256, prefill_chunk=16, mb_size=2, deterministic=True, temp=0.8, top_k=40,
                    seed=11, repeat_penalty=1.3, n_probs=k) as eng:
            outs[k], _ = eng.generate(prompts, 8)
            if k == 0:
                with pytest.raises(RuntimeError):
                    eng.logprobs()
            else:
                outs[("lp", k)] = eng.logprobs()
    assert outs[0] == outs[5] == outs[-1]
    for i in range(2):
        assert np.array_equal(outs[("lp", 5)][i][0], outs[("lp", -1)][i][0])
        assert outs[("lp", -1)][i][1].shape == (8, 0)


def test_generation_logprobs_are_raw_under_penalty(cuda, native, model_dir):
    """With a repeat penalty the record still holds the log-softmax of the RAW logits: eng.logits() is
    the row after the in-place penalty, undone here on the window's ids."""
    from mipipe.engine import Engine
    # a 512-token vocabulary and windows that hold two fifths of it: a random-init model never repeats a
    # penalised token on its own, here the sampler can hardly avoid one
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M", vocab=512)
    rng = np.random.default_rng(8)
    prompts = [[int(t) for t in rng.permutation(np.arange(3, 512))[:n]] for n in (230, 200)]
    rep, last_n, steps = 1.3, 200, 8
    with Engine(gguf=path, max_ctx=256, mb_size=2, temp=0.8, seed=5, repeat_penalty=rep,
                repeat_last_n=last_n, n_probs=5) as eng:
        eng.start(prompts)
        rows = [eng.logits(rows=2)]
        for _ in range(steps - 1):
            eng.decode(1)
            rows.append(eng.logits(rows=2))
        toks, rec = eng.tokens(), eng.logprobs()
    hit = 0
    for i, p in enumerate(prompts):
        seq = list(p)
        for s in range(steps):
            raw = rows[s][i].astype(np.float64)
            window = set(seq[-last_n:])
            for t in window:
                raw[t] = raw[t] * rep if raw[t] > 0 else raw[t] / rep
            ls = log_softmax64(raw)
            t = toks[i][s]
            assert abs(rec[i][0][s] - ls[t]) <= 2 * TOL, (i, s)       # (+ the rounding of undoing the penalty)
            if t in window:
                hit += 1
                assert abs(rec[i][0][s] - log_softmax64(rows[s][i])[t]) > 1e-2
            seq.append(t)
    assert hit > 0, "no sampled token was in its penalty window: the case does not bite"
