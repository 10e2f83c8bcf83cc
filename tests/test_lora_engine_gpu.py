"""LoRA adapters through the HIP engine on one MI355X: logits against the fp32 oracle over merged
weights (RefLlama over mipipe.lora.merged_tensors) at every row-count family, mixed micro-batches,
MoE attention adapters, a two-stage pipeline, the graph invariants and determinism."""
import numpy as np
import pytest
import torch

from conftest import make_model
from lora_helpers import ATTN_TARGETS, follow, make_adapter, merged_ref, nmse

pytestmark = pytest.mark.gpu

BOUND = 2e-4        # tests/test_engine_gpu.py: the engine against this oracle
MIN_EFFECT = 1e-2   # the adapter moves the oracle's logits by at least 50x the bound (asserted on the CPU)

MIXED = [None, (0, 1.0), (1, 0.5), (0, -1.0)]


def near_tie_ok(rl, tok):
    """test_engine_matches_reference's rule: another token than the oracle's only on a near-tie."""
    rtop = np.sort(rl)[-2:]
    return rl.argmax() == tok or rl.max() - rl[tok] < 1e-2 * (abs(rtop).max() + 1)


def oracle_for(base, adapters, bnd):
    return base if bnd is None else merged_ref(base, adapters[bnd[0]], bnd[1])


@pytest.mark.parametrize("name,ftype", [("tiny-gqa", "Q4_K_M"), ("tiny-qwen2", "Q8_0"), ("tiny-qwen3", "Q4_K_M"),
                                        ("tiny-k384", "Q8_0")])
def test_engine_matches_merged_reference(cuda, native, model_dir, name, ftype):
    """mb_size 1 (the M <= 4 family), all seven targets, graphs on: after the 37-token prompt in chunks
    of 16 and after each of 4 decode steps."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, name, ftype)
    base = RefLlama.from_gguf(path)
    pa, ad = make_adapter(model_dir, path, cfg, seed=31)
    ref = merged_ref(base, ad, 1.0)
    prompt = [int(t) for t in np.random.default_rng(0).integers(3, cfg.vocab, 37)]
    with Engine(gguf=path, max_ctx=256, prefill_chunk=16, graphs=True, lora_adapters=2) as eng:
        assert eng.load_adapter(pa) == 0
        eng.start([prompt], adapters=[(0, 1.0)])
        got = [eng.logits()[0]]
        for _ in range(4):
            eng.decode(1)
            got.append(eng.logits()[0])
        toks = eng.tokens()[0]
    want = follow(ref, prompt, toks[:4])
    plain = follow(base, prompt, toks[:4])
    for step in range(5):
        assert nmse(plain[step], want[step]) >= MIN_EFFECT, (step, nmse(plain[step], want[step]))
        assert nmse(got[step], want[step]) < BOUND, (step, nmse(got[step], want[step]))
        assert near_tie_ok(want[step], toks[step]), (step, toks[step], int(want[step].argmax()))


@pytest.fixture(scope="module")
def gqa(native, model_dir):
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
    base = RefLlama.from_gguf(path)
    pa, a = make_adapter(model_dir, path, cfg, seed=41)
    pb, b = make_adapter(model_dir, path, cfg, seed=42, ranks=(3, 8))
    return dict(path=path, cfg=cfg, base=base, paths=[pa, pb], ads=[a, b])


def _mixed_run(gqa, **kw):
    from mipipe.engine import Engine
    cfg = gqa["cfg"]
    rng = np.random.default_rng(9)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (9, 21, 5, 14, 30, 3, 17, 11)]
    binds = MIXED * 2
    with Engine(gguf=gqa["path"], max_ctx=256, n_mb=1, mb_size=8, prefill_chunk=16, lora_adapters=2, **kw) as eng:
        for p in gqa["paths"]:
            eng.load_adapter(p)
        eng.start(prompts, adapters=binds)
        got = [eng.logits(rows=8)]
        for _ in range(2):
            eng.decode(1)
            got.append(eng.logits(rows=8))
        toks = eng.tokens()
    return prompts, binds, got, toks


def test_mixed_batch_mb8(cuda, native, gqa):
    """mb_size 8 (the 5..64 row family), rows bound [none, A@1.0, B@0.5, A@-1.0] twice: each row matches
    its own oracle, the unbound rows the base oracle."""
    prompts, binds, got, toks = _mixed_run(gqa)
    for i, bnd in enumerate(binds):
        want = follow(oracle_for(gqa["base"], gqa["ads"], bnd), prompts[i], toks[i][:2])
        if bnd is not None:
            plain = follow(gqa["base"], prompts[i], toks[i][:2])
        for step in range(3):
            if bnd is not None:
                assert nmse(plain[step], want[step]) >= MIN_EFFECT, (i, step)
            assert nmse(got[step][i], want[step]) < BOUND, (i, step, nmse(got[step][i], want[step]))


def test_mixed_batch_deterministic(cuda, native, gqa):
    """deterministic: true: two runs of the mixed batch give bit-identical logits."""
    a = _mixed_run(gqa, deterministic=True)
    b = _mixed_run(gqa, deterministic=True)
    assert a[3] == b[3]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    # and they are right
    i = 1
    want = follow(oracle_for(gqa["base"], gqa["ads"], a[1][i]), a[0][i], a[3][i][:2])
    assert nmse(a[2][2][i], want[2]) < BOUND


def test_wide_batch_mb80(cuda, native, model_dir):
    """mb_size 80 on tiny-l3 Q4_K (gemm4, stored split-K partials and the deferred reduction): a
    third of the rows each on A, B and none; 8 sampled rows after the prompts and after 2 steps."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-l3", "Q4_K")
    base = RefLlama.from_gguf(path, device="cuda")
    pa, a = make_adapter(model_dir, path, cfg, seed=51)
    pb, b = make_adapter(model_dir, path, cfg, seed=52, ranks=(3, 8))
    rng = np.random.default_rng(5)
    mb = 80
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, int(n))] for n in rng.integers(3, 9, mb)]
    binds = [(None, (0, 1.0), (1, 1.0))[i % 3] for i in range(mb)]
    with Engine(gguf=path, max_ctx=64, n_mb=1, mb_size=mb, prefill_chunk=128, lora_adapters=2) as eng:
        eng.load_adapter(pa), eng.load_adapter(pb)
        eng.start(prompts, adapters=binds)
        lg0 = eng.logits(rows=mb)
        eng.decode(2)
        lg2 = eng.logits(rows=mb)
        toks = eng.tokens()
    refs = {None: base, 0: merged_ref(base, a, 1.0), 1: merged_ref(base, b, 1.0)}
    for r in (0, 1, 2, 15, 16, 40, 64, 79):
        ref = refs[None if binds[r] is None else binds[r][0]]
        want = follow(ref, prompts[r], toks[r][:2])
        if binds[r] is not None:
            assert nmse(follow(base, prompts[r], toks[r][:2])[2], want[2]) >= MIN_EFFECT, r
        assert nmse(lg0[r], want[0]) < BOUND, (r, nmse(lg0[r], want[0]))
        assert nmse(lg2[r], want[2]) < BOUND, (r, nmse(lg2[r], want[2]))
    del refs, base
    torch.cuda.empty_cache()


def test_moe_attention_adapter(cuda, native, model_dir):
    """tiny-moe Q8_0 with an attention-only adapter; one that carries ffn_down_exps is refused."""
    from mipipe import lora
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-moe", "Q8_0")
    base = RefLlama.from_gguf(path)
    pa, ad = make_adapter(model_dir, path, cfg, seed=61, targets=ATTN_TARGETS)
    ref = merged_ref(base, ad, 1.0)
    rng = np.random.default_rng(6)
    prompt = [int(t) for t in rng.integers(3, cfg.vocab, 23)]
    bad = str(model_dir / "moe-exps-lora.gguf")
    lora.write_adapter_gguf(bad, cfg.arch, 4.0, {"blk.0.ffn_down_exps.weight": (
        rng.standard_normal((4, cfg.d_ff)).astype(np.float32), rng.standard_normal((cfg.d_model, 4)).astype(np.float32))})
    with Engine(gguf=path, max_ctx=256, prefill_chunk=16, lora_adapters=1) as eng:
        with pytest.raises(RuntimeError, match="ffn_down_exps"):
            eng.load_adapter(bad)
        eng.load_adapter(pa)
        eng.start([prompt], adapters=[(0, 1.0)])
        got = [eng.logits()[0]]
        eng.decode(2)
        got.append(eng.logits()[0])
        toks = eng.tokens()[0]
    want = follow(ref, prompt, toks[:2])
    plain = follow(base, prompt, toks[:2])
    assert nmse(plain[0], want[0]) >= MIN_EFFECT
    assert nmse(got[0], want[0]) < BOUND, nmse(got[0], want[0])
    assert nmse(got[1], want[2]) < BOUND, nmse(got[1], want[2])


def test_pipeline_two_stages(cuda, native, gqa):
    """stages=2 on one GPU: every stage loads its own layers' pairs."""
    from mipipe.engine import Engine
    cfg = gqa["cfg"]
    prompt = [int(t) for t in np.random.default_rng(7).integers(3, cfg.vocab, 29)]
    ref = merged_ref(gqa["base"], gqa["ads"][0], 1.0)
    with Engine(gguf=gqa["path"], max_ctx=256, prefill_chunk=16, stages=2, devices=[0, 0], lora_adapters=1) as eng:
        eng.load_adapter(gqa["paths"][0])
        eng.start([prompt], adapters=[(0, 1.0)])
        lg0 = eng.logits()[0]
        eng.decode(3)
        lg3 = eng.logits()[0]
        toks = eng.tokens()[0]
    want = follow(ref, prompt, toks[:3])
    assert nmse(lg0, want[0]) < BOUND, nmse(lg0, want[0])
    assert nmse(lg3, want[3]) < BOUND, nmse(lg3, want[3])


def test_graph_invariants(cuda, native, gqa):
    """Load, bind, rebind to another adapter, unbind and unload leave the graph capture count alone,
    and the logits follow each change on the next step.  The oracle of a sequence whose KV was
    computed under several bindings: the merged models share one KV cache, each step runs on the
    model of the binding in force."""
    from mipipe.engine import Engine
    cfg, base = gqa["cfg"], gqa["base"]
    prompt = [int(t) for t in np.random.default_rng(8).integers(3, cfg.vocab, 12)]
    models = {None: base, 0: merged_ref(base, gqa["ads"][0], 1.0), 1: merged_ref(base, gqa["ads"][1], 1.0)}
    with Engine(gguf=gqa["path"], max_ctx=256, prefill_chunk=16, graphs=True, lora_adapters=2) as eng:
        caps = lambda: [s["graph_captures"] for s in eng.health()["stages"]]
        c0 = caps()
        assert c0 == [1]
        eng.start([prompt])
        base.reset()
        assert nmse(eng.logits()[0], base.forward(prompt, 0)[-1].numpy()) < BOUND
        cache = (base.cache_k, base.cache_v)
        pos = len(prompt)

        def oracle_step(key, tok):   # one token on model `key` over the shared cache (left unchanged)
            m = models[key]
            m.cache_k, m.cache_v = list(cache[0]), list(cache[1])
            lg = m.forward([tok], pos)[-1].numpy()
            return lg, (m.cache_k, m.cache_v)

        assert eng.load_adapter(gqa["paths"][0]) == 0 and eng.load_adapter(gqa["paths"][1]) == 1
        assert caps() == c0
        prev = None
        for key in (0, 1, None, 0):
            eng.set_slot_adapters([0], [key])
            assert caps() == c0
            tok = eng.tokens()[0][-1]
            eng.decode(1)
            want, new_cache = oracle_step(key, tok)
            stale, _ = oracle_step(prev, tok)            # what the binding before would have given
            assert nmse(stale, want) >= MIN_EFFECT, (key, nmse(stale, want))
            assert nmse(eng.logits()[0], want) < BOUND, (key, nmse(eng.logits()[0], want))
            cache, prev, pos = new_cache, key, pos + 1
        with pytest.raises(RuntimeError, match="bound to slot 0"):
            eng.unload_adapter(0)
        eng.set_slot_adapters([0], [None])
        eng.unload_adapter(0), eng.unload_adapter(1)
        assert caps() == c0 and eng.adapters() == []
        tok = eng.tokens()[0][-1]
        eng.decode(1)
        want, _ = oracle_step(None, tok)
        assert nmse(eng.logits()[0], want) < BOUND
        assert caps() == c0
