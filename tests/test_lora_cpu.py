"""LoRA adapters on the CPU backend (no GPU): the adapter loader's refusals, the engine's adapter
management, and CpuStage (plain f32, y += s * B (A x) per bound row) against the fp32 oracle over
merged weights (mipipe.lora.merged_tensors)."""
import os

import numpy as np
import pytest

from conftest import make_model
from lora_helpers import TARGETS, follow, make_adapter, make_pairs, merged_ref, nmse

BOUND = 2e-4        # tests/test_engine_gpu.py: the engine against this oracle
MIN_EFFECT = 1e-2   # the adapter must move the oracle's logits by 50x the bound


def cpu_engine(path, **kw):
    from mipipe.engine import Engine
    cfg = dict(gguf=path, backend="cpu", cpu_act="f32", max_ctx=128, prefill_chunk=16, threads=4)
    cfg.update(kw)
    return Engine(**cfg)


@pytest.fixture(scope="module")
def gqa(native, model_dir):
    """tiny-gqa Q8_0 with two adapters on all seven targets and their oracles."""
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    ref = RefLlama.from_gguf(path)
    pa, a = make_adapter(model_dir, path, cfg, seed=11)
    pb, b = make_adapter(model_dir, path, cfg, seed=12, ranks=(3, 8))
    return dict(path=path, cfg=cfg, ref=ref, pa=pa, a=a, pb=pb, b=b)


# ------------------------------------------------------------------ loader errors
def _write(model_dir, name, arch, pairs, alpha=4.0, **kw):
    from mipipe import lora
    p = os.path.join(str(model_dir), name + ".gguf")
    lora.write_adapter_gguf(p, arch, alpha, pairs, **kw)
    return p


def _ab(rng, N, K, r):
    return (rng.standard_normal((r, K)).astype(np.float32), rng.standard_normal((N, r)).astype(np.float32))


def test_loader_refusals_name_the_tensor_or_field(native, model_dir):
    path, cfg = make_model(model_dir, "tiny-gqa", "Q8_0")
    rng = np.random.default_rng(0)
    d, kv, F = cfg.d_model, cfg.n_head_kv * cfg.hd, cfg.d_ff
    good = {"blk.0.attn_q.weight": _ab(rng, d, d, 4)}
    cases = [
        ("other-embd", {"token_embd.weight": _ab(rng, cfg.vocab, d, 4)}, {}, "token_embd.weight"),
        ("other-out", {"output.weight": _ab(rng, cfg.vocab, d, 4)}, {}, "output.weight"),
        ("other-norm", {"blk.0.attn_norm.weight": _ab(rng, d, d, 4)}, {}, "attn_norm"),
        ("other-exps", {"blk.0.ffn_down_exps.weight": _ab(rng, d, F, 4)}, {}, "ffn_down_exps"),
        ("other-inp", {"blk.0.ffn_gate_inp.weight": _ab(rng, 4, d, 4)}, {}, "ffn_gate_inp"),
        ("layer-range", {f"blk.{cfg.n_layer}.attn_q.weight": _ab(rng, d, d, 4)}, {}, f"blk.{cfg.n_layer}.attn_q"),
        ("a-without-b", {"blk.1.attn_k.weight": (_ab(rng, kv, d, 4)[0], None)}, {}, "blk.1.attn_k.weight.lora_a"),
        ("bad-k", {"blk.0.ffn_down.weight": _ab(rng, d, F - 32, 4)}, {}, "blk.0.ffn_down.weight.lora_a"),
        ("bad-n", {"blk.0.attn_v.weight": _ab(rng, kv + 8, d, 4)}, {}, "blk.0.attn_v.weight.lora_b"),
        ("rank-differs", {"blk.2.ffn_up.weight": (_ab(rng, F, d, 4)[0], _ab(rng, F, d, 5)[1])}, {}, "blk.2.ffn_up.weight.lora_b"),
        ("rank-over", {"blk.0.attn_q.weight": _ab(rng, d, d, 24)}, {}, "lora_max_rank"),
        ("bad-general-type", good, dict(general_type="model"), "general.type"),
        ("bad-adapter-type", good, dict(adapter_type="control_vector"), "adapter.type"),
    ]
    with cpu_engine(path, lora_adapters=1, lora_max_rank=16) as eng:
        for name, pairs, kw, needle in cases:
            p = _write(model_dir, "refuse-" + name, cfg.arch, pairs, **kw)
            with pytest.raises(RuntimeError) as e:
                eng.load_adapter(p)
            assert needle in str(e.value), (name, str(e.value))
        p = _write(model_dir, "refuse-arch", "qwen2", good)
        with pytest.raises(RuntimeError, match="general.architecture"):
            eng.load_adapter(p)
        assert eng.adapters() == []
        # a subset of targets, per layer, is fine
        p = _write(model_dir, "subset", cfg.arch, {"blk.1.attn_v.weight": _ab(rng, kv, d, 3), "blk.3.ffn_down.weight": _ab(rng, d, F, 16)})
        assert eng.load_adapter(p) == 0
        (a,) = eng.adapters()
        assert (a["id"], a["path"], a["rank_min"], a["rank_max"], a["alpha"]) == (0, p, 3, 16, 4.0) and a["bytes"] > 0


def test_moe_takes_attention_adapters_only(native, model_dir):
    path, cfg = make_model(model_dir, "tiny-moe", "Q8_0")
    rng = np.random.default_rng(1)
    p = _write(model_dir, "moe-ffn", cfg.arch, {"blk.0.ffn_down.weight": _ab(rng, cfg.d_model, cfg.d_ff, 4)})
    with cpu_engine(path, lora_adapters=1) as eng:
        with pytest.raises(RuntimeError, match="blk.0.ffn_down.weight"):
            eng.load_adapter(p)


def test_capacity_unload_and_option(native, model_dir, gqa):
    with cpu_engine(gqa["path"]) as eng:
        with pytest.raises(RuntimeError, match="lora_adapters"):
            eng.load_adapter(gqa["pa"])
        with pytest.raises(RuntimeError, match="lora_adapters"):
            eng.set_slot_adapters([0], [0])
    with cpu_engine(gqa["path"], lora_adapters=2, n_mb=1, mb_size=2) as eng:
        from mipipe import _native as N
        weights = lambda: N.jcall(N.lib().mp_engine_info, eng._h)["weight_bytes_local"]
        w0 = weights()
        assert eng.load_adapter(gqa["pa"]) == 0 and eng.load_adapter(gqa["pb"]) == 1
        assert weights() == w0 + sum(a["bytes"] for a in eng.adapters()) > w0   # adapter bytes count as weights
        with pytest.raises(RuntimeError, match="in use"):
            eng.load_adapter(gqa["pa"])
        eng.unload_adapter(0)
        assert eng.load_adapter(gqa["pb"]) == 0          # the lowest free id
        with pytest.raises(RuntimeError, match="not loaded"):
            eng.set_slot_adapters([0], [5])
        with pytest.raises(RuntimeError, match="listed twice"):
            eng.set_slot_adapters([1, 1], [0, 1])
        with pytest.raises(ValueError, match="stacking"):
            eng.start([[5, 6, 7]], adapters=[[(0, 1.0), (1, 0.5)]])
        eng.start([[5, 6, 7], [8, 9]], adapters=[(1, 1.0), None])
        with pytest.raises(RuntimeError, match="bound to slot 0"):
            eng.unload_adapter(1)
        eng.unload_adapter(0)
        eng.release(0)
        eng.unload_adapter(1)
        assert eng.adapters() == [] and weights() == w0


def test_construction_refusals(native, model_dir, gqa):
    from mipipe.engine import Engine
    base = dict(gguf=gqa["path"], backend="cpu", max_ctx=128)
    with pytest.raises(RuntimeError, match='lora_adapters.*mode "mp"'):
        Engine(**base, lora_adapters=1, mode="mp", world=1, rank=0)
    with pytest.raises(RuntimeError, match="lora_adapters.*world"):
        Engine(**base, lora_adapters=1, world=2)
    with pytest.raises(RuntimeError, match="lora_adapters.*rpc"):
        Engine(**base, lora_adapters=1, rpc=["127.0.0.1:1"])
    with pytest.raises(RuntimeError, match="lora_adapters"):
        Engine(**base, lora_adapters=9)
    with pytest.raises(RuntimeError, match="lora_max_rank"):
        Engine(**base, lora_adapters=1, lora_max_rank=129)


# ------------------------------------------------------------------ the engine against the oracle
@pytest.mark.parametrize("name,ftype", [("stories15m", "F32"), ("tiny-qwen2", "Q8_0")])
def test_cpu_engine_matches_merged_reference(native, model_dir, name, ftype):
    """All seven targets, ranks 8 and 3, after the prompt and after each of 4 decode steps."""
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, name, ftype)
    base = RefLlama.from_gguf(path)
    pa, ad = make_adapter(model_dir, path, cfg, seed=21)
    assert set(k.split(".")[2] for k in ad["pairs"]) == set(TARGETS) and {A.shape[0] for A, _ in ad["pairs"].values()} == {8, 3}
    ref = merged_ref(base, ad, 1.0)
    prompt = [int(t) for t in np.random.default_rng(0).integers(3, cfg.vocab, 21)]
    with cpu_engine(path, lora_adapters=1) as eng:
        assert eng.load_adapter(pa) == 0
        eng.start([prompt], adapters=[(0, 1.0)])
        got = [eng.logits()[0]]
        for _ in range(4):
            eng.decode(1)
            got.append(eng.logits()[0])
        toks = eng.tokens()[0]
    want = follow(ref, prompt, toks[:4])
    plain = follow(base, prompt, toks[:4])
    for step, (g, w, b) in enumerate(zip(got, want, plain)):
        assert nmse(b, w) >= MIN_EFFECT, (step, nmse(b, w))   # the precondition: the adapter matters
        assert nmse(g, w) < BOUND, (step, nmse(g, w))


def test_cpu_mixed_batch(native, model_dir, gqa):
    """mb_size 4 with rows [none, A@1.0, B@0.5, A@-1.0]: every row matches its own oracle."""
    cfg, base = gqa["cfg"], gqa["ref"]
    rng = np.random.default_rng(3)
    prompts = [[int(t) for t in rng.integers(3, cfg.vocab, n)] for n in (9, 21, 5, 14)]
    binds = [None, (0, 1.0), (1, 0.5), (0, -1.0)]
    with cpu_engine(gqa["path"], lora_adapters=2, n_mb=1, mb_size=4) as eng:
        eng.load_adapter(gqa["pa"]), eng.load_adapter(gqa["pb"])
        eng.start(prompts, adapters=binds)
        got = [eng.logits(rows=4)]
        for _ in range(2):
            eng.decode(1)
            got.append(eng.logits(rows=4))
        toks = eng.tokens()
    for i, bnd in enumerate(binds):
        ref = base if bnd is None else merged_ref(base, gqa["a"] if bnd[0] == 0 else gqa["b"], bnd[1])
        want = follow(ref, prompts[i], toks[i][:2])
        plain = follow(base, prompts[i], toks[i][:2])
        for step in range(3):
            if bnd is not None:
                assert nmse(plain[step], want[step]) >= MIN_EFFECT, (i, step)
            assert nmse(got[step][i], want[step]) < BOUND, (i, step, nmse(got[step][i], want[step]))


def test_prefix_cache_never_crosses_adapters(native, model_dir, gqa):
    cfg, base = gqa["cfg"], gqa["ref"]
    P = [int(t) for t in np.random.default_rng(4).integers(3, cfg.vocab, 30)]
    ref_b = merged_ref(base, gqa["b"], 1.0)
    want = follow(ref_b, P, [])[0]
    with cpu_engine(gqa["path"], lora_adapters=2) as eng:
        eng.load_adapter(gqa["pa"]), eng.load_adapter(gqa["pb"])
        reused = lambda: eng.health()["prefix_reused_tokens"]
        eng.start([P], adapters=[(0, 1.0)])
        eng.release(0)
        r0 = reused()
        eng.admit([0], [P], adapters=[(1, 1.0)])
        assert nmse(follow(base, P, [])[0], want) >= MIN_EFFECT
        assert nmse(eng.logits()[0], want) < BOUND
        assert reused() == r0          # KV computed under A is not B's prefix
        eng.release(0)
        eng.admit([0], [P], adapters=[(1, 1.0)])
        assert reused() > r0           # the same adapter at the same scale: reused
        assert nmse(eng.logits()[0], want) < BOUND
        eng.release(0)
        r1 = reused()
        eng.admit([0], [P], adapters=[(1, 0.5)])
        assert reused() == r1          # another scale is another binding
        eng.release(0)
        eng.admit([0], [P])
        assert reused() == r1          # and so is the base model
        assert nmse(eng.logits()[0], follow(base, P, [])[0]) < BOUND


def test_checkpoint_refused_while_bound(native, model_dir, gqa, tmp_path):
    with cpu_engine(gqa["path"], lora_adapters=1, n_mb=1, mb_size=2) as eng:
        eng.load_adapter(gqa["pa"])
        eng.start([[5, 6, 7, 8], [9, 10, 11]], adapters=[(0, 1.0), None])
        eng.decode(1)
        with pytest.raises(RuntimeError, match="save_state.*slot 0.*adapter"):
            eng.save_state(str(tmp_path / "st"))
        eng.release(0)
        eng.save_state(str(tmp_path / "st"))


def test_rebind_between_steps_and_start_clears(native, model_dir, gqa):
    """A running slot's binding can change between decode calls; start() clears the bindings of the
    generation before it and keeps those passed to it."""
    cfg, base = gqa["cfg"], gqa["ref"]
    P = [int(t) for t in np.random.default_rng(5).integers(3, cfg.vocab, 12)]
    with cpu_engine(gqa["path"], lora_adapters=2) as eng:
        eng.load_adapter(gqa["pa"])
        eng.start([P], adapters=[(0, 1.0)])
        assert nmse(eng.logits()[0], follow(merged_ref(base, gqa["a"], 1.0), P, [])[0]) < BOUND
        eng.start([P])                                     # no adapters=: the old binding is gone
        assert nmse(eng.logits()[0], follow(base, P, [])[0]) < BOUND
        lg0 = eng.logits()[0].copy()
        eng.set_slot_adapters([0], [0], [1.0])             # bind the running slot
        eng.decode(1)
        tok = eng.tokens()[0][0]
        plain = follow(base, P, [tok])[1]
        assert nmse(eng.logits()[0], plain) >= MIN_EFFECT  # the step followed the binding
        eng.set_slot_adapters([0], [None])
        eng.start([P])
        assert np.array_equal(eng.logits()[0], lg0)        # (a mixed-binding KV is not reused as a prefix)


def test_pipeline_stages_load_their_own_layers(native, model_dir, gqa):
    cfg, base = gqa["cfg"], gqa["ref"]
    P = [int(t) for t in np.random.default_rng(6).integers(3, cfg.vocab, 19)]
    ref = merged_ref(base, gqa["a"], 1.0)
    with cpu_engine(gqa["path"], lora_adapters=1, stages=2) as eng:
        eng.load_adapter(gqa["pa"])
        eng.start([P], adapters=[(0, 1.0)])
        eng.decode(2)
        toks = eng.tokens()[0]
        assert nmse(eng.logits()[0], follow(ref, P, toks[:2])[2]) < BOUND


def test_adapter_file_roundtrip_f16(native, model_dir, gqa):
    """write_adapter_gguf / read_adapter, and an F16 adapter through the native loader."""
    from mipipe import lora
    from mipipe.utils import quants as Q
    cfg, base = gqa["cfg"], gqa["ref"]
    p16, ad16 = make_adapter(model_dir, gqa["path"], cfg, seed=11, dtype=Q.F16)
    for k, (A, B) in gqa["a"]["pairs"].items():
        assert np.array_equal(ad16["pairs"][k][0], A.astype(np.float16).astype(np.float32))
    assert ad16["alpha"] == 4.0 and ad16["arch"] == cfg.arch
    P = [int(t) for t in np.random.default_rng(7).integers(3, cfg.vocab, 10)]
    with cpu_engine(gqa["path"], lora_adapters=1) as eng:
        eng.load_adapter(p16)
        eng.start([P], adapters=[(0, 1.0)])
        assert nmse(eng.logits()[0], follow(merged_ref(base, ad16, 1.0), P, [])[0]) < BOUND


def test_tile_table_builder(native):
    """The builder the stages use: rows grouped by adapter in tiles of 16, -1 padded, with their scales."""
    from mipipe.ops import kernels as Kn
    ids = [1] * 17 + [-1, 0, 1]
    sc = [float(i) for i in range(20)]
    t = Kn.lora_tile_table(ids, sc, 2)
    assert t[0] == 3
    tiles = t[4:].reshape(-1, 36)
    assert list(tiles[0][:1]) == [0] and list(tiles[0][4:20]) == [18] + [-1] * 15
    assert tiles[1][0] == 1 and list(tiles[1][4:20]) == list(range(16))
    assert tiles[2][0] == 1 and list(tiles[2][4:20]) == [16, 19] + [-1] * 14
    assert list(tiles[2][20:22].view(np.float32)) == [16.0, 19.0]
    with pytest.raises(RuntimeError, match="out of range"):
        Kn.lora_tile_table([2], [1.0], 2)


# ------------------------------------------------------------------ the reader under ASan + UBSan
def test_adapter_reader_sanitized(native, model_dir, gqa):
    """csrc/runtime/lora.cpp in a stand-alone host program built with -fsanitize=address,undefined
    (make sanitize-lora), run as a plain executable over the test adapters and corrupted copies: header
    cut, a shape that overflows, an offset past the end, a truncated tensor.  Every file ends as "ok"
    or as a thrown error ("rejected: ..."), never as a sanitizer report."""
    import struct
    import subprocess
    from conftest import REPO
    r = subprocess.run(["make", "-s", "sanitize-lora"], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    exe = os.path.join(REPO, "build", "fuzz_lora_asan")
    raw = open(gqa["pa"], "rb").read()
    files, expect_ok = [gqa["pa"], gqa["pb"]], 2

    def variant(name, data):
        p = os.path.join(str(model_dir), "fuzz-" + name + ".gguf")
        with open(p, "wb") as f:
            f.write(data)
        files.append(p)

    variant("header-cut", raw[:40])
    variant("kv-cut", raw[:200])
    variant("half", raw[:len(raw) // 2])
    variant("tail-cut", raw[:-4096])
    # the first tensor info follows the metadata: find it by its name and damage ne / offset
    name = b"blk.0.attn_q.weight.lora_a"
    at = raw.index(name) + len(name)            # n_dims u32, ne u64 x 2, type u32, offset u64
    b = bytearray(raw)
    struct.pack_into("<QQ", b, at + 4, 1 << 62, 1 << 62)
    variant("ne-overflow", bytes(b))
    b = bytearray(raw)
    struct.pack_into("<Q", b, at + 4, (1 << 63) + 5)
    variant("ne-negative", bytes(b))
    b = bytearray(raw)
    struct.pack_into("<Q", b, at + 4 + 16 + 4, 1 << 60)
    variant("offset-past-end", bytes(b))
    b = bytearray(raw)
    struct.pack_into("<Q", b, at + 4 + 16 + 4, (1 << 64) - 32)
    variant("offset-wraps", bytes(b))
    b = bytearray(raw)
    struct.pack_into("<I", b, at + 4 + 16, 99)
    variant("bad-type", bytes(b))
    rng = np.random.default_rng(0)
    for k in range(6):                           # random byte damage in the header region
        b = bytearray(raw)
        for pos in rng.integers(8, 1500, 12):
            b[int(pos)] = int(rng.integers(0, 256))
        variant(f"noise{k}", bytes(b))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, gqa["path"]] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files), r.stdout
    assert all(l.startswith("ok ") for l in lines[:expect_ok]), lines[:expect_ok]
    assert all(l.startswith("rejected: ") for l in lines[expect_ok:expect_ok + 9]), lines
    assert all(l.startswith(("ok ", "rejected: ")) for l in lines), lines
