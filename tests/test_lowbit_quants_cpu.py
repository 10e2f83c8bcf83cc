"""Q2_K / Q3_K on the CPU side: the block formats (pinned by a second, scalar decoder written straight
from the format text), the plain quantizers, the native row dequantizer, the T16 packer against its
numpy mirror, the file-type mixes, and the CPU engine against the torch fp32 oracle."""
import numpy as np
import pytest

from conftest import make_model
from mipipe.utils import quants as Q

LOWBIT = [Q.Q3_K, Q.Q2_K]
CHUNK_BYTES = {Q.Q3_K: 1760, Q.Q2_K: 1344}
# relative RMS error of quantize -> dequantize on gaussian data: the plain quantizers measured
# 0.151-0.157 (Q3_K) and 0.323-0.339 (Q2_K) over seeds 0-4
TOL = {Q.Q3_K: 0.20, Q.Q2_K: 0.40}


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


def _f16(lo, hi):
    return float(np.array([lo, hi], np.uint8).view(np.float16)[0])


def _scalar_q2_k(blk):
    """One 84-byte block: scales[16], qs[64], f16 d, f16 dmin."""
    scales, qs = blk[0:16], blk[16:80]
    d, dmin = np.float32(_f16(blk[80], blk[81])), np.float32(_f16(blk[82], blk[83]))
    out = np.zeros(256, np.float32)
    for e in range(256):
        n, j, l = e // 128, (e % 128) // 32, e % 32
        q = (int(qs[32 * n + l]) >> (2 * j)) & 3
        sc = int(scales[e // 16]) & 15
        m = int(scales[e // 16]) >> 4
        out[e] = d * np.float32(sc) * np.float32(q) - dmin * np.float32(m)
    return out


def _scalar_q3_k(blk):
    """One 110-byte block: hmask[32], qs[64], scales[12], f16 d."""
    hmask, qs, scales = blk[0:32], blk[32:96], blk[96:108]
    d = np.float32(_f16(blk[108], blk[109]))
    out = np.zeros(256, np.float32)
    for e in range(256):
        n, j, l = e // 128, (e % 128) // 32, e % 32
        lo = (int(qs[32 * n + l]) >> (2 * j)) & 3
        hi = (int(hmask[l]) >> (4 * n + j)) & 1
        q = lo + 4 * hi - 4
        k = e // 16
        low4 = (int(scales[k]) & 15) if k < 8 else (int(scales[k - 8]) >> 4)
        high2 = (int(scales[8 + k % 4]) >> (2 * (k // 4))) & 3
        s_k = (low4 | (high2 << 4)) - 32
        out[e] = d * np.float32(s_k) * np.float32(q)
    return out


@pytest.mark.parametrize("qt", LOWBIT)
def test_format_pin_scalar_decoder(qt):
    """The vectorised dequantizer equals a dumb per-element decoder of the written format on random
    block bytes (every quant, high-bit and scale bit live)."""
    rng = np.random.default_rng(100 + qt)
    raw = Q.random_blocks(rng, qt, 4, 512, 0.05)
    bb = Q.BLOCK[qt][1]
    assert raw.nbytes == 4 * 512 // 256 * bb
    dec = _scalar_q2_k if qt == Q.Q2_K else _scalar_q3_k
    ref = np.concatenate([dec(b) for b in raw.reshape(-1, bb)])
    got = Q.dequantize(raw, qt)
    assert np.array_equal(got, ref)
    assert np.isfinite(got).all() and 0.005 < got.std() < 0.5


@pytest.mark.parametrize("qt", LOWBIT)
def test_quant_roundtrip_lowbit(qt):
    assert Q.TYPE_NAMES[qt] in ("Q3_K", "Q2_K") and Q.NAME_TO_TYPE[Q.TYPE_NAMES[qt]] == qt
    rng = np.random.default_rng(qt)
    x = rng.standard_normal(256 * 8).astype(np.float32)
    b = Q.quantize(x, qt)
    assert b.nbytes == Q.tensor_bytes(qt, x.shape)
    y = Q.dequantize(b, qt)
    rel = np.sqrt(np.mean((x - y) ** 2) / np.mean(x ** 2))
    print("relative rms", Q.TYPE_NAMES[qt], rel)
    assert rel <= TOL[qt], rel


def _rows(qt, n, k, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "quantized":
        return Q.quantize(rng.standard_normal((n, k)).astype(np.float32), qt)
    return Q.random_blocks(rng, qt, n, k, 0.05)


@pytest.mark.parametrize("kind", ["quantized", "random_blocks"])
@pytest.mark.parametrize("qt", LOWBIT)
def test_native_dequant_row_lowbit(native, qt, kind):
    K = 1024
    b = _rows(qt, 1, K, 7 + qt, kind)
    ref = Q.dequantize(b, qt).reshape(-1)
    out = np.zeros(K, np.float32)
    assert native.mp_dequant_row(qt, b.ctypes.data, out.ctypes.data, K) == 0
    np.testing.assert_allclose(out, ref, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("kind", ["quantized", "random_blocks"])
@pytest.mark.parametrize("qt", LOWBIT)
def test_t16_pack_layout_lowbit(native, qt, kind):
    """The C++ packer + the kernels' indexing (numpy mirror) reproduce the dequantized weights, at
    16 x the block bytes per chunk (no padding)."""
    from mipipe.ops.kernels import pack_t16, packed_dims
    from mipipe.utils.t16 import unpack_t16, PACK_OF, CHUNK
    n, k = 32, 512
    raw = _rows(qt, n, k, 11 + qt, kind)
    ref = Q.dequantize(raw, qt).reshape(n, k)
    packed = pack_t16(raw, qt, n, k)
    _, _, ntiles, nsb = packed_dims(qt, n, k)
    assert CHUNK[PACK_OF[qt]] == CHUNK_BYTES[qt] == 16 * Q.BLOCK[qt][1]
    assert packed.nbytes == native.mp_packed_bytes(qt, n, k) == ntiles * nsb * CHUNK_BYTES[qt]
    got = unpack_t16(packed, PACK_OF[qt], n, k)
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())


def test_tensor_type_lowbit_mixes():
    from mipipe.models.config import CONFIGS, tensor_type
    from mipipe.models.synthetic import llama_tensor_specs

    def types(name, ftype):
        return {t[2] for t in llama_tensor_specs(CONFIGS[name], ftype) if t[3] in ("w", "wo", "embd")}

    assert types("tiny-gqa", "Q3_K_M") >= {Q.Q3_K, Q.Q4_K, Q.Q5_K, Q.Q6_K}
    assert types("tiny-gqa", "Q2_K") == {Q.Q2_K, Q.Q3_K, Q.Q6_K}
    assert types("tiny-gqa", "Q3_K_S") == {Q.Q3_K, Q.Q6_K}
    assert Q.Q4_K not in types("tiny-gqa", "Q3_K_L")
    for ftype in ("Q3_K", "Q3_K_S", "Q3_K_M", "Q3_K_L", "Q2_K"):
        assert tensor_type(ftype, "attn_q", 0, 4, 288) == Q.Q4_0
        assert tensor_type(ftype, "token_embd", 0, 4, 512) == (Q.Q2_K if ftype == "Q2_K" else Q.Q3_K)
        assert tensor_type(ftype, "output", 0, 4, 512) == Q.Q6_K
    # Q3_K_M: attn_v Q5_K in layers 0-1, else Q4_K; attn_output Q4_K; ffn_down Q5_K below n_layer / 16
    assert [tensor_type("Q3_K_M", "attn_v", i, 32, 512) for i in (0, 1, 2, 31)] == [Q.Q5_K, Q.Q5_K, Q.Q4_K, Q.Q4_K]
    assert tensor_type("Q3_K_M", "attn_output", 0, 32, 512) == Q.Q4_K
    assert [tensor_type("Q3_K_M", "ffn_down", i, 32, 512) for i in (0, 1, 2)] == [Q.Q5_K, Q.Q5_K, Q.Q4_K]
    assert {tensor_type("Q3_K_L", nm, 9, 32, 512) for nm in ("attn_v", "attn_output", "ffn_down")} == {Q.Q5_K}
    assert {tensor_type("Q2_K", nm, 9, 32, 512) for nm in ("attn_v", "attn_output", "ffn_down")} == {Q.Q3_K}


@pytest.mark.parametrize("name,ftype", [("tiny-gqa", "Q3_K_M"), ("tiny-gqa", "Q2_K"), ("tiny-moe", "Q3_K_S")])
@pytest.mark.parametrize("act", ["f32", "q8"])
def test_cpu_engine_matches_reference_lowbit(native, model_dir, name, ftype, act):
    """The loop and bounds of test_cpu_engine_matches_reference: the new types have no integer dot,
    so under q8 their rows take the dequantized f32 dot while the Q4_K / Q5_K / Q6_K tensors of the
    same model keep the integer one."""
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, name, ftype)
    ref = RefLlama.from_gguf(path)
    rng = np.random.default_rng(0)
    prompt = [int(t) for t in rng.integers(3, cfg.vocab, 21)]
    tol = 1e-8 if act == "f32" else 2e-3
    with Engine(gguf=path, backend="cpu", max_ctx=128, prefill_chunk=16, threads=4, cpu_act=act) as eng:
        eng.start([prompt])
        lg = eng.logits()[0]
        ref.reset()
        rl = ref.forward(prompt, 0)[-1].numpy()
        assert nmse(lg, rl) < tol, nmse(lg, rl)
        pos = len(prompt)
        for step in range(4):
            tok = eng.tokens()[0][-1]
            top2 = np.sort(rl)[-2:]
            if act == "f32" or top2[1] - top2[0] > 0.05 * (abs(top2).max() + 1):
                assert tok == int(rl.argmax()), step
            eng.decode(1)
            lg = eng.logits()[0]
            rl = ref.forward([tok], pos)[-1].numpy()
            pos += 1
            assert nmse(lg, rl) < tol, (step, nmse(lg, rl))
