"""IQ4_XS / IQ4_NL / Q5_0 / Q5_1 on the CPU side: the block formats (pinned by a second, scalar decoder
written straight from the format text), the plain quantizers, the native row dequantizer, the T16
packer against its numpy mirror (ragged K included for the 32-weight-block types), the file-type
mixes, and the CPU engine against the torch fp32 oracle."""
import numpy as np
import pytest

from conftest import make_model
from mipipe.utils import quants as Q

NEW = [Q.IQ4_XS, Q.IQ4_NL, Q.Q5_0, Q.Q5_1]
BLOCK32 = [Q.IQ4_NL, Q.Q5_0, Q.Q5_1]
CHUNK_BYTES = {Q.IQ4_XS: 2176, Q.IQ4_NL: 2304, Q.Q5_0: 2816, Q.Q5_1: 3072}
# relative RMS error of quantize -> dequantize on 2048 standard normals, seeds 0-4, the plain
# quantizers of utils/quants.py: IQ4_NL 0.0785-0.0811, IQ4_XS 0.0792-0.0811, Q5_0 0.0415-0.0444,
# Q5_1 0.0376-0.0392
TOL = {Q.IQ4_NL: 0.10, Q.IQ4_XS: 0.10, Q.Q5_0: 0.055, Q.Q5_1: 0.05}
KVALUES = [-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113]


def nmse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


def _f16(lo, hi):
    return np.float32(np.array([lo, hi], np.uint8).view(np.float16)[0])


def _nibble(qs, l):
    """element l of a 32-weight block: low nibble of qs[l] for l < 16, high nibble of qs[l - 16]"""
    return (int(qs[l]) & 15) if l < 16 else (int(qs[l - 16]) >> 4)


def _scalar_q5_0(blk):
    """22 bytes: f16 d, qh[4] (a 32-bit little-endian word), qs[16]."""
    d = _f16(blk[0], blk[1])
    qh = sum(int(blk[2 + i]) << (8 * i) for i in range(4))
    out = np.zeros(32, np.float32)
    for e in range(32):
        q = _nibble(blk[6:22], e) | (((qh >> e) & 1) << 4)
        out[e] = d * np.float32(q - 16)
    return out


def _scalar_q5_1(blk):
    """24 bytes: f16 d, f16 m, qh[4], qs[16]."""
    d, m = _f16(blk[0], blk[1]), _f16(blk[2], blk[3])
    qh = sum(int(blk[4 + i]) << (8 * i) for i in range(4))
    out = np.zeros(32, np.float32)
    for e in range(32):
        q = _nibble(blk[8:24], e) | (((qh >> e) & 1) << 4)
        out[e] = d * np.float32(q) + m
    return out


def _scalar_iq4_nl(blk):
    """18 bytes: f16 d, qs[16]."""
    d = _f16(blk[0], blk[1])
    return np.array([d * np.float32(KVALUES[_nibble(blk[2:18], e)]) for e in range(32)], np.float32)


def _scalar_iq4_xs(blk):
    """136 bytes: f16 d, u16 scales_h, scales_l[4], qs[128]."""
    d = _f16(blk[0], blk[1])
    scales_h = int(blk[2]) | (int(blk[3]) << 8)
    scales_l = blk[4:8]
    out = np.zeros(256, np.float32)
    for ib in range(8):
        ls = ((int(scales_l[ib // 2]) >> (4 * (ib % 2))) & 15) | (((scales_h >> (2 * ib)) & 3) << 4)
        qs = blk[8 + 16 * ib: 8 + 16 * ib + 16]
        for l in range(32):
            out[32 * ib + l] = d * np.float32(ls - 32) * np.float32(KVALUES[_nibble(qs, l)])
    return out


SCALAR = {Q.Q5_0: _scalar_q5_0, Q.Q5_1: _scalar_q5_1, Q.IQ4_NL: _scalar_iq4_nl, Q.IQ4_XS: _scalar_iq4_xs}


def test_type_tables():
    assert (Q.Q5_0, Q.Q5_1, Q.IQ4_NL, Q.IQ4_XS) == (6, 7, 20, 23)
    assert Q.BLOCK[Q.Q5_0] == (32, 22) and Q.BLOCK[Q.Q5_1] == (32, 24)
    assert Q.BLOCK[Q.IQ4_NL] == (32, 18) and Q.BLOCK[Q.IQ4_XS] == (256, 136)
    for qt, name in ((Q.Q5_0, "Q5_0"), (Q.Q5_1, "Q5_1"), (Q.IQ4_NL, "IQ4_NL"), (Q.IQ4_XS, "IQ4_XS")):
        assert Q.TYPE_NAMES[qt] == name and Q.NAME_TO_TYPE[name] == qt


@pytest.mark.parametrize("qt", NEW)
def test_format_pin_scalar_decoder(qt):
    """The vectorised dequantizer equals a dumb per-element decoder of the written format on random
    block bytes (every quant, high-bit and scale bit live)."""
    rng = np.random.default_rng(100 + qt)
    raw = Q.random_blocks(rng, qt, 4, 512, 0.05)
    be, bb = Q.BLOCK[qt]
    assert raw.nbytes == 4 * 512 // be * bb
    ref = np.concatenate([SCALAR[qt](b) for b in raw.reshape(-1, bb)])
    got = Q.dequantize(raw, qt)
    assert np.array_equal(got, ref)
    assert np.isfinite(got).all() and 0.025 < got.std() < 0.1   # of the order of scale = 0.05


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("qt", NEW)
def test_quant_roundtrip(qt, seed):
    x = np.random.default_rng(seed).standard_normal(2048).astype(np.float32)
    b = Q.quantize(x, qt)
    assert b.nbytes == Q.tensor_bytes(qt, x.shape)
    y = Q.dequantize(b, qt)
    rel = np.sqrt(np.mean((x - y) ** 2) / np.mean(x ** 2))
    print("relative rms", Q.TYPE_NAMES[qt], seed, rel)
    assert rel <= TOL[qt], rel


@pytest.mark.parametrize("qt", NEW)
def test_zero_block_quantizes_to_zero_scale(qt):
    be, bb = Q.BLOCK[qt]
    b = Q.quantize(np.zeros(2 * be, np.float32), qt).reshape(-1, bb)
    assert (b[:, 0:2] == 0).all()
    assert (Q.dequantize(b, qt) == 0).all()


def _rows(qt, n, k, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "quantized":
        return Q.quantize(rng.standard_normal((n, k)).astype(np.float32), qt)
    return Q.random_blocks(rng, qt, n, k, 0.05)


CASES_ROW = [(qt, 1024) for qt in NEW] + [(qt, 1056) for qt in BLOCK32]
CASES_PACK = [(qt, 512) for qt in NEW] + [(qt, 416) for qt in BLOCK32]


@pytest.mark.parametrize("kind", ["quantized", "random_blocks"])
@pytest.mark.parametrize("qt,K", CASES_ROW)
def test_native_dequant_row(native, qt, K, kind):
    b = _rows(qt, 1, K, 7 + qt, kind)
    ref = Q.dequantize(b, qt).reshape(-1)
    out = np.zeros(K, np.float32)
    assert native.mp_dequant_row(qt, b.ctypes.data, out.ctypes.data, K) == 0
    np.testing.assert_allclose(out, ref, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("kind", ["quantized", "random_blocks"])
@pytest.mark.parametrize("qt,k", CASES_PACK)
def test_t16_pack_layout(native, qt, k, kind):
    """The C++ packer + the kernels' indexing (numpy mirror) reproduce the dequantized weights, at
    16 x the GGUF bytes of 256 weights per chunk (no padding); a ragged K tail decodes to zeros."""
    from mipipe.ops.kernels import pack_t16, packed_dims
    from mipipe.utils.t16 import unpack_t16, PACK_OF, CHUNK
    n = 32
    raw = _rows(qt, n, k, 11 + qt, kind)
    ref = Q.dequantize(raw, qt).reshape(n, k)
    packed = pack_t16(raw, qt, n, k)
    _, k_pad, ntiles, nsb = packed_dims(qt, n, k)
    be, bb = Q.BLOCK[qt]
    assert CHUNK[PACK_OF[qt]] == CHUNK_BYTES[qt] == 16 * bb * (256 // be)
    assert packed.nbytes == native.mp_packed_bytes(qt, n, k) == ntiles * nsb * CHUNK_BYTES[qt]
    got = unpack_t16(packed, PACK_OF[qt], n, k_pad)
    np.testing.assert_allclose(got[:, :k], ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max())
    assert (got[:, k:] == 0).all()


def test_tensor_type_mixes():
    from mipipe.models.config import CONFIGS, tensor_type
    from mipipe.models.synthetic import llama_tensor_specs

    def types(name, ftype):
        return {t[2] for t in llama_tensor_specs(CONFIGS[name], ftype) if t[3] in ("w", "wo", "embd")}

    assert types("tiny-gqa", "IQ4_XS") == {Q.IQ4_XS, Q.Q5_K, Q.Q6_K}
    assert types("tiny-gqa", "Q5_0") == {Q.Q5_0}
    assert types("tiny-gqa", "Q5_1") == {Q.Q5_1}
    assert types("tiny-gqa", "IQ4_NL") == {Q.IQ4_NL}
    # every projection of tiny-k384 but ffn_down has K = 384
    assert types("tiny-k384", "IQ4_XS") == {Q.IQ4_NL, Q.Q5_1, Q.Q8_0, Q.IQ4_XS}
    assert tensor_type("IQ4_XS", "attn_q", 0, 4, 512) == Q.IQ4_XS
    assert tensor_type("IQ4_XS", "token_embd", 0, 4, 512) == Q.IQ4_XS
    assert tensor_type("IQ4_XS", "output", 0, 4, 512) == Q.Q6_K
    assert tensor_type("IQ4_XS", "attn_v", 3, 4, 512) == Q.Q5_K
    assert [tensor_type("IQ4_XS", "ffn_down", i, 32, 512) for i in (0, 3, 4, 31)] == [Q.Q5_K, Q.Q5_K, Q.IQ4_XS, Q.IQ4_XS]
    assert tensor_type("IQ4_XS", "attn_q", 0, 4, 288) == Q.IQ4_NL
    assert tensor_type("IQ4_XS", "attn_v", 0, 4, 288) == Q.Q5_1
    assert tensor_type("IQ4_XS", "output", 0, 4, 288) == Q.Q8_0
    for ftype, qt in (("Q5_0", Q.Q5_0), ("Q5_1", Q.Q5_1), ("IQ4_NL", Q.IQ4_NL)):
        for nm in ("output", "attn_v", "ffn_down", "token_embd"):
            assert tensor_type(ftype, nm, 0, 4, 288) == qt and tensor_type(ftype, nm, 0, 4, 512) == qt
    # the old names answer as before
    assert tensor_type("Q4_K_M", "attn_q", 0, 4, 512) == Q.Q4_K and tensor_type("Q4_K_M", "attn_q", 0, 4, 288) == Q.Q8_0
    assert tensor_type("Q4_K_M", "output", 0, 4, 512) == Q.Q6_K and tensor_type("Q4_K", "output", 0, 4, 512) == Q.Q6_K
    assert tensor_type("Q5_K_M", "attn_q", 1, 4, 512) == Q.Q5_K and tensor_type("Q6_K", "attn_q", 0, 4, 288) == Q.Q8_0
    assert tensor_type("Q3_K_M", "attn_q", 0, 4, 288) == Q.Q4_0 and tensor_type("Q2_K", "attn_v", 9, 32, 512) == Q.Q3_K
    assert tensor_type("Q8_0", "attn_q", 0, 4, 288) == Q.Q8_0 and tensor_type("Q4_0", "output", 0, 4, 512) == Q.Q4_0


@pytest.mark.parametrize("name,ftype", [("tiny-gqa", "IQ4_XS"), ("tiny-gqa", "Q5_0"), ("tiny-moe", "IQ4_NL"),
                                        ("tiny-k384", "IQ4_XS")])
@pytest.mark.parametrize("act", ["f32", "q8"])
def test_cpu_engine_matches_reference(native, model_dir, name, ftype, act):
    """The loop and bounds of test_cpu_engine_matches_reference_lowbit: the new types have no integer
    dot, so under q8 their rows take the dequantized f32 dot while the Q5_K / Q6_K / Q8_0 tensors of
    the same model keep the integer one."""
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
