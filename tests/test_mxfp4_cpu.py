"""MXFP4 (ggml type 39) on the CPU side: the block format pinned by a scalar decoder on hand-written
blocks, the OCP quantizer, the T16 packer (scale clamp included), the file-type rules, the CPU engine."""
import numpy as np
import pytest

from conftest import make_model
from mipipe.utils import quants as Q

# relative RMS error of quantize -> dequantize on 2048 standard normals, seeds 0-4: 0.1275-0.1316
TOL = 0.16
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _scalar_mxfp4(blk):
    """17 bytes: u8 e, qs[16]; element l < 16 the low nibble of qs[l], l + 16 the high one; bit 3 the sign."""
    nib = [(int(blk[1 + l]) & 15) if l < 16 else (int(blk[1 + l - 16]) >> 4) for l in range(32)]
    return np.array([(-1.0 if n & 8 else 1.0) * E2M1[n & 7] * 2.0 ** (int(blk[0]) - 127) for n in nib])


def test_format_pin_scalar_decoder(native):
    assert Q.MXFP4 == 39 and Q.BLOCK[39] == (32, 17) and native.mp_packed_bytes(39, 16, 256) == 2176
    lo, hi = np.arange(16, dtype=np.uint8), (np.arange(16, dtype=np.uint8) * 7 + 3) % 16   # every nibble, both halves
    blocks = np.stack([np.concatenate([[e], lo | (hi << 4)]).astype(np.uint8) for e in (0, 1, 127, 254)])
    with np.errstate(over="ignore"):
        want = np.stack([_scalar_mxfp4(b) for b in blocks]).astype(np.float32)   # e = 254: 6 * 2^127 is inf in f32
    out = np.zeros(128, np.float32)
    assert native.mp_dequant_row(39, blocks.ctypes.data, out.ctypes.data, 128) == 0
    assert np.array_equal(out.reshape(4, 32), want) and np.array_equal(Q.dequantize(blocks, 39).reshape(4, 32), want)
    assert want[0, 1] == np.float32(2.0 ** -128) and want[2, 9] == -0.5 and want[2, 16] == 1.5


@pytest.mark.parametrize("seed", range(5))
def test_quant_roundtrip(seed):
    x = np.random.default_rng(seed).standard_normal(2048).astype(np.float32)
    b = Q.quantize(x, Q.MXFP4).reshape(-1, 17)
    y = Q.dequantize(b, Q.MXFP4)
    assert np.sqrt(((x - y) ** 2).mean() / (x ** 2).mean()) < TOL
    amax, s = np.abs(x.reshape(-1, 32)).max(axis=1), 2.0 ** (b[:, 0].astype(np.float64) - 127)
    assert (amax <= 6 * s).all() and (amax > 3 * s).all()      # the smallest power of two with amax / s <= 6


def test_integer_dot_matches_fp64(native):
    """cpu_qdot.cpp: codes x int8 activation blocks.  Against the f64 dot of the dequantized rows with the
    int8-rounded x, the bound tests/test_formats.py holds the other integer dots to (f32 summation only)."""
    rng = np.random.default_rng(70)
    N, K = 24, 1024
    b = Q.quantize(rng.standard_normal((N, K)).astype(np.float32) * 0.05, Q.MXFP4)
    wd = Q.dequantize(b, Q.MXFP4).reshape(N, K).astype(np.float64)
    x = rng.standard_normal(K).astype(np.float32)
    x[::97] *= 20.0
    y, ys = np.zeros(N, np.float32), np.zeros(N, np.float32)
    assert native.mp_qdot_rows(Q.MXFP4, b.ctypes.data, N, K, x.ctypes.data, y.ctypes.data, ys.ctypes.data) == 1
    xb = x.reshape(-1, 32)
    d = np.abs(xb).max(1, keepdims=True) / np.float32(127)
    ref8 = wd @ (np.clip(np.rint(xb / d), -127, 127) * d).reshape(-1).astype(np.float64)
    np.testing.assert_allclose(y, ref8, rtol=2e-5, atol=2e-5 * np.abs(ref8).max())
    assert np.array_equal(y, ys)


@pytest.mark.parametrize("k", [512, 416])
def test_t16_pack_layout(native, k):
    """C++ packer -> numpy mirror of the kernels' indexing; scale bytes outside [99, 128] are clamped."""
    from mipipe.ops.kernels import pack_t16, packed_dims
    from mipipe.utils.t16 import unpack_t16, PACK_OF
    n = 32
    raw = Q.random_blocks(np.random.default_rng(k), Q.MXFP4, n, k, scale=0.05).reshape(n, k // 32, 17).copy()
    raw[3, 1, 0], raw[5, 2, 0] = 98, 130
    ref = Q.dequantize(raw, Q.MXFP4).reshape(n, k).astype(np.float64)
    ref[3, 32:64] = 0
    ref[5, 64:96] /= 4
    got = unpack_t16(pack_t16(raw.reshape(-1), Q.MXFP4, n, k), PACK_OF[Q.MXFP4], n, packed_dims(Q.MXFP4, n, k)[1])
    assert np.array_equal(got[:, :k].astype(np.float64), ref) and (got[:, k:] == 0).all()


def test_tensor_type_rules():
    from mipipe.models.config import CONFIGS
    from mipipe.models.synthetic import llama_tensor_specs

    def types(name, ftype, kinds=("w", "wo", "embd")):
        return {t[2] for t in llama_tensor_specs(CONFIGS[name], ftype) if t[3] in kinds}

    for name in ("tiny-gqa", "tiny-moe", "tiny-k384"):      # tiny-k384: K = 384, a multiple of 32 only
        assert Q.MXFP4 in types(name, "MXFP4", ("w", "wo")) and types(name, "MXFP4", ("embd",)) == {Q.Q8_0}
    assert {t[2] for t in llama_tensor_specs(CONFIGS["tiny-k384"], "MXFP4") if "attn_q" in t[0]} == {Q.MXFP4}
    assert types("tiny-gqa", "MXFP4_MOE") == {Q.Q8_0} and types("tiny-moe", "MXFP4_MOE") == {Q.Q8_0, Q.MXFP4}


@pytest.mark.parametrize("act", ["f32", "q8"])
def test_cpu_engine_matches_reference(native, model_dir, act):
    from mipipe.engine import Engine
    from mipipe.models.reference import RefLlama
    path, cfg = make_model(model_dir, "tiny-gqa", "MXFP4")
    ref = RefLlama.from_gguf(path)
    prompt = [int(t) for t in np.random.default_rng(0).integers(3, cfg.vocab, 21)]
    with Engine(gguf=path, backend="cpu", max_ctx=128, prefill_chunk=16, threads=4, cpu_act=act) as eng:
        eng.start([prompt])
        lg = eng.logits()[0]
        eng.decode(4)
        out = eng.tokens()
    ref.reset()
    toks, pos, seq = [], 0, prompt
    for _ in range(5):
        toks.append(int(ref.forward(seq, pos)[-1].argmax()))
        pos, seq = pos + len(seq), toks[-1:]
    rl = ref.reset() or ref.forward(prompt, 0)[-1].numpy().astype(np.float64)
    assert ((lg - rl) ** 2).sum() / (rl ** 2).sum() < (1e-8 if act == "f32" else 2e-3)   # test_iq4_q5_quants_cpu.py's bounds
    assert act == "q8" or out[0][-5:] == toks
