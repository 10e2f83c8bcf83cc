"""mx8_gemm keeps an MX-FP8 copy of every quantized non-MoE projection, (1 + 1/32) B per weight of the
32-row x 256-k padded matrix: the memory budget must see those bytes (checked before any stage is built)."""
import re

import pytest

from conftest import make_model


@pytest.mark.parametrize("source", ["synthetic", "gguf"])
def test_mx8_gemm_copies_count_in_memory_budget(native, model_dir, source):
    from mipipe.engine import Engine
    if source == "gguf":
        path, cfg = make_model(model_dir, "tiny-gqa", "Q4_K_M")
        kw = dict(gguf=path)
        n_layer, d, f, hq, hkv = cfg.n_layer, cfg.d_model, cfg.d_ff, cfg.n_head, cfg.n_head_kv
        hd = d // hq
    else:
        kw = dict(synthetic=dict(n_layer=3, d_model=512, n_head=8, n_head_kv=2, d_ff=1536, vocab=2048), ftype="Q4_K")
        n_layer, d, f, hq, hkv, hd = 3, 512, 1536, 8, 2, 64

    def weights_mib(**extra):
        with pytest.raises(RuntimeError) as ei:
            Engine(max_ctx=128, gpu_mem_gib=1e-9, **kw, **extra)
        m = re.search(r"weights ([\d.]+) \+ KV", str(ei.value))
        assert m, str(ei.value)
        return float(m.group(1))

    pad = lambda n: (n + 31) // 32 * 32
    padk = lambda k: (k + 255) // 256 * 256
    mats = [(hq * hd, d), (hkv * hd, d), (hkv * hd, d), (d, hq * hd), (f, d), (f, d), (d, f)]
    expect = n_layer * sum(pad(n) * padk(k) * 33 / 32 for n, k in mats) / 1048576.0
    extra = weights_mib(mx8_gemm=True) - weights_mib()
    assert abs(extra - expect) < 0.01, (extra, expect)
    with pytest.raises(RuntimeError, match="mutually exclusive"):
        Engine(max_ctx=128, int8_gemm=True, mx8_gemm=True, **kw)
