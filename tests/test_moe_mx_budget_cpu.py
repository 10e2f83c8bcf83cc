"""mx8_gemm on a MoE model keeps a B image of the attention projections and of every expert's gate/up and
down (33/32 B per padded weight as MX-FP8, 17/32 B for an MXFP4 tensor's own nibbles): the memory budget
must see those bytes.  int8_gemm keeps skipping MoE layers.  Method of tests/test_mx8_budget_cpu.py."""
import re

import pytest

from conftest import make_model


@pytest.mark.parametrize("source,ftype,c_attn,c_exp", [
    ("synthetic", "Q4_K", 33, 33), ("synthetic", "MXFP4", 17, 17),       # synthetic MXFP4: every projection
    ("gguf", "Q4_K_M", 33, 33), ("gguf", "MXFP4_MOE", 33, 17)])          # MXFP4_MOE: Q8_0 attention, MXFP4 experts
def test_moe_images_count_in_memory_budget(native, model_dir, source, ftype, c_attn, c_exp):
    from mipipe.engine import Engine
    from mipipe.models.config import CONFIGS
    cfg = CONFIGS["tiny-moe"]
    if source == "gguf":
        kw = dict(gguf=make_model(model_dir, "tiny-moe", ftype)[0])
    else:
        kw = dict(synthetic=dict(n_layer=cfg.n_layer, d_model=cfg.d_model, n_head=cfg.n_head, n_head_kv=cfg.n_head_kv,
                                 d_ff=cfg.d_ff, vocab=cfg.vocab, n_expert=cfg.n_expert, n_expert_used=cfg.n_expert_used),
                  ftype=ftype)
    d, f, hd = cfg.d_model, cfg.d_ff, cfg.d_model // cfg.n_head

    def weights_mib(**extra):
        with pytest.raises(RuntimeError) as ei:
            Engine(max_ctx=128, gpu_mem_gib=1e-9, **kw, **extra)
        m = re.search(r"weights ([\d.]+) \+ KV", str(ei.value))
        assert m, str(ei.value)
        return float(m.group(1))

    pad = lambda n: (n + 31) // 32 * 32
    padk = lambda k: (k + 255) // 256 * 256
    attn = sum(pad(n) * padk(k) for n, k in [(cfg.n_head * hd, d), (cfg.n_head_kv * hd, d), (cfg.n_head_kv * hd, d),
                                             (d, cfg.n_head * hd)]) * c_attn / 32
    expert = (pad(2 * f) * padk(d) + pad(d) * padk(f)) * c_exp / 32
    expect = cfg.n_layer * (attn + cfg.n_expert * expert) / 1048576.0
    base = weights_mib()
    extra = weights_mib(mx8_gemm=True) - base
    assert abs(extra - expect) < 0.01, (extra, expect)
    assert abs(weights_mib(int8_gemm=True) - base) < 0.01
