"""attn_encode vs attn_prefill time on one layer chunk at the gte-Qwen2-7B attention shape:
28 query heads, 4 kv heads, hd 128, 64 prompts of 512 tokens, f16 and fp8 KV.  Device events,
warm-up, alternating the two kernels; run it under `rocprofv3 --kernel-trace --stats` for the
kernels' own times (docs/PERFORMANCE.md)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mipipe.ops.kernels import attn_encode, attn_prefill, v_layout, v_pages_to_blocked  # noqa: E402

Hq, Hkv, hd, Dp, NP, L = 28, 4, 128, 128, 64, 512
M, pages_per = NP * L, L // 64
res = {}
for fp8 in (False, True):
    g = torch.Generator().manual_seed(1)
    q = (torch.randn(M, Hq, Dp, generator=g) / hd ** 0.5).half().cuda()
    n_pages = NP * pages_per
    k = torch.randn(n_pages, Hkv, 64, Dp, generator=g)
    v = torch.randn(n_pages, Hkv, Dp, 64, generator=g)
    if fp8:
        k, v = (t.to(torch.float8_e4m3fn).view(torch.uint8) for t in (k, v))
    else:
        k, v = k.half(), v.half()
    k, v = k.cuda(), v_pages_to_blocked(v).cuda()
    bt = torch.randperm(n_pages, generator=g).int().view(NP, pages_per).cuda()
    slot = torch.arange(NP, dtype=torch.int32).repeat_interleave(L).cuda()
    pos = torch.arange(L, dtype=torch.int32).repeat(NP).cuda()
    segs = [(i * L, L) for i in range(NP)]
    with v_layout(True):
        enc = lambda: attn_encode(q, slot, bt, k, v, Hkv, hd, segs, [L] * NP, kv_fp8=fp8)
        cau = lambda: attn_prefill(q, pos, slot, bt, k, v, Hkv, hd, segs, kv_fp8=fp8)
        for _ in range(3):
            enc(); cau()
        torch.cuda.synchronize()
        t = {"encode": [], "causal": []}
        for _ in range(20):
            for name, f in (("encode", enc), ("causal", cau)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); f(); b.record()
                torch.cuda.synchronize()
                t[name].append(a.elapsed_time(b))
    for name in t:
        s = sorted(t[name])
        res[f"{'fp8' if fp8 else 'f16'}_{name}_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}
print(json.dumps(res, indent=1))
