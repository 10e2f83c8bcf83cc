"""Times the LoRA shrink + expand launches of one target group (csrc/kernels/lora.hip) alone:

    python tools/lora_bench.py [M=256] [K=8192] [N=8192] [r=16] [targets=1] [adapters=1] [bound=1.0] [iters=200]

M rows, `bound` of them (a fraction) spread round robin over `adapters` adapters, `targets` stacked
targets of N columns each reading K inputs at rank r.  Prints one JSON line with the mean time of the
pair of launches (HIP events around `iters` back-to-back pairs after a warm-up) and, for scale, the
A + B bytes the bound adapters' pairs hold."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mipipe.ops import kernels as Kn

o = dict(M=256, K=8192, N=8192, r=16, targets=1, adapters=1, bound=1.0, iters=200)
for a in sys.argv[1:]:
    k, v = a.split("=")
    o[k] = float(v) if k == "bound" else int(v)
M, K, N, r, nt, na = o["M"], o["K"], o["N"], o["r"], o["targets"], o["adapters"]
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
x = torch.randn(M, K, generator=g).half().to(dev)
y = torch.zeros(M, nt * N, dtype=torch.float32, device=dev)
rp = Kn.lora_rank_pad(r)
pairs = {}
for a in range(na):
    for t in range(nt):
        A = torch.zeros(rp, K, dtype=torch.float16)
        B = torch.zeros(N, rp, dtype=torch.float16)
        A[:r] = (torch.randn(r, K, generator=g) / np.sqrt(K)).half()
        B[:, :r] = (torch.randn(N, r, generator=g) * 0.01).half()
        pairs[(a, 0, t)] = (A.to(dev), B.to(dev))
n_bound = int(round(o["bound"] * M))
ids = [(m % na) if m < n_bound else -1 for m in range(M)]
max_tiles = max(Kn.lora_max_tiles(M, 8), 1)
tiles = torch.from_numpy(Kn.lora_tile_table(ids, None, 8, max_tiles)).to(dev)
tgt = Kn.lora_target_table(pairs, 8, 1, dev)
rcap = Kn.lora_rank_pad(max(r, 64))
part = Kn.lora_part(max_tiles, K, nt, rcap, dev)
args = (tiles, max_tiles, tgt, 8, 1, 0, list(range(nt)), [N] * nt, [N * t for t in range(nt)], x, K, y, part, rcap)


def pair():
    Kn.lora_shrink(*args)
    Kn.lora_expand(*args)


for _ in range(20):
    pair()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(o["iters"]):
    pair()
e1.record()
torch.cuda.synchronize()
us = e0.elapsed_time(e1) * 1000.0 / o["iters"]
o.update(us_per_pair=round(us, 2), tiles=int(tiles[0]), max_tiles=max_tiles, ab_bytes=na * nt * 2 * rp * (K + N))
print("LORA_BENCH", json.dumps(o))
