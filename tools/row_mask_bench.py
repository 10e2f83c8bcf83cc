"""row_mask_kernel (csrc/kernels/row_mask.hip) at M = 64 rows, n = 128256 logits, 1/64 of the tokens allowed:
300 launches with every row on, then 100 with every row off (the early exit).  Meant to run under the
profiler, in a run of its own; the kernel trace's durations are the figure (the event times printed here
include the Python launch path):

    rocprofv3 --kernel-trace --stats -d OUT -o rm --output-format csv -- python tools/row_mask_bench.py
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from mipipe.ops import kernels as K
M, n = 64, 128256
nw = (n + 31) // 32
rng = np.random.default_rng(0)
allow = rng.random((M, nw * 32)) < 1 / 64
bits = np.packbits(allow.reshape(M, -1, 8), axis=2, bitorder="little").reshape(M, -1).view(np.uint32)
dev = torch.device("cuda:0")
b = torch.from_numpy(bits.view(np.int32)).to(dev)
on = torch.ones(M, dtype=torch.int32, device=dev)
off = torch.zeros(M, dtype=torch.int32, device=dev)
lg = torch.randn(M, n, device=dev)
for _ in range(200):
    K.row_mask(lg, b, on)
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for name, flag in (("on", on), ("off", off)):
    ev[0].record()
    for _ in range(100):
        K.row_mask(lg, b, flag)
    ev[1].record()
    torch.cuda.synchronize()
    print(f"ROWMASK events {name}: {ev[0].elapsed_time(ev[1]) * 10:.2f} us per launch")
banned = int((~allow[:, :n]).sum())
print(f"ROWMASK banned logits {banned}, bytes stored {banned * 4}, bits read {M * nw * 4}")
