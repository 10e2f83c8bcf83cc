#!/usr/bin/env python3
"""Cost of one context shift on the device: launch_kv_shift over every layer of a model against a
device-to-device hipMemcpyAsync of the same bytes.

Default shape: Llama-3-70B (Hkv 8, hd 128), 80 layers, one slot at old_len 2048, n_keep 4, n_discard 1024.
A pass is what HipStage::kv_shift enqueues: one launch per layer on one stream.  Bytes moved by a pass
= 2 x the tail's K bytes (every K row of a position >= n_keep + n_discard read and written once); the
copy pass moves the same bytes (one copy of the tail's K bytes per layer: read + write).  Each pass
is timed with HIP events after warm-up passes, kernel and copy passes alternating; the median is
reported, with the fastest pass.  The layers' caches (0.7 GB at f16) exceed the 256 MiB Infinity Cache,
so a pass streams from HBM like a shift in a running engine.  One JSON line per KV type."""
import argparse, ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mipipe import _native as N
from mipipe.ops.kernels import kv_shift, rope_cs_table, v_layout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=80)
    ap.add_argument("--hkv", type=int, default=8)
    ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--old-len", type=int, default=2048)
    ap.add_argument("--keep", type=int, default=4)
    ap.add_argument("--discard", type=int, default=1024)
    ap.add_argument("--types", default="f16,fp8")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kv_shift_bench: no GPU")
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    Dp = 64 if a.hd <= 64 else 128
    n_old = (a.old_len + 63) // 64
    nd, r0 = a.discard // 64, a.keep % 64
    first = a.keep // 64 + (1 if r0 else 0)
    row = list(range(n_old))                                  # one slot: pages 0 .. n_old - 1
    merge = row[first + nd - 1] if r0 else -1
    new = row[:first] + row[first + nd:]
    bt = torch.tensor([new + [n_old] * (n_old - len(new))], dtype=torch.int32, device="cuda")
    rec = [(0, a.keep, a.discard, a.old_len, merge)]
    cs = rope_cs_table(a.old_len, a.hd, 500000.0).cuda()
    moved = a.old_len - a.keep - a.discard
    for kv in a.types.split(","):
        fp8 = kv == "fp8"
        eb = 1 if fp8 else 2
        shape = (n_old + 1, a.hkv, 64, Dp)
        mk = (lambda: torch.randint(0, 120, shape, dtype=torch.uint8, device="cuda")) if fp8 else \
             (lambda: torch.randn(shape, dtype=torch.float16, device="cuda"))
        kc, vc = [mk() for _ in range(a.layers)], [mk() for _ in range(a.layers)]
        tail_bytes = moved * a.hkv * Dp * eb                  # per layer
        src = [torch.empty(tail_bytes, dtype=torch.uint8, device="cuda") for _ in range(a.layers)]
        dst = [torch.empty(tail_bytes, dtype=torch.uint8, device="cuda") for _ in range(a.layers)]
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        # the C entry point with its arguments built once: a pass is 80 calls of a few microseconds
        # each, and the wrapper's own argument handling would be most of what the events see
        recs = np.ascontiguousarray(np.asarray(rec, np.int32))
        args = [(ctypes.c_void_p(kc[li].data_ptr()), ctypes.c_void_p(vc[li].data_ptr()), ctypes.c_void_p(bt.data_ptr()), 1,
                 n_old, n_old, a.hkv, a.hd, Dp, int(fp8), ctypes.c_void_p(cs.data_ptr()), a.old_len, recs.ctypes.data, 1, st)
                for li in range(a.layers)]
        op = N.lib().mp_op_kv_shift

        def shift_pass():
            for ar in args:
                if op(*ar) != 0:
                    N.check(-1, "kv_shift")

        cargs = [(ctypes.c_void_p(dst[li].data_ptr()), ctypes.c_void_p(src[li].data_ptr()), tail_bytes, 3, st)   # 3: device to device
                 for li in range(a.layers)]

        def copy_pass():
            for ar in cargs:
                if hip.hipMemcpyAsync(*ar) != 0:
                    sys.exit("hipMemcpyAsync failed")

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3                  # us

        with v_layout(True):
            kv_shift(kc[0], vc[0], bt, cs, rec, a.hkv, a.hd, Dp, n_old, kv_fp8=fp8)   # the checked wrapper once
            for _ in range(a.warmup):
                shift_pass()
                copy_pass()
            torch.cuda.synchronize()
            ts, tc = [], []
            for _ in range(a.iters):
                ts.append(timed(shift_pass))
                tc.append(timed(copy_pass))
        total = 2.0 * tail_bytes * a.layers
        out = {"kv": kv, "layers": a.layers, "hkv": a.hkv, "hd": a.hd, "old_len": a.old_len, "n_keep": a.keep,
               "n_discard": a.discard, "moved_rows": moved, "bytes_moved": total,
               "shift_us_median": statistics.median(ts), "shift_us_min": min(ts),
               "copy_us_median": statistics.median(tc), "copy_us_min": min(tc)}
        out["shift_gbps"] = total / out["shift_us_median"] / 1e3
        out["copy_gbps"] = total / out["copy_us_median"] / 1e3
        out["shift_over_copy"] = out["shift_us_median"] / out["copy_us_median"]
        print(json.dumps(out), flush=True)
        del kc, vc, src, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
