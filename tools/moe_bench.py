#!/usr/bin/env python3
"""Micro-benchmark of the grouped MoE GEMMs -- the dequantising gemm4 MoE mode and the
scaled-MFMA route of the mx8_gemm mode (moe_mx.hip, --route mx) -- on the Mixtral 8x7B or Qwen3-30B-A3B
(--model qwen3moe) expert shapes: routed gate/up (SwiGLU into per-slot h) and down (weighted atomics
into y), at M tokens, random router logits.  --type MXFP4 times the fp4 B image against gemm4's MXFP4.  Weights cold: the timed loop cycles
through enough copies of the expert stack to defeat the 256 MiB Infinity Cache.  One JSON line per
(phase, M, knob setting); a target for rocprofv3 --pmc passes.

    python tools/moe_bench.py --M 64,256 --knob GEMM4_MOE64=0,1
    python tools/moe_bench.py --model qwen3moe --type MXFP4 --route gemm4,mx --M 96,256,512
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mipipe import _native as N  # noqa: E402
from mipipe.ops.kernels import EPI_ATOMIC, EPI_SWIGLU, moe_route, moe_router, pack_type, packed_dims, quant_rows_mx8  # noqa: E402
from mipipe.utils import quants as Q  # noqa: E402

E, K_TOP, D, F = 8, 2, 4096, 14336
MODELS = {"mixtral": (8, 2, 4096, 14336), "qwen3moe": (128, 8, 2048, 768)}


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def experts(L, qt, n, k, copies, seed):
    pt = pack_type(qt)
    nbytes = L.mp_packed_bytes(qt, n, k)
    stacks = []
    for c in range(copies):
        W = torch.empty(E * nbytes, dtype=torch.uint8, device="cuda")
        for e in range(E):
            L.mp_init_packed(ctypes.c_void_p(W.data_ptr() + e * nbytes), nbytes, pt, 1.0 / k ** 0.5,
                             seed + 31 * c + e, st())
        stacks.append(W)
    return stacks, pt, nbytes


def images(L, stacks, pt, nbytes, ntiles, nsb):
    """The B images of every expert stack (moe_mx.hip): fp4 for MXFP4, else unpack + MX-FP8 re-quantization."""
    fp4 = pt == pack_type(Q.MXFP4)
    ng = (ntiles + 1) // 2
    wb, sb = ng * nsb * (4096 if fp4 else 8192), ng * nsb * 256
    tmp = None if fp4 else torch.empty(ntiles * 16, nsb * 256, dtype=torch.float16, device="cuda")
    out = []
    for W in stacks:
        img = torch.empty(E * wb, dtype=torch.uint8, device="cuda")
        sc = torch.empty(E * sb, dtype=torch.uint8, device="cuda")
        for e in range(E):
            src, dst, dsc = (ctypes.c_void_p(t.data_ptr() + e * n) for t, n in ((W, nbytes), (img, wb), (sc, sb)))
            if fp4:
                N.check(L.mp_op_relayout_mx4(src, ntiles, nsb, dst, dsc, st()), "relayout_mx4")
            else:
                N.check(L.mp_op_unpack(pt, src, ntiles, nsb, ctypes.c_void_p(tmp.data_ptr()), nsb * 256, st()), "unpack")
                N.check(L.mp_op_requant_mx8(ctypes.c_void_p(tmp.data_ptr()), nsb * 256, ntiles * 16, ntiles, nsb, dst, dsc,
                                            st()), "requant_mx8")
        out.append((img, sc))
    return out, wb, sb, int(fp4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", default="256")
    ap.add_argument("--phases", default="gateup,down")
    ap.add_argument("--down-type", default="Q6_K", choices=["Q4_K", "Q6_K"])
    ap.add_argument("--model", default="mixtral", choices=sorted(MODELS))
    ap.add_argument("--type", default="Q4_K", choices=["Q4_K", "MXFP4"], help="MXFP4: gate/up and down both")
    ap.add_argument("--route", default="gemm4", help="gemm4, mx or both (comma-separated)")
    ap.add_argument("--knob", action="append", default=[], metavar="NAME=V[,V..]")
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--copies", type=int, default=3, help="expert stacks cycled (3 x 528 MB defeats the MALL)")
    a = ap.parse_args()
    global E, K_TOP, D, F
    E, K_TOP, D, F = MODELS[a.model]
    L = N.lib()
    knobs = [[]]
    for kv in a.knob:
        name, vals = kv.split("=", 1)
        knobs = [kk + [(name, int(v))] for kk in knobs for v in vals.split(",")]
    gqt = Q.MXFP4 if a.type == "MXFP4" else Q.Q4_K
    dqt = Q.MXFP4 if a.type == "MXFP4" else Q.Q6_K if a.down_type == "Q6_K" else Q.Q4_K
    gu, gpt, gbytes = experts(L, gqt, 2 * F, D, a.copies, 7)
    dn, dpt, dbytes = experts(L, dqt, D, F, a.copies, 9)
    _, kg_pad, g_ntiles, g_nsb = packed_dims(gqt, 2 * F, D)
    _, kd_pad, d_ntiles, d_nsb = packed_dims(dqt, D, F)
    routes = a.route.split(",")
    if "mx" in routes:
        gu_mx, g_wb, g_sb, g_fmt = images(L, gu, gpt, gbytes, g_ntiles, g_nsb)
        dn_mx, d_wb, d_sb, d_fmt = images(L, dn, dpt, dbytes, d_ntiles, d_nsb)
    for M in [int(x) for x in a.M.split(",")]:
        g = torch.Generator().manual_seed(M)
        logits = torch.randn(M, E, generator=g).cuda()
        x = torch.randn(M, kg_pad, generator=g).half().cuda()
        if E <= 64:
            counts, lists, weights = moe_route(logits, K_TOP)
        else:   # the fused router's bucketing (E <= 128), from a random dense router
            _, counts, lists, weights = moe_router(x, (torch.randn(E, kg_pad, generator=g) / kg_pad ** 0.5).half().cuda(), K_TOP)
        h = torch.zeros(M * K_TOP, kd_pad, dtype=torch.float16, device="cuda")
        y = torch.zeros(M, D, device="cuda")

        xq, hq = quant_rows_mx8(x), quant_rows_mx8(torch.randn(M * K_TOP, kd_pad, generator=g).half().cuda())
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())

        def run_mx(phase, i):   # (the activation quantization is a launch of its own in the stage: not timed here)
            gate = phase == "gateup"
            img, sc = (gu_mx if gate else dn_mx)[i % a.copies]
            q, s = xq if gate else hq
            N.check(L.mp_op_moe_gemm_mx(EPI_SWIGLU if gate else EPI_ATOMIC, ptr(img), g_wb if gate else d_wb, ptr(sc),
                                        g_sb if gate else d_sb, g_fmt if gate else d_fmt, g_ntiles if gate else d_ntiles,
                                        g_nsb if gate else d_nsb, ptr(q), q.stride(0), ptr(s), s.stride(0), 0 if gate else 1,
                                        M, E, K_TOP, ptr(counts), ptr(lists), lists.shape[1], ptr(weights),
                                        None if gate else ptr(y), 0 if gate else D, ptr(h) if gate else None,
                                        kd_pad if gate else 0, F if gate else D, st()), "moe_gemm_mx")

        def run(phase, i):
            if route == "mx":
                return run_mx(phase, i)
            if phase == "gateup":
                W = gu[i % len(gu)]
                N.check(L.mp_op_moe_gemm4(gpt, EPI_SWIGLU, ctypes.c_void_p(W.data_ptr()), gbytes, g_ntiles, g_nsb,
                                          ctypes.c_void_p(x.data_ptr()), kg_pad, 0, M, E, K_TOP,
                                          ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(lists.data_ptr()),
                                          lists.shape[1], ctypes.c_void_p(weights.data_ptr()), None, 0,
                                          ctypes.c_void_p(h.data_ptr()), kd_pad, F, st()), "moe gate/up")
            else:
                W = dn[i % len(dn)]
                N.check(L.mp_op_moe_gemm4(dpt, EPI_ATOMIC, ctypes.c_void_p(W.data_ptr()), dbytes, d_ntiles, d_nsb,
                                          ctypes.c_void_p(h.data_ptr()), kd_pad, 1, M, E, K_TOP,
                                          ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(lists.data_ptr()),
                                          lists.shape[1], ctypes.c_void_p(weights.data_ptr()),
                                          ctypes.c_void_p(y.data_ptr()), D, None, 0, D, st()), "moe down")

        for kn in knobs:
            for name, v in kn:
                N.check(L.mp_set_knob(name.encode(), v), "knob")
            for route, phase in [(r, ph) for r in routes for ph in a.phases.split(",")]:
                for i in range(2):
                    run(phase, i)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.iters):
                    run(phase, i)
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / a.iters
                nb = (gbytes if phase == "gateup" else dbytes) * E
                flops = 2.0 * M * K_TOP * (2 * F * D if phase == "gateup" else D * F)
                print(json.dumps(dict(route=route, type=a.type, model=a.model, phase=phase, M=M, knobs=dict(kn) or None, us=round(us, 1),
                                      weight_GBps=round(nb / us / 1e3, 1), TFLOPs=round(flops / us / 1e6, 1))),
                      flush=True)


if __name__ == "__main__":
    main()
