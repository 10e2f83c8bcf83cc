"""Numpy reference of the T16 packed-weight layout (csrc/runtime/qtypes.h, csrc/kernels/dequant.h).

`unpack_t16(packed, ptype, n, k)` decodes the packed bytes exactly the way the HIP dequantizers
index them (lane l = 16g + r, half h, MFMA step s, element j -> k = 64g + 32h + 8s + j), in f32.  It is the CPU-side oracle
that the C++ packer is tested against (the GPU unpack kernel is tested against the same function).
"""
from __future__ import annotations

import numpy as np

from . import quants as Q

P_F16, P_Q8_0, P_Q4_K, P_Q5_K, P_Q6_K, P_Q4_0, P_BF16 = 0, 1, 2, 3, 4, 5, 6
P_Q3_K, P_Q2_K = 8, 9   # (7 is P_I8, which has no GGUF type)
P_Q5_0, P_Q5_1, P_IQ4_NL, P_IQ4_XS = 10, 11, 12, 13
CHUNK = {P_F16: 8192, P_Q8_0: 4352, P_Q4_K: 2304, P_Q5_K: 2816, P_Q6_K: 3360, P_Q4_0: 2304, P_BF16: 8192,
         P_Q3_K: 1760, P_Q2_K: 1344, P_Q5_0: 2816, P_Q5_1: 3072, P_IQ4_NL: 2304, P_IQ4_XS: 2176}
PACK_OF = {Q.F32: P_F16, Q.F16: P_F16, Q.BF16: P_BF16, Q.Q8_0: P_Q8_0, Q.Q4_0: P_Q4_0,
           Q.Q4_K: P_Q4_K, Q.Q5_K: P_Q5_K, Q.Q6_K: P_Q6_K, Q.Q3_K: P_Q3_K, Q.Q2_K: P_Q2_K,
           Q.Q5_0: P_Q5_0, Q.Q5_1: P_Q5_1, Q.IQ4_NL: P_IQ4_NL, Q.IQ4_XS: P_IQ4_XS}


def _f16(b2):
    return np.frombuffer(np.ascontiguousarray(b2).tobytes(), np.float16).astype(np.float32)


def _bf16(b2):
    u = np.frombuffer(np.ascontiguousarray(b2).tobytes(), np.uint16).astype(np.uint32) << 16
    return u.view(np.float32)


def unpack_t16(packed: np.ndarray, ptype: int, n: int, k: int) -> np.ndarray:
    n_pad = (n + 15) // 16 * 16
    k_pad = (k + 255) // 256 * 256
    ntiles, nsb = n_pad // 16, k_pad // 256
    cb = CHUNK[ptype]
    P = np.asarray(packed, np.uint8).reshape(ntiles, nsb, cb)
    out = np.zeros((n_pad, k_pad), np.float32)
    lane = np.arange(64)
    g, r = lane >> 4, lane & 15
    for t in range(ntiles):
        for sb in range(nsb):
            c = P[t, sb]
            for h in range(2):
                for s in range(4):
                    for j in range(8):
                        kk = sb * 256 + 64 * g + 32 * h + 8 * s + j           # [64]
                        row = 16 * t + r
                        pos = (j & 1) * 4 + (j >> 1)                          # nibble position
                        if ptype in (P_Q4_K, P_Q5_K, P_Q6_K, P_Q4_0, P_Q5_0, P_Q5_1):
                            dw = c[h * 1024 + lane * 16 + s * 4 + pos // 2]
                            q = (dw >> ((pos & 1) * 4)) & 15
                        if ptype in (P_Q4_K, P_Q5_K):
                            hdr0 = 2048 if ptype == P_Q4_K else 2560
                            hdr = np.stack([c[hdr0 + 16 * rr: hdr0 + 16 * rr + 16] for rr in r])
                            d = _f16(hdr[:, 0:2])
                            dmin = _f16(hdr[:, 2:4])
                            # per lane group g: v = sc(2g) | m(2g) << 6 | sc(2g+1) << 12 | m(2g+1) << 18,
                            # byte b of v at header byte 4 + 4b + g
                            v = sum(hdr[lane, 4 + 4 * b + g].astype(np.int64) << (8 * b) for b in range(3))
                            sh = 12 * h
                            sc, mn = (v >> sh) & 63, (v >> (sh + 6)) & 63
                            if ptype == P_Q5_K:
                                qh = c[2048 + h * 256 + lane * 4 + (8 * s + pos) // 8]
                                q = q + (((qh >> ((8 * s + pos) % 8)) & 1) << 4)
                            v = d * sc * q - dmin * mn
                        elif ptype in (P_Q3_K, P_Q2_K):
                            # quants [lane] 16 B: dword 2 (s >> 1) + h, field at bit 16 (j & 1) + 8 (s & 1) + 2 (j >> 1)
                            bit = 32 * (2 * (s >> 1) + h) + 16 * (j & 1) + 8 * (s & 1) + 2 * (j >> 1)
                            q = ((c[lane * 16 + bit // 8] >> (bit % 8)) & 3).astype(np.float32)
                            sub = 2 * h + (s >> 1)                            # of the lane group's 4 sub-blocks
                            if ptype == P_Q2_K:
                                # scale bytes [r] 16 B (sc | m << 4 of sub-block 4g + sub), (d, dmin) [r] 4 B
                                sm = c[1024 + 16 * r + 4 * g + sub]
                                d = _f16(np.stack([c[1280 + 4 * rr: 1280 + 4 * rr + 2] for rr in r]))
                                dmin = _f16(np.stack([c[1282 + 4 * rr: 1282 + 4 * rr + 2] for rr in r]))
                                v = d * (sm & 15) * q - dmin * (sm >> 4)
                            else:
                                # high bits [lane] 8 B: dword h, bit 8 s + 4 (j & 1) + (j >> 1); scales [r] 12 B:
                                # byte b of v_g = u(4g) | u(4g+1) << 6 | u(4g+2) << 12 | u(4g+3) << 18 (u = s_k + 32)
                                # at byte 4 b + g; d [r] 2 B
                                hb = 8 * s + pos
                                hi = (c[1024 + lane * 8 + 4 * h + hb // 8] >> (hb % 8)) & 1
                                vg = sum(c[1536 + 12 * r + 4 * b + g].astype(np.int64) << (8 * b) for b in range(3))
                                sk = ((vg >> (6 * sub)) & 63).astype(np.float32) - 32
                                d = _f16(np.stack([c[1728 + 2 * rr: 1728 + 2 * rr + 2] for rr in r]))
                                v = d * sk * (q + 4 * hi - 4)
                        elif ptype in (P_Q5_0, P_Q5_1):
                            # Q4_K nibbles, the Q5_K high-bit plane, d [r] 16 B (block 2g + h), Q5_1: m [r] 16 B
                            qh = c[2048 + h * 256 + lane * 4 + (8 * s + pos) // 8]
                            q = (q + (((qh >> ((8 * s + pos) % 8)) & 1) << 4)).astype(np.float32)
                            blk = 2 * g + h
                            d = _f16(np.stack([c[2560 + 16 * rr + 2 * bb: 2560 + 16 * rr + 2 * bb + 2] for rr, bb in zip(r, blk)]))
                            if ptype == P_Q5_0:
                                v = d * (q - 16)
                            else:
                                m = _f16(np.stack([c[2816 + 16 * rr + 2 * bb: 2816 + 16 * rr + 2 * bb + 2] for rr, bb in zip(r, blk)]))
                                v = d * q + m
                        elif ptype in (P_IQ4_NL, P_IQ4_XS):
                            # codebook nibbles: element j at bit 8 (j & 3) + 4 (j >> 2) of dword s
                            idx = (c[h * 1024 + lane * 16 + s * 4 + (j & 3)] >> (4 * (j >> 2))) & 15
                            blk = 2 * g + h
                            if ptype == P_IQ4_NL:
                                d = _f16(np.stack([c[2048 + 16 * rr + 2 * bb: 2048 + 16 * rr + 2 * bb + 2] for rr, bb in zip(r, blk)]))
                            else:
                                # header [r] 8 B as in GGUF: d, scales_h, scales_l[4]
                                hdr = np.stack([c[2048 + 8 * rr: 2048 + 8 * rr + 8] for rr in r])
                                sh = hdr[:, 2].astype(np.int64) | (hdr[:, 3].astype(np.int64) << 8)
                                ls = ((hdr[lane, 4 + blk // 2] >> (4 * (blk % 2))) & 15) | (((sh >> (2 * blk)) & 3) << 4)
                                d = _f16(hdr[:, 0:2]) * (ls.astype(np.float32) - 32)
                            v = d * Q.KVALUES_IQ4[idx]
                        elif ptype == P_Q6_K:
                            i = j >> 1
                            bit = 16 * s + ((8 + 2 * i) if (j & 1) else 2 * i)
                            qh = c[2048 + h * 512 + lane * 8 + bit // 8]
                            q = q + (((qh >> (bit % 8)) & 3) << 4)
                            scl = np.stack([c[3072 + 16 * rr: 3072 + 16 * rr + 16] for rr in r]).view(np.int8)
                            d = _f16(np.stack([c[3328 + 2 * rr: 3328 + 2 * rr + 2] for rr in r]))
                            sub = 4 * g + 2 * h + (s >> 1)
                            v = d * scl[np.arange(64), sub].astype(np.float32) * (q.astype(np.float32) - 32)
                        elif ptype == P_Q4_0:
                            blk = 2 * g + h
                            d = _f16(np.stack([c[2048 + 16 * rr + 2 * bb: 2048 + 16 * rr + 2 * bb + 2] for rr, bb in zip(r, blk)]))
                            v = d * (q.astype(np.float32) - 8)
                        elif ptype == P_Q8_0:
                            u = c[h * 2048 + lane * 32 + s * 8 + j].astype(np.float32)
                            blk = 2 * g + h
                            d = _f16(np.stack([c[4096 + 16 * rr + 2 * bb: 4096 + 16 * rr + 2 * bb + 2] for rr, bb in zip(r, blk)]))
                            v = d * (u - 128)
                        else:  # F16 / BF16 (same layout)
                            b2 = np.stack([c[h * 4096 + s * 1024 + l * 16 + 2 * j: h * 4096 + s * 1024 + l * 16 + 2 * j + 2]
                                           for l in lane])
                            v = _bf16(b2) if ptype == P_BF16 else _f16(b2)
                        out[row, kk] = v
    return out[:n, :k]
