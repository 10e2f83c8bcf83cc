"""Non-causal flash attention (attn_encode.hip, mp_op_attn_encode) against a float64 numpy softmax
attention over keys [0, kv_len) of each prompt.  One packed chunk holds prompts of 1, 63, 64, 65 and
200 tokens in distinct slots (with G = 16 the last is 25 tiles; with n_split = 2 its four pages go to
two workgroups and the short prompts' second split is empty), in pages named by a shuffled block table.
Every cache byte that is not a live key is NaN or +-Inf (an e4m3 NaN byte), so one dead column read or
multiplied shows as a non-finite output.  q is u + 0.3 noise; keys 0, 63, 64 and kv_len - 1 of a prompt
are 3 u / sqrt(hd) + noise (score 3 against ~0) with |v| = 2: a row that misses one -- its own later
keys, a page edge, the last key -- moves by far more than the tolerance.

Tolerance: rtol = atol = 5e-3, as test_attn_prefill_oracle_gpu.py for the causal kernel (the same
rounding points; with |v| <= 2 the f16 roundings of P and of the output are at most 1e-3 each).
Largest |err| / (atol + rtol |ref|) on the MI355X over the 24 cases: 0.065 .. 0.075."""
import functools

import numpy as np
import pytest
import torch

from test_attn_decode_gpu import _decode, _round_cache, _store

RTOL, ATOL, LOG2E = 5e-3, 5e-3, 1.4426950408889634
LENS = (1, 63, 64, 65, 200)
MAX_PAGES = 5   # 200 keys take 4: one table entry per slot stays on the poisoned spare page


def _poison(shape, fp8):
    n = int(np.prod(shape))
    if fp8:
        return torch.tensor([0x7F, 0xFF], dtype=torch.uint8).repeat(n // 2 + 1)[:n].view(shape).clone()
    bits = torch.tensor([0x7E00, 0x7C00, 0xFC00 - 0x10000], dtype=torch.int16)   # NaN, +Inf, -Inf
    return bits.repeat(n // 3 + 1)[:n].view(shape).clone().view(torch.float16)


@functools.lru_cache(maxsize=None)
def case(Hq, Hkv, hd, Dp, fp8):
    g = torch.Generator().manual_seed(100 * Hq + hd + fp8)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    G, rt = Hq // Hkv, np.sqrt(hd)
    slots = [int(s) for s in torch.randperm(len(LENS) + 1, generator=g)][:len(LENS)]
    need = [(L + 63) // 64 for L in LENS]
    n_pages = sum(need) + 3   # the trash page behind the unused table entries and two spare ones
    perm = [int(p) for p in torch.randperm(n_pages, generator=g)]
    bt = torch.full((len(LENS) + 1, MAX_PAGES), perm[0], dtype=torch.int32)
    kc, vc = _poison((n_pages, Hkv, 64, Dp), fp8), _poison((n_pages, Hkv, Dp, 64), fp8)
    u = torch.nn.functional.normalize(rnd(Hkv, hd), dim=-1) * rt
    q, ref = torch.zeros(sum(LENS), Hq, Dp, dtype=torch.float16), np.zeros((sum(LENS), Hq, hd))
    segs, slot, row, nxt = [], [], 0, 1
    for s, L, n in zip(slots, LENS, need):
        K, V = 0.3 * rnd(L, Hkv, hd) / rt, rnd(L, Hkv, hd).clamp(-2, 2)
        for j in {0, 63, 64, L - 1} & set(range(L)):
            K[j] += 3 * u / rt
            V[j] = 2.0 * torch.sign(V[j])
        K, V = _round_cache(K, fp8), _round_cache(V, fp8)
        for i in range(n):
            page, lo, hi = perm[nxt], 64 * i, min(64 * i + 64, L)
            bt[s, i], nxt = page, nxt + 1
            kc[page, :, :hi - lo, :] = _store(torch.nn.functional.pad(K[lo:hi].transpose(0, 1), (0, Dp - hd)), fp8)
            vc[page, :, :, :hi - lo] = _store(torch.nn.functional.pad(V[lo:hi].permute(1, 2, 0), (0, 0, 0, Dp - hd)), fp8)
        q[row:row + L, :, :hd] = ((u.repeat_interleave(G, 0) + 0.3 * rnd(L, Hq, hd)) / rt).to(torch.float16)
        # the oracle: exp2-domain scores from the kernel's MFMA operand, softmax and P.V in float64
        qs = (q[row:row + L, :, :hd].float() * np.float32(LOG2E)).to(torch.float16).double().numpy()
        Kx, Vx = (np.repeat(t.numpy(), G, axis=1) for t in (K, V))            # [L][Hq][hd]
        s2 = np.einsum("thd,jhd->htj", qs, Kx)
        p = np.exp2(s2 - s2.max(-1, keepdims=True))
        ref[row:row + L] = np.einsum("htj,jhd->thd", p / p.sum(-1, keepdims=True), Vx)
        segs, slot, row = segs + [(row, L)], slot + [s] * L, row + L
    assert np.isfinite(ref).all() and not torch.isfinite(_decode(kc)[perm[0]]).any()
    return q, torch.tensor(slot, dtype=torch.int32), bt, kc, vc, segs, ref


@pytest.mark.gpu
@pytest.mark.parametrize("n_split", [1, 2])
@pytest.mark.parametrize("blocked", [False, True], ids=["vt", "vblk"])
@pytest.mark.parametrize("fp8", [False, True], ids=["f16", "fp8"])
@pytest.mark.parametrize("Hq,Hkv,hd,Dp", [(4, 4, 64, 64), (8, 2, 128, 128), (16, 1, 96, 128)])
def test_attn_encode_matches_fp64_oracle(cuda, native, Hq, Hkv, hd, Dp, fp8, blocked, n_split):
    from mipipe.ops.kernels import attn_encode, v_layout, v_pages_to_blocked
    q, slot, bt, kc, vc, segs, ref = case(Hq, Hkv, hd, Dp, fp8)
    vd = v_pages_to_blocked(vc) if blocked else vc
    with v_layout(blocked):   # the thread's layout is put back on the way out
        out = attn_encode(q.cuda(), slot.cuda(), bt.cuda(), kc.cuda(), vd.cuda(), Hkv, hd, segs, list(LENS),
                          n_split=n_split, split_pages=2, kv_fp8=fp8)
        torch.cuda.synchronize()
    got = out.cpu().double().numpy().reshape(ref.shape)
    assert np.isfinite(got).all(), "a dead key reached the output"
    ratio = np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))
    print(f"error ratio attn_encode: {ratio.max():.3f}")
    assert ratio.max() <= 1.0, ("worst (row, head, d):", np.unravel_index(ratio.argmax(), ratio.shape))
