"""The LoRA shrink / expand kernels (csrc/kernels/lora.hip) through mipipe.ops.kernels against torch
fp64 on the same f16-rounded A, B and x.

Tolerance: the bound the dense kernel tests put on F16 weights against `x @ deq.T`
(tests/test_gemvs_gpu.py and tests/test_gemm4_gpu.py: NMSE < 1e-5), applied to the delta alone
(Y after - Y before, over the bound rows' columns) and to the sum.  Everything the kernels must not
touch is compared bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5
N_ADAPTERS, N_LAYERS, LAYER = 4, 2, 1


def nmse(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).sum() / ((b ** 2).sum() + 1e-30))


def run_case(M, K, targets, ids, scales, seed=0, ld_pad=8):
    """targets: [(target id, N, {adapter: rank})] (an adapter missing from the dict has no pair for
    that target); ids / scales: per row.  Returns nothing; asserts everything."""
    from mipipe.ops import kernels as Kn
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    ldx = (K + 7) // 8 * 8 + 8
    x = torch.full((M, ldx), float("nan"), dtype=torch.float16)   # columns >= K are never read
    x[:, :K] = torch.randn(M, K, generator=g).half()
    n_tot = sum(n for _, n, _ in targets)
    ldy = n_tot + ld_pad
    y0 = torch.randn(M, ldy, generator=g) * 3.0 + 0.5
    yoff = np.cumsum([0] + [n for _, n, _ in targets])[:-1]
    pairs, keep = {}, []
    ref = y0.double().clone()
    ids = list(ids)
    for ti, (tg, n, ranks) in enumerate(targets):
        for a, r in ranks.items():
            rp = Kn.lora_rank_pad(r)
            A = torch.zeros(rp, K, dtype=torch.float16)
            B = torch.zeros(n, rp, dtype=torch.float16)
            A[:r] = (torch.randn(r, K, generator=g) / np.sqrt(K)).half()
            B[:, :r] = (torch.randn(n, r, generator=g) * (2.0 / np.sqrt(r))).half()
            Ad, Bd = A.to(dev), B.to(dev)
            keep += [Ad, Bd]
            pairs[(a, LAYER, tg)] = (Ad, Bd)
            rows = [m for m in range(M) if ids[m] == a]
            if rows:
                t = x[rows, :K].double() @ A.double().T
                sc = torch.tensor([scales[m] for m in rows], dtype=torch.float64)[:, None]
                ref[rows, yoff[ti]:yoff[ti] + n] += sc * (t @ B.double().T)
    tab_h = Kn.lora_tile_table(ids, scales, N_ADAPTERS)
    max_tiles = max(Kn.lora_max_tiles(M, N_ADAPTERS), 1)
    n_tiles = int(tab_h[0])
    assert n_tiles == sum((sum(1 for i in ids if i == a) + 15) // 16 for a in range(N_ADAPTERS)) <= max_tiles
    tiles = torch.from_numpy(tab_h).to(dev)
    tgt_tab = Kn.lora_target_table(pairs, N_ADAPTERS, N_LAYERS, dev)
    rcap = Kn.lora_rank_pad(64)
    xd = x.to(dev)
    outs = []
    for _ in range(2):
        y = y0.clone().to(dev)
        part = Kn.lora_part(max_tiles, K, len(targets), rcap, dev)   # NaN-filled: expand may read only what shrink stored
        args = (tiles, max_tiles, tgt_tab, N_ADAPTERS, N_LAYERS, LAYER, [t for t, _, _ in targets],
                [n for _, n, _ in targets], list(yoff), xd, K, y, part, rcap)
        Kn.lora_shrink(*args)
        Kn.lora_expand(*args)
        torch.cuda.synchronize()
        outs.append(y.cpu())
    y = outs[0]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs differ"
    # what must not be written, bit for bit
    touched = torch.zeros(M, ldy, dtype=torch.bool)
    for ti, (tg, n, ranks) in enumerate(targets):
        for m in range(M):
            if ids[m] in ranks:
                touched[m, yoff[ti]:yoff[ti] + n] = True
    assert torch.equal(y.view(torch.int32)[~touched], y0.view(torch.int32)[~touched]), "an untouched element changed"
    assert not torch.isnan(y).any()
    if touched.any():
        d_got = (y.double() - y0.double())[touched]
        d_ref = (ref - y0.double())[touched]
        assert float((d_ref ** 2).sum()) > 0 or all(scales[m] == 0 for m in range(M) if ids[m] >= 0)
        if float((d_ref ** 2).sum()) > 0:
            # (the f32 rounding of y0 + delta sits far below the bound: |y0| and |delta| are both O(1))
            assert nmse(d_got, d_ref) < TOL, nmse(d_got, d_ref)
        assert nmse(y[touched], ref[touched]) < TOL
    # a zero scale adds exactly nothing
    for m in range(M):
        if ids[m] >= 0 and scales[m] == 0:
            assert torch.equal(y[m].view(torch.int32), y0[m].view(torch.int32))


MID = dict(M=17, K=512, N=384, r=16)


def _one(M, K, N, r, seed):
    # rows alternate between adapter 1 and none, except at M = 1
    ids = [1 if (m % 3 != 2 or M == 1) else -1 for m in range(M)]
    scales = [1.0 + 0.25 * (m % 4) for m in range(M)]
    run_case(M, K, [(3, N, {1: r})], ids, scales, seed)


@pytest.mark.parametrize("M", [1, 5, 17, 64, 67])
def test_rows(cuda, native, M):
    _one(M, MID["K"], MID["N"], MID["r"], 10 + M)


@pytest.mark.parametrize("K", [384, 512, 1056])
def test_input_width(cuda, native, K):
    _one(MID["M"], K, MID["N"], MID["r"], 100 + K)


@pytest.mark.parametrize("N", [128, 384, 1032])
def test_output_width(cuda, native, N):
    _one(MID["M"], MID["K"], N, MID["r"], 200 + N)


@pytest.mark.parametrize("r", [3, 8, 16, 40, 64])
def test_rank(cuda, native, r):
    _one(MID["M"], MID["K"], MID["N"], r, 300 + r)


def test_qkv_group_three_targets_one_absent(cuda, native):
    """q, k, v of different N and ranks; adapter 0 has no v pair, adapter 2 no q pair."""
    M = 37
    ids = [(-1, 0, 2)[m % 3] for m in range(M)]
    scales = [0.5 + 0.1 * m for m in range(M)]
    run_case(M, 512, [(0, 512, {0: 8}), (1, 128, {0: 40, 2: 3}), (2, 136, {2: 16})], ids, scales, seed=7)


def test_k_split_28672(cuda, native):
    """K = 28672 (the 70B ffn_down input): 28 workgroup splits of 4 wave slices each."""
    ids = [0] * 17
    run_case(17, 28672, [(6, 256, {0: 16})], ids, [1.0] * 17, seed=8)


@pytest.mark.parametrize("name", ["all_none", "all_one", "three_interleaved", "seventeen_rows", "row_scales"])
def test_row_maps(cuda, native, name):
    M = 40
    if name == "all_none":
        ids, scales = [-1] * M, [1.0] * M
    elif name == "all_one":
        ids, scales = [2] * M, [1.0] * M
    elif name == "three_interleaved":
        ids, scales = [(0, -1, 1, 3, -1)[m % 5] for m in range(M)], [1.0 + 0.5 * (m % 3) for m in range(M)]
    elif name == "seventeen_rows":   # a full tile plus a one-row tile
        ids, scales = [1 if m < 17 else -1 for m in range(M)], [1.0] * M
    else:
        ids = [0 if m % 2 else 1 for m in range(M)]
        scales = [(0.0, -1.5, 1.0, 0.25)[m % 4] for m in range(M)]
    run_case(M, 512, [(0, 384, {0: 8, 1: 24, 2: 64, 3: 3})], ids, scales, seed=400 + len(name))
