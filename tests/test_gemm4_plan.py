"""gemm4 launch plans (csrc/runtime/gemm4_plan.cpp, C API mp_gemm4_plan / mp_moe_gemm4_plan): a pure
host function of shape, weight type and knobs, so no GPU is needed.

tests/golden/gemm4_plan.json holds the decisions the selection code made before it became the plan
(the old `namespace mp` block of gemm4.hip, compiled as a host program whose launch stub recorded
its template arguments, the clamped split count, the stages per split, the weight DMA mode and the
grid).  One group per (knob setting, weight type, ntiles, nsb [, E, k]); a row is `row` in the file:
M, epi, mode, ok, bm, nwv, tw, nsplit, per, wnt, grid_x, grid_y, grid_z, with mode = allow_split |
2 * partial_stores for a dense launch and per_slot for a MoE one; a launch that did not happen
(ok 0) has zeros."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm4_plan.json")
EPI_STORE, EPI_ATOMIC, EPI_SWIGLU = 0, 1, 2
P_Q4_K = 2


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def K(native):
    from mipipe.ops import kernels
    return kernels


def _with_knobs(knobs, fn):
    from mipipe import _native as N
    try:
        for name, v in knobs.items():
            N.check(N.lib().mp_set_knob(name.encode(), v), "knob")
        return fn()
    finally:
        for name in knobs:
            N.lib().mp_reset_knob(name.encode())


def _plan(K, g, M, epi, mode):
    if g["kind"] == "dense":
        return K.gemm4_plan(g["ptype"], epi, M, g["ntiles"], g["nsb"], bool(mode & 1), bool(mode & 2))
    return K.moe_gemm4_plan(g["ptype"], epi, M, g["k"], g["E"], g["ntiles"], g["nsb"], bool(mode))


def _walk(K, golden):
    """(group, row, plan) over the whole recorded grid, each group under its knobs."""
    for g in golden["groups"]:
        plans = _with_knobs(g["knobs"], lambda: [_plan(K, g, r[0], r[1], r[2]) for r in g["rows"]])
        for r, pl in zip(g["rows"], plans):
            yield g, r, pl


def test_golden_covers_the_required_grid(golden):
    """The fixture holds what the plan is specified against (so a trimmed file cannot pass quietly)."""
    assert golden["row"][3:] == ["ok", "bm", "nwv", "tw", "nsplit", "per", "wnt", "grid_x", "grid_y", "grid_z"]
    dense = [g for g in golden["groups"] if g["kind"] == "dense"]
    moe = [g for g in golden["groups"] if g["kind"] == "moe"]
    dflt = {(g["ntiles"], g["nsb"]) for g in dense if not g["knobs"]}
    assert dflt >= {(640, 32), (512, 32), (3584, 32), (512, 112), (8016, 32), (384, 16), (256, 16), (1792, 16), (256, 56),
                    (13, 5), (40, 8), (40, 9), (32, 32), (64, 32)}
    assert {r[0] for g in dense for r in g["rows"]} >= {65, 96, 128, 129, 200, 256, 300, 512, 2048}
    assert {(r[1], r[2]) for g in dense for r in g["rows"]} >= {(0, 1), (1, 1), (1, 0), (2, 1), (1, 3)}
    assert {g["ptype"] for g in dense if not g["knobs"]} >= {0, 1, 2, 3, 4, 6}
    want = [{"GEMM3_BM": v} for v in (96, 128, 256)] + [{"GEMM4_NW": v} for v in (4, 7, 8)]
    want += [{"GEMM4_TW4": v} for v in (0, 2, 3, 4, 5, 6)] + [{"GEMM4_TW4": 4, "GEMM4_NW": 7}]
    want += [{"GEMM3_SPLIT": v} for v in (1, 3, 4, 8, 42, 128)] + [{"GEMM2_SPLIT_WG": v} for v in (128, 512)]
    want += [{"GEMM4_WNT": v} for v in (1, 2)]
    for pt in (2, 4, 0):   # Q4_K, Q6_K, F16
        have = [g["knobs"] for g in dense if g["ptype"] == pt]
        assert all(k in have for k in want), pt
    assert {(g["E"], g["k"], g["ntiles"], g["nsb"]) for g in moe} >= {(8, 2, 1792, 16), (8, 2, 256, 56), (128, 8, 96, 8),
                                                                      (128, 8, 128, 3)}
    assert {r[0] for g in moe for r in g["rows"]} >= {65, 256, 512, 2048}
    assert {(r[1], r[2]) for g in moe for r in g["rows"]} >= {(2, 0), (2, 1), (1, 0), (1, 1)}
    have = [g["knobs"] for g in moe]
    for k in [{"GEMM4_MOE64": v} for v in (0, 1, 3)] + [{}, {"GEMM4_TW4": 3}, {"GEMM4_NW": 7}, {"GEMM3_SPLIT": 4}]:
        assert k in have, k


def test_plan_matches_recorded_decisions(K, golden):
    n = 0
    for g, r, pl in _walk(K, golden):
        got = [pl[f] for f in K.GEMM4_PLAN_FIELDS]
        assert got == r[3:], (g["kind"], g["knobs"], g["ptype"], g["ntiles"], g["nsb"], r[:3], got, r[3:])
        n += 1
    assert n > 5000


@pytest.mark.parametrize("ntiles,nsb,epi,partial,want", [
    # 70B gate/up, SwiGLU, M 256: one 256-row block, 4 waves x 64 columns, 224 column groups
    (3584, 32, EPI_SWIGLU, False, dict(bm=256, nwv=4, tw=4, nsplit=1, per=128, wnt=1, grid_x=224, grid_y=1, grid_z=1)),
    # 8B gate/up, SwiGLU, M 256: 128-row tiles (256-row ones would leave 112 workgroups), 7 waves fill 256 CUs
    (1792, 16, EPI_SWIGLU, False, dict(bm=128, nwv=7, tw=2, nsplit=1, per=64, wnt=0, grid_x=256, grid_y=1, grid_z=1)),
    # 70B down, partial stores, M 256: 64 workgroups -> 4 splits of 112 stages
    (512, 112, EPI_ATOMIC, True, dict(bm=128, nwv=8, tw=2, nsplit=4, per=112, wnt=0, grid_x=64, grid_y=4, grid_z=1)),
])
def test_plan_hand_derived(K, ntiles, nsb, epi, partial, want):
    """Three Q4_K decisions at default knobs, worked out by hand from the rules."""
    pl = K.gemm4_plan(P_Q4_K, epi, 256, ntiles, nsb, True, partial)
    assert pl["ok"] == 1
    assert {f: pl[f] for f in want} == want


def test_plan_internal_consistency(K, golden):
    from mipipe import _native as N
    L = N.lib()
    assert L.mp_gemm4_geometry_count() == 17
    for g, r, pl in _walk(K, golden):
        M, moe = r[0], g["kind"] == "moe"
        if not pl["ok"]:
            assert all(pl[f] == 0 for f in K.GEMM4_PLAN_FIELDS)
            continue
        ctx = (g, r)
        cdiv = lambda a, b: (a + b - 1) // b   # noqa: E731
        assert pl["grid_x"] == cdiv(g["ntiles"], pl["tw"] * pl["nwv"]) * cdiv(M, pl["bm"]), ctx
        assert pl["nsplit"] * pl["per"] >= 4 * g["nsb"] > (pl["nsplit"] - 1) * pl["per"], ctx
        assert pl["grid_y"] == pl["nsplit"] and pl["grid_z"] == (g["E"] if moe else 1), ctx
        assert pl["in_table"] == 1 and L.mp_gemm4_has_geometry(g["ptype"], pl["bm"], pl["nwv"], pl["tw"], int(moe)) == 1, ctx
    # not in the table: the dense 64-row tile, a 5-wave tile, any tile of a type gemm4 does not take
    assert L.mp_gemm4_has_geometry(P_Q4_K, 64, 8, 2, 0) == 0
    assert L.mp_gemm4_has_geometry(P_Q4_K, 64, 8, 2, 1) == 1
    assert L.mp_gemm4_has_geometry(P_Q4_K, 128, 5, 2, 0) == 0
    assert L.mp_gemm4_has_geometry(0, 256, 8, 2, 0) == 0    # F16: the 128-row 8 x 32 tile only
    assert L.mp_gemm4_has_geometry(5, 128, 8, 2, 0) == 0    # Q4_0


def test_scratch_sizing_uses_the_launch_plan(K, golden):
    """HipStage::alloc_runtime sizes the split-K partial buffer from plan_gemm4(ptype, ATOMIC, M,
    ntiles, nsb, true, true).nsplit: the partial-store launch of the same arguments runs that many
    splits, whatever epilogue and allow_split its caller names."""
    for g in golden["groups"]:
        if g["kind"] != "dense":
            continue
        def both():   # noqa: E306
            out = []
            for M in sorted({r[0] for r in g["rows"]}):
                size = K.gemm4_plan(g["ptype"], EPI_ATOMIC, M, g["ntiles"], g["nsb"], True, True)
                run = K.gemm4_plan(g["ptype"], EPI_STORE, M, g["ntiles"], g["nsb"], False, True)
                out.append((size, run))
            return out
        for size, run in _with_knobs(g["knobs"], both):
            assert size == run
            assert not size["ok"] or size["nsplit"] >= 2
