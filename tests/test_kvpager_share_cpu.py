"""KvPager shared pages (csrc/runtime/kvpager.h: reference counts, share, release, the write
invariant) through the host-only hook mp_kvpager_script: a list of pager calls on a fresh pager."""
import numpy as np
import pytest

ENSURE, SHARE, RELEASE, SHIFT, GRANT = range(5)
N_SLOTS, MAX_PAGES, N_PAGES = 4, 8, 12
TRASH = N_PAGES
# slot 0 (the donor): 200 tokens = pages 0..3; slots 1 and 2 share its first 2 pages and get a
# private tail page each (4, 5); slot 3 never shares: pages 6, 7
SETUP = [(ENSURE, 0, 200, 0), (SHARE, 1, 0, 2), (SHARE, 2, 0, 2), (GRANT, 1, 128, 150), (GRANT, 2, 128, 129),
         (ENSURE, 3, 100, 0)]


def run(native, ops):
    a = np.asarray(ops, dtype=np.int32).reshape(-1, 4)
    table = np.zeros((N_SLOTS, MAX_PAGES), dtype=np.int32)
    free, n_free = np.zeros(N_PAGES, dtype=np.int32), np.zeros(1, dtype=np.int32)
    shared = np.zeros(N_SLOTS, dtype=np.int32)
    total = native.mp_kvpager_script(N_SLOTS, MAX_PAGES, N_PAGES, a.ctypes.data, len(a), table.ctypes.data,
                                     free.ctypes.data, n_free.ctypes.data, shared.ctypes.data)
    if total < 0:
        raise RuntimeError(native.mp_last_error().decode())
    return total, table, free[:n_free[0]].tolist(), shared.tolist()


def test_share_tables(native):
    total, table, free, shared = run(native, SETUP)
    assert total == 2 and shared == [2, 2, 2, 0]
    assert table[0, :5].tolist() == [0, 1, 2, 3, TRASH]
    assert table[1, :4].tolist() == [0, 1, 4, TRASH] and table[2, :4].tolist() == [0, 1, 5, TRASH]
    assert table[3, :3].tolist() == [6, 7, TRASH]
    assert free == [8, 9, 10, 11]


@pytest.mark.parametrize("order", [(0, 1, 2), (1, 2, 0), (2, 0, 1)], ids=["donor-first", "donor-last", "donor-mid"])
def test_release_returns_pages_at_count_zero_once(native, order):
    seen = set(range(8, 12))
    for n in range(1, 4):
        total, table, free, shared = run(native, SETUP + [(RELEASE, s, 0, 0) for s in order[:n]])
        assert len(free) == len(set(free)), "a page entered the free list twice"
        live = set(order[n:])
        assert ({0, 1} <= set(free)) == (not live), "shared pages are freed by their last holder only"
        assert total == (2 if len(live) >= 2 else 0)
        for s in order[:n]:
            assert (table[s] == TRASH).all()
        seen |= set(free)
    assert sorted(free) == [0, 1, 2, 3, 4, 5, 8, 9, 10, 11] and seen == set(free)


def test_unshared_free_order_is_unchanged(native):
    # the never-sharing slot's pages come back highest table entry first, exactly as without sharing
    _, _, free, _ = run(native, SETUP + [(RELEASE, 3, 0, 0)])
    assert free == [6, 7, 8, 9, 10, 11]
    _, _, plain, _ = run(native, [(ENSURE, 0, 200, 0), (ENSURE, 1, 100, 0), (RELEASE, 0, 0, 0)])
    assert plain == [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]
    # a released donor's private pages too; its shared ones stay out until the last holder leaves
    _, _, free, _ = run(native, SETUP + [(RELEASE, 0, 0, 0)])
    assert free == [2, 3, 8, 9, 10, 11]


@pytest.mark.parametrize("ops, msg", [
    ([(SHIFT, 1, 0, 64)], "slot 1 holds shared pages"),
    ([(SHIFT, 0, 128, 64)], "slot 0 holds shared pages"),
    ([(GRANT, 1, 127, 200)], "into a shared page"),
    ([(GRANT, 0, 100, 300)], "into a shared page"),
    ([(SHARE, 3, 0, 1)], "already owns"),
    ([(RELEASE, 3, 0, 0), (SHARE, 3, 0, 5)], "5 pages of the 4"),
])
def test_refusals(native, ops, msg):
    with pytest.raises(RuntimeError, match=msg):
        run(native, SETUP + ops)

