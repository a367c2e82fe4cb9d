"""The batch and the host reference of tests/test_gpu_walker_order.py, checked without a device (tests/walker_order.py)."""
import math

import numpy as np
import pytest

import walker_order as wo

DIMS = (2, 3, 4, 5, 6, 7, 8)


@pytest.mark.parametrize("D", DIMS)
def test_base_walkers_are_sorted_and_their_coordinates_well_apart(D):
    """more than 1e-3 apart: no order of a base walker is a tie, and no two orders of it are the same row"""
    b = wo.build_batch(D)
    base = wo.base_walkers(D)
    assert base.shape == (wo.n_base(D), D) and base.dtype == np.float32
    assert np.diff(base.astype(np.float64), axis=-1).min() > 1e-3 and np.abs(base).max() < wo.BOX_L
    assert not wo.tie_rows(b.x[b.base >= 0]).any()


@pytest.mark.parametrize("D", DIMS)
def test_every_order_of_every_base_walker_once_half_odd_half_even(D):
    b = wo.build_batch(D)
    base = wo.base_walkers(D)
    xs, inv = wo.host_reference(b.x)
    fact = math.factorial(D)
    assert np.array_equal(np.bincount(b.base[b.base >= 0], minlength=wo.n_base(D)), np.full(wo.n_base(D), fact))
    for n in range(wo.n_base(D)):
        rows = b.base == n
        assert np.array_equal(xs[rows], np.broadcast_to(base[n], (fact, D)))
        assert len({r.tobytes() for r in b.x[rows]}) == fact                       # D! different rows
        assert int((inv[rows] & 1).sum()) * 2 == fact
        assert inv[rows].min() == 0 and inv[rows].max() == D * (D - 1) // 2        # the sorted and the reversed order are among them
    # the shuffle spread them: the orders of base walker 0 do not sit in one 32-walker tile
    assert len(set(np.flatnonzero(b.base == 0) // 32)) > 1


@pytest.mark.parametrize("D", DIMS)
def test_pair_count_has_the_parity_of_the_cycle_decomposition(D):
    """the `>` pair count against an independent parity: the row is base[perm], so the permutation is known"""
    perms = wo.permutations(D)
    assert len(perms) == math.factorial(D) and len({tuple(p) for p in perms}) == len(perms)
    rows = wo.base_walkers(D)[0][perms]
    _, inv = wo.host_reference(rows)
    assert np.array_equal(inv & 1, np.array([wo.parity_by_cycles(list(p)) for p in perms]))
    assert wo.parity_by_cycles([0, 1, 2]) == 0 and wo.parity_by_cycles([1, 0, 2]) == 1 and wo.parity_by_cycles([1, 2, 0]) == 0


@pytest.mark.parametrize("D", DIMS)
def test_special_rows_and_their_inversions(D):
    b = wo.build_batch(D)
    xs, inv = wo.host_reference(b.x)
    names = [k for k, _ in wo.special_rows(D)]
    assert set(names) >= {"ascending", "descending", "adjacent tie", "all equal"}
    assert ("tie of non-adjacent arrivals" in names) == (D >= 3) and ("+0 -0" in names) == (D == 2) == ("-0 +0" in names)
    for name, row in wo.special_rows(D):
        at = np.flatnonzero(b.kind == name)
        assert len(at) >= 1 and any(np.array_equal(b.x[i], row) for i in at), name
        for i in at:
            assert b.base[i] == -1 and inv[i] == wo.SPECIAL_INVERSIONS[name](D), (name, inv[i])
    assert np.array_equal(b.kind != "", b.base < 0)
    one = dict(wo.special_rows(D))
    assert one["adjacent tie"][0] == one["adjacent tie"][1] and len(set(one["all equal"])) == 1
    if D >= 3:
        a, bb, c = one["tie of non-adjacent arrivals"][:3]
        assert a == c and bb > a
    assert wo.tie_rows(b.x).sum() == (3 if D >= 3 else 4)          # D = 2: the adjacent tie, all equal, and the two rows of zeros
    assert (np.diff(xs, axis=-1) >= 0).all()


def test_stable_sort_leaves_signed_zeros_in_arrival_order():
    x = np.array([[0.0, -0.0], [-0.0, 0.0]], np.float32)
    xs, inv = wo.host_reference(x)
    assert np.array_equal(xs.view(np.int32), x.view(np.int32)) and np.array_equal(inv, [0, 0])
    assert np.array_equal(x.view(np.uint32), np.array([[0, 0x80000000], [0x80000000, 0]], np.uint32))
    b = wo.build_batch(2)
    xs, _ = wo.host_reference(b.x)
    for name in ("+0 -0", "-0 +0"):
        i = int(np.flatnonzero(b.kind == name)[0])
        assert np.array_equal(xs[i].view(np.int32), b.x[i].view(np.int32)) and np.signbit(b.x[i]).sum() == 1


@pytest.mark.parametrize("D", DIMS)
def test_no_batch_is_a_whole_number_of_tiles(D):
    b = wo.build_batch(D)
    assert len(b.x) % 32 != 0 and len(b.x) >= wo.n_base(D) * math.factorial(D) + 4
    assert len(b.x) > max(wo.RAGGED) and all(B % 32 for B in wo.RAGGED)
    assert b.x.dtype == np.float32 and b.x.flags["C_CONTIGUOUS"] and np.isfinite(b.x).all()
    again = wo.build_batch(D)
    assert np.array_equal(again.x.view(np.int32), b.x.view(np.int32))


def test_refused_pairs_are_what_the_built_shapes_rule_gives():
    """mfma_shape_built: one row block up to D = 8, two row blocks up to D = 4; every other kernel serves every shape"""
    assert {wo.n_row_blocks(23), wo.n_row_blocks(33)} == {1, 2} and wo.n_row_blocks(23) == 1
    rule = {("mfma", (D, kn)) for D, kn in wo.SHAPES if not wo.mfma_shape_built(D, wo.n_row_blocks(kn))}
    assert rule == {("mfma", (D, kn)) for D, kn in wo.SHAPES if wo.n_row_blocks(kn) == 2 and D >= 5}
    assert wo.REFUSED == rule == {("mfma", (5, 33))}
    assert len(set(wo.SHAPES)) == 11 and set(wo.KERNELS) == {"mfma", "wave", "scalar", "auto"}
