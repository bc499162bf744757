"""tests/_reduce_ref.py on the CPU: each stage of the stated order on inputs where another order gives another bit.  With
u = 2^-53, 1 + u rounds to 1 (ties to even) and 1 + 2 u does not: (1 + u) + u = 1, 1 + (u + u) = 1 + 2 u."""
import math

import numpy as np

import _reduce_ref as rr

U = 2.0 ** -53


def one(values, grid=1):
    """K = 1: {item: value} -> the rows of a launch of `grid` workgroups over max(item) + 1 items"""
    n = max(values) + 1
    t = np.zeros((n, 1))
    for i, v in values.items():
        t[i, 0] = v
    return rr.rows_device(t, np.ones(n, bool), grid)[0][:, 0]


def test_every_stage_adds_in_the_stated_order():
    assert one({0: 1.0, 256: U, 512: U})[0] == 1.0                  # a thread's items in stride order
    assert one({0: U, 256: U, 512: 1.0})[0] == 1.0 + 2 * U
    assert one({0: 1.0, 32: U, 48: U})[0] == 1.0                    # the butterfly starts at m = 32: lane 0 meets lane 32 first
    assert one({0: 1.0, 16: U, 48: U})[0] == 1.0 + 2 * U            # lanes 16 and 48 meet at m = 32, lane 0 meets their sum at m = 16
    assert one({0: 1.0, 1: U, 33: U})[0] == 1.0 + 2 * U             # lanes 1 and 33 meet at m = 32, lane 0 meets their sum at m = 1
    assert one({0: 1.0, 64: U, 128: U})[0] == 1.0                   # the waves: (w0 + w1) + w2
    assert one({64: U, 128: U, 192: 1.0})[0] == 1.0 + 2 * U         # ((w0 + w1) + w2) + w3
    rows = one({0: 1.0, 256: U, 512: U}, grid=3)
    assert rows.tolist() == [1.0, U, U] and rr.combine(rows[:, None]) == [1.0]      # the rows in block order from 0.0
    assert rr.combine(rows[::-1, None]) == [1.0 + 2 * U]


def test_counts_grids_and_the_any_order_bound():
    g = np.random.default_rng(0)
    for n, grid in ((1, 1), (257, 2), (1000, 3), (5000, 4)):
        t = g.uniform(0, 1, (n, 3)) * 2.0 ** g.integers(-20, 20, (n, 3))
        active = g.random(n) < 0.7
        rows, counts = rr.rows_device(np.where(active[:, None], t, 0.0), active, grid)
        assert rows.shape == (grid, 3) and int(counts.sum()) == int(active.sum())
        assert counts.tolist() == [int(active[np.arange(n) // 256 % grid == b].sum()) for b in range(grid)]
        tot = rr.total(np.where(active[:, None], t, 0.0), active, grid)
        for k in range(3):
            exact = math.fsum(t[active, k])
            assert abs(tot[k] - exact) <= max(int(active.sum()), 1) * U * exact
    assert rr.blocks_for(1, 1024) == 1 and rr.blocks_for(0, 1024) == 1 and rr.blocks_for(257, 1024) == 2
    assert rr.blocks_for(10 ** 7, 1024, 256, 4) == 1024 and rr.blocks_for(10 ** 7, 1024, 64, 4) == 256 and rr.blocks_for(10 ** 7, 256, 304, 1) == 256
