"""The order of the ordered double sums (csrc/pnr_reduce_dev.h; DESIGN.md section 8 "Ordered reductions") restated in numpy
float64, for K terms and a given grid: `rows_device` is pnr_block_sum_rows after the kernel's grid-stride loop (a thread's items
in stride order, the wave's xor butterfly m = 32 .. 1, the four waves as ((w0 + w1) + w2) + w3, one row per workgroup) and
`combine` is pnr_rows_total (the rows in block order from 0.0).  Every operation is one IEEE double addition, so the result
is the kernel's bit for bit wherever the per-item terms are.  Users: _icp_ref.py (28 terms), the depth metrics (5) and the
cloud metrics (2)."""
import numpy as np

BLOCK = 256


def blocks_for(n, max_blocks, compute_units=256, per_cu=1):
    """the grid of a kernel whose entry point clamps ceil(n / 256) to [1, max_blocks] and caps it at per_cu workgroups a compute unit"""
    return max(1, min((n + BLOCK - 1) // BLOCK, max_blocks, compute_units * per_cu))


def rows_device(terms, active, grid):
    """terms (n, K) float64, active (n) bool -> ((grid, K) float64, (grid) int64): the rows a launch of `grid` workgroups writes,
    in the kernel's order of additions, and the active items of each workgroup.  An item that is not active adds nothing."""
    terms = np.asarray(terms, np.float64)
    n, K = terms.shape
    threads = grid * BLOCK
    trips = max((n + threads - 1) // threads, 1)
    pad = np.zeros((trips * threads, K))
    pad[:n] = terms
    padc = np.zeros(trips * threads, np.int64)
    padc[:n] = np.asarray(active, bool)
    acc = np.zeros((threads, K))
    for k in range(trips):                      # a thread's items in stride order
        chunk = pad[k * threads:(k + 1) * threads]
        acc = np.where(padc[k * threads:(k + 1) * threads, None] != 0, acc + chunk, acc)
    v = acc.reshape(grid, 4, 64, K)
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):              # the butterfly: every lane adds its partner's value
        v = v + v[:, :, lane ^ m]
    w = v[:, :, 0]
    rows = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    return rows, padc.reshape(trips, grid, BLOCK).sum((0, 2))


def combine(rows):
    """(K) Python floats: the rows (n_rows, K) added in block order from 0.0"""
    rows = np.asarray(rows, np.float64)
    tot = [0.0] * rows.shape[1]
    for row in rows:
        tot = [tot[k] + float(row[k]) for k in range(len(tot))]
    return tot


def total(terms, active, grid):
    """(K) float64: what the two launches leave in zeroed sums"""
    return np.array(combine(rows_device(terms, active, grid)[0]), np.float64)
