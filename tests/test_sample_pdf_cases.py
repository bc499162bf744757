"""CPU checks of tests/_sample_pdf_cases.py, the inputs of the sample_pdf sweeps: properties of the INPUTS, computed from the
oracle's pdf in numpy -- nothing here runs a kernel."""
import numpy as np
import pytest

import _sample_pdf_cases as cases
from oracle import c_oracle as co


def test_cases_hold_rows_on_both_sides_of_the_scan_regime():
    """For nw = Nc - 2 <= 64 the kernels run the CDF as a parallel scan on rows whose pdf values are all 0 or >= 2^-28 and sum to
    less than 1.999, and as the sequential chain on the others: every such case must hold rows of both kinds.  (nw > 64 always
    runs the chain.)  Nc = 3 is the one exception the arithmetic forces: its single pdf value is x / x = 1 for every finite
    weight, so no finite row can leave the regime; there every row must be inside it."""
    for Nc in range(3, 67):
        _, _, z, w = cases.case(Nc)
        inside = cases.scan_regime(w)
        assert inside.any(), Nc
        if Nc == 3:
            assert inside.all() and np.all(cases.oracle_pdf(w) == 1.0)
        else:
            assert (~inside).any(), Nc
        fam = np.arange(w.shape[0]) % cases.N_FAMILIES
        assert inside[np.isin(fam, (1, 2, 6))].all(), Nc                    # pure-floor rows: uniform pdf
        assert Nc == 3 or not inside[fam == 7].any(), Nc                     # the spike: floor pdf 1e-9 < 2^-28


def test_case_shapes_and_families():
    for Nc in (3, 4, 8, 9, 10, 64, 65, 256):
        rays, t_rand, z, w = cases.case(Nc)
        R = cases.R_CASE
        assert rays.shape == (R, 8) and t_rand.shape == z.shape == w.shape == (R, Nc)
        assert R % 64 != 0 and R > 64 and all(a.dtype == np.float32 for a in (rays, t_rand, z, w))
        assert np.array_equal(z, co.stratified(rays, Nc, t_rand=t_rand)) and (np.diff(z, axis=1) >= 0).all()
        assert np.isfinite(w).all() and (w >= 0).all()
        fam = np.arange(R) % cases.N_FAMILIES
        assert (w[fam == 1] == 0).all() and (w[fam == 2] == np.float32(1e-30)).all()
        assert ((w[fam == 3] == 0).sum(1) >= Nc // 2).all()
        assert ((w[fam == 4] == np.float32(3e4)).sum(1) == (Nc > 8)).all() and ((w[fam == 5] == np.float32(1e9)).sum(1) == (Nc > 8)).all()
        assert (w[fam == 6][:, 1:-1] == 0).all() and (w[fam == 6][:, [0, -1]] > 0).all()
        assert ((w[fam == 7] > 0).sum(1) == 1).all() and (w[fam == 7][:, [0, -1]] == 0).all()
        # the same case twice is the same arrays: tests may compute a reference once and share it
        again = cases.case(Nc)
        assert all(np.array_equal(a, b) for a, b in zip((rays, t_rand, z, w), again))


@pytest.mark.parametrize("Nc", [4, 9, 34, 64])
def test_spike_rows_hit_the_small_denominator_branch(Nc):
    """family 7: all bins but the spike's have cdf[above] - cdf[below] < 1e-5 (the `denom = 1` branch): with deterministic u every
    sample of such a row has an index at one of the two edges of the spike's bin or sits at a flat stretch's start"""
    _, _, z, w = cases.case(Nc)
    p = cases.oracle_pdf(w[7::cases.N_FAMILIES])
    assert ((p < 1e-5).sum(1) == Nc - 3).all() and (p.max(1) > 0.99).all()


def test_fine_count_lists():
    assert cases.nf_general(3) == [1, 2, 63, 64, 65, 128, 192, 509] and cases.nf_general(256) == [1, 2, 63, 64, 65, 128, 192, 256]
    assert cases.nf_general(448) == [1, 2, 63, 64] and cases.nf_cpu(7) == [1, 2, 7, 63, 64, 65, 128, 192, 505]
    assert cases.nf_inference(3) == [1, 2, 3, 63, 64, 65, 127, 128, 129, 192, 253]
    assert cases.nf_inference(64) == [1, 2, 3, 63, 64, 65, 127, 128, 129, 192] and cases.nf_inference(63) == [1, 2, 3, 63, 64, 65, 127, 128, 129, 192, 193]
    for Nc in range(3, 65):
        assert all(Nc + nf <= 256 for nf in cases.nf_inference(Nc)) and 256 - Nc in cases.nf_inference(Nc)
