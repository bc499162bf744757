"""Inputs of the sample_pdf sweeps (tests/test_oracle.py on the CPU, tests/test_gpu_sample_pdf_sweep.py on the GPU): one case
per coarse sample count Nc, built so that every shape-dependent branch of the sampler meets rows on both of its sides.

Rays are random with given jitter, z = co.stratified of them.  The weights repeat eight families row by row (row r is family
r % 8):

  0  Gaussian peaks x a random scale          -- compositing-like weights
  1  all zero                                  -- the 1e-5 floor alone: uniform pdf
  2  all 1e-30                                 -- vanishes against the floor
  3  every second weight zero
  4  one 3e4 among uniform^4 (Nc > 8)          -- pdf of the floor = 1e-5 / 3e4 < 2^-28
  5  one 1e9 among uniform^4 (Nc > 8)          -- the floor is absorbed by the sum
  6  only the two END weights non-zero         -- those are ignored (weights[1:-1]): a pure floor
  7  one 1e4 spike inside a zero floor         -- every bin but one has denom < 1e-5

The kernels compute the CDF of a row of nw = Nc - 2 <= 64 pdf values with a parallel scan when `scan_regime` holds for it
(every pdf value 0 or >= 2^-28 and their sum < 1.999: then no float64 add of the running sum rounds) and with the sequential
chain otherwise.  Family 7 is outside the regime for every nw >= 2 (1e-5 / 1e4 = 1e-9 < 2^-28 = 3.7e-9), families 1, 2 and 6
are always inside; test_sample_pdf_cases.py::test_cases_hold_rows_on_both_sides_of_the_scan_regime checks that on the
oracle's own pdf."""
import numpy as np

from oracle import c_oracle as co

R_CASE = 67                    # ragged, and more than one wave's worth of lanes
N_FAMILIES = 8
NF_GENERAL = (1, 2, 63, 64, 65, 128, 192)          # + 512 - Nc: nf_general


def nf_general(Nc):
    """the fine counts of the general-body sweep at Nc (Nc + Nf <= 512)"""
    return sorted({nf for nf in NF_GENERAL + (512 - Nc,) if nf >= 1 and Nc + nf <= 512})


def nf_cpu(Nc):
    """the CPU sweep adds Nf = Nc"""
    return sorted(set(nf_general(Nc)) | {Nc})


def nf_inference(Nc):
    """the fine counts of the inference-instance sweep at Nc <= 64 (Nc + Nf <= 256; the instance itself takes Nf <= 192, so
    256 - Nc is one of its shapes only at Nc = 64 and goes to the general body below that)"""
    return sorted({nf for nf in (1, 2, 3, 63, 64, 65, 127, 128, 129, 192, 256 - Nc) if nf >= 1 and Nc + nf <= 256})


def rays(rng, R, near=0.5, far=60.0):
    o = rng.normal(0, 1, (R, 3)) + np.array([0, 1.5, 0])
    d = rng.normal(0, 0.3, (R, 3)) + np.array([0, 0, 1.0])
    return np.concatenate([o, d, np.full((R, 1), near), np.full((R, 1), far)], 1).astype(np.float32)


def weights(rng, R, Nc):
    """(R, Nc) float32, family r % 8 in row r"""
    i = np.arange(Nc)[None]
    w = np.empty((R, Nc), np.float32)
    for r in range(R):
        fam = r % N_FAMILIES
        base = (rng.uniform(0, 1, Nc) ** 4).astype(np.float32)
        inner = int(rng.integers(1, Nc - 1))                    # a column that weights[1:-1] keeps
        if fam == 0:
            row = np.zeros(Nc)
            for _ in range(int(rng.integers(1, 4))):
                row = row + np.exp(-0.5 * ((i[0] - rng.uniform(0, Nc)) / rng.uniform(0.5, 6)) ** 2)
            row = row * rng.uniform(0.05, 1)
        elif fam == 1:
            row = np.zeros(Nc)
        elif fam == 2:
            row = np.full(Nc, 1e-30)
        elif fam == 3:
            row = base.copy()
            row[r // N_FAMILIES % 2::2] = 0.0
        elif fam in (4, 5):
            row = base.copy()
            if Nc > 8:
                row[inner] = 3.0e4 if fam == 4 else 1.0e9
        elif fam == 6:
            row = np.zeros(Nc)
            row[0], row[-1] = rng.uniform(0.1, 1, 2)
        else:
            row = np.zeros(Nc)
            row[inner] = 1.0e4
        w[r] = row
    return w


def case(Nc, R=R_CASE, seed=0):
    """(rays, t_rand, z, w) of the sweep at Nc; z = co.stratified(rays, Nc, t_rand=t_rand)"""
    rng = np.random.default_rng(100003 * seed + Nc)
    ry = rays(rng, R)
    t_rand = rng.random((R, Nc)).astype(np.float32)
    z = co.stratified(ry, Nc, t_rand=t_rand)
    return ry, t_rand, z, weights(rng, R, Nc)


def uniforms(Nc, Nf, R=R_CASE, seed=0):
    return np.random.default_rng(7919 * seed + 521 * Nc + Nf).random((R, Nf)).astype(np.float32)


def oracle_pdf(w):
    """pdf rows as pnro_sample_pdf forms them: (w[1:-1] + 1e-5) / torch.sum of that, in float32.  The sum's ORDER does not
    matter to scan_regime's thresholds (a factor 2^-28 and 1.999 against one ulp), so numpy's own float32 sum serves."""
    x = (w[:, 1:-1].astype(np.float32) + np.float32(1e-5)).astype(np.float32)
    return (x / x.sum(1, dtype=np.float32)[:, None]).astype(np.float32)


def scan_regime(w):
    """per row: may the kernels run the CDF as a parallel scan?  (every pdf value 0 or >= 2^-28, float64 sum < 1.999)"""
    p = oracle_pdf(w)
    ok = ((p == 0) | (p >= np.float32(2.0 ** -28))).all(1)
    return ok & (p.astype(np.float64).sum(1) < 1.999)
