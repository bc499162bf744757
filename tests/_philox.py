"""numpy Philox4x32-10 and the in-kernel stream contract of include/pnr.h ("in-kernel RNG"), test side: what the kernels of
panopticnerf_amd/csrc/pnr_philox.h must draw, computed independently of them."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: (..., 4) uint32, key: (..., 2) uint32 (broadcast) -> (..., 4) uint32"""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i] for i in range(4)]
    key = np.asarray(key, dtype=np.uint64)
    k0, k1 = key[..., 0], key[..., 1]
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & MASK
            k1 = (k1 + np.uint64(W1)) & MASK
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & MASK, p0 & MASK]
    return np.stack(c, -1).astype(np.uint32)


def stream_words(seed, offset, tag, ray_base, n_rays, n):
    """(n_rays, n) uint32: word j & 3 of the block of sample j of global ray ray_base + r"""
    seed, offset = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    j = np.arange(n, dtype=np.uint64)
    g = (np.uint64(ray_base) + np.arange(n_rays, dtype=np.uint64)) & MASK
    ctr = np.zeros((n_rays, n, 4), dtype=np.uint64)
    ctr[..., 0] = (j >> np.uint64(2)) | np.uint64(int(tag) << 24)
    ctr[..., 1] = g[:, None]
    ctr[..., 2] = offset & 0xFFFFFFFF
    ctr[..., 3] = offset >> 32
    blocks = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    return np.take_along_axis(blocks, (j & np.uint64(3)).astype(np.int64)[None, :, None].repeat(n_rays, 0), 2)[..., 0]


def uniforms(words):
    """fp32 in [0, 1): (w >> 8) * 2^-24 (exact)"""
    return ((words >> 8).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def normals64(words):
    """float64 Box-Muller on the word pairs (2k, 2k + 1) of each block (n a multiple of 4: whole blocks)"""
    w = words.astype(np.float64)
    a, b = w[..., 0::2], w[..., 1::2]
    u1 = (np.floor(a / 256) + 1) * 2.0 ** -24
    u2 = np.floor(b / 256) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.empty(words.shape, dtype=np.float64)
    out[..., 0::2] = r * np.cos(2 * np.pi * u2)
    out[..., 1::2] = r * np.sin(2 * np.pi * u2)
    return out
