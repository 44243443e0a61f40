"""NumPy restatement of the dropout keep-mask stream of csrc/common.h (philox4x32 / u32_to_unit / keep_scale), vectorised over counters.  Test-only:
tests/test_gpu_storage_ops.py pins the keep pattern of every pooled-dropout entry to it, element for element."""
import numpy as np

# Philox-4x32-10: the two multipliers, the two Weyl key increments, and the two FIXED counter words (c2, c3) -- the kernels key the stream by
# (element-quad index -> c0 c1, seed -> k0 k1) and hold the upper counter half constant
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
PHILOX_CTR_WORD2, PHILOX_CTR_WORD3 = 0x243F6A88, 0x85A308D3
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32(ctr, seed):
    """the four 32-bit outputs of counter `ctr` (array of quad indices) under key `seed`: uint32 array of shape ctr.shape + (4,)"""
    ctr = np.asarray(ctr, np.uint64)
    c0, c1 = ctr & _MASK, ctr >> np.uint64(32)
    c2 = np.full_like(c0, PHILOX_CTR_WORD2); c3 = np.full_like(c0, PHILOX_CTR_WORD3)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                     # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def u32_to_unit(u):
    """the top 24 bits as a float32 in [0, 1) (exact)"""
    return (np.asarray(u, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def keep_scale(quad_idx, rate, seed):
    """inverted-dropout factors of element quads `quad_idx`: float32 array quad_idx.shape + (4,), each 0 or 1 / (1 - rate) as the kernels compute it in fp32"""
    r = np.float32(rate)
    s = np.float32(1.0) / (np.float32(1.0) - r)
    return np.where(u32_to_unit(philox4x32(quad_idx, seed)) >= r, s, np.float32(0.0)).astype(np.float32)


def keep_scale_dense(shape, rate, seed):
    """keep_scale of a dense NHWC tensor whose quad index is the flat element index / 4 (shape[-1] % 4 == 0), in the tensor's shape"""
    n = int(np.prod(shape)) // 4
    return keep_scale(np.arange(n, dtype=np.uint64), rate, seed).reshape(shape)
