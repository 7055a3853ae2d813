"""numpy restatement of the drop-out keep flags (include/unet_hip.h, unet_forward_dropout): Philox4x32-10 (Salmon, Moraes,
Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) keyed by the seed, counted by (element group, step, site).
Imported by the drop-out tests like the other *_ref modules; test_dropout_cpu.py holds it to the published known answers."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (broadcastable), key: 2 -> the 4 output words as uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint32) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c[0].astype(np.uint64)
            p1 = M1 * c[2].astype(np.uint64)
            hi0, lo0 = (p0 >> _32).astype(np.uint32), p0.astype(np.uint32)
            hi1, lo1 = (p1 >> _32).astype(np.uint32), p1.astype(np.uint32)
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
            k0, k1 = np.uint32(k0 + W0), np.uint32(k1 + W1)
    return c


def threshold(p):
    """keep <=> word >= threshold: (uint32) min(floor(p * 2^32), 2^32 - 1), p taken as the float32 the library receives."""
    return np.uint32(min(np.floor(float(np.float32(p)) * 4294967296.0), 4294967295.0))


def scale(p):
    """1.0f / (1.0f - p) in fp32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_flags(seed, step, site, first, n, p):
    """uint8 [n]: the keep flags of elements first .. first+n-1 (64-bit linear NHWC indices) of `site`'s tensor."""
    idx = np.uint64(first) + np.arange(n, dtype=np.uint64)
    g = idx >> np.uint64(2)
    j = (idx & np.uint64(3)).astype(np.int64)
    gu, inv = np.unique(g, return_inverse=True)
    c3 = np.uint32(((step >> 32) & 0x7FFFFFFF) | (site << 31))
    words = philox4x32_10((gu.astype(np.uint32), (gu >> _32).astype(np.uint32), np.uint32(step & 0xFFFFFFFF), c3),
                          (seed & 0xFFFFFFFF, seed >> 32))
    r = np.stack(words, axis=1)[inv.ravel(), j]
    return (r >= threshold(p)).astype(np.uint8)
