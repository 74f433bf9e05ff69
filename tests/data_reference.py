"""numpy restatement of the device-resident data set's contract (include/mapdit.h, "Device-resident latent data set"), written from
the published definitions: Philox4x32-10 with uint64 arithmetic, the cycle-walking Feistel permutation, Box-Muller normals in fp64
from the same words, and the step -> (epoch, first) arithmetic.  Imports nothing from the package."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
TAG_PERM, TAG_NOISE = 0x5045524D, 0x4E4F4953
MASK32 = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (or scalars) of counters; returns the four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                 # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return c0, c1, c2, c3


def key(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def uniforms(words):
    """u = ((w >> 8) + 0.5) 2^-24 in fp64 (exact)."""
    return ((words >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals(seed, c1, c2, c3, n):
    """out[i] = normal i & 3 of counter (i >> 2, c1, c2, c3), fp64 [n]."""
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    u = [uniforms(w) for w in philox(g, c1, c2, c3, *key(seed))]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1)
    return z.reshape(-1)[:n]


def feistel_bits(N):
    """b: the smallest even number >= max(2, bit length of N - 1)."""
    b = max(2, int(N - 1).bit_length())
    return b + (b & 1)


def perm(seed, epoch, N, positions):
    """perm_{seed,epoch,N} of every position (int64 array)."""
    half = feistel_bits(N) // 2
    mask = np.uint64((1 << half) - 1)
    k0, k1 = key(seed)
    x = np.asarray(positions, dtype=np.uint64).copy()
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        v = x[todo]
        L, R = v >> np.uint64(half), v & mask
        for rnd in range(4):
            L, R = R, L ^ (philox(R, rnd, epoch, TAG_PERM, k0, k1)[0] & mask)
        x[todo] = (L << np.uint64(half)) | R
        todo &= x >= np.uint64(N)
    return x.astype(np.int64)


def position(step, global_batch, N):
    """0-based optimiser step -> (epoch, first): E = N // B whole batches per epoch, the last N % B positions of an epoch are dropped."""
    E = N // global_batch
    if E < 1:
        raise ValueError("data set smaller than the global batch")
    return step // E, (step % E) * global_batch
