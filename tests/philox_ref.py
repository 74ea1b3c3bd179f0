"""Host reference of the library's noise generator (numpy only, no GPU).

Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) keyed and
counted as bdl_kernels.hpp philox_normal4 does, then Box-Muller in float64:

    counter = (group lo32, chain lo32, step lo32, step hi32)   group = element // 4
    key     = (seed lo32, seed hi32)
    u(x)    = fl32((x >> 8) + 0.5) * 2^-24       in (0, 1]; the top bucket rounds to 1.0
    r_a = sqrt(-2 ln u(x)), r_b = sqrt(-2 ln u(z))
    elements 4*group .. 4*group+3 = r_a cos(2 pi u(y)), r_a sin(2 pi u(y)),
                                    r_b cos(2 pi u(w)), r_b sin(2 pi u(w))

Written from the published algorithm, not from the device code: the device
tests compare the kernels' stream against this one.
"""
import numpy as np

# Draws of seed 0, chain 0 whose radius uniform falls in an end bucket, as
# (group, step, word: 0 = x -> elements 4g, 4g+1; 2 = z -> elements 4g+2, 4g+3),
# found by a search over groups < 1024 and steps < 2^15:
TAIL_BOTTOM = [(437, 21968, 0), (261, 27675, 0)]  # word >> 8 == 0: u = 2^-25, the largest radius
TAIL_TOP = [(346, 28112, 0), (743, 252, 2)]       # word >> 8 == 2^24 - 1: u = 1, radius 0

M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_S32 = np.uint64(32)


def _u64(x):
    """Python ints (up to 2^64 - 1) or arrays as uint64 arrays."""
    if isinstance(x, (int, np.integer)):
        return np.array(int(x) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    return np.asarray(x).astype(np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten Philox4x32 rounds over uint64 arrays holding 32-bit words
    (broadcast against each other); returns the four output words."""
    c0, c1, c2, c3, k0, k1 = (_u64(v) & M32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = _MUL0 * c0  # 32 x 32 -> 64 bits: never overflows uint64
        p1 = _MUL1 * c2
        hi0, lo0 = p0 >> _S32, p0 & M32
        hi1, lo1 = p1 >> _S32, p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + _W0) & M32
        k1 = (k1 + _W1) & M32
    return c0, c1, c2, c3


def raw_words(groups, seed, chain, step):
    """The four 32-bit words of each float4 group (uint64 arrays), in this
    project's counter / key layout."""
    g, seed, chain, step = _u64(groups), _u64(seed), _u64(chain), _u64(step)
    return philox4x32_10(g & M32, chain & M32, step & M32, step >> _S32,
                         seed & M32, seed >> _S32)


def u01(x):
    """fl32((x >> 8) + 0.5) * 2^-24 as float32.  The sum rounds once in fp32
    (25 significant bits for x >> 8 >= 2^23: ties to even, so the top bucket
    gives 2^24); the power-of-two scale is exact — the same value as the
    single fused multiply-add fma(x >> 8, 2^-24, 2^-25) the device issues."""
    a = (_u64(x) >> np.uint64(8)).astype(np.float32)  # < 2^24: exact
    return (a + np.float32(0.5)) * np.float32(2.0 ** -24)


def normals(n, seed, chain, step, offset=0):
    """The n N(0,1) values of elements [4*offset, 4*offset + n) of the
    (seed, chain, step) stream, in float64."""
    ng = (int(n) + 3) // 4
    x, y, z, w = raw_words(np.arange(ng, dtype=np.uint64) + np.uint64(offset), seed, chain, step)
    ux, uy, uz, uw = (u01(v).astype(np.float64) for v in (x, y, z, w))
    ra, rb = np.sqrt(-2.0 * np.log(ux)), np.sqrt(-2.0 * np.log(uz))
    ta, tb = 2.0 * np.pi * uy, 2.0 * np.pi * uw
    out = np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=1)
    return out.reshape(-1)[:int(n)]
