"""The host reference of the noise generator (tests/philox_ref.py) against
published known answers, and its counter / key layout.  No GPU: the device
tests (test_gpu_noise_stream.py) compare the kernels with this reference."""
import numpy as np

import philox_ref as P

# Random123 kat_vectors, philox4x32 with 10 rounds: counter x4, key x2 -> output x4
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _words(*a):
    return tuple(int(v) for v in a)


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        assert _words(*P.philox4x32_10(*ctr, *key)) == want
    # vectorised: the three at once, and inputs above 32 bits are masked
    c = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    k = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    out = P.philox4x32_10(*c, *k)
    assert [tuple(int(o[j]) for o in out) for j in range(3)] == [k[2] for k in KAT]
    hi = np.uint64(0xABCD00000000)
    masked = P.philox4x32_10(*(v | hi for v in c), *(v | hi for v in k))
    assert all(np.array_equal(a, b) for a, b in zip(masked, out))


def test_raw_words_layout():
    """counter = (group, chain, step lo, step hi), key = (seed lo, seed hi)."""
    g, seed, chain, step = 9, 0x9E3779B97F4A7C15, 7, (3 << 32) + 5
    want = P.philox4x32_10(g, chain, 5, 3, 0x7F4A7C15, 0x9E3779B9)
    assert _words(*P.raw_words(g, seed, chain, step)) == _words(*want)
    # the first known answer is group 0 of the all-zero key
    assert _words(*P.raw_words(0, 0, 0, 0)) == KAT[0][2]
    # and the second the all-ones one: every word of the layout is used in full
    assert _words(*P.raw_words(0xFFFFFFFF, 2 ** 64 - 1, 0xFFFFFFFF, 2 ** 64 - 1)) == KAT[1][2]
    # the third: distinct words in every position
    assert _words(*P.raw_words(0x243f6a88, (0x299f31d0 << 32) | 0xa4093822, 0x85a308d3,
                               (0x03707344 << 32) | 0x13198a2e)) == KAT[2][2]
    groups = np.arange(64, dtype=np.uint64)

    def w(seed, chain, step):
        return np.stack(P.raw_words(groups, seed, chain, step))

    # the step's high half and the seed's high half reach the generator
    assert not np.any(np.all(w(1, 2, 5) == w(1, 2, 2 ** 32 + 5), axis=0))
    assert not np.any(np.all(w(1, 2, 5) == w(1 + 2 ** 32, 2, 5), axis=0))
    # step and chain sit in different counter words
    assert not np.any(np.all(w(1, 2, 5) == w(1, 5, 2), axis=0))
    # only the low 32 bits of group and chain are counted (the library refuses
    # launches that would reach them: test_abi.py)
    assert np.array_equal(np.stack(P.raw_words(groups + np.uint64(2 ** 32), 1, 2, 5)), w(1, 2, 5))
    assert np.array_equal(w(1, 2 + 2 ** 32, 5), w(1, 2, 5))


def test_u01_is_the_single_rounding_of_the_bucket_centre():
    """(a + 0.5f) * 2^-24 in fp32 equals fl32 of the exact (a + 0.5) * 2^-24 —
    what one fused multiply-add returns — for every 24-bit a; the value lies
    in (0, 1] and the top bucket rounds to 1.0."""
    a = np.arange(1 << 24, dtype=np.uint64)
    u = P.u01(a << np.uint64(8))
    assert u.dtype == np.float32
    exact = (a.astype(np.float64) + 0.5) * 2.0 ** -24  # exact in float64
    assert np.array_equal(u, exact.astype(np.float32))
    assert u[0] == np.float32(2.0 ** -25) and u[-1] == np.float32(1.0) and u.min() > 0
    # the low 8 bits of a word are not used
    assert np.array_equal(P.u01((a[:4096] << np.uint64(8)) | np.uint64(0xFF)), u[:4096])


def test_normals_shape_prefix_and_offset():
    z = P.normals(4099, 42, 5, 123)
    assert z.dtype == np.float64 and z.shape == (4099,) and np.all(np.isfinite(z))
    assert np.array_equal(P.normals(1001, 42, 5, 123), z[:1001])      # element i independent of n
    assert np.array_equal(P.normals(99, 42, 5, 123, offset=1000), z[4000:])
    # Box-Muller by hand for group 3
    x, y, zz, w = (int(v) for v in P.raw_words(3, 42, 5, 123))
    import math
    # the bucket centre rounded to fp32, then everything in Python floats (float64)
    ua, ta, ub, tb = (float(np.float32(((v >> 8) + 0.5) / 2 ** 24)) for v in (x, y, zz, w))
    ra, rb = math.sqrt(-2 * math.log(ua)), math.sqrt(-2 * math.log(ub))
    want = [ra * math.cos(2 * math.pi * ta), ra * math.sin(2 * math.pi * ta),
            rb * math.cos(2 * math.pi * tb), rb * math.sin(2 * math.pi * tb)]
    np.testing.assert_allclose(z[12:16], want, rtol=1e-14, atol=0)
    # a standard normal sample: loose moment bounds (5 sigma of the estimators)
    big = P.normals(1 << 18, 7, 0, 1)
    n = big.size
    assert abs(big.mean()) < 5 / np.sqrt(n) and abs(big.var() - 1) < 5 * np.sqrt(2 / n)


def test_tail_buckets_named_by_the_device_test_exist():
    """The draws test_gpu_noise_stream.py uses for the tails: u's lowest bucket
    (radius sqrt(50 ln 2), the largest the generator produces) and its top
    bucket (u = 1: radius exactly 0)."""
    for group, step, word in P.TAIL_BOTTOM:
        assert int(P.raw_words(group, 0, 0, step)[word]) >> 8 == 0
        z = P.normals(4 * (group + 1), 0, 0, step)[4 * group + word:4 * group + word + 2]
        np.testing.assert_allclose(np.hypot(*z), np.sqrt(50 * np.log(2)), rtol=1e-15)
    for group, step, word in P.TAIL_TOP:
        assert int(P.raw_words(group, 0, 0, step)[word]) >> 8 == 2 ** 24 - 1
        z = P.normals(4 * (group + 1), 0, 0, step)[4 * group + word:4 * group + word + 2]
        assert np.all(z == 0.0)
