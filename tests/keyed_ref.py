"""Numpy restatement of the keyed sampling formulas (include/t2s_hip.h, "keyed sampling"; csrc/sampling.hip): uint64 hashes with
wrapping arithmetic, the Gaussian in float64.  The references of tests/test_keyed_ref_cpu.py and tests/test_keyed_kernels_gpu.py."""
import numpy as np

GOLD = np.uint64(0x9E3779B97F4A7C15)
NOISE_DOMAIN = np.uint64(0x5741564547)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
TWO_M53 = 2.0 ** -53


def mix(x):
    """splitmix64's finaliser on a uint64 array (a new array)."""
    x = np.array(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= M1
        x ^= x >> np.uint64(27)
        x *= M2
        x ^= x >> np.uint64(31)
    return x


def flat_mask(n, seed, keep_prob, offset=0):
    """What t2s_bernoulli_mask(buf, n, seed, offset, keep_prob) stores: uint8 [n]."""
    thr = np.uint32(np.float32(keep_prob) * np.float32(16777216.0))
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(offset)) * GOLD + np.uint64(seed)
    return ((mix(x) >> np.uint64(40)).astype(np.uint32) < thr).astype(np.uint8)


def keyed_mask(n_steps, B, row, seeds, keep_prob):
    """t2s_bernoulli_mask_keyed written out on its own: uint8 [n_steps, B, row], element (t, b, j) from the hash of t row + j under
    seeds[b]."""
    assert len(seeds) == B
    thr = np.uint32(np.float32(keep_prob) * np.float32(16777216.0))
    t = np.arange(n_steps, dtype=np.uint64)[:, None, None]
    j = np.arange(row, dtype=np.uint64)[None, None, :]
    s = np.array([int(v) for v in seeds], dtype=np.uint64)[None, :, None]
    with np.errstate(over="ignore"):
        x = (t * np.uint64(row) + j) * GOLD + s
    return ((mix(x) >> np.uint64(40)).astype(np.uint32) < thr).astype(np.uint8)


def _sincospi(x):
    """(sin(pi x), cos(pi x)) for float64 x in [0, 2): the argument is reduced exactly (x - k / 2 is exact) to |r| <= 1/4 before it
    meets pi, so the result carries the few-ulp error of numpy's sin / cos on a small argument and nothing from the product 2 pi u."""
    k = np.rint(2.0 * x)
    r = x - 0.5 * k
    s, c = np.sin(np.pi * r), np.cos(np.pi * r)
    q = k.astype(np.int64) & 3
    sn = np.choose(q, [s, c, -s, -c])
    cs = np.choose(q, [c, -s, -c, s])
    return sn, cs


def unit_noise(seed, G, L, t0=0):
    """The unit Gaussian draws n of one entry: float64 [G, L], columns t0 .. t0 + L - 1 (t0 even)."""
    assert t0 % 2 == 0
    with np.errstate(over="ignore"):
        key = mix(np.array([int(seed)], dtype=np.uint64) * GOLD + NOISE_DOMAIN)[0]
        nq = (L + 1) // 2
        c = np.arange(G, dtype=np.uint64)[:, None]
        q = np.arange(nq, dtype=np.uint64)[None, :] + np.uint64(t0 // 2)
        p = (c << np.uint64(40)) | q
        a = mix((np.uint64(2) * p) * GOLD + key)
        h = mix((np.uint64(2) * p + np.uint64(1)) * GOLD + key)
    u1 = ((a >> np.uint64(11)).astype(np.float64) + 1.0) * TWO_M53          # (0, 1]: (a >> 11) + 1 <= 2^53 is exact
    u2 = (h >> np.uint64(11)).astype(np.float64) * TWO_M53                  # [0, 1)
    r = np.sqrt(-2.0 * np.log(u1))
    sn, cs = _sincospi(2.0 * u2)
    out = np.empty((G, 2 * nq), dtype=np.float64)
    out[:, 0::2] = r * cs
    out[:, 1::2] = r * sn
    return out[:, :L]


def keyed_noise(seeds, G, L, sigma=1.0, sigmas=None):
    """t2s_wg_noise_keyed: (z float32 [B, G, L] as the kernel's arithmetic gives it from the float64 draws - one rounding to f32, one
    f32 product with sigma_b -, the float64 draws [B, G, L])."""
    n = np.stack([unit_noise(s, G, L) for s in seeds])
    sg = np.full(len(seeds), np.float32(sigma), dtype=np.float32) if sigmas is None else np.asarray(sigmas, dtype=np.float32)
    return sg[:, None, None] * n.astype(np.float32), n


def noise_bound(ref):
    """The GPU value check: |got - ref| <= 2^-24 |ref| + 2^-40 - one f32 rounding (half an ulp is at most 2^-24 |ref|) plus room for
    the double-precision log and sincospi, whose few ulp are about 1e-15 at |n| <= 8.6."""
    return 2.0 ** -24 * np.abs(ref) + 2.0 ** -40
