"""The numpy reference of the keyed sampling kernels (tests/keyed_ref.py) against the formulas' own claims, without a GPU: the keyed
mask is the flat hash of each entry's seed, the Gaussian is a unit Gaussian without visible structure along any axis of its counter,
a value depends on (seed, channel, column) alone, and the GPU value bound leaves room for one f32 rounding and nothing else."""
import numpy as np
import pytest

import keyed_ref as K

SEEDS = (0, 1, 2, 1234, 2 ** 62 - 1)
G, L = 8, 2 ** 18
N_SD = 5.0          # the bar tests/test_tacotron_fwd_kernels_gpu.py::test_bernoulli_mask_mean holds the mask hash to


@pytest.mark.parametrize("n_steps,B,row", [(1, 1, 1), (3, 1, 512), (5, 3, 512), (2, 8, 7), (61, 9, 512)])
def test_keyed_mask_is_the_flat_hash_per_entry(n_steps, B, row):
    seeds = [(0x1234567 * (b + 1) ** 3 + b) % 2 ** 63 for b in range(B)]
    seeds[-1] = 2 ** 63 - 1
    for p in (0.5, 0.9):
        got = K.keyed_mask(n_steps, B, row, seeds, p)
        assert got.shape == (n_steps, B, row) and got.dtype == np.uint8
        for b in range(B):
            assert np.array_equal(got[:, b].reshape(-1), K.flat_mask(n_steps * row, seeds[b], p)), (b, p)
    assert (K.keyed_mask(n_steps, B, row, seeds, 1.0) == 1).all()


@pytest.fixture(scope="module")
def draws():
    """seed -> float64 [G, L] for SEEDS and their successors: computed once, read only"""
    out = {}
    for s in SEEDS:
        for v in (s, s + 1):
            if v not in out:
                out[v] = K.unit_noise(v, G, L)
                out[v].setflags(write=False)
    return out


def test_unit_gaussian_statistics(draws):
    """Mean, variance and kurtosis; autocorrelation along the columns at lags 1 - 3 (lag 1 also split into the two members of one
    Box-Muller pair and the neighbours across two pairs, and the pair's squares, which share a radius); adjacent channels; seeds s
    and s + 1.  Each statistic within 5 standard deviations of its sampling distribution under independent unit Gaussians."""
    worst = 0.0
    for s in SEEDS:
        x = draws[s]
        N = x.size
        stats = [("mean", x.mean(), 1 / np.sqrt(N)),
                 ("variance", (x * x).mean() - 1.0, np.sqrt(2.0 / N)),
                 ("kurtosis", (x ** 4).mean() / (x * x).mean() ** 2 - 3.0, np.sqrt(24.0 / N))]
        for lag in (1, 2, 3):
            prod = x[:, :-lag] * x[:, lag:]
            stats.append(("autocorrelation lag %d" % lag, prod.mean(), 1 / np.sqrt(prod.size)))
        a, b = x[:, 0::2], x[:, 1::2]
        stats.append(("inside a pair", (a * b).mean(), 1 / np.sqrt(a.size)))
        stats.append(("across two pairs", (b[:, :-1] * a[:, 1:]).mean(), 1 / np.sqrt(a.size - G)))
        stats.append(("squares inside a pair", ((a * a - 1) * (b * b - 1)).mean(), 2 / np.sqrt(a.size)))     # var(x^2 - 1) = 2 each
        stats.append(("adjacent channels", (x[:-1] * x[1:]).mean(), 1 / np.sqrt(x[1:].size)))
        stats.append(("seed and seed + 1", (x * draws[s + 1]).mean(), 1 / np.sqrt(N)))
        for name, value, sd in stats:
            worst = max(worst, abs(value) / sd)
            print("PARITY keyed noise seed %d %s: %+.3e = %.2f sd" % (s, name, value, abs(value) / sd))
            assert abs(value) <= N_SD * sd, (s, name, value, sd)
        assert np.isfinite(x).all() and np.abs(x).max() <= np.sqrt(106 * np.log(2.0))
    print("PARITY keyed noise: worst statistic %.2f sd" % worst)


def test_value_depends_on_seed_channel_column_only(draws):
    for s in (0, 1234):
        full = draws[s]
        for L2 in (1, 2, 3, 96, 97, 1025):
            assert np.array_equal(K.unit_noise(s, G, L2), full[:, :L2]), (s, L2)
        assert np.array_equal(K.unit_noise(s, 2, 97), full[:2, :97])                    # fewer channels
        assert np.array_equal(K.unit_noise(s, G, 50, t0=46), full[:, 46:96])            # a window further on
    z3, n3 = K.keyed_noise([7, 1234, 0], G, 97)
    for b, s in enumerate((7, 1234, 0)):                                                # any B, any place in the batch
        z1, n1 = K.keyed_noise([s], G, 97)
        assert np.array_equal(z3[b], z1[0]) and np.array_equal(n3[b], n1[0])
    assert np.array_equal(n3[1], draws[1234][:, :97])
    assert not np.array_equal(n3[0], n3[1])


def test_sigma_is_one_f32_product():
    z1, n = K.keyed_noise([5, 6], 2, 97)
    assert z1.dtype == np.float32 and np.array_equal(z1, n.astype(np.float32))
    z, _ = K.keyed_noise([5, 6], 2, 97, sigma=0.666)
    assert np.array_equal(z, np.float32(0.666) * z1)
    z, _ = K.keyed_noise([5, 6], 2, 97, sigma=9.0, sigmas=[0.5, 0.0])
    assert np.array_equal(z[0], np.float32(0.5) * z1[0]) and (z[1] == 0).all()


def test_bound_leaves_room_for_one_rounding_only(draws):
    """float32(ref) itself lies within the GPU test's bound of ref, and uses nearly all of it: the bound admits the single f32
    rounding of a correctly computed draw and no second one."""
    worst = 0.0
    for s in SEEDS:
        ref = draws[s]
        err = np.abs(ref.astype(np.float32).astype(np.float64) - ref)
        bound = K.noise_bound(ref)
        assert (err <= bound).all()
        worst = max(worst, float((err / bound).max()))
    print("PARITY keyed noise: |f32(ref) - ref| reaches %.4f of the bound" % worst)
    assert 0.9 < worst <= 1.0
