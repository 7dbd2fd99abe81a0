"""t2s_bernoulli_mask_keyed / t2s_wg_noise_keyed (csrc/sampling.hip) called directly on guarded buffers, against the numpy
restatement of tests/keyed_ref.py (tests/test_keyed_ref_cpu.py pins that reference's own properties).

Masks are compared for EQUALITY with the reference and with the existing t2s_bernoulli_mask under each entry's seed.  Noise values
are held to |got - ref| <= 2^-24 |ref| + 2^-40 against the float64 draws times sigma - the single f32 rounding plus room for the
double-precision log and sincospi (a few ulp: about 1e-15 at |n| <= 8.6) - with no element exempt; invariance under B, the entry's
place and L, and the sigma product, are compared bit for bit.

Every destination is a view into a larger tensor filled with 0xAB bytes, which must come back untouched around it."""
import ctypes

import numpy as np
import pytest
import torch

import keyed_ref as K
from text2speech_amd import _lib
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

GUARD = 64                  # elements either side
FILL_BYTE = 0xAB
FILL_F32 = float(np.frombuffer(bytes([FILL_BYTE] * 4), dtype=np.float32)[0])         # -1.2e-12: what four 0xAB bytes read as


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def tile(lib):
    t = lib.t2s_noise_tile()
    assert t > 0 and t % 2 == 0
    return t


class Guarded:
    """n elements of `dtype` inside a larger tensor of 0xAB bytes: GUARD + shift elements in front, GUARD behind."""

    def __init__(self, n, dtype, shift=0):
        item = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full(((n + 2 * GUARD + shift) * item,), FILL_BYTE, dtype=torch.uint8, device=DEV)
        self.lo, self.n, self.item = (GUARD + shift) * item, n * item, item
        self.t = self.raw[self.lo:self.lo + self.n].view(dtype)

    def guards_intact(self):
        return bool((self.raw[:self.lo] == FILL_BYTE).all()) and bool((self.raw[self.lo + self.n:] == FILL_BYTE).all())

    def untouched(self):
        return bool((self.raw == FILL_BYTE).all())


def _seeds_dev(seeds):
    return torch.tensor([int(s) for s in seeds], dtype=torch.int64, device=DEV)


def _seeds_for(B, salt=0):
    s = [(0x9E3779B1 * (b + 1 + salt) ** 3 + 977 * b) % 2 ** 63 for b in range(B)]
    s[-1] = 2 ** 63 - 1 - salt
    return s


# ---------------------------------------------------------------------------------------------------------------- masks
def _keyed_mask(lib, n_steps, B, row, seeds, p):
    buf = Guarded(n_steps * B * row, torch.uint8)
    sd = _seeds_dev(seeds)
    assert lib.t2s_bernoulli_mask_keyed(buf.t.data_ptr(), n_steps, B, row, sd.data_ptr(), p, _st()) == 0
    torch.cuda.synchronize()
    assert buf.guards_intact(), "bernoulli_mask_keyed[%d, %d, %d]: wrote outside the mask" % (n_steps, B, row)
    return buf.t.cpu().numpy().reshape(n_steps, B, row)


def _flat_mask(n, seed, p):
    buf = Guarded(n, torch.uint8)
    _lib.call("t2s_bernoulli_mask", ctypes.c_void_p(buf.t.data_ptr()), n, int(seed), 0, p, _st())
    torch.cuda.synchronize()
    return buf.t.cpu().numpy()


@pytest.mark.parametrize("n_steps,B,row", [(1, 1, 1), (3, 1, 512), (5, 3, 512), (2, 8, 7), (61, 9, 512)])
def test_keyed_mask_bits(lib, n_steps, B, row):
    seeds = _seeds_for(B)
    for p in (0.5, 0.9):
        got = _keyed_mask(lib, n_steps, B, row, seeds, p)
        assert set(np.unique(got)) <= {0, 1}
        assert np.array_equal(got, K.keyed_mask(n_steps, B, row, seeds, p)), "keyed mask differs from the reference at p = %.1f" % p
        for b in range(B):
            assert np.array_equal(got[:, b].reshape(-1), _flat_mask(n_steps * row, seeds[b], p)), \
                "entry %d is not t2s_bernoulli_mask under its seed (p = %.1f)" % (b, p)
    assert (_keyed_mask(lib, n_steps, B, row, seeds, 1.0) == 1).all(), "keep_prob = 1 is not all ones"


# ---------------------------------------------------------------------------------------------------------------- noise
def _noise(lib, B, G, L, seeds, sigma=1.0, sigmas=None, shift=0):
    buf = Guarded(B * G * L, torch.float32, shift)
    sd = _seeds_dev(seeds)
    sg = None if sigmas is None else torch.tensor(sigmas, dtype=torch.float32, device=DEV)
    rc = lib.t2s_wg_noise_keyed(buf.t.data_ptr(), B, G, L, sd.data_ptr(), sigma, None if sg is None else sg.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert buf.guards_intact(), "wg_noise_keyed[%d, %d, %d]: wrote outside z" % (B, G, L)
    return buf.t.cpu().numpy().reshape(B, G, L)


def _lengths(tile):
    return [1, 2, 3, 96, 97, tile - 1, tile, tile + 1, 2 * tile + 1]


@pytest.fixture(scope="module")
def ref_draws(tile):
    """(seed, G) -> float64 [G, 2 tile + 1] unit draws: computed once, shorter calls read a prefix (the CPU test pins that property
    of the reference)"""
    cache = {}

    def get(seed, G):
        if (seed, G) not in cache:
            cache[(seed, G)] = K.unit_noise(seed, G, 2 * tile + 1)
            cache[(seed, G)].setflags(write=False)
        return cache[(seed, G)]
    return get


@pytest.mark.parametrize("G", [8, 2])
@pytest.mark.parametrize("B", [1, 3])
def test_keyed_noise_values(lib, tile, ref_draws, B, G):
    seeds = _seeds_for(B, salt=G)
    worst = 0.0
    for i, L in enumerate(_lengths(tile)):
        got = _noise(lib, B, G, L, seeds, shift=i % 2)          # (an odd shift: rows off the 8-byte boundary, the scalar stores)
        assert got.dtype == np.float32 and np.isfinite(got).all()
        ref = np.stack([ref_draws(s, G)[:, :L] for s in seeds])
        err, bound = np.abs(got.astype(np.float64) - ref), K.noise_bound(ref)
        worst = max(worst, float((err / bound).max()))
        print("PARITY wg_noise_keyed[B=%d G=%d L=%d]: max |got - ref| / bound = %.4f" % (B, G, L, float((err / bound).max())))
        assert (err <= bound).all(), "L = %d: %d elements outside the bound, worst %.3f of it" % (L, int((err > bound).sum()), worst)
    assert worst > 0.5          # the bound is one rounding wide: a result that never comes near it was not rounded from these draws


def test_keyed_noise_invariance(lib, tile):
    """entry b of a B = 3 call is the B = 1 call with its seed; the first 97 columns of a longer call are the L = 97 call"""
    G = 8
    seeds = _seeds_for(3, salt=5)
    for L in (97, tile + 1):
        batch = _noise(lib, 3, G, L, seeds)
        for b, s in enumerate(seeds):
            assert np.array_equal(batch[b], _noise(lib, 1, G, L, [s])[0]), (L, b)
    short = _noise(lib, 3, G, 97, seeds)
    for L in (tile + 1, 2 * tile + 1):
        assert np.array_equal(_noise(lib, 3, G, L, seeds)[:, :, :97], short), L
    assert np.array_equal(_noise(lib, 1, 2, 97, seeds[:1]), short[:1, :2])          # fewer channels: the same rows
    assert not np.array_equal(short[0], short[1])


def test_keyed_noise_sigma(lib, tile):
    G, L = 8, tile + 1
    seeds = _seeds_for(3, salt=9)
    one = _noise(lib, 3, G, L, seeds)
    assert np.array_equal(_noise(lib, 3, G, L, seeds, sigma=0.666), np.float32(0.666) * one)
    sig = [0.5, 0.0, 1.25]
    got = _noise(lib, 3, G, L, seeds, sigma=9.0, sigmas=sig)           # sigmas overrides sigma per entry
    for b, s in enumerate(sig):
        assert np.array_equal(got[b], np.float32(s) * one[b]), b
    assert (_noise(lib, 3, G, L, seeds, sigma=0.0) == 0).all()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_buffers_alone(lib):
    st = _st()
    mask = Guarded(4 * 3 * 8, torch.uint8)
    z = Guarded(3 * 2 * 8, torch.float32)
    seeds = _seeds_dev([1, 2, 3])
    sig = torch.ones(3, dtype=torch.float32, device=DEV)
    mp, zp, sp, gp = mask.t.data_ptr(), z.t.data_ptr(), seeds.data_ptr(), sig.data_ptr()
    big = 2 ** 40
    cases = [
        ("mask NULL", lambda: lib.t2s_bernoulli_mask_keyed(None, 4, 3, 8, sp, 0.5, st)),
        ("mask seeds NULL", lambda: lib.t2s_bernoulli_mask_keyed(mp, 4, 3, 8, None, 0.5, st)),
        ("mask n_steps = 0", lambda: lib.t2s_bernoulli_mask_keyed(mp, 0, 3, 8, sp, 0.5, st)),
        ("mask n_steps < 0", lambda: lib.t2s_bernoulli_mask_keyed(mp, -1, 3, 8, sp, 0.5, st)),
        ("mask B = 0", lambda: lib.t2s_bernoulli_mask_keyed(mp, 4, 0, 8, sp, 0.5, st)),
        ("mask B = 65536", lambda: lib.t2s_bernoulli_mask_keyed(mp, 4, 65536, 8, sp, 0.5, st)),
        ("mask row = 0", lambda: lib.t2s_bernoulli_mask_keyed(mp, 4, 3, 0, sp, 0.5, st)),
        ("mask keep_prob = 0", lambda: lib.t2s_bernoulli_mask_keyed(mp, 4, 3, 8, sp, 0.0, st)),
        ("mask keep_prob = 1.5", lambda: lib.t2s_bernoulli_mask_keyed(mp, 4, 3, 8, sp, 1.5, st)),
        ("mask keep_prob = nan", lambda: lib.t2s_bernoulli_mask_keyed(mp, 4, 3, 8, sp, float("nan"), st)),
        ("noise z NULL", lambda: lib.t2s_wg_noise_keyed(None, 3, 2, 8, sp, 1.0, None, st)),
        ("noise seeds NULL", lambda: lib.t2s_wg_noise_keyed(zp, 3, 2, 8, None, 1.0, None, st)),
        ("noise B = 0", lambda: lib.t2s_wg_noise_keyed(zp, 0, 2, 8, sp, 1.0, None, st)),
        ("noise B = 65536", lambda: lib.t2s_wg_noise_keyed(zp, 65536, 2, 8, sp, 1.0, None, st)),
        ("noise G = 0", lambda: lib.t2s_wg_noise_keyed(zp, 3, 0, 8, sp, 1.0, None, st)),
        ("noise G = 65536", lambda: lib.t2s_wg_noise_keyed(zp, 3, 65536, 8, sp, 1.0, None, st)),
        ("noise L = 0", lambda: lib.t2s_wg_noise_keyed(zp, 3, 2, 0, sp, 1.0, None, st)),
        ("noise L < 0", lambda: lib.t2s_wg_noise_keyed(zp, 3, 2, -8, sp, 1.0, None, st)),
        ("noise L = 2^40", lambda: lib.t2s_wg_noise_keyed(zp, 3, 2, big, sp, 1.0, None, st)),
        ("noise sigma < 0", lambda: lib.t2s_wg_noise_keyed(zp, 3, 2, 8, sp, -0.5, None, st)),
        ("noise sigma = inf", lambda: lib.t2s_wg_noise_keyed(zp, 3, 2, 8, sp, float("inf"), None, st)),
        ("noise sigma = nan", lambda: lib.t2s_wg_noise_keyed(zp, 3, 2, 8, sp, float("nan"), None, st)),
        ("noise sigma = nan under sigmas", lambda: lib.t2s_wg_noise_keyed(zp, 3, 2, 8, sp, float("nan"), gp, st)),
    ]
    for name, call in cases:
        assert call() == -1, "%s was accepted" % name
    torch.cuda.synchronize()
    assert mask.untouched() and z.untouched(), "a refused call wrote"
    assert abs(FILL_F32) < 1e-11 and bool((z.t == FILL_F32).all())
