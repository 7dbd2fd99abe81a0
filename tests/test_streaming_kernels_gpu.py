"""t2s_wg_noise_keyed_at (csrc/sampling.hip) and t2s_wg_audio_window (csrc/waveglow_ops.hip) called directly on guarded buffers.
The first against slices of ONE t2s_wg_noise_keyed buffer, bit for bit - every parity of the offset and of the length, the
1024-column tile's edges, per-entry offsets and temperatures - and near 2^39, where no whole buffer exists, against the numpy
restatement (tests/keyed_ref.py) and against itself one column on.  The second against t2s_wg_audio_squeeze plus a slice, bit for
bit.  A refused call leaves its buffer untouched."""
import numpy as np
import pytest
import torch

import keyed_ref as K
from text2speech_amd import _lib
from wg_bwd_util import DEV

pytestmark = pytest.mark.gpu

EINVAL = -1
G = 8
GUARD = 64                  # elements either side
FILL_BYTE = 0xAB
FILL_F32 = float(np.frombuffer(bytes([FILL_BYTE] * 4), dtype=np.float32)[0])         # -1.2e-12: what four 0xAB bytes read as


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


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def tile(lib):
    return lib.t2s_noise_tile()


@pytest.fixture(scope="module")
def whole(lib, tile):
    """one t2s_wg_noise_keyed buffer [3, G, 4 tile + 7] under three seeds and three temperatures, and the same under one sigma"""
    B, L = 3, 4 * tile + 7
    seeds, sigmas = _seeds_for(B), [0.666, 1.0, 0.25]
    sd = _seeds_dev(seeds)
    sg = torch.tensor(sigmas, dtype=torch.float32, device=DEV)
    z = torch.empty(B, G, L, dtype=torch.float32, device=DEV)
    zs = torch.empty(B, G, L, dtype=torch.float32, device=DEV)
    assert lib.t2s_wg_noise_keyed(z.data_ptr(), B, G, L, sd.data_ptr(), 1.0, sg.data_ptr(), _st()) == 0
    assert lib.t2s_wg_noise_keyed(zs.data_ptr(), B, G, L, sd.data_ptr(), 0.666, None, _st()) == 0
    torch.cuda.synchronize()
    return dict(B=B, L=L, seeds=seeds, sd=sd, sigmas=sigmas, sg=sg, z=z.cpu().numpy(), zs=zs.cpu().numpy())


def _at(lib, B, L, col0, sd, sigma=1.0, sg=None, col0s=None, shift=0):
    buf = Guarded(B * G * L, torch.float32, shift)
    c0 = None if col0s is None else torch.tensor(col0s, dtype=torch.int64, device=DEV)
    rc = lib.t2s_wg_noise_keyed_at(buf.t.data_ptr(), B, G, L, col0, None if c0 is None else c0.data_ptr(), sd.data_ptr(), sigma,
                                   None if sg is None else sg.data_ptr(), _st())
    assert rc == 0
    torch.cuda.synchronize()
    assert buf.guards_intact(), "wg_noise_keyed_at[B %d, L %d, col0 %r]: wrote outside z" % (B, L, col0 if col0s is None else col0s)
    got = buf.t.cpu().numpy().reshape(B, G, L)
    assert not (got.view(np.uint32) == np.float32(FILL_F32).view(np.uint32)).any(), "an element was left unwritten"
    return got


def test_noise_at_is_a_slice_of_the_whole_buffer(lib, tile, whole):
    """offsets 0, 1, tile - 1, tile, tile + 1 x lengths 1, 2, 3, 96, 97, tile, tile + 1 (both parities of both), each on a buffer
    that starts on an 8-byte boundary and on one that does not (shift = 1 element)"""
    n = 0
    for col0 in (0, 1, tile - 1, tile, tile + 1):
        for L in (1, 2, 3, 96, 97, tile, tile + 1):
            for shift in (0, 1):
                got = _at(lib, whole["B"], L, col0, whole["sd"], 0.666, None, shift=shift)
                assert np.array_equal(got.view(np.uint32), whole["zs"][:, :, col0:col0 + L].view(np.uint32)), (col0, L, shift)
                n += 1
    print("noise_keyed_at: %d (offset, length, alignment) cases bit-equal to slices of one t2s_wg_noise_keyed buffer" % n)


def test_noise_at_per_entry_offsets_and_sigmas(lib, tile, whole):
    """B = 3, col0s = (1, tile, 2 tile + 3) with the scalar col0 ignored, one temperature per entry"""
    for L in (tile + 1, 97):
        col0s = [1, tile, 2 * tile + 3]
        got = _at(lib, 3, L, 5, whole["sd"], 1.0, whole["sg"], col0s=col0s)
        for b, c0 in enumerate(col0s):
            assert np.array_equal(got[b].view(np.uint32), whole["z"][b, :, c0:c0 + L].view(np.uint32)), (L, b)


def test_noise_at_near_2_to_39(lib):
    """no whole buffer reaches there: the values against the numpy reference (the value bound of tests/test_keyed_kernels_gpu.py),
    and the run one column on - the other parity - bit-equal where the two overlap"""
    seeds = _seeds_for(1)
    sd = _seeds_dev(seeds)
    col0, L = 2 ** 39 - 64, 131
    a = _at(lib, 1, L, col0, sd, 1.0)
    b = _at(lib, 1, L, col0 + 1, sd, 1.0)
    assert np.array_equal(a[:, :, 1:].view(np.uint32), b[:, :, :-1].view(np.uint32))
    ref = K.unit_noise(seeds[0], G, L, t0=col0)
    err = np.abs(a[0].astype(np.float64) - ref)
    print("noise_keyed_at at 2^39 - 64: max |got - ref| / bound = %.4f" % float((err / K.noise_bound(ref)).max()))
    assert (err <= K.noise_bound(ref)).all()
    # the last offset the entry point takes: col0 + L = 2^40 - 1
    c = _at(lib, 1, 4, 2 ** 40 - 5, sd, 1.0)
    assert np.isfinite(c).all()


def test_noise_at_refusals(lib):
    buf = Guarded(3 * 2 * 8, torch.float32)
    sd = _seeds_dev(_seeds_for(3))
    zp, sp, st = buf.t.data_ptr(), sd.data_ptr(), _st()
    big = 2 ** 40
    calls = [
        ("z NULL", lambda: lib.t2s_wg_noise_keyed_at(None, 3, 2, 8, 0, None, sp, 1.0, None, st)),
        ("seeds NULL", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 2, 8, 0, None, None, 1.0, None, st)),
        ("B = 0", lambda: lib.t2s_wg_noise_keyed_at(zp, 0, 2, 8, 0, None, sp, 1.0, None, st)),
        ("B = 65536", lambda: lib.t2s_wg_noise_keyed_at(zp, 65536, 2, 8, 0, None, sp, 1.0, None, st)),
        ("G = 0", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 0, 8, 0, None, sp, 1.0, None, st)),
        ("G = 65536", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 65536, 8, 0, None, sp, 1.0, None, st)),
        ("L = 0", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 2, 0, 0, None, sp, 1.0, None, st)),
        ("L < 0", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 2, -8, 0, None, sp, 1.0, None, st)),
        ("L = 2^40", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 2, big, 0, None, sp, 1.0, None, st)),
        ("sigma < 0", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 2, 8, 0, None, sp, -0.5, None, st)),
        ("sigma = inf", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 2, 8, 0, None, sp, float("inf"), None, st)),
        ("sigma = nan", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 2, 8, 0, None, sp, float("nan"), None, st)),
        ("col0 < 0", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 2, 8, -1, None, sp, 1.0, None, st)),
        ("col0 + L = 2^40", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 2, 8, big - 8, None, sp, 1.0, None, st)),
        ("col0 = 2^40", lambda: lib.t2s_wg_noise_keyed_at(zp, 3, 2, 8, big, None, sp, 1.0, None, st)),
    ]
    for label, call in calls:
        assert call() == EINVAL, "accepted: " + label
    torch.cuda.synchronize()
    assert buf.untouched(), "a refused call wrote"


# ---------------------------------------------------------------------------------------------------------------- audio window
def _squeezed(lib, z, B, L):
    audio = torch.empty(B, L * G, dtype=torch.float32, device=DEV)
    assert lib.t2s_wg_audio_squeeze(audio.data_ptr(), z.data_ptr(), B, L * G, G, L, 1, _st()) == 0
    torch.cuda.synchronize()
    return audio.cpu().numpy()


@pytest.mark.parametrize("B,L", [(1, 37), (3, 300)])
def test_audio_window_is_squeeze_plus_slice(lib, B, L):
    """G = 8; k0 / k1 at 0, 1 and L; dst_off and ld_dst off any 16-byte boundary (odd numbers of floats, and a buffer that starts
    4 bytes past one); guard words around dst and between its rows' windows"""
    gen = torch.Generator().manual_seed(7 + L)
    z = torch.randn(B, G, L, generator=gen).to(DEV)
    want = _squeezed(lib, z, B, L)
    n = 0
    for k0, k1 in ((0, 1), (0, L), (1, L), (L - 1, L), (1, 2), (5, 30)):
        for dst_off, pad, shift in ((0, 0, 0), (3, 5, 1), (1, 2, 0)):
            keep = (k1 - k0) * G
            ld = dst_off + keep + pad
            buf = Guarded(B * ld, torch.float32, shift)
            assert lib.t2s_wg_audio_window(z.data_ptr(), B, G, L, k0, k1, buf.t.data_ptr(), ld, dst_off, _st()) == 0
            torch.cuda.synchronize()
            assert buf.guards_intact(), (k0, k1, dst_off, pad)
            got = buf.t.cpu().numpy().reshape(B, ld)
            assert np.array_equal(got[:, dst_off:dst_off + keep].view(np.uint32), want[:, k0 * G:k1 * G].view(np.uint32)), (k0, k1)
            fill = np.float32(FILL_F32).view(np.uint32)
            assert (got[:, :dst_off].view(np.uint32) == fill).all() and (got[:, dst_off + keep:].view(np.uint32) == fill).all(), \
                "wrote a row outside its window"
            n += 1
    print("audio_window[B %d, L %d]: %d (k0, k1, dst_off, ld_dst) cases bit-equal to audio_squeeze + slice" % (B, L, n))


def test_audio_window_refusals(lib):
    L = 16
    z = torch.zeros(2, G, L, dtype=torch.float32, device=DEV)
    buf = Guarded(2 * L * G, torch.float32)
    zp, dp, st = z.data_ptr(), buf.t.data_ptr(), _st()
    ld = L * G
    calls = [
        ("z NULL", lambda: lib.t2s_wg_audio_window(None, 2, G, L, 0, L, dp, ld, 0, st)),
        ("dst NULL", lambda: lib.t2s_wg_audio_window(zp, 2, G, L, 0, L, None, ld, 0, st)),
        ("B = 0", lambda: lib.t2s_wg_audio_window(zp, 0, G, L, 0, L, dp, ld, 0, st)),
        ("B = 65536", lambda: lib.t2s_wg_audio_window(zp, 65536, G, L, 0, L, dp, ld, 0, st)),
        ("G = 0", lambda: lib.t2s_wg_audio_window(zp, 2, 0, L, 0, L, dp, ld, 0, st)),
        ("L = 0", lambda: lib.t2s_wg_audio_window(zp, 2, G, 0, 0, 0, dp, ld, 0, st)),
        ("k0 < 0", lambda: lib.t2s_wg_audio_window(zp, 2, G, L, -1, L, dp, ld, 0, st)),
        ("k0 = k1", lambda: lib.t2s_wg_audio_window(zp, 2, G, L, 4, 4, dp, ld, 0, st)),
        ("k0 > k1", lambda: lib.t2s_wg_audio_window(zp, 2, G, L, 5, 4, dp, ld, 0, st)),
        ("k1 > L", lambda: lib.t2s_wg_audio_window(zp, 2, G, L, 0, L + 1, dp, ld, 0, st)),
        ("dst_off < 0", lambda: lib.t2s_wg_audio_window(zp, 2, G, L, 0, L, dp, ld, -1, st)),
        ("ld_dst = 0", lambda: lib.t2s_wg_audio_window(zp, 2, G, L, 0, L, dp, 0, 0, st)),
        ("the window does not fit the row", lambda: lib.t2s_wg_audio_window(zp, 2, G, L, 0, L, dp, ld, 1, st)),
        ("ld_dst one short", lambda: lib.t2s_wg_audio_window(zp, 2, G, L, 0, L, dp, ld - 1, 0, st)),
    ]
    for label, call in calls:
        assert call() == EINVAL, "accepted: " + label
    torch.cuda.synchronize()
    assert buf.untouched(), "a refused call wrote"
