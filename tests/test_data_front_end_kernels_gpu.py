"""t2s_pcm16_gather and t2s_gate_targets (csrc/audio_ops.hip, csrc/t2s_api_audio.hip) called directly on guarded buffers, against the
restatements of tests/data_ref.py.

t2s_pcm16_gather: the result is BIT-EQUAL to numpy.float32(x) / numpy.float32(32768) placed into zeros.  The pool holds every int16 code
and is a view that starts 2, 6 or 14 bytes into a larger tensor (its base is not 16-byte aligned); rows start at every 2-byte phase
0 .. 7 of a 16-byte granule, at the pool's first and last sample, in front of the pool, behind it, and close enough to its end that
start + count runs past it; counts 0, 1, N - 1, N, N + 5.  The output is 16-byte aligned with NaN sentinels in front, behind and in
the columns N .. ldo; with ldo = N + 3 (or an odd N) rows 1 and 2 of a batch of 3 are not 16-byte aligned.

With max_wav_value = 32767 the result is compared with numpy's own float32 division in ulps: measured 0 ulp (the kernel's division
is the correctly rounded one), asserted <= 1 ulp as the entry point documents."""
import numpy as np
import pytest
import torch

import data_ref as D
from text2speech_amd import _lib
from wg_bwd_util import DEV, Guarded

pytestmark = pytest.mark.gpu

POOL_LEN = 65536 + 37
NS = (1, 7, 255, 256, 257, 2049)


def _st():
    return _lib.current_stream()


@pytest.fixture(scope="module")
def codes():
    """Every int16 code, shuffled, and 37 more: int16 numpy [POOL_LEN]"""
    gen = np.random.RandomState(29)
    mid = np.concatenate([np.arange(-32768, 32768), gen.randint(-32768, 32768, POOL_LEN - 65536 - 6)])
    gen.shuffle(mid)
    c = np.concatenate([[-32768, 32767, -1], mid, [1, -32768, 32767]]).astype(np.int16)          # the extremes at both ends
    assert c.size == POOL_LEN and len(np.unique(c)) == 65536
    return c


def _pool_view(codes, byte_offset):
    """the pool as a view `byte_offset` bytes into a larger int16 device tensor whose other elements hold 12345"""
    big = torch.full((POOL_LEN + 64,), 12345, dtype=torch.int16, device=DEV)
    assert big.data_ptr() % 16 == 0 and byte_offset % 2 == 0
    view = big[byte_offset // 2:byte_offset // 2 + POOL_LEN]
    view.copy_(torch.from_numpy(codes))
    assert view.data_ptr() % 16 == byte_offset
    return big, view


def _rows(N):
    starts = [4000 + p for p in range(8)] + [0, POOL_LEN - 1, -3, -(1 << 40), POOL_LEN, POOL_LEN + 9, 1 << 40,
                                              POOL_LEN - 2, POOL_LEN - N // 2 - 1, POOL_LEN - N]
    counts = sorted({0, 1, N - 1, N, N + 5})
    rows = [(s, c) for s in starts for c in counts]
    rows += [(4003, -1), (4003, -(1 << 40)), (4003, 1 << 40), ((1 << 62) + 5, 1 << 62)]
    return rows


def _run(lib, pool, rows, N, ldo, mwv=32768.0):
    B = len(rows)
    out = Guarded(B, ldo)
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    rc = lib.t2s_pcm16_gather(pool.data_ptr(), pool.numel(), table.data_ptr(), B, N, mwv, out.t.data_ptr(), ldo, _st())
    assert rc == 0
    torch.cuda.synchronize()
    out.assert_guards("t2s_pcm16_gather N %d ldo %d" % (N, ldo))
    if ldo > N:
        assert bool(out.untouched(out.t[:, N:]).all()), "columns N .. ldo were written (N %d ldo %d)" % (N, ldo)
    return out.t[:, :N].cpu().numpy()


@pytest.mark.parametrize("byte_offset", [2, 6, 14])
@pytest.mark.parametrize("B", [1, 3])
def test_pcm16_gather_bit_equal(codes, B, byte_offset):
    lib = _lib.load()
    _big, pool = _pool_view(codes, byte_offset)
    launches = 0
    for N in NS:
        rows = _rows(N)
        want_all = D.pcm16_gather_ref(codes, rows, N)
        assert float(np.abs(want_all).max()) > 0.9
        for ldo in (N, N + 3):
            for r0 in range(0, len(rows), B):
                sel = [(r0 + k) % len(rows) for k in range(B)]
                got = _run(lib, pool, [rows[k] for k in sel], N, ldo)
                want = want_all[sel]
                bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
                assert bad.size == 0, "N %d ldo %d rows %r: first mismatch at %r: got %r want %r" % (
                    N, ldo, [rows[k] for k in sel], bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
                launches += 1
    print("GATHER B %d pool at +%d bytes: %d launches bit-equal" % (B, byte_offset, launches))


def test_pcm16_gather_every_code_in_one_row(codes):
    """one row across the whole pool (33 blocks of 2048 outputs): every code, and the scalar head and tail at the pool's two ends"""
    lib = _lib.load()
    for byte_offset in (2, 6, 14):
        _big, pool = _pool_view(codes, byte_offset)
        for N in (POOL_LEN, POOL_LEN + 11):
            got = _run(lib, pool, [(0, POOL_LEN + 100)], N, N)
            want = D.pcm16_gather_ref(codes, [(0, POOL_LEN + 100)], N)
            assert np.array_equal(got.view(np.int32), want.view(np.int32))
            assert np.array_equal(got[0, :POOL_LEN], (torch.from_numpy(codes).float() / 32768).numpy())


def test_pcm16_gather_other_max_wav_value(codes):
    """max_wav_value = 32767: within 1 ulp of numpy's float32 division (measured: 0 ulp)."""
    lib = _lib.load()
    _big, pool = _pool_view(codes, 6)
    worst = 0
    for start in (0, 5):
        N = POOL_LEN - start
        got = _run(lib, pool, [(start, N)], N, N, 32767.0)
        want = D.pcm16_gather_ref(codes, [(start, N)], N, 32767.0)
        assert np.array_equal(np.signbit(got), np.signbit(want))
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        worst = max(worst, int(ulps.max()))
    print("GATHER max_wav_value 32767: worst distance from numpy's f32 division %d ulp" % worst)
    assert worst <= 1


@pytest.mark.parametrize("T", [1, 255, 256, 257])
def test_gate_targets(T):
    lib = _lib.load()
    frames = [-1, 0, 1, 2, T - 1, T, T + 1, -(1 << 31), (1 << 31) - 1]
    for sel in (frames, frames[4:5], frames[::-1][:3]):
        B = len(sel)
        out = Guarded(B, T)
        fr = torch.tensor(sel, dtype=torch.int32, device=DEV)
        assert lib.t2s_gate_targets(fr.data_ptr(), B, T, out.t.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        out.assert_guards("t2s_gate_targets T %d" % T)
        got = out.t.cpu()
        for b, f in enumerate(sel):
            want = D.gate_ref(f, T)
            assert torch.equal(got[b], want), "T %d frames %d: got %r" % (T, f, got[b].tolist()[:8])
            assert not bool(torch.signbit(got[b]).any())
