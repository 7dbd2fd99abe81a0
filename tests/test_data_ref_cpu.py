"""tests/data_ref.py pinned on the CPU against values written out by hand and against plain numpy / torch expressions."""
import numpy as np
import torch

import data_ref as D


def test_gather_ref_is_numpys_division_placed_into_zeros():
    pool = np.array([-32768, -1, 0, 1, 2, 32767, 100, -100], dtype=np.int16)
    table = [(0, 3), (5, 8), (6, 0), (-1, 4), (8, 4), (7, 4), (2, 100), (3, -2)]
    got = D.pcm16_gather_ref(pool, table, 4)
    want = np.zeros((8, 4), dtype=np.float32)
    want[0, :3] = [-1.0, -1.0 / 32768, 0.0]
    want[1, :3] = [32767.0 / 32768, 100.0 / 32768, -100.0 / 32768]              # clamped to the pool's end
    want[5, :1] = [-100.0 / 32768]
    want[6, :4] = [0.0, 1.0 / 32768, 2.0 / 32768, 32767.0 / 32768]              # clamped to N
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert not np.signbit(got[got == 0]).any(), "padding is +0"
    # exact for every code with 32768; numpy's own f32 division otherwise
    codes = np.arange(-32768, 32768, dtype=np.int16)
    full = D.pcm16_gather_ref(codes, [(0, 65536)], 65536)[0]
    assert np.array_equal(full.astype(np.float64) * 32768.0, codes.astype(np.float64))
    assert np.array_equal(full, (torch.from_numpy(codes).float() / 32768).numpy())
    other = D.pcm16_gather_ref(codes, [(0, 65536)], 65536, 32767.0)[0]
    assert np.array_equal(other, codes.astype(np.float32) / np.float32(32767))


def test_mel2samp_audio_ref():
    clips = [np.arange(10, dtype=np.int16) * 100, np.array([-32768, 32767, 5], dtype=np.int16)]
    got = D.mel2samp_audio_ref(clips, [0, 1, 0], [3, 0, 6], 4)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 4)
    assert got[0].tolist() == [300 / 32768, 400 / 32768, 500 / 32768, 600 / 32768]
    assert got[1].tolist() == [-1.0, 32767 / 32768, 5 / 32768, 0.0]
    assert got[2].tolist() == [600 / 32768, 700 / 32768, 800 / 32768, 900 / 32768]


def test_collate_ref_by_hand():
    text = [torch.tensor([4, 5]), torch.tensor([7, 8, 9]), torch.tensor([1])]
    mel = [torch.full((2, 3), 1.0), torch.full((2, 1), 2.0), torch.full((2, 4), 3.0)]
    tp, il, mp, gp, sp, ol, order = D.collate_ref([(t, m, s) for t, m, s in zip(text, mel, (10, 11, 12))], 3)
    assert order == [1, 0, 2] and il.tolist() == [3, 2, 1]
    assert tp.tolist() == [[7, 8, 9], [4, 5, 0], [1, 0, 0]]
    assert tuple(mp.shape) == (3, 2, 6) and ol.tolist() == [1, 3, 4]
    assert mp[0, 0].tolist() == [2, 0, 0, 0, 0, 0] and mp[1, 1].tolist() == [1, 1, 1, 0, 0, 0] and mp[2, 0].tolist() == [3, 3, 3, 3, 0, 0]
    assert gp.tolist() == [[1, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1], [0, 0, 0, 1, 1, 1]]
    assert sp.tolist() == [10.0, 11.0, 12.0]
