"""The data front end (text2speech_amd/data.py) where no GPU is needed: the two entry points are exported and refuse bad arguments
before anything is launched, the restatements of tests/data_ref.py behave as the reference's loaders do at their edges, the gathered
row width gives the collate's frame count, and PcmPool refuses what is not 1-D int16."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import data_ref as D


def _lib_loaded():
    from text2speech_amd import _lib
    return _lib, _lib.load()


def test_symbols_exported_and_declared():
    _lib, lib = _lib_loaded()
    for name in ("t2s_pcm16_gather", "t2s_gate_targets"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert _lib.SIGNATURES["t2s_pcm16_gather"][1] is ctypes.c_long and _lib.SIGNATURES["t2s_pcm16_gather"][5] is ctypes.c_float
    assert lib.t2s_abi_version() == 4


def test_entry_points_refuse_before_any_launch():
    """Made-up pointers: every call here must return T2S_EINVAL (-1) without touching them.  Only where there is no device, as in
    tests/test_audio_ragged_cpu.py: a check that went missing would launch on those pointers."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only on a machine without a GPU")
    _, lib = _lib_loaded()
    POOL, TABLE, OUT = 0x10000, 0x20000, 0x30000

    def gather(pool=POOL, pool_len=1000, table=TABLE, B=2, N=16, mwv=32768.0, out=OUT, ldo=16):
        return lib.t2s_pcm16_gather(pool, pool_len, table, B, N, mwv, out, ldo, None)

    assert gather(pool=None) == -1 and gather(table=None) == -1 and gather(out=None) == -1
    assert gather(pool_len=0) == -1 and gather(pool_len=-5) == -1
    assert gather(B=0) == -1 and gather(B=-1) == -1 and gather(B=65536) == -1
    assert gather(N=0) == -1 and gather(N=-3) == -1
    assert gather(ldo=15) == -1, "ldo below N"
    for bad in (0.0, -32768.0, float("nan"), float("inf"), float("-inf")):
        assert gather(mwv=bad) == -1, bad

    def gate(frames=TABLE, B=2, T=16, out=OUT):
        return lib.t2s_gate_targets(frames, B, T, out, None)

    assert gate(frames=None) == -1 and gate(out=None) == -1
    assert gate(B=0) == -1 and gate(B=-2) == -1 and gate(B=65536) == -1
    assert gate(T=0) == -1 and gate(T=-1) == -1


# ---- the restatements at their edges --------------------------------------------------------------------------------------------------
def test_crop_draws_follow_one_generator_in_index_order():
    from text2speech_amd import data
    seg = 400
    lengths = [1000, 150, 400, 401, 399, 5000, 400]
    for seed in (1234, 7):
        rng = random.Random(seed)
        want = []
        for n in lengths:                                   # the reference's loop, short clips skipped
            want.append(rng.randint(0, n - seg) if n >= seg else 0)
        assert D.crop_starts_ref(lengths, seg, seed) == want
        assert data.crop_starts(lengths, seg, random.Random(seed)) == want
    # skipping is visible: with the short clips taken out, the long ones get the same draws
    long_only = [n for n in lengths if n >= seg]
    all_ = D.crop_starts_ref(lengths, seg, 3)
    assert [s for s, n in zip(all_, lengths) if n >= seg] == D.crop_starts_ref(long_only, seg, 3)


def test_a_clip_of_exactly_segment_length_consumes_a_draw():
    seg = 400
    rng = random.Random(11)
    assert rng.randint(0, 0) == 0
    after_one = rng.randint(0, 10 ** 9)
    assert D.crop_starts_ref([400, 10 ** 9 + 400], seg, 11) == [0, after_one]
    first = random.Random(11).randint(0, 10 ** 9)           # a clip one sample shorter draws nothing: the next clip gets the first draw
    assert D.crop_starts_ref([399, 10 ** 9 + 400], seg, 11) == [0, first]
    assert first != after_one


def _batch(text_lens, frames, n_mel=3, seed=2):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randint(1, 50, (n,), generator=gen), torch.randn(n_mel, f, generator=gen), float(k))
            for k, (n, f) in enumerate(zip(text_lens, frames))]


def test_collate_order_on_ties_is_torch_sort():
    text_lens = [5, 9, 5, 9, 2, 5]
    batch = _batch(text_lens, [4, 7, 3, 2, 9, 5])
    out = D.collate_ref(batch, 1)
    want_len, want_order = torch.sort(torch.LongTensor(text_lens), dim=0, descending=True)
    assert out[6] == want_order.tolist() and torch.equal(out[1], want_len)
    for row, k in enumerate(out[6]):
        text, mel, _ = batch[k]
        assert torch.equal(out[0][row, :text.numel()], text) and int(out[0][row, text.numel():].abs().sum()) == 0
        assert torch.equal(out[2][row, :, :mel.size(1)], mel) and float(out[2][row, :, mel.size(1):].abs().sum()) == 0.0
        assert int(out[5][row]) == mel.size(1)
        assert torch.equal(out[3][row], D.gate_ref(mel.size(1), out[3].size(1)))
    assert out[4].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0], "speaker ids stay in batch order (utils/data_utils.py:132-135)"
    assert out[0].dtype == torch.int64 and out[2].dtype == torch.float32 and out[4].dtype == torch.float32 \
        and out[5].dtype == torch.int64


def test_target_length_rounding():
    assert [D.target_len_ref(n, 1) for n in (1, 2, 7)] == [1, 2, 7]
    assert [D.target_len_ref(n, 3) for n in (1, 2, 3, 4, 7, 9)] == [3, 3, 3, 6, 9, 9]
    for step in (1, 3):
        out = D.collate_ref(_batch([3, 4], [7, 5]), step)
        assert out[2].size(2) == out[3].size(1) == (7 if step == 1 else 9)
        assert float(out[2][:, :, 7:].abs().sum()) == 0.0


def test_gate_rows():
    assert D.gate_ref(1, 5).tolist() == [1.0] * 5, "frames = 1: all ones"
    assert D.gate_ref(0, 5).tolist() == [1.0] * 5 and D.gate_ref(-1, 5).tolist() == [1.0] * 5
    assert D.gate_ref(2, 5).tolist() == [0.0, 1.0, 1.0, 1.0, 1.0]
    assert D.gate_ref(5, 5).tolist() == [0.0] * 4 + [1.0]
    assert D.gate_ref(6, 5).tolist() == [0.0] * 5
    out = D.collate_ref(_batch([3], [1]), 1)
    assert out[3].tolist() == [[1.0]]


# ---- the width of the gathered rows -----------------------------------------------------------------------------------------------------
def test_gather_width_gives_the_collates_frame_count():
    from text2speech_amd.data import gather_width
    n = 0
    for hop in range(4, 257):
        for k in (1, 2, 3, 7):
            for longest in (k * hop - 1, k * hop, k * hop + 1):
                for step in (1, 3):
                    t_out = D.target_len_ref(1 + longest // hop, step)
                    w = gather_width(longest, t_out, hop)
                    assert 1 + w // hop == t_out and w >= longest, (hop, longest, step, w)
                    assert w % 4 == 0 or -(-w // 4) * 4 >= t_out * hop, "rounded to 16-byte rows wherever the frame count allows"
                    n += 1
    assert n == 253 * 4 * 3 * 2
    with pytest.raises(ValueError):
        gather_width(100, 3, 16)


# ---- PcmPool ----------------------------------------------------------------------------------------------------------------------------
def test_pool_refuses_what_is_not_1d_int16():
    from text2speech_amd import _lib, data
    ok = np.arange(10, dtype=np.int16)
    for bad in (ok.astype(np.float32), ok.astype(np.int32), ok.reshape(2, 5), torch.zeros(4), torch.zeros(4, dtype=torch.int32),
                torch.zeros(2, 2, dtype=torch.int16), [1, 2, 3], np.zeros(0, dtype=np.int16)):
        with pytest.raises(_lib.T2SError):
            data.PcmPool([ok, bad], 22050)
    with pytest.raises(_lib.T2SError):
        data.PcmPool([], 22050)


def test_wav_files_round_trip(tmp_path):
    from scipy.io.wavfile import write
    from text2speech_amd import _lib, data
    gen = np.random.RandomState(4)
    clips = [gen.randint(-32768, 32768, n).astype(np.int16) for n in (1, 100, 4097)]
    clips[1][:2] = [-32768, 32767]
    paths = []
    for k, c in enumerate(clips):
        paths.append(os.path.join(str(tmp_path), "clip%d.wav" % k))
        write(paths[-1], 22050, c)
    got = data.PcmPool.read_wav_files(paths, 22050)
    assert len(got) == 3 and all(g.dtype == np.int16 and np.array_equal(g, c) for g, c in zip(got, clips))
    with pytest.raises(ValueError, match="22050 SR doesn't match target 16000 SR"):
        data.PcmPool.from_wav_files(paths, 16000)
    stereo = os.path.join(str(tmp_path), "stereo.wav")
    write(stereo, 22050, np.zeros((50, 2), dtype=np.int16))
    floats = os.path.join(str(tmp_path), "floats.wav")
    write(floats, 22050, np.zeros(50, dtype=np.float32))
    for bad in (stereo, floats):
        with pytest.raises(_lib.T2SError):
            data.PcmPool.from_wav_files([paths[0], bad], 22050)
