"""Plain numpy / torch restatements of the reference's two training data loaders, the expected values of the data front-end tests
(text2speech_amd/data.py).  The loader modules themselves import packages this project does not depend on, so each function here
cites the reference lines it restates; tests/test_data_ref_cpu.py pins them.  A plain module, imported by the tests."""
import random

import numpy as np
import torch


def pcm16_gather_ref(pool, table, N, max_wav_value=32768.0):
    """include/t2s_hip.h, t2s_pcm16_gather: f32 [B, N] = pool[start + t] / max_wav_value for t < c, +0 behind; c is count clamped
    to [0, N] and to the pool, 0 for a start outside it.  numpy's own float32 division."""
    pool = np.asarray(pool)
    assert pool.dtype == np.int16 and pool.ndim == 1
    out = np.zeros((len(table), N), dtype=np.float32)
    for b, (start, count) in enumerate(table):
        start, count = int(start), int(count)
        c = min(max(count, 0), N)
        if start < 0 or start >= pool.size:
            c = 0
        c = min(c, pool.size - start) if c else 0
        out[b, :c] = pool[start:start + c].astype(np.float32) / np.float32(max_wav_value)
    return out


def crop_starts_ref(lengths, segment_length, seed=1234):
    """waveglow/mel2samp.py:94-100 over the entries in order, `random` being a fresh random.Random(seed): a clip of at least
    segment_length samples draws randint(0, len - segment_length); a shorter one draws nothing (its start counts as 0)."""
    rng = random.Random(seed)
    starts = []
    for n in lengths:
        if n >= segment_length:
            max_audio_start = n - segment_length
            starts.append(rng.randint(0, max_audio_start))
        else:
            starts.append(0)
    return starts


def mel2samp_audio_ref(clips, indices, starts, segment_length, max_wav_value=32768.0):
    """waveglow/mel2samp.py:57, 94-103 per entry and the default collate's stack: int16 -> float, crop at the given start or zero
    pad to segment_length, divide by MAX_WAV_VALUE.  f32 torch [B, segment_length]."""
    rows = []
    for i, s in zip(indices, starts):
        audio = torch.from_numpy(np.asarray(clips[i])).float()
        if audio.size(0) >= segment_length:
            audio = audio[s:s + segment_length]
        else:
            audio = torch.nn.functional.pad(audio, (0, segment_length - audio.size(0)), "constant")
        rows.append(audio / max_wav_value)
    return torch.stack(rows)


def target_len_ref(max_target_len, n_frames_per_step):
    """utils/data_utils.py:127-130"""
    if max_target_len % n_frames_per_step != 0:
        max_target_len += n_frames_per_step - max_target_len % n_frames_per_step
    return max_target_len


def gate_ref(frames, T):
    """utils/data_utils.py:140-146 for one row of T frames: gate[frames - 1:] = 1 - with the kernel's stated ends: frames <= 0 the
    whole row 1, frames > T the whole row 0 (Python's negative index would wrap; the entry point does not)."""
    gate = torch.zeros(T)
    gate[min(max(frames - 1, 0), T):] = 1
    return gate


def collate_ref(batch, n_frames_per_step):
    """utils/data_utils.py:107-150 (TextMelCollate.__call__).  batch: a list of (text int tensor [n], mel f32 [n_mel, frames],
    speaker id).  Returns text_padded, input_lengths, mel_padded, gate_padded, speaker_id, output_lengths - and, seventh, the sorted
    order.  NOTE the reference fills speaker_id in batch order, not in sorted order (lines 132-135): restated as it is."""
    input_lengths, ids_sorted_decreasing = torch.sort(torch.LongTensor([len(x[0]) for x in batch]), dim=0, descending=True)
    max_input_len = int(input_lengths[0])
    text_padded = torch.zeros(len(batch), max_input_len, dtype=torch.int64)
    for i in range(len(ids_sorted_decreasing)):
        text = batch[ids_sorted_decreasing[i]][0]
        text_padded[i, :text.size(0)] = text
    num_mels = batch[0][1].size(0)
    max_target_len = target_len_ref(max(x[1].size(1) for x in batch), n_frames_per_step)
    speaker_id = torch.FloatTensor([float(x[2]) for x in batch])
    mel_padded = torch.zeros(len(batch), num_mels, max_target_len)
    gate_padded = torch.zeros(len(batch), max_target_len)
    output_lengths = torch.zeros(len(batch), dtype=torch.int64)
    for i in range(len(ids_sorted_decreasing)):
        mel = batch[ids_sorted_decreasing[i]][1]
        mel_padded[i, :, :mel.size(1)] = mel
        gate_padded[i, mel.size(1) - 1:] = 1
        output_lengths[i] = mel.size(1)
    return text_padded, input_lengths, mel_padded, gate_padded, speaker_id, output_lengths, ids_sorted_decreasing.tolist()
