"""float64 (or any dtype) references of the audio entry points that take per-entry lengths - t2s_stft_transform_ragged,
t2s_mel_from_mag_ragged, t2s_stft_inverse_ragged, t2s_pcm16 (include/t2s_hip.h) - built PER ENTRY from the references of their
partners in tests/tail_ref_util.py: slice the entry, evaluate the partner's reference on it alone, place the result into zeros.  So
"every entry gets what it gets alone, and zeros behind its end" is the construction here, not a property to be checked.  Plain numpy /
torch, no device: imported by tests/test_audio_ragged_kernels_gpu.py and pinned by tests/test_audio_ragged_cpu.py."""
import numpy as np
import torch

import tail_ref_util as R


def frame_counts(lengths, hop):
    return [int(n) // hop + 1 for n in lengths]


def stft_transform_ragged_ref(audio, lengths, fwd, n_fft, hop, dtype=torch.float64):
    """audio [B, T] (the padding may hold anything, NaN included) -> (ft, mag, phase) as R.stft_transform_ref lays them out at
    F = T // hop + 1; entry b fills frames f < lengths[b] // hop + 1, zeros behind."""
    B, T = audio.shape
    c, F_ = n_fft // 2 + 1, T // hop + 1
    ft, mag, ph = torch.zeros(B, F_, 2 * c, dtype=dtype), torch.zeros(B, c, F_, dtype=dtype), torch.zeros(B, c, F_, dtype=dtype)
    for b, n in enumerate(lengths):
        f1, m1, p1 = R.stft_transform_ref(audio[b:b + 1, :n].contiguous(), fwd, n_fft, hop, dtype=dtype)
        Fb = n // hop + 1
        assert f1.shape == (1, Fb, 2 * c)
        ft[b, :Fb], mag[b, :, :Fb], ph[b, :, :Fb] = f1[0], m1[0], p1[0]
    return ft, mag, ph


def mel_ragged_ref(magT, mel_basis_p, B, F_, frames, clip, dtype=torch.float64):
    """magT [B F, ld] -> mel [B, n_mel, F]: R.mel_ref of entry b's first frames[b] rows, zeros (not log(clip)) behind."""
    ld = magT.size(1)
    out = torch.zeros(B, mel_basis_p.size(0), F_, dtype=dtype)
    rows = magT.view(B, F_, ld)
    for b, fb in enumerate(frames):
        out[b, :, :fb] = R.mel_ref(rows[b, :fb].contiguous(), mel_basis_p, 1, fb, clip, dtype=dtype)[0]
    return out


def stft_inverse_ragged_ref(mag, ph, frames, inv_t, n_fft, hop, win_sq, bias=None, strength=0.0, dtype=torch.float64):
    """mag, ph [B, c, F] (frames behind an entry's end may hold anything) -> [B, hop (F - 1)]: R.stft_inverse_ref of entry b's first
    frames[b] frames in its first hop (frames[b] - 1) samples, zeros behind."""
    B, c, F_ = mag.shape
    out = torch.zeros(B, hop * (F_ - 1), dtype=dtype)
    for b, fb in enumerate(frames):
        one = R.stft_inverse_ref(mag[b:b + 1, :, :fb].contiguous(), ph[b:b + 1, :, :fb].contiguous(), inv_t, n_fft, hop, win_sq,
                                 bias=bias, strength=strength, dtype=dtype)
        out[b, :hop * (fb - 1)] = one[0]
    return out


def pcm16_ref(x, lengths=None):
    """x [B, N] float32 or float16 (torch or numpy) -> int16 numpy [B, N]: trunc(float32(x) * 32768) toward zero, saturated to
    [-32768, 32767], NaN -> 0, 0 at and behind lengths[b].  The product is exact in float32 (a power of two) unless it overflows
    to +-inf, which saturates; so float64 arithmetic on the float32 values gives the same integers."""
    v = (x.detach().cpu().float().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float32)).astype(np.float64) * 32768.0
    with np.errstate(invalid="ignore"):
        t = np.trunc(v)
    t = np.where(np.isnan(v), 0.0, np.clip(t, -32768.0, 32767.0))
    out = t.astype(np.int16)
    if lengths is not None:
        for b, n in enumerate(lengths):
            out[b, max(int(n), 0):] = 0
    return out
