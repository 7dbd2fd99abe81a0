// Launchers of the audio front-end / back-end kernels (audio_ops.hip).  `lengths` / `frames` ([B] int32, device) may be NULL: every
// entry then has the batch's extent.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

hipError_t t2s_launch_reflect_pad(const float* x, int B, int T, const int* lengths, int pad, float* xp, long ldp, hipStream_t s);
hipError_t t2s_launch_stft_mag_phase(const float* ft, int B, int F, int c, long ld_ft, const int* lengths, int hop, int T, int pad,
                                     float* mag, float* phase, float* magT, long ld_mt, hipStream_t s);
hipError_t t2s_launch_stft_recombine(const float* mag, const float* phase, int B, int F, int c, const int* frames, const float* bias,
                                     float strength, float* rc, long ld_rc, hipStream_t s);
hipError_t t2s_launch_stft_overlap_add(const float* frames_buf, const float* win_sq, int B, int F, const int* frames, int n_fft,
                                       int hop, float scale, float tiny, float* out, int n_out, hipStream_t s);
hipError_t t2s_launch_log_clamp(float* x, int B, int n_mel, int F, const int* frames, float clip, hipStream_t s);
hipError_t t2s_launch_pcm16(const void* x, int is_half, int B, int N, long ldx, const int* lengths, short* out, hipStream_t s);
// training batches from a pool of int16 clips: `table` [B][2] int64 (start, count) on the device, any value safe
hipError_t t2s_launch_pcm16_gather(const short* pool, long pool_len, const long* table, int B, int N, float max_wav, float* out,
                                   long ldo, hipStream_t s);
hipError_t t2s_launch_gate_targets(const int* frames, int B, int T, float* gate, hipStream_t s);
