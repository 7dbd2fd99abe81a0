// Cross-workgroup hand-offs of the Tacotron-2 kernels: the one protocol behind the split BiLSTM recurrence and its BPTT
// (lstm_seq_split_kernel, lstm_seq_bwd_split_kernel), the one-launch attention forward (att_energy_mfma_kernel<true>), the attention
// backward with the cell folded in (att_bwd_fused_kernel) and the paced helper stream (pace_wait_kernel and its start signals).
//
// Granule: a value travels as one naturally aligned 8-byte word (tag << 32) | float bits, written by ONE relaxed agent-scope
// store (global_store_dwordx2 sc1); the consumer lane polls its own granule with a relaxed agent-scope load (global_load_dwordx2
// sc1) until the tag is the one it expects (MI355X_MICROARCH.md handoff-1to1 / "R2's granule").  sc1 stores write through to
// memory and sc1 loads bypass the CU's L1, and the value arrives in the same untorn 8-byte word as its tag: no flag, no fence, no
// L2 write-back.  Tags are never 0 (a step number + 1), so a buffer zeroed before its first use matches nothing; a tag is used
// once per buffer and zeroing (or an epoch in the tag) keeps a previous use's granules from matching.  Where slots are reused
// within a launch they alternate by step parity: a producer overwrites slot s & 1 at step s + 2, after it has seen every
// partner's step s + 1, which the partners publish after reading step s.
//
// Every wait is bounded (T2S_SPIN_MAX polls, seconds): on expiry the kernel raises its buffer's error word (handoff_raise) and its
// workgroup leaves; the host reads the word (Tacotron engine check_lstm_xbuf()).  The workgroup-level side (the LDS failure flag,
// the barriers around it, which thread raises, leaving the loop or the kernel) belongs to each kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

constexpr int T2S_SPIN_MAX = 1 << 22;          // polls before a bounded wait gives up

static __device__ __forceinline__ void handoff_publish(unsigned long long* slot, unsigned tag, float v) {
    const unsigned long long g = ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v);
    __hip_atomic_store(slot, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);         // global_store_dwordx2 sc1
}
// polls until the granule carries `tag`, then v = its value; false on expiry (v untouched)
static __device__ __forceinline__ bool handoff_await(const unsigned long long* slot, unsigned tag, float& v) {
    for (int it = 0; it < T2S_SPIN_MAX; ++it) {
        const unsigned long long g = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // global_load_dwordx2 sc1
        if ((unsigned)(g >> 32) == tag) { v = __uint_as_float((unsigned)g); return true; }
        __builtin_amdgcn_s_sleep(1);
    }
    return false;
}
static __device__ __forceinline__ void handoff_raise(unsigned long long* err) {
    __hip_atomic_store(err, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Pace counter: the first thread of a launch stores step + 1 as the kernel starts (everything in front of it on its stream has
// completed); a one-wave kernel on a helper stream polls until the counter has reached a value (wrap-safe comparison).
static __device__ __forceinline__ void pace_signal(unsigned* flag, unsigned val) {
    __hip_atomic_store(flag, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// false on expiry
static __device__ __forceinline__ bool pace_await(const unsigned* flag, unsigned val) {
    for (int it = 0; it < T2S_SPIN_MAX; ++it) {
        const unsigned v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int)(v - val) >= 0) return true;
        __builtin_amdgcn_s_sleep(2);
    }
    return false;
}

// Split BiLSTM exchange buffer (t2s_taco_encoder_lstm_split / _bwd_split): [2 B groups][2 step parities][256 units] granules, then
// the error word.  The tag of step s is (epoch << 12) + s + 1: 12 bits for the step (T < SPLIT_LSTM_T_LIMIT) and 20 for the
// caller's launch counter, so that nothing a previous launch left matches.
constexpr int SPLIT_LSTM_T_LIMIT = 4095;
constexpr unsigned SPLIT_LSTM_EPOCH_MASK = 0xFFFFFu;
static __device__ __forceinline__ unsigned split_lstm_tag(unsigned epoch, int s) { return (epoch << 12) + 1u + (unsigned)s; }
static __host__ __device__ __forceinline__ size_t split_lstm_err_word(int B) { return (size_t)2 * B * 2 * 256; }
