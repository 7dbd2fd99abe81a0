"""Every refusal of the filter's classes (audio.SosFilter / FilterStream, the designs, PcmPool.filter, DeliveryStream's two keywords,
longform.filter_long) and of its entry points (t2s_sos_filter / t2s_sos_window return T2S_EINVAL before anything is launched), without
a device."""
import numpy as np
import pytest
import torch

import filter_ref as R
from text2speech_amd import _lib, audio, data, longform as L

T2SError = _lib.T2SError
OK = R.ACCURACY_CASES["highpass_80_o4_44800"]


def test_design_refusals():
    for k in (float("nan"), float("inf"), "0.97", None, True):
        with pytest.raises(T2SError, match="sos_preemphasis"):
            audio.sos_preemphasis(k)
    for k in (1.0, -1.0, 1.5, float("nan"), "0.97"):
        with pytest.raises(T2SError, match="sos_deemphasis"):
            audio.sos_deemphasis(k)
    for args in ((4, 80.0, "bandstop", 44800), (0, 80.0, "highpass", 44800), (2.5, 80.0, "highpass", 44800), (True, 80.0, "highpass", 44800),
                 (4, 80.0, "highpass", 0), (4, 80.0, "highpass", float("nan")), (4, 0.0, "highpass", 44800), (4, 22400.0, "lowpass", 44800),
                 (4, (300.0, 3400.0), "lowpass", 8000), (4, 300.0, "bandpass", 8000), (4, (3400.0, 300.0), "bandpass", 8000),
                 (4, (300.0, 4000.0), "bandpass", 8000), (4, "80", "highpass", 44800), (17, 80.0, "highpass", 44800),
                 (9, (300.0, 3400.0), "bandpass", 8000)):
        with pytest.raises(T2SError, match="sos_butter"):
            audio.sos_butter(*args)
    assert audio.sos_butter(16, 3000.0, "lowpass", 44800).shape == (8, 6) and audio.sos_butter(8, (300.0, 3400.0), "bandpass", 8000).shape == (8, 6)


def test_sos_filter_refusals():
    for rate in (0, -8000, float("nan"), "8000", True):
        with pytest.raises(T2SError, match="sampling_rate"):
            audio.SosFilter(OK, rate)
    with pytest.raises(T2SError, match="no CPU path"):
        audio.SosFilter(OK, device="cpu")
    with pytest.raises(T2SError, match="section 1 has a pole of radius"):
        audio.SosFilter([OK[0], [1.0, 0.0, 0.0, 1.0, -2.0, 1.0]])
    with pytest.raises(T2SError, match="section 0 has a0 = 0.5"):
        audio.SosFilter([[1.0, 0.0, 0.0, 0.5, 0.0, 0.0]])
    with pytest.raises(T2SError, match="9 sections"):
        audio.SosFilter(np.tile(OK[:1], (9, 1)))
    with pytest.raises(T2SError, match="not finite"):
        audio.SosFilter([[1.0, 0.0, float("inf"), 1.0, 0.0, 0.0]])
    f = audio.SosFilter(OK, 44800)                              # constructing needs no device
    assert f.n_sections == 2 and f.sampling_rate == 44800 and f.table().shape == (R.TAB_DOUBLES,)
    x = torch.zeros(2, 100)
    with pytest.raises(T2SError, match="audio must be a tensor"):
        f.filter_batch([0.0] * 10)
    with pytest.raises(T2SError, match="gain"):
        f.filter_batch(x, gain="loud")
    with pytest.raises(T2SError, match="gain"):
        f.filter_batch(x, gain=float("nan"))
    with pytest.raises(T2SError, match="a gain tensor must be float64"):
        f.filter_batch(x, gain=torch.ones(2))
    with pytest.raises(T2SError, match="a gain tensor must be float64"):
        f.filter_batch(x, gain=torch.ones(3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        f.filter_batch(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f.forward(x)


def test_filter_stream_refusals():
    with pytest.raises(T2SError, match="must be an audio.SosFilter"):
        audio.FilterStream(OK)
    st = audio.SosFilter(OK).stream()
    assert isinstance(st, audio.FilterStream) and st.position == 0
    with pytest.raises(T2SError, match="nothing has been pushed"):
        st.report()
    with pytest.raises(T2SError, match="a piece must be a tensor"):
        st.push([1.0, 2.0])
    with pytest.raises(T2SError, match="a piece must be a tensor"):
        st.push(torch.zeros(10))
    with pytest.raises(T2SError, match="expected float32 or float16"):
        st.push(torch.zeros(1, 10, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        st.push(torch.zeros(1, 10))
    with pytest.raises(T2SError, match="no CPU path"):
        st.open(1, "cpu")
    for B in (0, 65536):
        with pytest.raises(T2SError, match="rows"):
            audio.SosFilter(OK).stream().open(B, "cuda")


def test_pool_delivery_and_longform_refusals():
    pool = data.PcmPool._of(torch.zeros(10, dtype=torch.int16), torch.tensor([10]), 8000)
    with pytest.raises(T2SError, match="filt must be an audio.SosFilter"):
        pool.filter(OK)
    with pytest.raises(T2SError, match="designed for 44800 Hz, the pool holds 8000 Hz"):
        pool.filter(audio.SosFilter(OK, 44800))
    with pytest.raises(T2SError) as e:
        audio.DeliveryStream(44800)
    assert str(e.value) == "DeliveryStream: nothing to do - ask for another rate, a limiter or an encoding"
    with pytest.raises(T2SError) as e:
        audio.DeliveryStream(44800, 44800, None, None, "f32", None, None)      # the two keywords stand behind `encoding`
    assert "nothing to do" in str(e.value)
    ds = audio.DeliveryStream(44800, pre_filter=audio.SosFilter(OK, 44800))
    assert ds.latency == 0 and ds.pre_filter is not None and ds.post_filter is None
    assert audio.DeliveryStream(44800, 8000, post_filter=audio.SosFilter(OK)).latency == audio.DeliveryStream(44800, 8000).latency
    with pytest.raises(T2SError, match="pre_filter must be an audio.SosFilter"):
        audio.DeliveryStream(44800, pre_filter=OK)
    with pytest.raises(T2SError, match="post_filter must be an audio.SosFilter"):
        audio.DeliveryStream(44800, 8000, post_filter="telephone")
    with pytest.raises(T2SError, match="pre_filter was designed for 8000 Hz, it runs at 44800 Hz"):
        audio.DeliveryStream(44800, 8000, pre_filter=audio.SosFilter(OK, 8000))
    with pytest.raises(T2SError, match="post_filter was designed for 44800 Hz, it runs at 8000 Hz"):
        audio.DeliveryStream(44800, 8000, post_filter=audio.SosFilter(OK, 44800))
    with pytest.raises(T2SError, match="nothing has been pushed"):
        ds.filter_report()
    r = L.LongForm(torch.zeros(1, 10), torch.tensor([10]), torch.zeros(2, dtype=torch.int64), ["a"], torch.zeros(1, dtype=torch.bool))
    with pytest.raises(T2SError, match="filt must be an audio.SosFilter"):
        L.filter_long(r, OK)
    with pytest.raises(T2SError, match="expected a LongForm"):
        L.filter_long(r.audio, audio.SosFilter(OK))
    with pytest.raises(T2SError, match="pcm16=False"):
        L.filter_long(r._replace(audio=r.audio.to(torch.int16)), audio.SosFilter(OK))


def test_entry_points_reject_bad_arguments():
    """Every t2s_sos_filter / t2s_sos_window rule, one broken at a time, on a valid tuple of made-up aligned pointers - so this runs
    only where there is no device: a tuple accepted by mistake fails there as a HIP error and reaches no GPU.  The valid tuple itself
    is never called (it would launch)."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only on a machine without a GPU (tests/test_filter_kernels_gpu.py runs the list on real buffers)")
    lib = _lib.load()
    n, B, Ln = 2, 2, 100
    need = lib.t2s_sos_scratch(B, Ln, n)
    assert need == B * 2 * n
    P = lambda k: 0x7000_0000_0000 + 0x100000 * k                # noqa: E731  (distinct, far apart, 8-byte aligned)
    base = dict(src=P(1), src_kind=1, src_len=B * Ln, table=P(2), n_rows=B, max_count=Ln, gains=P(3), tab=P(4), n_sections=n,
                scratch=P(5), scratch_len=need, dst=P(6), dst_kind=1, dst_len=B * Ln, max_out=Ln, counts=P(7), stream=None)
    k = 0
    for label, changes in R.filter_refusals():
        a = R.apply_changes(base, changes)
        assert lib.t2s_sos_filter(*[a[p] for p in R.FILTER_PARAMS]) == -1, label
        k += 1
    wbase = dict(carry_in=P(1), carry_out=P(2), piece=P(3), is_half=0, B=B, n=Ln, ldp=Ln, N0=0, gains=P(4), tab=P(5), n_sections=n,
                 scratch=P(6), scratch_len=need, out=P(7), ldo=Ln, counts=P(8), stream=None)
    for label, changes in R.window_refusals():
        a = R.apply_changes(wbase, changes)
        assert lib.t2s_sos_window(*[a[p] for p in R.WINDOW_PARAMS]) == -1, label
        k += 1
    assert k > 55
    # the geometry calls refuse with -1
    assert lib.t2s_sos_scratch(0, 10, 1) == lib.t2s_sos_scratch(1, 10, 0) == lib.t2s_sos_scratch(1, 10, 9) == lib.t2s_sos_scratch(65536, 10, 1) == -1
    assert lib.t2s_sos_scratch(1, 2 ** 31, 1) == -1 and lib.t2s_sos_window_carry(9) == -1
