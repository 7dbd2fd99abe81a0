"""Host-side argument handling of keyed sampling (text2speech_amd/sampling.py and the checks in front of WaveGlow.infer /
infer_batch): what is accepted, what raises, before any device is touched."""
import pytest
import torch

from text2speech_amd import _lib, sampling, synth


def test_check_seed():
    assert sampling.check_seed(0) == 0 and sampling.check_seed(2 ** 63 - 1) == 2 ** 63 - 1
    assert sampling.check_seed(torch.tensor(7)) == 7
    for bad in (-1, 2 ** 63, 1.5, "3", None):
        with pytest.raises(ValueError):
            sampling.check_seed(bad)


def test_seeds_tensor():
    t = sampling.seeds_tensor([1, 2 ** 62 + 5, 0], 3, "cpu")
    assert t.dtype == torch.int64 and t.tolist() == [1, 2 ** 62 + 5, 0]
    assert sampling.seeds_tensor((4, 5), 2, "cpu").tolist() == [4, 5]
    assert sampling.seeds_tensor(torch.tensor([4, 5]), 2, "cpu").tolist() == [4, 5]
    for bad, B in (([1, 2], 3), ([1, 2, 3, 4], 3), ([1, -2, 3], 3), ([1, 2, 2 ** 63], 3), ([1.5, 2, 3], 3), (5, 1),
                   (torch.tensor([1, -2, 3]), 3), (torch.tensor([1, 2]), 3), (torch.tensor([[1, 2, 3]]), 3),
                   (torch.tensor([1, 2, 3], dtype=torch.int32), 3), (torch.tensor([1.0, 2.0, 3.0]), 3)):
        with pytest.raises(ValueError):
            sampling.seeds_tensor(bad, B, "cpu")


def test_sigmas_tensor():
    assert sampling.sigmas_tensor(0.666, 3, "cpu") == (0.666, None)
    s, t = sampling.sigmas_tensor(torch.tensor([0.5, 0.0, 1.0], dtype=torch.float64), 3, "cpu")
    assert t.dtype == torch.float32 and t.tolist() == [0.5, 0.0, 1.0] and s >= 0
    for bad in (torch.tensor([0.5, 1.0]), torch.tensor([0.5, -1.0, 1.0]), torch.tensor([0.5, float("inf"), 1.0]),
                torch.tensor([0.5, float("nan"), 1.0]), torch.tensor([1, 2, 3]), torch.tensor([[0.5, 1.0, 1.0]])):
        with pytest.raises(ValueError):
            sampling.sigmas_tensor(bad, 3, "cpu")


def test_vocoder_argument_rules_without_a_device():
    from text2speech_amd.glow import WaveGlow
    m = WaveGlow(**synth.WAVEGLOW_SMALL)
    mel = torch.zeros(2, 80, 4)
    assert m._keyed_args("infer", mel, 0.666, None, None) == (None, 0.666, None)           # no seed: as before
    assert m._keyed_args("infer", mel, torch.tensor(0.5), None, None) == (None, 0.5, None)
    with pytest.raises(_lib.T2SError, match="needs seed"):
        m._keyed_args("infer", mel, torch.tensor([0.5, 0.5]), None, None)
    with pytest.raises(_lib.T2SError, match="not both"):
        m._keyed_args("infer", mel, 0.666, (mel, []), 3)
    with pytest.raises(_lib.T2SError, match="CUDA/HIP"):
        m._keyed_args("infer", mel, 0.666, None, 3)                                         # a host mel: no CPU fallback
    with pytest.raises(_lib.T2SError):
        m.draw_noise([1, 2], 8)                                                             # the model is on the host
