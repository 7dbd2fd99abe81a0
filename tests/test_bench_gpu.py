"""bench.py's plain run on the GPU: one JSON line with the headline keys, exactly --steps timed steps, and --dump-outputs writing
what the last timed WaveGlow forward returned - the same as this process's forward of the same seeded weights and inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from text2speech_amd import _lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    from text2speech_amd.glow import WaveGlow
    batch, segment = 1, 4096
    out_dir = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(batch), "--segment", str(segment), "--dump-outputs", out_dir],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] - batch * segment / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    for key in ("roofline", "waveglow_train", "tacotron", "cpu_baseline"):
        assert not line.get(key), key          # measured with --full only

    _lib.load()
    cfg = synth.WAVEGLOW_DEFAULT
    m = WaveGlow(**cfg)
    m.load_state_dict(synth.waveglow_state(cfg))
    m = m.to("cuda:0").eval()
    mel, audio = synth.waveglow_inputs(batch, segment, seed=1234)
    with torch.no_grad():
        z, log_s, log_det = m((mel.cuda(), audio.cuda()))
    torch.cuda.synchronize()
    want = {"z": z}
    want.update(("log_s_%02d" % i, t) for i, t in enumerate(log_s))
    want.update(("log_det_W_%02d" % i, t) for i, t in enumerate(log_det))
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in want)
    for name, t in want.items():
        got = np.load(os.path.join(out_dir, name + ".npy"))
        assert got.dtype == np.float32 and got.shape == tuple(t.shape), name
        assert _rel(got, t.cpu().numpy()) < 1e-5, name
