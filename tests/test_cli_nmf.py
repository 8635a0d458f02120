"""`dsp decompose` through click's runner: its usage errors need no device; the round trip does."""
import re

import numpy as np
import pytest
import scipy.io.wavfile
from click.testing import CliRunner

from sygnals_amd.cli.main import cli


def _wav(path, fs=22050, n=8192):
    t = np.arange(n) / fs
    x = (0.5 * np.sin(2 * np.pi * 440 * t) + 0.3 * np.sin(2 * np.pi * 1500 * t) * (t > 0.2)
         + 0.01 * np.random.default_rng(0).standard_normal(n)).astype(np.float32)
    scipy.io.wavfile.write(path, fs, x)
    return x


def test_usage_errors(tmp_path):
    wav, out = tmp_path / "a.wav", tmp_path / "o.npz"
    _wav(wav)
    run = CliRunner().invoke
    r = run(cli, ["dsp", "decompose", str(wav)])
    assert r.exit_code == 2 and "-o / --output is required" in r.output
    r = run(cli, ["dsp", "decompose", str(wav), "-o", str(tmp_path / "o.csv")])
    assert r.exit_code == 2 and "must be an .npz file" in r.output
    for k in ("0", "65"):
        r = run(cli, ["dsp", "decompose", str(wav), "-o", str(out), "--components", k])
        assert r.exit_code == 2 and "--components must be in [1, 64]" in r.output
    r = run(cli, ["dsp", "decompose", str(wav), "-o", str(out), "--iterations", "-1"])
    assert r.exit_code == 2 and "--iterations must be non-negative" in r.output
    r = run(cli, ["dsp", "decompose", str(wav), "-o", str(out), "--seed", "-1"])
    assert r.exit_code == 2 and "--seed must be non-negative" in r.output
    r = run(cli, ["dsp", "decompose", str(wav), "-o", str(out), "--loss", "itakura-saito"])
    assert r.exit_code == 2
    assert not out.exists()
    assert "--components" in run(cli, ["dsp", "decompose", "--help"]).output


@pytest.mark.gpu
def test_round_trip(tmp_path):
    """The command writes what ops.nmf returns for the input's magnitudes and the seed, bit for bit, in librosa's
    orientation, and prints the divergence of the start and of the result."""
    from sygnals_amd import ops
    wav, out = tmp_path / "a.wav", tmp_path / "o.npz"
    x = _wav(wav)
    run = CliRunner().invoke
    for loss in ("frobenius", "kullback-leibler"):
        r = run(cli, ["dsp", "decompose", str(wav), "-o", str(out), "--components", "3", "--iterations", "12", "--loss", loss,
                      "--seed", "5"])
        assert r.exit_code == 0, r.output
        m = re.search(r"Decomposed 17 frames x 1025 bins into 3 components in 12 iterations \(" + loss +
                      r"\), divergence ([0-9.e+-]+) -> ([0-9.e+-]+), saved to 'o.npz'", r.output)
        assert m, r.output
        z = np.load(out)
        S = ops.cabs_pow(ops.stft2048_c2c(ops.to_device_f32(x[None])), 1)
        A, C, tr = ops.nmf(S, 3, n_iter=12, beta_loss=loss, seed=5, return_trace=True)
        assert np.array_equal(z["components"], C[0].T.cpu().numpy()) and z["components"].shape == (1025, 3)
        assert np.array_equal(z["activations"], A[0].T.cpu().numpy()) and z["activations"].shape == (3, 17)
        assert np.array_equal(z["divergence"], tr[0, [0, -1]].cpu().numpy()) and str(z["loss"]) == loss
        assert float(m.group(2)) < float(m.group(1))
