"""`dsp griffinlim` through click's runner: its usage errors need no device; the round trip does."""
import re

import numpy as np
import pytest
import scipy.io.wavfile
from click.testing import CliRunner

from sygnals_amd.cli.main import cli


def _wav(path, fs=22050, n=8192):
    from tests import inverse_ref as R
    x = R.tones_noise(n, 0, fs).astype(np.float32)
    scipy.io.wavfile.write(path, fs, x)
    return x


def test_usage_errors(tmp_path):
    wav, out = tmp_path / "a.wav", tmp_path / "o.wav"
    _wav(wav)
    run = CliRunner().invoke
    r = run(cli, ["dsp", "griffinlim", str(wav)])
    assert r.exit_code == 2 and "-o / --output is required" in r.output
    r = run(cli, ["dsp", "griffinlim", str(wav), "-o", str(out), "--n-iter", "-1"])
    assert r.exit_code == 2 and "--n-iter must be non-negative" in r.output
    for m in ("1", "-0.5", "1.5"):
        r = run(cli, ["dsp", "griffinlim", str(wav), "-o", str(out), "--momentum", m])
        assert r.exit_code == 2 and "--momentum must be in [0, 1)" in r.output
    r = run(cli, ["dsp", "griffinlim", str(wav), "-o", str(out), "--from", "cqt"])
    assert r.exit_code == 2
    r = run(cli, ["dsp", "griffinlim", str(wav), "-o", str(out), "--from", "mfcc", "--n-mels", "12"])
    assert r.exit_code == 2 and "--n-mfcc in [1, n_mels]" in r.output
    short = tmp_path / "s.wav"
    _wav(short, n=300)
    r = run(cli, ["dsp", "griffinlim", str(short), "-o", str(out)])
    assert r.exit_code == 2 and "at least 512" in r.output
    assert not out.exists()
    assert "--n-mfcc" in run(cli, ["dsp", "griffinlim", "--help"]).output


@pytest.mark.gpu
def test_round_trip(tmp_path):
    """The command writes what ops.griffinlim returns for the input's magnitudes and the seed, bit for bit, and prints that
    run's last spectral convergence; from mel and MFCC it runs and says what it did."""
    from sygnals_amd import ops
    wav, out = tmp_path / "a.wav", tmp_path / "o.wav"
    x = _wav(wav)
    run = CliRunner().invoke
    r = run(cli, ["dsp", "griffinlim", str(wav), "-o", str(out), "--n-iter", "8", "--seed", "3"])
    assert r.exit_code == 0, r.output
    m = re.search(r"Rebuilt 8192 samples from stft in 8 iterations, spectral convergence ([0-9.]+), saved to 'o.wav'", r.output)
    assert m, r.output
    sc = float(m.group(1))
    fs, y = scipy.io.wavfile.read(out)
    assert fs == 22050 and y.shape == (8192,) and y.dtype == np.int16          # (the package writes 16-bit PCM)
    S = ops.cabs_pow(ops.stft2048_c2c(ops.to_device_f32(x[None])), 1)
    want, trace = ops.griffinlim(S, 8, 0.99, "random", 3, length=8192, return_trace=True)
    pcm = np.round(np.clip(want[0].cpu().numpy().astype(np.float64), -1.0, 1.0) * 32767.0).astype(np.int16)
    assert np.array_equal(y, pcm) and f"{float(trace[0, -1].item()):.6f}" == m.group(1)
    assert 0.0 < sc < float(trace[0, 0].item())                    # eight iterations are below the random start
    r = run(cli, ["dsp", "griffinlim", str(wav), "-o", str(out), "--n-iter", "0", "--from", "mel", "--n-mels", "40"])
    assert r.exit_code == 0 and "from mel in 0 iterations, spectral convergence n/a" in r.output, r.output
    r = run(cli, ["dsp", "griffinlim", str(wav), "-o", str(out), "--n-iter", "2", "--from", "mfcc", "--n-mels", "40"])
    assert r.exit_code == 0 and "from mfcc in 2 iterations" in r.output, r.output
