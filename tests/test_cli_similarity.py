"""`dsp separate-repeating` through click's runner: its usage errors need no device; the round trip does."""
import numpy as np
import pytest
import scipy.io.wavfile
from click.testing import CliRunner

from sygnals_amd.cli.main import cli


def _wav(path, fs=22050, n=16384):
    t = np.arange(n) / fs
    x = (0.4 * np.sin(2 * np.pi * 330 * t) * (np.sin(2 * np.pi * 4 * t) > 0) + 0.2 * np.sin(2 * np.pi * (900 + 400 * t) * t)
         + 0.01 * np.random.default_rng(0).standard_normal(n)).astype(np.float32)
    scipy.io.wavfile.write(path, fs, x)
    return x


def test_usage_errors(tmp_path):
    wav, out = tmp_path / "a.wav", tmp_path / "bg.wav"
    _wav(wav)
    run = CliRunner().invoke
    r = run(cli, ["dsp", "separate-repeating", str(wav)])
    assert r.exit_code == 2 and "-o / --output is required" in r.output
    for opt in ("--width-seconds", "--margin-background", "--margin-foreground", "--power"):
        for v in ("0", "-1.5"):
            r = run(cli, ["dsp", "separate-repeating", str(wav), "-o", str(out), opt, v])
            assert r.exit_code == 2 and f"{opt} must be positive" in r.output, r.output
    r = run(cli, ["dsp", "separate-repeating", str(wav), "-o", str(out), "--metric", "cityblock"])
    assert r.exit_code == 2
    assert not out.exists()
    assert "--margin-foreground" in run(cli, ["dsp", "separate-repeating", "--help"]).output


@pytest.mark.gpu
def test_round_trip(tmp_path):
    """The command writes what core.decompose.separate_repeating returns for the clip, bit for bit."""
    from sygnals_amd.core.decompose import separate_repeating
    wav, bg, fg = tmp_path / "a.wav", tmp_path / "bg.wav", tmp_path / "fg.wav"
    x = _wav(wav)
    r = CliRunner().invoke(cli, ["dsp", "separate-repeating", str(wav), "-o", str(bg), "--foreground", str(fg), "--width-seconds",
                                 "0.1", "--margin-background", "3", "--power", "1"])
    assert r.exit_code == 0, r.output
    assert "frames at least 4 apart" in r.output and "background saved to 'bg.wav', foreground to 'fg.wav'" in r.output
    wf, wb = separate_repeating(x, 22050, width_seconds=0.1, margin_background=3.0, power=1.0)
    for path, want in ((bg, wb), (fg, wf)):
        fs, got = scipy.io.wavfile.read(path)
        assert fs == 22050 and got.shape == want.shape
        assert np.array_equal(got, want) if got.dtype == np.float32 else np.max(np.abs(got / 32768.0 - want)) <= 2.0 / 32768
    assert np.max(np.abs(wf + wb)) > 0
