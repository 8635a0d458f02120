"""`dsp structure` through click's runner: its usage errors need no device; the round trip does."""
import numpy as np
import pytest
import scipy.io.wavfile
from click.testing import CliRunner

from sygnals_amd.cli.main import cli


def _wav(path, fs=22050, n=32768):
    """Four stretches of different tones."""
    t = np.arange(n) / fs
    f = np.repeat([330.0, 880.0, 330.0, 1500.0], n // 4)
    x = (0.4 * np.sin(2 * np.pi * f * t) + 0.01 * np.random.default_rng(0).standard_normal(n)).astype(np.float32)
    scipy.io.wavfile.write(path, fs, x)
    return x


def test_usage_errors(tmp_path):
    wav, out = tmp_path / "a.wav", tmp_path / "s.csv"
    _wav(wav)
    run = CliRunner().invoke
    r = run(cli, ["dsp", "structure", str(wav)])
    assert r.exit_code == 2 and "-k" in r.output
    for k in ("0", "-2"):
        r = run(cli, ["dsp", "structure", str(wav), "-k", k, "-o", str(out)])
        assert r.exit_code == 2 and "-k / --segments must be at least 1" in r.output, r.output
    for w in ("4", "0", "65"):
        r = run(cli, ["dsp", "structure", str(wav), "-k", "3", "--median", w])
        assert r.exit_code == 2 and "--median must be odd and in [1, 63]" in r.output, r.output
    r = run(cli, ["dsp", "structure", str(wav), "-k", "3", "--enhance", "0"])
    assert r.exit_code == 2 and "--enhance must be at least 1" in r.output
    r = run(cli, ["dsp", "structure", str(wav), "-k", "3", "--feature", "cqt"])
    assert r.exit_code == 2
    r = run(cli, ["dsp", "structure", str(wav), "-k", "500"])
    assert r.exit_code == 2 and "the clip has 65 frames" in r.output
    assert not out.exists()
    assert "--enhance" in run(cli, ["dsp", "structure", "--help"]).output


@pytest.mark.gpu
def test_round_trip(tmp_path):
    """The command writes what core.structure.structure_segments returns for the clip."""
    import pandas as pd

    from sygnals_amd.core.structure import structure_segments
    wav, out = tmp_path / "a.wav", tmp_path / "s.csv"
    x = _wav(wav)
    for extra, kw in (([], {}), (["--feature", "chroma", "--enhance", "5", "--median", "3"], dict(feature="chroma", enhance=5, median=3))):
        r = CliRunner().invoke(cli, ["dsp", "structure", str(wav), "-k", "4", "-o", str(out)] + extra)
        assert r.exit_code == 0, r.output
        assert "into 4 segments" in r.output and "saved to 's.csv'" in r.output
        want = structure_segments(x, 22050, 4, **kw)
        tab = pd.read_csv(out)
        assert list(tab.columns) == ["segment", "start_frame", "start_time"]
        assert np.array_equal(tab["start_frame"].to_numpy(), want) and want[0] == 0 and np.all(np.diff(want) > 0)
        assert np.allclose(tab["start_time"].to_numpy(), want * 512.0 / 22050)
