"""`features fbank`: bad values are usage errors without a device; on the GPU the command's table equals the mirror's."""
import numpy as np
import pytest
import scipy.io.wavfile


def _wav(tmp_path, n=8000, sr=16000):
    wav = tmp_path / "a.wav"
    g = np.random.default_rng(5)
    scipy.io.wavfile.write(wav, sr, (0.1 * g.standard_normal(n)).astype(np.float32))
    return wav


def test_cli_usage_errors(tmp_path):
    import pandas as pd
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    wav = _wav(tmp_path)
    run = CliRunner().invoke
    base = ["features", "fbank", str(wav), "-o", str(tmp_path / "o.csv")]
    for opts, words in ((["--num-mel-bins", "2"], "num_mel_bins = 2 is not served"),
                        (["--num-mel-bins", "300"], "num_mel_bins = 300 is not served"),
                        (["--frame-length", "5"], "frame_length = 5.0 ms at 16000.0 Hz is 80 samples, padded to 128: not served"),
                        (["--frame-length", "200"], "padded to 4096: not served"),
                        (["--frame-shift", "0.01"], "is below one sample"),
                        (["--window-type", "hann"], "window_type = 'hann' is not served"),
                        (["--dither", "-1"], "must be non-negative"),
                        (["--seed", "-3"], "seed must be an integer in [0, 2^64)"),
                        (["--mfcc", "--num-ceps", "0"], "num_ceps = 0 is not served"),
                        (["--mfcc", "--num-ceps", "24"], "num_ceps = 24 is not served at num_mel_bins = 23"),
                        (["--mfcc", "--cepstral-lifter", "-2"], "cepstral_lifter must be non-negative")):
        r = run(cli, base + opts)
        assert r.exit_code == 2 and words in r.output, (opts, r.output)
    (tmp_path / "short").mkdir()
    short = _wav(tmp_path / "short", n=1000)
    r = run(cli, ["features", "fbank", str(short), "-o", str(tmp_path / "o.csv"), "--frame-length", "100"])
    assert r.exit_code == 2 and "is shorter than one frame of 1600 samples" in r.output, r.output
    assert run(cli, base + ["--num-mel-bins", "many"]).exit_code == 2
    series = tmp_path / "s.csv"
    pd.DataFrame({"value": np.arange(50.0)}).to_csv(series, index=False)
    r = run(cli, ["features", "fbank", str(series), "-o", str(tmp_path / "o.csv")])
    assert r.exit_code == 2 and "is not recognized as audio" in r.output
    helptext = run(cli, ["features", "fbank", "--help"]).output
    for opt in ("--num-mel-bins", "--frame-length", "--frame-shift", "--window-type", "--dither", "--no-snip-edges", "--use-energy",
                "--htk-compat", "--subtract-mean", "--mfcc", "--num-ceps", "--cepstral-lifter"):
        assert opt in helptext


@pytest.mark.gpu
def test_cli_round_trip(tmp_path):
    import pandas as pd
    from click.testing import CliRunner
    from sygnals_amd.cli.main import cli
    from sygnals_amd import io as sio
    from sygnals_amd.core.features import kaldi as KF
    from pathlib import Path
    wav = _wav(tmp_path)
    signal, sr = sio.read_data(Path(wav))
    run = CliRunner().invoke
    out = tmp_path / "f.csv"
    r = run(cli, ["features", "fbank", str(wav), "-o", str(out), "--num-mel-bins", "40", "--use-energy", "--no-snip-edges"])
    assert r.exit_code == 0, r.output
    tab = pd.read_csv(out)
    ref = KF.fbank(signal, sample_frequency=float(sr), num_mel_bins=40, use_energy=True, snip_edges=False)
    assert ref.shape == (50, 41) and list(tab.columns) == ["time"] + [f"fbank_{i}" for i in range(41)]
    np.testing.assert_allclose(tab.iloc[:, 1:].to_numpy(), ref, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(tab["time"].to_numpy(), np.arange(50) * 0.01)
    out = tmp_path / "m.npz"
    r = run(cli, ["features", "fbank", str(wav), "-o", str(out), "--mfcc", "--num-ceps", "10", "--htk-compat", "--subtract-mean"])
    assert r.exit_code == 0, r.output
    ref = KF.mfcc(signal, sample_frequency=float(sr), num_ceps=10, htk_compat=True, subtract_mean=True)
    z = np.load(out)
    assert ref.shape == (48, 10)
    np.testing.assert_array_equal(z["mfcc"], ref)
