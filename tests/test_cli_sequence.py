"""`dsp viterbi` through click's runner: its usage errors need no device; the round trip does."""
import numpy as np
import pytest
from click.testing import CliRunner

from sygnals_amd.cli.main import cli


def _npz(path, S=4, T=50, key="prob"):
    rng = np.random.default_rng(5)
    p = rng.random((S, T)) + 1e-3
    p = (p / p.sum(axis=0)).astype(np.float32)
    np.savez(path, **{key: p})
    return p


def test_usage_errors(tmp_path):
    src, out = tmp_path / "p.npz", tmp_path / "o.npz"
    _npz(src)
    run = CliRunner().invoke
    r = run(cli, ["dsp", "viterbi", str(src)])
    assert r.exit_code == 2 and "--output" in r.output
    for v in ("-0.1", "1.5"):
        r = run(cli, ["dsp", "viterbi", str(src), "-o", str(out), "--self-prob", v])
        assert r.exit_code == 2 and "--self-prob must lie in [0, 1]" in r.output, r.output
    for v in ("0", "-3"):
        r = run(cli, ["dsp", "viterbi", str(src), "-o", str(out), "--transition", "local", "--width", v])
        assert r.exit_code == 2 and "--width must be at least 1" in r.output, r.output
    r = run(cli, ["dsp", "viterbi", str(src), "-o", str(out), "--transition", "local", "--width", "9"])
    assert r.exit_code == 2 and "width=9 must be an integer in [1, 4]" in r.output, r.output
    r = run(cli, ["dsp", "viterbi", str(src), "-o", str(out), "--key", "posterior"])
    assert r.exit_code == 2 and "holds no array 'posterior' (it holds: prob)" in r.output
    for opt, v in (("--kind", "fuzzy"), ("--transition", "banded")):
        assert run(cli, ["dsp", "viterbi", str(src), "-o", str(out), opt, v]).exit_code == 2
    bad = tmp_path / "bad.npz"
    np.savez(bad, prob=np.full((4, 50), 2.0, dtype=np.float32))
    r = run(cli, ["dsp", "viterbi", str(bad), "-o", str(out)])
    assert r.exit_code == 2 and "prob must lie in [0, 1]" in r.output
    np.savez(bad, prob=np.full((4, 50), 0.1, dtype=np.float32))
    r = run(cli, ["dsp", "viterbi", str(bad), "-o", str(out), "--kind", "discriminative"])
    assert r.exit_code == 2 and "sum to 1 over the states" in r.output
    np.savez(bad, prob=np.ones(7, dtype=np.float32))
    r = run(cli, ["dsp", "viterbi", str(bad), "-o", str(out)])
    assert r.exit_code == 2 and "must be a 2-D array" in r.output
    assert not out.exists()
    assert "--self-prob" in run(cli, ["dsp", "viterbi", "--help"]).output


@pytest.mark.gpu
def test_round_trip(tmp_path):
    """The command writes what core.sequence returns for the file's array."""
    import pandas as pd
    from sygnals_amd.core import sequence as SQ
    src, out, table = tmp_path / "p.npz", tmp_path / "o.npz", tmp_path / "o.csv"
    p = _npz(src, key="post")
    r = CliRunner().invoke(cli, ["dsp", "viterbi", str(src), "-o", str(out), "--key", "post", "--kind", "discriminative",
                                 "--transition", "cycle", "--self-prob", "0.8"])
    assert r.exit_code == 0, r.output
    assert "Viterbi path (discriminative, 4 states, 50 frames) saved to 'o.npz'" in r.output
    want, logp = SQ.viterbi_discriminative(p, SQ.transition_cycle(4, 0.8), return_logp=True)
    with np.load(out) as z:
        assert np.array_equal(z["states"], want) and z["states"].dtype == np.uint16 and float(z["logp"]) == logp
    r = CliRunner().invoke(cli, ["dsp", "viterbi", str(src), "-o", str(table), "--key", "post", "--kind", "binary"])
    assert r.exit_code == 0, r.output
    df = pd.read_csv(table)
    wb = SQ.viterbi_binary(p, SQ.transition_loop(2, 0.9))
    assert list(df.columns) == ["frame"] + [f"state_{l}" for l in range(4)] and np.array_equal(df["frame"], np.arange(50))
    assert all(np.array_equal(df[f"state_{l}"], wb[l]) for l in range(4))
