"""tests/loudness_ref.py, the float64 restatement the device meter is held to, is itself held to the standards' known
answers: BS.1770's 48 kHz coefficient table, its 997 Hz calibration tone, EBU Tech 3341's gating cases, Tech 3342's
loudness-range case and Tech 3341's true-peak tolerance.  No device."""
import numpy as np
import pytest
from scipy.signal import sosfreqz

from sygnals_amd import _loudness as LD
from tests import loudness_ref as R


def tone(fs, seconds, dbfs, f=997.0, channels=1):
    n = np.arange(int(round(fs * seconds)))
    x = 10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * f * n / fs)
    return np.tile(x, (channels, 1))


def test_48k_coefficients_are_the_standards_table():
    sos = LD.k_weighting_sos(48000)
    want = [[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
            [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]]
    assert np.max(np.abs(sos - np.array(want))) <= 1e-12
    sos[0, 0] = 0.0                                   # the caller's own copy: the cached design is not touched
    assert abs(LD.k_weighting_sos(48000)[0, 0] - want[0][0]) <= 1e-12


def test_design_at_44100_has_the_48k_gain_at_997_hz():
    g = []
    for fs in (48000, 44100):
        _, h = sosfreqz(LD.k_weighting_sos(fs), worN=[997.0], fs=fs)
        g.append(20 * np.log10(abs(h[0])))
    assert abs(g[1] - g[0]) <= 0.01


@pytest.mark.parametrize("fs", [7999, 384001, 44100.5, "48k", None, True])
def test_rates_outside_the_served_range_are_refused(fs):
    with pytest.raises(ValueError, match="served: integer sampling rates from 8000 to 384000 Hz"):
        LD.k_weighting_sos(fs)


def test_the_refusal_gives_the_chunk_reason_for_low_rates_only():
    for fs, low in ((7999, True), (4000, True), (384001, False), (44100.5, False), ("48k", False)):
        with pytest.raises(ValueError) as e:
            LD.check_fs(fs)
        assert ("a 100 ms segment must span more than one 256-sample chunk" in str(e.value)) == low


def test_full_scale_997_hz_mono_reads_minus_3_01():
    assert abs(R.integrated(tone(48000, 20, 0.0), 48000) - (-3.01)) <= 0.01


def test_tech3341_case1_stereo_tone_at_minus_23_dbfs():
    assert abs(R.integrated(tone(48000, 20, -23.0, channels=2), 48000) - (-23.0)) <= 0.1


def test_tech3341_relative_gate():
    x = np.concatenate([tone(48000, 10, -36.0, channels=2), tone(48000, 60, -23.0, channels=2), tone(48000, 10, -36.0, channels=2)], axis=1)
    assert abs(R.integrated(x, 48000) - (-23.0)) <= 0.1


def test_absolute_gate_drops_a_stretch_at_minus_80_dbfs():
    parts = [tone(48000, 10, -36.0, channels=2), tone(48000, 30, -23.0, channels=2), tone(48000, 20, -80.0, channels=2),
             tone(48000, 30, -23.0, channels=2), tone(48000, 10, -36.0, channels=2)]
    x = np.concatenate(parts, axis=1)
    assert abs(R.integrated(x, 48000) - (-23.0)) <= 0.1
    l = R.momentary(x, 48000)
    assert (l < -70).sum() >= 190            # the quiet stretch's blocks lie under the absolute gate


def test_tech3342_case1_loudness_range():
    x = np.concatenate([tone(48000, 20, -20.0, channels=2), tone(48000, 20, -30.0, channels=2)], axis=1)
    assert abs(R.loudness_range(x, 48000) - 10.0) <= 1.0


def test_true_peak_of_a_quarter_rate_sine_at_45_degrees():
    fs = 48000
    n = np.arange(fs)
    x = np.sin(2 * np.pi * (fs / 4) * n / fs + np.pi / 4)
    assert abs(np.max(np.abs(x)) - 0.7071) < 1e-4
    d = R.dbtp(R.true_peak(x, fs))
    assert -0.4 <= d <= 0.2
    assert [LD.true_peak_up(f) for f in (8000, 95999, 96000, 191999, 192000, 384000)] == [4, 4, 2, 2, 1, 1]


def test_segment_arithmetic():
    s = [LD.segment_start(j, 11025) for j in range(6)]
    assert s == [0, 1102, 2205, 3307, 4410, 5512] and set(np.diff(s)) == {1102, 1103}
    assert [LD.segment_start(j, 44100) for j in range(4)] == [0, 4410, 8820, 13230]
    assert np.array_equal(LD.segment_start(np.arange(4), 44100), [0, 4410, 8820, 13230])
    for fs in (11025, 44100, 8000):
        s4, s30 = LD.segment_start(4, fs), LD.segment_start(30, fs)
        assert LD.n_blocks(s4 - 1, fs, LD.MOMENTARY) == 0 and LD.n_blocks(s4, fs, LD.MOMENTARY) == 1
        assert LD.n_blocks(s30 - 1, fs, LD.SHORT_TERM) == 0 and LD.n_blocks(s30, fs, LD.SHORT_TERM) == 1
        assert LD.n_segments(LD.segment_start(7, fs), fs) in (6, 7)      # s_7 = 7717 at 11 025 Hz holds 6 whole segments
    rng = np.random.default_rng(0)
    x = rng.standard_normal(2 * 11025)
    seg = R.segment_powers(x, 11025)
    assert seg.shape == (1, 20)
    z = R.block_powers(seg, 11025, 4)
    assert z.shape == (17,) and np.isclose(z[1], seg[0, 1:5].sum() / (5512 - 1102))


def test_a_clip_one_sample_short_of_a_block_reads_minus_inf():
    for fs in (48000, 11025):
        x = tone(fs, 1, -20.0)[:, :LD.segment_start(4, fs) - 1]
        assert R.integrated(x, fs) == -np.inf and R.momentary(x, fs).size == 0 and R.loudness_range(x, fs) == 0.0
    assert R.integrated(np.zeros(48000), 48000) == -np.inf
    assert np.all(np.isneginf(R.momentary(np.zeros(48000), 48000)))


def test_channel_weights_and_ranks():
    assert list(LD.channel_weights(2)) == [1, 1] and list(LD.channel_weights(5)) == [1, 1, 1, 1.41, 1.41]
    assert list(LD.channel_weights(4, [1, 1, 0, 2])) == [1, 1, 0, 2]
    for C, w in ((4, None), (6, None), (2, [1.0]), (2, [1.0, -1.0]), (2, [1.0, np.nan])):
        with pytest.raises(ValueError, match="channel"):
            LD.channel_weights(C, w)
    for n in range(2, 400):
        lo, hi = LD.lra_ranks(n)
        assert lo == int(np.floor((n - 1) * 0.10 + 0.5 + 1e-9)) and hi == int(np.floor((n - 1) * 0.95 + 0.5 + 1e-9))


def test_gain_rule():
    assert R.gain(-np.inf, 0.5, -23.0) == 1.0
    assert np.isclose(R.gain(-20.0, 0.5, -23.0), 10 ** (-3 / 20))
    assert np.isclose(R.gain(-30.0, 0.5, -16.0, -1.0) * 0.5, 10 ** (-1 / 20))        # the limit binds
    assert np.isclose(R.gain(-30.0, 0.01, -16.0, -1.0), 10 ** (14 / 20))             # it does not
