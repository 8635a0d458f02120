"""Click commands of the device backend.

`features extract` keeps the option surface of sygnals/cli/features_cmd.py:30-113
(-o/--output, repeatable -f/--feature incl. 'all', --frame-length 2048, --hop-length 512;
.csv -> DataFrame, .npz -> dict of arrays; ValueError -> click.UsageError).  The `dsp` and
`filter` groups follow the surface documented in the reference's README.md:483-533, 704-900 --
in the reference snapshot those groups are commented out (sygnals/cli/main.py:29-33, 115-119), so
they are provided here rather than kept.  The `augment` group keeps the option names of
sygnals/cli/augment_cmd.py (add-noise: --snr, --noise-type, --seed; time-stretch: --rate; -o/--output), to which add-noise
adds --generator host|device and --exponent (the device noise generator; the default, host, is the reference's draw);
pitch-shift is not offered; spec-augment (time warp, frequency and time masks on the tables `features extract` writes) is
this package's own.  Run stand-alone as `python -m sygnals_amd.cli.main ...`
or attach the features / dsp / filter groups to the reference CLI through the plugin (register_cli_commands); `augment`
is not attached there: the reference CLI already owns a group of that name.
"""
from __future__ import annotations

import logging
from pathlib import Path

import click
import numpy as np
import pandas as pd

from .. import io as sio

logger = logging.getLogger(__name__)


@click.group("sygnals-amd")
def cli():
    """MI355X backend for the sygnals feature-extraction hot path."""


# ---------------------------------------------------------------- features
@click.group("features")
def features_cmd():
    """Extract, transform, and manage signal features."""


@features_cmd.command("extract")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False, resolve_path=True))
@click.option("-o", "--output", type=click.Path(resolve_path=True), required=True,
              help="Output file path for extracted features (e.g., features.csv, features.npz).")
@click.option("-f", "--feature", "features", multiple=True, required=True,
              help="Feature(s) to extract (e.g., 'spectral_centroid', 'mfcc'). Use 'all'. Can be repeated.")
@click.option("--frame-length", type=int, default=2048, show_default=True, help="Analysis frame length (samples).")
@click.option("--hop-length", type=int, default=512, show_default=True, help="Hop length between frames (samples).")
def features_extract(input_file, output, features, frame_length, hop_length):
    """Extract features from an audio signal."""
    from ..core.features.manager import extract_features
    input_path, output_path = Path(input_file), Path(output)
    feature_list = list(features)
    if len(feature_list) == 1 and feature_list[0].lower() == "all":
        feature_list = ["all"]
    try:
        res = sio.read_data(input_path)
        if not isinstance(res, tuple) or len(res) != 2:
            raise click.UsageError(f"Input file '{input_path.name}' is not recognized as audio.")
        signal, sr = res
        if signal.ndim != 1:
            logger.warning("Input audio is multi-channel. Converting to mono by averaging for feature extraction.")
            signal = np.mean(signal, axis=0)
        fmt = "dict_of_arrays" if output_path.suffix.lower() == ".npz" else "dataframe"
        out = extract_features(y=signal, sr=sr, features=feature_list, frame_length=frame_length,
                               hop_length=hop_length, output_format=fmt)
        if (isinstance(out, pd.DataFrame) and out.empty) or (isinstance(out, dict) and
                                                             not any(k != "time" for k in out)):
            click.echo("Warning: No features extracted or signal too short.")
            return
        sio.save_data(out, output_path)
        click.echo(f"Successfully extracted features from '{input_path.name}' and saved to '{output_path.name}'.")
    except FileNotFoundError:
        raise click.UsageError(f"Input file not found: {input_path}")
    except ValueError as e:
        raise click.UsageError(f"Error during feature extraction: {e}")


def _post_rows(data):
    """A table or dict that `features extract` wrote -> (time or None, names, [K, T] float32); every column but `time`."""
    if isinstance(data, pd.DataFrame):
        cols = {c: data[c].to_numpy() for c in data.columns}
    elif isinstance(data, dict):
        cols = {}
        for k, v in data.items():
            v = np.asarray(v)
            if v.ndim == 2 and k != "time":
                cols.update({f"{k}_{i}": v[i] for i in range(v.shape[0])})
            else:
                cols[k] = v
    else:
        raise click.UsageError("Input must be a table (.csv) or an .npz that `features extract` wrote.")
    time = cols.pop("time", None)
    names = [k for k, v in cols.items() if np.ndim(v) == 1 and np.issubdtype(np.asarray(v).dtype, np.number)]
    if not names:
        raise click.UsageError("The input holds no feature columns (every numeric column but `time` is a row).")
    if len({len(cols[k]) for k in names}) != 1:
        raise click.UsageError("The feature columns have different lengths.")
    return time, names, np.stack([np.asarray(cols[k], dtype=np.float32) for k in names])


@features_cmd.command("post")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False, resolve_path=True))
@click.option("-o", "--output", type=click.Path(resolve_path=True), required=True,
              help="Output file path (same layout as the input: .csv or .npz).")
@click.option("--cmvn", type=click.Choice(["global", "sliding"]), default=None, help="Per-utterance mean / variance normalisation.")
@click.option("--cmvn-window", type=int, default=600, show_default=True, help="Frames of the sliding CMVN window.")
@click.option("--no-variance", is_flag=True, help="Subtract the mean only.")
@click.option("--deltas", type=click.IntRange(0, 2), default=0, show_default=True, help="Append delta (1) and delta-delta (2).")
@click.option("--width", type=int, default=9, show_default=True, help="Frames of the delta filter (odd, at least 3).")
@click.option("--mode", default="interp", show_default=True, help="Edge mode of the delta filter.")
@click.option("--stack", type=int, default=None, help="Context stacking: copies of every row (n_steps).")
@click.option("--delay", type=int, default=1, show_default=True, help="Frames between stacked copies (non-zero, either sign).")
def features_post(input_file, output, cmvn, cmvn_window, no_variance, deltas, width, mode, stack, delay):
    """Normalise (CMVN), append deltas and stack context on extracted features."""
    from ..core.features import dynamics as DN
    time, names, x = _post_rows(sio.read_data(Path(input_file)))
    T = x.shape[1]
    if deltas and mode == "interp" and T < width:
        raise click.UsageError(f"--mode interp needs at least --width frames: the input has {T} frames and --width is {width} "
                               "(give a smaller --width or another --mode).")
    if cmvn == "sliding" and cmvn_window < 1:
        raise click.UsageError("--cmvn-window must be at least 1.")
    try:
        if stack is not None:
            from .. import _dynamics as DY
            DY.check_stack(stack, delay, "--stack / --delay")
        window = None if cmvn is None else ("global" if cmvn == "global" else cmvn_window)
        y = DN.feature_post_batch(x[None], cmvn=window, variance=not no_variance, deltas=deltas, width=width, mode=mode)
        out_names = [n + suffix for suffix in ("", "_delta", "_delta2")[:deltas + 1] for n in names]
        if stack is not None:
            y = DN.stack_memory_batch(y, stack, delay)
            out_names = out_names + [f"{n}_m{i}" for i in range(1, stack) for n in out_names]
        y = y[0].cpu().numpy()
    except ValueError as e:
        raise click.UsageError(str(e))
    out = {} if time is None else {"time": np.asarray(time)}
    out.update({n: y[i] for i, n in enumerate(out_names)})
    sio.save_data(out if Path(output).suffix.lower() == ".npz" else pd.DataFrame(out), Path(output))
    click.echo(f"Post-processed {len(names)} feature rows x {T} frames into {len(out_names)} rows, saved to '{Path(output).name}'.")


@features_cmd.command("chroma")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False, resolve_path=True))
@click.option("-o", "--output", type=click.Path(resolve_path=True), required=True,
              help="Output file path (.npz: time, the matrix and tuning; any other suffix: a table time, chroma_0 ...).")
@click.option("--kind", type=click.Choice(["stft", "cqt", "cens", "tonnetz"]), default="stft", show_default=True,
              help="chroma_stft, chroma_cqt, chroma_cens or tonnetz.")
@click.option("--tuning", default="auto", show_default=True, help="Deviation from A440 in fractions of a bin, or auto (estimated).")
@click.option("--hop-length", type=int, default=512, show_default=True, help="Hop length between frames (samples).")
@click.option("--norm", type=click.Choice(["inf", "1", "2", "none"]), default=None,
              help="Per-frame norm (default: inf; 2 for cens; tonnetz: the norm of its chroma).")
def features_chroma(input_file, output, kind, tuning, hop_length, norm):
    """Chroma (STFT, CQT, CENS) or tonnetz features of an audio signal."""
    from ..core.features import tonal as TN
    if tuning.strip().lower() == "auto":
        tun = None
    else:
        try:
            tun = float(tuning)
        except ValueError:
            raise click.UsageError(f"--tuning: cannot read '{tuning}' as a number (write e.g. 0.12, or auto).")
    if hop_length < 1:
        raise click.UsageError("--hop-length must be at least 1.")
    nrm = {None: 2 if kind == "cens" else np.inf, "inf": np.inf, "1": 1, "2": 2, "none": None}[norm]
    res = sio.read_data(Path(input_file))
    if not isinstance(res, tuple) or len(res) != 2 or not res[1]:
        raise click.UsageError(f"Input file '{Path(input_file).name}' is not recognized as audio.")
    signal, sr = res
    if signal.ndim != 1:
        signal = np.mean(signal, axis=0)
    try:
        y = signal[None, :]
        if kind == "stft":
            m, t = TN.chroma_stft_batch(y, sr, norm=nrm, hop_length=hop_length, tuning=tun, return_tuning=True)
        elif kind == "cqt":
            m, t = TN.chroma_cqt_batch(y, sr, hop_length=hop_length, norm=nrm, tuning=tun, return_tuning=True)
        elif kind == "cens":
            m, t = TN.chroma_cens_batch(y, sr, hop_length=hop_length, norm=nrm, tuning=tun, return_tuning=True)
        else:
            m, t = TN.tonnetz_batch(y, sr, hop_length=hop_length, norm=nrm, tuning=tun, return_tuning=True)
        tun = float(t[0])                            # the estimate where --tuning is auto
        m = m[0].cpu().numpy()
    except ValueError as e:
        raise click.UsageError(str(e))
    name = "tonnetz" if kind == "tonnetz" else "chroma"
    time = np.arange(m.shape[1]) * hop_length / float(sr)
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"time": time, name: m, "tuning": np.array(tun)}, Path(output))
    else:
        table = {"time": time}
        table.update({f"{name}_{i}": m[i] for i in range(m.shape[0])})
        sio.save_data(pd.DataFrame(table), Path(output))
    click.echo(f"{name} ({kind}: {m.shape[0]} rows x {m.shape[1]} frames, tuning {tun:+.2f}) saved to '{Path(output).name}'.")


@features_cmd.command("pcen")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False, resolve_path=True))
@click.option("-o", "--output", type=click.Path(resolve_path=True), required=True,
              help="Output file path (.npz: time and the matrix; any other suffix: a table time, pcen_0 ...).")
@click.option("--n-mels", type=int, default=128, show_default=True, help="Mel bands.")
@click.option("--n-fft", type=int, default=2048, show_default=True, help="Analysis frame length (samples).")
@click.option("--hop-length", type=int, default=512, show_default=True, help="Hop length between frames (samples).")
@click.option("--gain", type=float, default=0.98, show_default=True, help="Gain of the smoother (alpha), non-negative.")
@click.option("--bias", type=float, default=2.0, show_default=True, help="Bias (delta), non-negative.")
@click.option("--power", type=float, default=0.5, show_default=True, help="Compression exponent (r), non-negative.")
@click.option("--time-constant", type=float, default=0.4, show_default=True, help="Time constant of the smoother (seconds).")
@click.option("--eps", type=float, default=1e-6, show_default=True, help="Stabiliser, strictly positive.")
@click.option("--max-size", type=int, default=1, show_default=True, help="Bands of the running maximum the smoother follows.")
@click.option("--scale", type=float, default=float(2 ** 31), show_default=True, help="Factor on the magnitude mel block.")
def features_pcen(input_file, output, n_mels, n_fft, hop_length, gain, bias, power, time_constant, eps, max_size, scale):
    """PCEN (per-channel energy normalisation) of the mel spectrogram of an audio signal."""
    from .. import _pcen as PC
    from ..core.features import pcen as PN
    if n_mels < 1:
        raise click.UsageError("--n-mels must be at least 1.")
    if n_fft < 2:
        raise click.UsageError("--n-fft must be at least 2.")
    if hop_length < 1:
        raise click.UsageError("--hop-length must be at least 1.")
    try:
        PC.check_params(n_mels, gain, bias, power, eps, 1.0, "features pcen")
        PC.check_max_size(max_size, n_mels, "features pcen")
        PC.check_scale(scale, "features pcen")
        if not time_constant > 0:
            raise ValueError("features pcen: --time-constant must be strictly positive.")
    except ValueError as e:
        raise click.UsageError(str(e))
    res = sio.read_data(Path(input_file))
    if not isinstance(res, tuple) or len(res) != 2 or not res[1]:
        raise click.UsageError(f"Input file '{Path(input_file).name}' is not recognized as audio.")
    signal, sr = res
    if signal.ndim != 1:
        signal = np.mean(signal, axis=0)
    try:
        m = PN.pcen_mel_batch(signal[None, :], sr, n_fft=n_fft, hop=hop_length, n_mels=n_mels, scale=scale, gain=gain, bias=bias,
                              power=power, time_constant=time_constant, eps=eps, max_size=max_size)[0].cpu().numpy()
    except ValueError as e:
        raise click.UsageError(str(e))
    time = np.arange(m.shape[1]) * hop_length / float(sr)
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"time": time, "pcen": m}, Path(output))
    else:
        table = {"time": time}
        table.update({f"pcen_{i}": m[i] for i in range(m.shape[0])})
        sio.save_data(pd.DataFrame(table), Path(output))
    click.echo(f"pcen ({m.shape[0]} bands x {m.shape[1]} frames) saved to '{Path(output).name}'.")


@features_cmd.command("fbank")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False, resolve_path=True))
@click.option("-o", "--output", type=click.Path(resolve_path=True), required=True,
              help="Output file path (.npz: time and the matrix; any other suffix: a table time, fbank_0 ... or mfcc_0 ...).")
@click.option("--num-mel-bins", type=int, default=23, show_default=True, help="Mel bands (3 ... 256).")
@click.option("--frame-length", type=float, default=25.0, show_default=True, help="Window length (milliseconds).")
@click.option("--frame-shift", type=float, default=10.0, show_default=True, help="Shift between frames (milliseconds).")
@click.option("--window-type", default="povey", show_default=True, help="hamming, hanning, povey, rectangular or blackman.")
@click.option("--dither", type=float, default=0.0, show_default=True, help="Dither (standard deviations of added noise).")
@click.option("--seed", type=int, default=0, show_default=True, help="Seed of the dither.")
@click.option("--no-snip-edges", is_flag=True, help="Frames centred on multiples of the shift, the clip reflected at its ends.")
@click.option("--use-energy", is_flag=True, help="Add the log-energy column (fbank) or put it in place of coefficient 0 (MFCC).")
@click.option("--htk-compat", is_flag=True, help="HTK's column order: the energy / coefficient 0 last.")
@click.option("--subtract-mean", is_flag=True, help="Subtract each column's mean over the frames.")
@click.option("--mfcc", "as_mfcc", is_flag=True, help="Write MFCCs instead of the log filterbank.")
@click.option("--num-ceps", type=int, default=13, show_default=True, help="Cepstral coefficients (with --mfcc).")
@click.option("--cepstral-lifter", type=float, default=22.0, show_default=True, help="Kaldi's lifter (with --mfcc; 0: none).")
def features_fbank(input_file, output, num_mel_bins, frame_length, frame_shift, window_type, dither, seed, no_snip_edges,
                   use_energy, htk_compat, subtract_mean, as_mfcc, num_ceps, cepstral_lifter):
    """Kaldi-compatible log mel filterbank energies (or MFCCs) of an audio signal."""
    from .. import _kaldi as KD
    from ..core.features import kaldi as KF
    res = sio.read_data(Path(input_file))
    if not isinstance(res, tuple) or len(res) != 2 or not res[1]:
        raise click.UsageError(f"Input file '{Path(input_file).name}' is not recognized as audio.")
    signal, sr = res
    if signal.ndim != 1:
        signal = np.mean(signal, axis=0)
    kw = dict(num_mel_bins=num_mel_bins, frame_length=frame_length, frame_shift=frame_shift, window_type=window_type,
              dither=dither, snip_edges=not no_snip_edges, use_energy=use_energy, htk_compat=htk_compat,
              subtract_mean=subtract_mean)
    if as_mfcc:
        kw.update(num_ceps=num_ceps, cepstral_lifter=cepstral_lifter)
    who = "features fbank"
    try:
        spec = KD.check(who, as_mfcc, float(sr), kw)
        KD.check_seed(who, seed)
        if KD.frames_of(spec, signal.shape[0]) < 1:
            raise ValueError(f"{who}: the input ({signal.shape[0]} samples) is shorter than one frame of {spec.wl} samples.")
        m = (KF.mfcc if as_mfcc else KF.fbank)(signal, sample_frequency=float(sr), seed=seed, **kw)
    except ValueError as e:
        raise click.UsageError(str(e))
    name = "mfcc" if as_mfcc else "fbank"
    time = np.arange(m.shape[0]) * spec.hop / float(sr)
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"time": time, name: m}, Path(output))
    else:
        table = {"time": time}
        table.update({f"{name}_{i}": m[:, i] for i in range(m.shape[1])})
        sio.save_data(pd.DataFrame(table), Path(output))
    click.echo(f"{name} ({m.shape[0]} frames x {m.shape[1]} columns) saved to '{Path(output).name}'.")


# ---------------------------------------------------------------- dsp
@click.group("dsp")
def dsp_cmd():
    """Perform core Digital Signal Processing (DSP) operations."""


def _load_signal(path, fs):
    x, sr = sio.signal_from(sio.read_data(path))
    if x.ndim != 1:
        x = np.mean(x, axis=0)
    return x, (fs if fs is not None else sr)


@dsp_cmd.command("fft")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--fs", type=float, required=True, help="Sampling frequency (Hz).")
@click.option("--window", default="hann", show_default=True)
@click.option("--n", type=int, default=None, help="FFT length. Defaults to signal length.")
def dsp_fft(input_file, output, fs, window, n):
    """Compute the Fast Fourier Transform (FFT)."""
    from ..core.dsp import compute_fft
    try:
        x, _ = _load_signal(input_file, fs)
        freqs, spec = compute_fft(x, fs=fs, n=n, window=window if window and window.lower() != "none" else None)
    except ValueError as e:
        raise click.UsageError(str(e))
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"frequencies": freqs, "spectrum": spec, "fs": np.array(fs)}, output)
    else:
        sio.save_data(pd.DataFrame({"Frequency": freqs, "Magnitude": np.abs(spec), "Phase": np.angle(spec)}), output)
    click.echo(f"FFT saved to '{Path(output).name}'.")


@dsp_cmd.command("ifft")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--n", type=int, default=None, help="Length of the output signal.")
def dsp_ifft(input_file, output, n):
    """Compute the Inverse Fast Fourier Transform (IFFT)."""
    from ..core.dsp import compute_ifft
    res = sio.read_data(input_file)
    if isinstance(res, dict) and "spectrum" in res:
        spec = np.asarray(res["spectrum"])
    elif isinstance(res, pd.DataFrame) and {"Magnitude", "Phase"} <= set(res.columns):
        spec = res["Magnitude"].to_numpy() * np.exp(1j * res["Phase"].to_numpy())
    else:
        raise click.UsageError("Input must be an NPZ with 'spectrum' or a CSV with Magnitude and Phase columns.")
    try:
        x = compute_ifft(spec, n=n)
    except ValueError as e:
        raise click.UsageError(str(e))
    sio.save_data(x, output)
    click.echo(f"IFFT saved to '{Path(output).name}'.")


@dsp_cmd.command("psd-welch")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--fs", type=float, required=True)
@click.option("--window", default="hann", show_default=True)
@click.option("--nperseg", type=int, default=None)
@click.option("--noverlap", type=int, default=None)
@click.option("--nfft", type=int, default=None)
@click.option("--detrend", type=click.Choice(["none", "constant", "linear"]), default="constant", show_default=True)
@click.option("--scaling", type=click.Choice(["density", "spectrum"]), default="density", show_default=True)
def dsp_welch(input_file, output, fs, window, nperseg, noverlap, nfft, detrend, scaling):
    """Estimate Power Spectral Density using Welch's method."""
    from ..core.dsp import compute_psd_welch
    try:
        x, _ = _load_signal(input_file, fs)
        f, p = compute_psd_welch(x, fs=fs, window=window, nperseg=nperseg, noverlap=noverlap, nfft=nfft,
                                 detrend=False if detrend == "none" else detrend, scaling=scaling)
    except ValueError as e:
        raise click.UsageError(str(e))
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"frequencies": f, "psd": p}, output)
    else:
        sio.save_data(pd.DataFrame({"Frequency": f, "PSD": p}), output)
    click.echo(f"Welch PSD saved to '{Path(output).name}'.")


@dsp_cmd.command("psd-periodogram")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--fs", type=float, required=True)
@click.option("--window", default="hann", show_default=True)
@click.option("--nfft", type=int, default=None)
@click.option("--detrend", type=click.Choice(["none", "constant", "linear"]), default="constant", show_default=True)
@click.option("--scaling", type=click.Choice(["density", "spectrum"]), default="density", show_default=True)
def dsp_periodogram(input_file, output, fs, window, nfft, detrend, scaling):
    """Estimate Power Spectral Density using Periodogram."""
    from ..core.dsp import compute_psd_periodogram
    try:
        x, _ = _load_signal(input_file, fs)
        f, p = compute_psd_periodogram(x, fs=fs, window=window, nfft=nfft,
                                       detrend=False if detrend == "none" else detrend, scaling=scaling)
    except ValueError as e:
        raise click.UsageError(str(e))
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"frequencies": f, "psd": p}, output)
    else:
        sio.save_data(pd.DataFrame({"Frequency": f, "PSD": p}), output)
    click.echo(f"Periodogram PSD saved to '{Path(output).name}'.")


def _save_series(y, sr, output):
    if Path(output).suffix.lower() == ".wav":
        if sr is None:
            raise click.UsageError("Writing audio needs a sampling rate; the input file carries none.")
        sio.save_data((y, int(sr)), output)
    else:
        sio.save_data(y, output)


@dsp_cmd.command("convolution")
@click.argument("input_file_1", type=click.Path(exists=True, dir_okay=False))
@click.argument("input_file_2", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--mode", type=click.Choice(["full", "valid", "same"]), default="same", show_default=True)
def dsp_convolution(input_file_1, input_file_2, output, mode):
    """Apply convolution to a 1D signal using a 1D kernel."""
    from ..core.dsp import apply_convolution
    x, sr = _load_signal(input_file_1, None)
    k, _ = _load_signal(input_file_2, None)
    try:
        y = apply_convolution(x, k, mode=mode)
    except ValueError as e:
        raise click.UsageError(str(e))
    _save_series(y, sr if mode == "same" else None, output)
    click.echo(f"Convolution ({mode}) saved to '{Path(output).name}'.")


@dsp_cmd.command("correlation")
@click.argument("input_file_1", type=click.Path(exists=True, dir_okay=False))
@click.argument("input_file_2", type=click.Path(exists=True, dir_okay=False), required=False)
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--mode", type=click.Choice(["full", "valid", "same"]), default="full", show_default=True)
@click.option("--method", type=click.Choice(["auto", "direct", "fft"]), default="auto", show_default=True)
def dsp_correlation(input_file_1, input_file_2, output, mode, method):
    """Compute cross-correlation (two inputs) or autocorrelation (one input)."""
    from ..core.dsp import compute_autocorrelation, compute_correlation
    x, _ = _load_signal(input_file_1, None)
    try:
        if input_file_2 is None:
            y = compute_autocorrelation(x, mode=mode, method=method)
        else:
            y = compute_correlation(x, _load_signal(input_file_2, None)[0], mode=mode, method=method)
    except ValueError as e:
        raise click.UsageError(str(e))
    _save_series(y, None, output)
    click.echo(f"{'Auto' if input_file_2 is None else 'Cross-'}correlation saved to '{Path(output).name}'.")


DTW_FRAME, DTW_HOP, DTW_MFCC = 2048, 512, 13


@dsp_cmd.command("dtw")
@click.argument("input_file_1", type=click.Path(exists=True, dir_okay=False))
@click.argument("input_file_2", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--metric", type=click.Choice(["euclidean", "sqeuclidean", "cityblock", "cosine"]), default="euclidean",
              show_default=True)
@click.option("--subseq", is_flag=True, help="Align the first input to a part of the second.")
@click.option("--on", "on", type=click.Choice(["mfcc", "chroma", "samples"]), default=None,
              help="What is aligned: the MFCC sequences (13 coefficients, frame 2048, hop 512; the default for audio), the "
                   "chroma sequences (chroma_cqt, hop 512, tuning estimated per input) or the raw samples (the default for "
                   "CSV / NPZ series).")
def dsp_dtw(input_file_1, input_file_2, output, metric, subseq, on):
    """Align two signals by dynamic time warping (librosa.sequence.dtw's default steps)."""
    from .. import ops
    from ..core.alignment import dtw
    x, sr_x = _load_signal(input_file_1, None)
    y, sr_y = _load_signal(input_file_2, None)
    if on is None:
        on = "mfcc" if (sr_x and sr_y) else "samples"
    hop = 1
    try:
        if on in ("mfcc", "chroma"):
            if not sr_x or not sr_y:
                raise click.UsageError(f"--on {on} needs inputs that carry a sampling rate (audio); use --on samples for a series.")
            if sr_x != sr_y:
                raise click.UsageError(f"The inputs have different sampling rates ({sr_x} Hz and {sr_y} Hz): bring them to one "
                                       "rate with `dsp resample` first.")
            hop = DTW_HOP
            if on == "chroma":
                from ..core.features.tonal import chroma_cqt_batch
                X, Y = (chroma_cqt_batch(ops.to_device_f32(v[None, :]), sr_x, hop_length=DTW_HOP)[0] for v in (x, y))
            else:
                X, Y = (ops.mfcc_batch(ops.to_device_f32(v[None, :]), sr_x, DTW_FRAME, DTW_HOP, n_mfcc=DTW_MFCC)[0] for v in (x, y))
        else:
            X, Y = x, y
        D, wp = dtw(X, Y, metric=metric, subseq=subseq)
    except ValueError as e:
        raise click.UsageError(str(e))
    cost = float(D[wp[0, 0], wp[0, 1]])
    if Path(output).suffix.lower() == ".npz":                        # the path as librosa returns it: end first
        sio.save_data({"path": wp, "cost": np.array(cost), "metric": np.array(metric), "hop_length": np.array(hop)}, output)
    else:                                                            # the table runs in time order
        wp = wp[::-1]
        tx, ty = (wp[:, i] * hop / float(sr) if sr else wp[:, i].astype(np.float64) for i, sr in ((0, sr_x), (1, sr_y)))
        try:
            sio.save_data(pd.DataFrame({"index_x": wp[:, 0], "index_y": wp[:, 1], "time_x": tx, "time_y": ty}), output)
        except ValueError as e:
            raise click.UsageError(str(e))
    click.echo(f"DTW path ({len(wp)} steps) saved to '{Path(output).name}'.")


@dsp_cmd.command("viterbi")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--key", default="prob", show_default=True, help="The array of the NPZ file that holds the probabilities.")
@click.option("--kind", type=click.Choice(["plain", "discriminative", "binary"]), default="plain", show_default=True,
              help="plain: [S, T] likelihoods; discriminative: [S, T] posteriors, each frame summing to 1; binary: [n_labels, T] "
                   "probabilities that each label is active.")
@click.option("--transition", type=click.Choice(["uniform", "loop", "cycle", "local"]), default="loop", show_default=True)
@click.option("--self-prob", "self_prob", type=float, default=0.9, show_default=True,
              help="Probability of staying in a state (loop, cycle).")
@click.option("--width", type=int, default=3, show_default=True, help="Width of the band in states (local).")
def dsp_viterbi(input_file, output, key, kind, transition, self_prob, width):
    """Decode the most likely state sequence of PROB.npz (librosa.sequence.viterbi and its variants).  An NPZ output holds
    `states` and `logp`; any other suffix a table frame, state (one state column per label for --kind binary)."""
    from ..core import sequence as SQ
    if not 0.0 <= self_prob <= 1.0:
        raise click.UsageError(f"--self-prob must lie in [0, 1] (got {self_prob:g}).")
    if width < 1:
        raise click.UsageError(f"--width must be at least 1 (got {width}).")
    res = sio.read_data(input_file)
    if not isinstance(res, dict):
        raise click.UsageError("The input must be an NPZ file that holds the probabilities ([S, T], or [n_labels, T] for --kind binary).")
    if key not in res:
        raise click.UsageError(f"The input holds no array '{key}' (it holds: {', '.join(sorted(res))}); name it with --key.")
    prob = np.asarray(res[key])
    if prob.ndim != 2 or prob.dtype.kind != "f":
        raise click.UsageError(f"'{key}' must be a 2-D array of floating-point probabilities, got shape {prob.shape} of {prob.dtype}.")
    n = 2 if kind == "binary" else prob.shape[0]
    try:
        if transition == "uniform":
            tr = SQ.transition_uniform(n)
        elif transition == "loop":
            tr = SQ.transition_loop(n, self_prob)
        elif transition == "cycle":
            tr = SQ.transition_cycle(n, self_prob)
        else:
            tr = SQ.transition_local(n, width)
        decode = {"plain": SQ.viterbi, "discriminative": SQ.viterbi_discriminative, "binary": SQ.viterbi_binary}[kind]
        states, logp = decode(prob, tr, return_logp=True)
    except ValueError as e:
        raise click.UsageError(str(e))
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"states": states, "logp": np.asarray(logp, dtype=np.float64)}, output)
    else:
        cols = {"frame": np.arange(prob.shape[1])}
        if kind == "binary":
            cols.update({f"state_{l}": states[l] for l in range(states.shape[0])})
        else:
            cols["state"] = states
        try:
            sio.save_data(pd.DataFrame(cols), output)
        except ValueError as e:
            raise click.UsageError(str(e))
    click.echo(f"Viterbi path ({kind}, {n} states, {prob.shape[1]} frames) saved to '{Path(output).name}'.")


def _load_pair(input_file_1, input_file_2, fs):
    """Two signals of ONE sampling rate: --fs when given, else the rate the files carry (both, and equal) or none."""
    x, sr_x = _load_signal(input_file_1, None)
    y, sr_y = _load_signal(input_file_2, None)
    if fs is None and sr_x and sr_y and sr_x != sr_y:
        raise click.UsageError(f"The inputs have different sampling rates ({sr_x} Hz and {sr_y} Hz): bring them to one "
                               "rate with `dsp resample` first.")
    return x, y, (fs if fs is not None else (sr_x or sr_y))


def _welch_options(f):
    for opt in (click.option("--scaling", type=click.Choice(["density", "spectrum"]), default="density", show_default=True),
                click.option("--detrend", type=click.Choice(["none", "constant", "linear"]), default="constant", show_default=True),
                click.option("--nfft", type=int, default=None),
                click.option("--noverlap", type=int, default=None),
                click.option("--nperseg", type=int, default=None),
                click.option("--window", default="hann", show_default=True),
                click.option("--fs", type=float, default=None, help="Sampling frequency (Hz); default: the files' own, else 1."),
                click.option("-o", "--output", required=True, type=click.Path()),
                click.argument("input_file_2", type=click.Path(exists=True, dir_okay=False)),
                click.argument("input_file_1", type=click.Path(exists=True, dir_okay=False))):
        f = opt(f)
    return f


@dsp_cmd.command("csd")
@_welch_options
def dsp_csd(input_file_1, input_file_2, output, fs, window, nperseg, noverlap, nfft, detrend, scaling):
    """Estimate the cross-spectral density of two signals (Welch's method, scipy.signal.csd)."""
    from ..core.dsp import compute_csd
    x, y, fs = _load_pair(input_file_1, input_file_2, fs)
    try:
        f, p = compute_csd(x, y, fs=fs or 1.0, window=window, nperseg=nperseg, noverlap=noverlap, nfft=nfft,
                           detrend=False if detrend == "none" else detrend, scaling=scaling)
    except ValueError as e:
        raise click.UsageError(str(e))
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"frequencies": f, "csd": p}, output)
    else:
        sio.save_data(pd.DataFrame({"Frequency (Hz)": f, "Real": p.real, "Imag": p.imag, "Magnitude": np.abs(p),
                                    "Phase": np.angle(p)}), output)
    click.echo(f"Cross-spectral density saved to '{Path(output).name}'.")


@dsp_cmd.command("coherence")
@_welch_options
def dsp_coherence(input_file_1, input_file_2, output, fs, window, nperseg, noverlap, nfft, detrend, scaling):
    """Estimate the magnitude-squared coherence of two signals (scipy.signal.coherence; --scaling has no effect on it)."""
    from ..core.dsp import compute_coherence
    x, y, fs = _load_pair(input_file_1, input_file_2, fs)
    try:
        f, c = compute_coherence(x, y, fs=fs or 1.0, window=window, nperseg=nperseg, noverlap=noverlap, nfft=nfft,
                                 detrend=False if detrend == "none" else detrend)
    except ValueError as e:
        raise click.UsageError(str(e))
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"frequencies": f, "coherence": c}, output)
    else:
        sio.save_data(pd.DataFrame({"Frequency (Hz)": f, "Coherence": c}), output)
    click.echo(f"Coherence saved to '{Path(output).name}'.")


@dsp_cmd.command("delay")
@click.argument("input_file_1", type=click.Path(exists=True, dir_okay=False))
@click.argument("input_file_2", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--fs", type=float, default=None, help="Sampling frequency (Hz); default: the files' own, else 1.")
@click.option("--max-lag", type=int, default=None, help="Largest lag searched, in samples.")
@click.option("--max-delay", type=float, default=None, help="Largest delay searched, in seconds.")
@click.option("--weighting", type=click.Choice(["none", "phat"]), default="phat", show_default=True)
def dsp_delay(input_file_1, input_file_2, output, fs, max_lag, max_delay, weighting):
    """Estimate the delay of the first signal against the second (generalised cross-correlation)."""
    from ..core.alignment import estimate_delay
    if max_lag is not None and max_delay is not None:
        raise click.UsageError("--max-lag and --max-delay cannot be combined: give one of them.")
    x, y, fs = _load_pair(input_file_1, input_file_2, fs)
    fs = fs or 1.0
    if max_delay is not None:
        if not (max_delay >= 0):
            raise click.UsageError("--max-delay must be at least 0 seconds.")
        max_lag = int(np.floor(max_delay * fs + 1e-9))
    try:
        delay, lag, peak = estimate_delay(x, y, fs=fs, max_lag=max_lag, weighting=weighting)
    except ValueError as e:
        raise click.UsageError(str(e))
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"delay_seconds": np.array(delay), "lag": np.array(lag), "peak": np.array(peak), "fs": np.array(fs),
                       "weighting": np.array(weighting)}, output)
    else:
        sio.save_data(pd.DataFrame({"delay_seconds": [delay], "lag": [lag], "peak": [peak]}), output)
    click.echo(f"Delay {delay:.9g} s (lag {lag}) saved to '{Path(output).name}'.")


@dsp_cmd.command("beats")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--hop-length", type=int, default=512, show_default=True)
@click.option("--start-bpm", type=float, default=120.0, show_default=True, help="Centre of the tempo prior.")
@click.option("--tightness", type=float, default=100.0, show_default=True)
@click.option("--no-trim", is_flag=True, help="Keep leading and trailing beats with weak onsets.")
@click.option("--bpm", type=float, default=None, help="Track at this tempo instead of estimating it.")
@click.option("--units", type=click.Choice(["time", "frames", "samples"]), default="time", show_default=True)
def dsp_beats(input_file, output, hop_length, start_bpm, tightness, no_trim, bpm, units):
    """Estimate the tempo and track the beats of an audio file (librosa.beat.beat_track)."""
    from ..core.rhythm import beat_track
    if bpm is not None and not bpm > 0:
        raise click.UsageError("--bpm must be positive.")
    if not tightness > 0:
        raise click.UsageError("--tightness must be positive.")
    if hop_length < 1:
        raise click.UsageError("--hop-length must be positive.")
    x, sr = _load_signal(input_file, None)
    if not sr:
        raise click.UsageError("`dsp beats` needs an input that carries a sampling rate (audio).")
    try:
        tempo, frames = beat_track(x, sr=sr, hop_length=hop_length, start_bpm=start_bpm, tightness=tightness, trim=not no_trim,
                                   bpm=bpm, units="frames")
    except ValueError as e:
        raise click.UsageError(str(e))
    times = frames * hop_length / float(sr)
    beats = {"time": times, "frames": frames, "samples": frames * hop_length}[units]
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"tempo": np.array(tempo), "beats": beats, "hop_length": np.array(hop_length), "units": np.array(units)},
                      output)
    else:
        try:
            sio.save_data(pd.DataFrame({"index": np.arange(len(frames)), "frame": frames, "time": times}), output)
        except ValueError as e:
            raise click.UsageError(str(e))
    click.echo(f"Tempo {tempo:.6g} BPM, {len(frames)} beats saved to '{Path(output).name}'.")


@dsp_cmd.command("hilbert")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
def dsp_hilbert(input_file, output):
    """Compute the Analytic Signal using the Hilbert Transform (output is complex)."""
    from ..core.transforms import hilbert_transform
    x, _ = _load_signal(input_file, None)
    try:
        a = hilbert_transform(x)
    except ValueError as e:
        raise click.UsageError(str(e))
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"analytic_signal": a, "envelope": np.abs(a)}, output)
    else:
        sio.save_data(pd.DataFrame({"Real": a.real, "Imag": a.imag, "Envelope": np.abs(a)}), output)
    click.echo(f"Analytic signal saved to '{Path(output).name}'.")


def parse_s_values(text: str) -> np.ndarray:
    """'1.0,0.5+0.2j' -> complex128 array; each token goes through complex().  A bad or empty token is a usage error."""
    out = []
    for tok in text.split(","):
        try:
            out.append(complex(tok.strip()))
        except ValueError:
            raise click.UsageError(f"--s-values: cannot read '{tok.strip()}' as a complex number (write sigma+omegaj, e.g. 0.5+0.2j).")
    return np.asarray(out, dtype=np.complex128)


@dsp_cmd.command("laplace")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--s-values", "s_values", required=True,
              help="Comma-separated list of complex 's' values (sigma+j*omega), e.g. '0.1+0.5j,1.0'.")
@click.option("--t-step", type=float, default=None, help="Time step between samples (1/fs). Required if the input carries no rate.")
def dsp_laplace(input_file, output, s_values, t_step):
    """Compute the Numerical Laplace Transform for specified s-values."""
    from ..core.transforms import laplace_transform_numerical
    s = parse_s_values(s_values)
    x, sr = _load_signal(input_file, None)
    if t_step is None:
        if not sr:
            raise click.UsageError("--t-step is required: the input file carries no sampling rate.")
        t_step = 1.0 / float(sr)
    try:
        F = laplace_transform_numerical(x, s, t_step)
    except ValueError as e:
        raise click.UsageError(str(e))
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"s_values": s, "laplace": F, "t_step": np.array(t_step)}, output)
    else:
        sio.save_data(pd.DataFrame({"s_real": s.real, "s_imag": s.imag, "Real": F.real, "Imag": F.imag, "Magnitude": np.abs(F)}),
                      output)
    click.echo(f"Laplace transform saved to '{Path(output).name}'.")


def parse_scale_values(text: str) -> np.ndarray:
    """'1,2.5,8' -> float64 array.  A bad or empty token is a usage error."""
    out = []
    for tok in text.split(","):
        try:
            out.append(float(tok.strip()))
        except ValueError:
            raise click.UsageError(f"--scale-values: cannot read '{tok.strip()}' as a number (write e.g. 1,2.5,8).")
    return np.asarray(out, dtype=np.float64)


@dsp_cmd.command("cwt")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--scales", "num_scales", type=int, default=None,
              help="Number of scales, spaced geometrically from 1 to max(2, length / 8).")
@click.option("--scale-values", "scale_values", default=None, help="Comma-separated list of scales, e.g. '1,2,4,8'.")
@click.option("--wavelet", default="morl", show_default=True, help="morl, mexh, gaus1 or cmorB-C (e.g. cmor1.5-1.0).")
@click.option("--magnitude", is_flag=True, help="Save |W| instead of the coefficients.")
@click.option("--stride", type=int, default=1, show_default=True, help="Keep every H-th column of the time axis.")
def dsp_cwt(input_file, output, num_scales, scale_values, wavelet, magnitude, stride):
    """Compute the Continuous Wavelet Transform (a scalogram) over a list of scales."""
    from ..core import transforms as TR
    if (num_scales is None) == (scale_values is None):
        raise click.UsageError("Give exactly one of --scales N and --scale-values 'a,b,...'.")
    if num_scales is not None and num_scales < 1:
        raise click.UsageError("--scales must be at least 1.")
    if stride < 1:
        raise click.UsageError("--stride must be at least 1.")
    x, sr = _load_signal(input_file, None)
    period = 1.0 / float(sr) if sr else 1.0
    try:
        scales = TR.scalogram_scales(num_scales, x.size) if num_scales is not None else parse_scale_values(scale_values)
        W, freqs = TR.continuous_wavelet_transform(x, scales, wavelet, sampling_period=period)
    except ValueError as e:
        raise click.UsageError(str(e))
    W = W[:, ::stride]
    if magnitude:
        W = np.abs(W)
    if Path(output).suffix.lower() == ".npz":
        sio.save_data({"scales": np.asarray(scales, dtype=np.float64), "frequencies": freqs, "coefficients": W,
                       "wavelet": np.array(wavelet)}, output)
    else:
        S, n = W.shape
        cols = {"scale": np.repeat(scales, n), "frequency": np.repeat(freqs, n),
                "time": np.tile(np.arange(n) * stride * period, S)}
        if np.iscomplexobj(W):
            cols.update(real=W.real.ravel(), imag=W.imag.ravel())
        else:
            cols["value"] = W.ravel()
        try:
            sio.save_data(pd.DataFrame(cols), output)
        except ValueError as e:
            raise click.UsageError(str(e))
    click.echo(f"CWT ({W.shape[0]} scales x {W.shape[1]} columns, {wavelet}) saved to '{Path(output).name}'.")


@dsp_cmd.command("cepstrum")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--kind", type=click.Choice(["real", "complex"]), default="real", show_default=True)
@click.option("--n", "n", type=int, default=None, help="Transform length (the input is zero-padded or cut); default: its length.")
@click.option("--frames", is_flag=True, help="The real cepstrum of every frame (a cepstrogram) instead of the whole signal.")
@click.option("--n-fft", "n_fft", type=int, default=2048, show_default=True, help="Frame length (with --frames).")
@click.option("--hop", type=int, default=512, show_default=True, help="Hop between frames (with --frames).")
@click.option("--n-ceps", "n_ceps", type=int, default=None, help="Quefrencies kept per frame (with --frames); default n_fft / 2 + 1.")
def dsp_cepstrum(input_file, output, kind, n, frames, n_fft, hop, n_ceps):
    """Compute the real or complex cepstrum of a signal, or the cepstrogram of its frames."""
    from .. import _cepstrum, ops
    from ..core import dsp as D
    if frames and kind == "complex":
        raise click.UsageError("--frames gives the real cepstrum of every frame: it cannot be combined with --kind complex.")
    if frames and n is not None:
        raise click.UsageError("--n is the whole signal's transform length: with --frames give --n-fft.")
    if n is not None and n < (2 if kind == "complex" else 1):
        raise click.UsageError(f"--n must be at least {2 if kind == 'complex' else 1}.")
    if frames and (n_fft < 2 or hop < 1):
        raise click.UsageError("--n-fft must be at least 2 and --hop at least 1.")
    x, sr = _load_signal(input_file, None)
    unit = 1.0 / float(sr) if sr else 1.0
    cols = {}
    try:
        if frames:
            _cepstrum.check_n_ceps(n_ceps, n_fft)                    # refused before a copy
            c = ops.cepstrogram(ops.to_device_f32(x[None, :]), n_fft, hop, n_ceps=n_ceps)[0].cpu().numpy().astype(np.float64)
        elif kind == "real":
            c = D.real_cepstrum(x, n)
        else:
            c, ndelay = D.complex_cepstrum(x, n)
            cols["ndelay"] = np.array(ndelay)
    except ValueError as e:
        raise click.UsageError(str(e))
    quef = np.arange(c.shape[0]) * unit
    if Path(output).suffix.lower() == ".npz":
        data = {"cepstrum": c, "quefrency": quef, **cols}
        if frames:
            data.update(n_fft=np.array(n_fft), hop_length=np.array(hop))
        sio.save_data(data, output)
    else:
        if frames:
            Q, T = c.shape
            table = {"quefrency": np.repeat(quef, T), "time": np.tile(np.arange(T) * hop * unit, Q), "value": c.ravel()}
        else:
            table = {"quefrency": quef, "value": c}
            if cols:
                table["ndelay"] = np.full(c.shape[0], int(cols["ndelay"]))
        try:
            sio.save_data(pd.DataFrame(table), output)
        except ValueError as e:
            raise click.UsageError(str(e))
    what = f"Cepstrogram ({c.shape[0]} quefrencies x {c.shape[1]} frames)" if frames else f"{kind.capitalize()} cepstrum ({c.shape[0]} points)"
    click.echo(f"{what} saved to '{Path(output).name}'.")


@dsp_cmd.command("lpc")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--order", type=int, required=True, help="Prediction order, 1 ... min(64, N - 2) for N samples (a frame's with --frames).")
@click.option("--method", type=click.Choice(["burg", "autocorr"]), default="burg", show_default=True)
@click.option("--frames", is_flag=True, help="The coefficients of every frame instead of the whole signal.")
@click.option("--frame-length", "frame_length", type=int, default=2048, show_default=True, help="Frame length (with --frames), at most 2048.")
@click.option("--hop", type=int, default=512, show_default=True, help="Hop between frames (with --frames).")
@click.option("--envelope", is_flag=True, help="Also save the all-pole spectral envelope in dB.")
@click.option("--n-fft", "n_fft", type=int, default=2048, show_default=True, help="Points of the envelope's frequency grid (with --envelope).")
def dsp_lpc(input_file, output, order, method, frames, frame_length, hop, envelope, n_fft):
    """Compute linear prediction coefficients (LPC) of a signal or of its frames, and their spectral envelope."""
    from .. import _lpc, ops
    try:
        if frames:
            N, hop = _lpc.check_frame(frame_length, hop)
            _lpc.check_order(order, N)                           # refused before the file is read
        if envelope:
            _lpc.check_n_fft(n_fft)
        x, sr = _load_signal(input_file, None)
        if not frames:
            _lpc.check_row(x.size)
            _lpc.check_order(order, x.size)
        y = ops.to_device_f32(np.asarray(x)[None, :])
        if frames:
            a, k, err = ops.lpc_frames(y, order, N, hop, True, method, None, True, True)
        else:
            a, k, err = ops.lpc_rows(y, order, method, None, None, True, True)
            a, k, err = a[:, :, None], k[:, :, None], err[:, None]
        env = ops.lpc_envelope(a, err, n_fft, db=True)[0].cpu().numpy().astype(np.float64) if envelope else None
    except ValueError as e:
        raise click.UsageError(str(e))
    a, k, err = (t[0].cpu().numpy().astype(np.float64) for t in (a, k, err))
    freqs = np.arange(n_fft // 2 + 1) * ((float(sr) if sr else 1.0) / n_fft)
    if not frames:
        a, k, err = a[:, 0], k[:, 0], err[0]
        env = env[:, 0] if envelope else None
    if Path(output).suffix.lower() == ".npz":
        data = {"a": a, "k": k, "err": np.asarray(err), "order": np.array(order), "method": np.array(method)}
        if frames:
            data.update(frame_length=np.array(N), hop_length=np.array(hop))
        if envelope:
            data.update(envelope=env, frequencies=freqs)
        sio.save_data(data, output)
    else:
        T = a.shape[1] if frames else 1
        A2, K2 = a.reshape(order + 1, T), k.reshape(order, T)
        table = {"frame": np.tile(np.arange(T), order + 1), "index": np.repeat(np.arange(order + 1), T), "a": A2.ravel(),
                 "k": np.concatenate([np.full(T, np.nan), K2.ravel()]), "err": np.tile(np.reshape(err, T), order + 1)}
        try:
            sio.save_data(pd.DataFrame(table), output)
        except ValueError as e:
            raise click.UsageError(str(e))
    what = f"LPC (order {order}, {method}, {a.shape[1]} frames)" if frames else f"LPC (order {order}, {method})"
    click.echo(f"{what} saved to '{Path(output).name}'.")


def parse_window_spec(text: str):
    """'kaiser:5.0' -> ('kaiser', 5.0); 'hann' -> 'hann' (firwin's window specification)."""
    name, *params = [t.strip() for t in text.split(":")]
    if not name:
        raise click.UsageError("--window: empty window name (write e.g. kaiser:5.0 or hann).")
    try:
        return (name, *[float(v) for v in params]) if params else name
    except ValueError:
        raise click.UsageError(f"--window: cannot read the parameters of '{text}' as numbers (write e.g. kaiser:5.0).")


@dsp_cmd.command("resample")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--target-sr", "target_sr", type=int, required=True, help="Sampling rate of the output (Hz).")
@click.option("--fs", type=int, default=None, help="Sampling rate of the input (Hz). Required if the input carries no rate.")
@click.option("--window", default="kaiser:5.0", show_default=True, help="Window of the anti-aliasing filter design, name[:param].")
@click.option("--padtype", default="constant", show_default=True, help="How the signal is extended past its ends.")
def dsp_resample(input_file, output, target_sr, fs, window, padtype):
    """Resample a signal to another sampling rate (polyphase, scipy.signal.resample_poly)."""
    from ..core.dsp import resample
    if target_sr <= 0:
        raise click.UsageError("--target-sr must be a positive sampling rate.")
    if fs is not None and fs <= 0:
        raise click.UsageError("--fs must be a positive sampling rate.")
    w = parse_window_spec(window)
    x, sr = _load_signal(input_file, fs)
    if not sr:
        raise click.UsageError("--fs is required: the input file carries no sampling rate.")
    try:
        y = resample(x, sr, target_sr, window=w, padtype=padtype)
    except ValueError as e:
        raise click.UsageError(str(e))
    _save_series(y, target_sr, output)
    click.echo(f"Resampled signal ({sr} Hz -> {target_sr} Hz, {y.size} samples) saved to '{Path(output).name}'.")


@dsp_cmd.command("loudness")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("--fs", type=int, default=None, help="Sampling rate of the input (Hz). Required if the input carries no rate.")
@click.option("--target", type=float, default=None, help="Normalise to this integrated loudness (LUFS) and write -o.")
@click.option("--peak-limit", "peak_limit", type=float, default=None,
              help="With --target: lower the gain so that the true peak stays at or under this level (dBTP).")
@click.option("-o", "--output", default=None, type=click.Path(), help="Where --target writes the normalised signal.")
def dsp_loudness(input_file, fs, target, peak_limit, output):
    """Measure integrated loudness (LUFS), loudness range (LU) and true peak (dBTP) after ITU-R BS.1770 / EBU R128;
    with --target, write the signal normalised to that loudness.  A multi-channel file is mixed down first."""
    from ..core.audio import loudness as LN
    if target is not None and output is None:
        raise click.UsageError("--target needs -o / --output: where to write the normalised signal.")
    if target is None and (output is not None or peak_limit is not None):
        raise click.UsageError("-o / --output and --peak-limit go with --target (without it the command only measures).")
    x, sr = _load_signal(input_file, fs)
    if not sr:
        raise click.UsageError("--fs is required: the input file carries no sampling rate.")
    try:
        m = LN.loudness_metrics(x, sr)
        click.echo(f"I = {m['I']:.2f} LUFS, LRA = {m['LRA']:.2f} LU, TP = {m['TP_dbtp']:.2f} dBTP "
                   f"({np.size(x)} samples at {int(sr)} Hz)")
        if target is not None:
            y = LN.normalize_loudness(x, sr, target, peak_limit)
    except ValueError as e:
        raise click.UsageError(str(e))
    if target is not None:
        _save_series(y, sr, output)
        click.echo(f"Normalised to {target:g} LUFS, saved to '{Path(output).name}'.")


@dsp_cmd.command("griffinlim")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", default=None, type=click.Path(), help="Where the rebuilt clip is written (.wav or a series).")
@click.option("--n-iter", "n_iter", type=int, default=32, show_default=True)
@click.option("--momentum", type=float, default=0.99, show_default=True)
@click.option("--seed", type=int, default=0, show_default=True, help="Seed of the random starting phases.")
@click.option("--from", "source", type=click.Choice(["stft", "mel", "mfcc"]), default="stft", show_default=True,
              help="What the input is reduced to before it is inverted.")
@click.option("--n-mels", "n_mels", type=int, default=128, show_default=True)
@click.option("--n-mfcc", "n_mfcc", type=int, default=13, show_default=True)
@click.option("--fs", type=int, default=None, help="Sampling rate of the input (Hz) if the file carries none.")
def dsp_griffinlim(input_file, output, n_iter, momentum, seed, source, n_mels, n_mfcc, fs):
    """Analyse INPUT (STFT magnitudes, mel power or MFCC; n_fft 2048, hop 512), throw the phases away, rebuild a clip by
    Griffin-Lim and print the final spectral convergence.  From mel and MFCC the magnitudes are the clipped minimum-norm
    inverse of the mel basis (torchaudio's InverseMelScale, not librosa's NNLS)."""
    if output is None:
        raise click.UsageError("-o / --output is required: where to write the rebuilt clip.")
    if n_iter < 0:
        raise click.UsageError(f"--n-iter must be non-negative (got {n_iter}).")
    if not 0 <= momentum < 1:
        raise click.UsageError(f"--momentum must be in [0, 1) (got {momentum:g}).")
    if n_mels < 1 or n_mels > 1025 or n_mfcc < 1 or n_mfcc > n_mels:
        raise click.UsageError(f"--n-mels must be in [1, 1025] and --n-mfcc in [1, n_mels] (got {n_mels}, {n_mfcc}).")
    x, sr = _load_signal(input_file, fs)
    if source != "stft" and not sr:
        raise click.UsageError("--fs is required: the input file carries no sampling rate.")
    if np.size(x) < 512:
        raise click.UsageError(f"The input has {np.size(x)} samples; at least 512 (two frames) are needed.")
    from .. import ops
    try:
        y = ops.to_device_f32(np.asarray(x, dtype=np.float32)[None])
        L = int(y.shape[1])
        D = ops.stft2048_c2c(y)
        S = ops.cabs_pow(D, 1)
        if source != "stft":
            mel = ops.mel_dense(ops.cabs_pow(D, 2), ops._dev(ops.T.mel_filterbank(float(sr), 2048, n_mels)))
            if source == "mfcc":
                mel = ops.mfcc_to_mel(ops.mel_mfcc(mel, n_mfcc, top_db=None, ref=1.0), n_mels)
            S = ops.mel_to_stft(mel, float(sr))
        out, trace = ops.griffinlim(S, n_iter, momentum, "random", seed, length=L, return_trace=True)
    except ValueError as e:
        raise click.UsageError(str(e))
    _save_series(out[0].cpu().numpy(), sr, output)
    sc = f"{float(trace[0, -1].item()):.6f}" if n_iter else "n/a (no iteration)"
    click.echo(f"Rebuilt {L} samples from {source} in {n_iter} iterations, spectral convergence {sc}, "
               f"saved to '{Path(output).name}'.")


@dsp_cmd.command("decompose")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", default=None, type=click.Path(), help="Where components and activations are written (.npz).")
@click.option("--components", "n_components", type=int, default=8, show_default=True)
@click.option("--iterations", "n_iter", type=int, default=200, show_default=True)
@click.option("--loss", type=click.Choice(["frobenius", "kullback-leibler"]), default="frobenius", show_default=True)
@click.option("--seed", type=int, default=0, show_default=True, help="Seed of the random starting factors.")
def dsp_decompose(input_file, output, n_components, n_iter, loss, seed):
    """Factor the STFT magnitudes of INPUT (n_fft 2048, hop 512) into spectral components [1025, K] and their activations
    [K, T] by multiplicative-update NMF, and print the divergence before and after."""
    if output is None:
        raise click.UsageError("-o / --output is required: where to write components and activations (.npz).")
    if Path(output).suffix.lower() != ".npz":
        raise click.UsageError(f"-o / --output must be an .npz file: two matrices are written (got '{Path(output).name}').")
    if not 1 <= n_components <= 64:
        raise click.UsageError(f"--components must be in [1, 64] (got {n_components}).")
    if n_iter < 0:
        raise click.UsageError(f"--iterations must be non-negative (got {n_iter}).")
    if seed < 0:
        raise click.UsageError(f"--seed must be non-negative (got {seed}).")
    x, sr = _load_signal(input_file, None)
    if np.size(x) < 1:
        raise click.UsageError("The input is empty.")
    from .. import ops
    try:
        y = ops.to_device_f32(np.asarray(x, dtype=np.float32)[None])
        S = ops.cabs_pow(ops.stft2048_c2c(y), 1)
        A0, C0 = ops.nmf(S, n_components, n_iter=0, seed=seed)
        A, C = ops.nmf(S, A0=A0, C0=C0, n_iter=n_iter, beta_loss=loss)
        d0, d1 = (float(ops.nmf_divergence(S, a, c, loss)[0].item()) for a, c in ((A0, C0), (A, C)))
    except ValueError as e:
        raise click.UsageError(str(e))
    sio.save_data({"components": C[0].T.contiguous().cpu().numpy(), "activations": A[0].T.contiguous().cpu().numpy(),
                   "divergence": np.array([d0, d1]), "loss": np.array(loss)}, output)
    click.echo(f"Decomposed {S.shape[1]} frames x 1025 bins into {n_components} components in {n_iter} iterations ({loss}), "
               f"divergence {d0:.6g} -> {d1:.6g}, saved to '{Path(output).name}'.")


@dsp_cmd.command("separate-repeating")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", default=None, type=click.Path(), help="Where the background (the repeating part) is written.")
@click.option("--foreground", default=None, type=click.Path(), help="Where the foreground (what does not repeat) is written.")
@click.option("--width-seconds", "width_seconds", type=float, default=2.0, show_default=True,
              help="Frames closer than this are not compared with each other.")
@click.option("--metric", type=click.Choice(["cosine", "euclidean", "sqeuclidean"]), default="cosine", show_default=True)
@click.option("--margin-background", "margin_b", type=float, default=2.0, show_default=True)
@click.option("--margin-foreground", "margin_f", type=float, default=10.0, show_default=True)
@click.option("--power", type=float, default=2.0, show_default=True, help="Exponent of the soft masks.")
@click.option("--fs", type=int, default=None, help="Sampling rate of the input (Hz) if the file carries none.")
def dsp_separate_repeating(input_file, output, foreground, width_seconds, metric, margin_b, margin_f, power, fs):
    """Split INPUT into a repeating background and a foreground by similarity (REPET-SIM): every STFT frame (n_fft 2048,
    hop 512) is replaced by the median of its nearest frames at least --width-seconds away, and two soft masks divide the
    clip between what that median explains and the rest."""
    if output is None:
        raise click.UsageError("-o / --output is required: where to write the background.")
    for name, v in (("--width-seconds", width_seconds), ("--margin-background", margin_b), ("--margin-foreground", margin_f),
                    ("--power", power)):
        if not (v > 0 and np.isfinite(v)):
            raise click.UsageError(f"{name} must be positive (got {v:g}).")
    x, sr = _load_signal(input_file, fs)
    if not sr:
        raise click.UsageError("--fs is required: the input file carries no sampling rate.")
    if np.size(x) < 1:
        raise click.UsageError("The input is empty.")
    from ..core.decompose import separate_repeating
    try:
        fg, bg = separate_repeating(np.asarray(x, dtype=np.float32), float(sr), width_seconds=width_seconds, metric=metric,
                                    margin_background=margin_b, margin_foreground=margin_f, power=power)
    except ValueError as e:
        raise click.UsageError(str(e))
    _save_series(bg, sr, output)
    if foreground is not None:
        _save_series(fg, sr, foreground)
    width = max(1, int(round(width_seconds * float(sr) / 512)))
    click.echo(f"Separated {np.size(x)} samples ({metric}, frames at least {width} apart), background saved to "
               f"'{Path(output).name}'" + (f", foreground to '{Path(foreground).name}'." if foreground is not None else "."))


@dsp_cmd.command("structure")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-k", "--segments", "k", type=int, required=True, help="Number of segments to cut the clip into.")
@click.option("--feature", type=click.Choice(["mfcc", "chroma"]), default="mfcc", show_default=True)
@click.option("--enhance", type=int, default=None, help="Enhance the diagonal paths of the recurrence matrix with filters of N frames.")
@click.option("--median", type=int, default=None, help="Median-filter the recurrence matrix along its diagonals over W frames (odd).")
@click.option("-o", "--output", default=None, type=click.Path(), help="Where the segment table is written (CSV).")
@click.option("--fs", type=int, default=None, help="Sampling rate of the input (Hz) if the file carries none.")
def dsp_structure(input_file, k, feature, enhance, median, output, fs):
    """Cut INPUT into -k segments: features (n_fft 2048, hop 512), their affinity recurrence matrix, optionally its diagonal
    paths enhanced (--enhance) and median-filtered (--median), the matrix's rows appended to the features, and a Ward
    clustering of neighbouring frames.  Writes segment, start_frame, start_time."""
    if k < 1:
        raise click.UsageError(f"-k / --segments must be at least 1 (got {k}).")
    if enhance is not None and enhance < 1:
        raise click.UsageError(f"--enhance must be at least 1 (got {enhance}).")
    if median is not None and (median < 1 or median > 63 or median % 2 == 0):
        raise click.UsageError(f"--median must be odd and in [1, 63] (got {median}).")
    x, sr = _load_signal(input_file, fs)
    if not sr:
        raise click.UsageError("--fs is required: the input file carries no sampling rate.")
    if np.size(x) < 1:
        raise click.UsageError("The input is empty.")
    from ..core.structure import structure_segments
    try:
        bounds = structure_segments(np.asarray(x, dtype=np.float32), float(sr), k, feature=feature, enhance=enhance, median=median)
    except ValueError as e:
        raise click.UsageError(str(e))
    import pandas as pd
    table = pd.DataFrame({"segment": np.arange(len(bounds)), "start_frame": bounds, "start_time": bounds * 512.0 / float(sr)})
    if output is not None:
        table.to_csv(output, index=False)
    click.echo(f"Cut {np.size(x)} samples into {len(bounds)} segments ({feature}"
               + (f", paths enhanced over {enhance} frames" if enhance else "") + (f", diagonal median over {median} frames" if median else "")
               + "), starts at frames " + " ".join(str(int(b)) for b in bounds)
               + (f", saved to '{Path(output).name}'." if output is not None else "."))


@dsp_cmd.command("stft")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--n-fft", type=int, default=2048, show_default=True)
@click.option("--hop-length", type=int, default=None)
@click.option("--window", default="hann", show_default=True)
def dsp_stft(input_file, output, n_fft, hop_length, window):
    """Compute the Short-Time Fourier Transform (saved as NPZ: stft, n_fft, hop_length)."""
    from ..core.dsp import compute_stft
    x, _ = _load_signal(input_file, None)
    try:
        X = compute_stft(x, n_fft=n_fft, hop_length=hop_length, window=window)
    except ValueError as e:
        raise click.UsageError(str(e))
    sio.save_data({"stft": X, "n_fft": np.array(n_fft), "hop_length": np.array(hop_length or n_fft // 4)}, output)
    click.echo(f"STFT saved to '{Path(output).name}'.")


# ---------------------------------------------------------------- filter
@click.group("filter")
def filter_cmd():
    """Apply IIR filters (zero-phase or causal), FIR filters and equalizers."""


@filter_cmd.command("apply")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("--type", "ftype", required=True, type=click.Choice(["lowpass", "highpass", "bandpass", "bandstop"]))
@click.option("--cutoff", required=True, help="Cutoff (Hz); comma-separated pair for bandpass/bandstop.")
@click.option("--fs", type=float, default=None, help="Sampling frequency (Hz) if the file carries none.")
@click.option("--order", type=int, default=5, show_default=True)
@click.option("--family", type=click.Choice(["butter", "cheby1", "cheby2", "ellip", "bessel"]), default="butter",
              show_default=True, help="IIR family.")
@click.option("--rp", type=float, default=None, help="Pass-band ripple (dB): cheby1 and ellip.")
@click.option("--rs", type=float, default=None, help="Stop-band attenuation (dB): cheby2 and ellip.")
@click.option("--causal", is_flag=True, default=False,
              help="Filter causally from rest (scipy.signal.sosfilt) instead of zero-phase.")
@click.option("-o", "--output", required=True, type=click.Path())
def filter_apply(input_file, ftype, cutoff, fs, order, family, rp, rs, causal, output):
    """Apply an IIR filter (Butterworth unless --family says otherwise) to a signal or audio file. Uses zero-phase
    filtering unless --causal is given."""
    from ..core.filters import apply_sos_filter, apply_sos_filter_causal, design_butterworth_sos, design_iir_sos
    x, sr = _load_signal(input_file, fs)
    if sr is None:
        raise click.UsageError("--fs is required: the input file carries no sampling rate.")
    parts = [float(c) for c in str(cutoff).split(",")]
    cut = parts[0] if len(parts) == 1 else (parts[0], parts[1])
    try:
        if family == "butter" and rp is None and rs is None:
            sos = design_butterworth_sos(cut, sr, order, ftype)
        else:
            sos = design_iir_sos(cut, sr, order, ftype, family=family, rp=rp, rs=rs)
        if not causal and sos.shape[0] > 8:
            raise click.UsageError(f"This design has {sos.shape[0]} second-order sections; zero-phase filtering serves at "
                                   "most 8. Lower --order, or filter causally with --causal (up to 32 sections).")
        y = apply_sos_filter_causal(sos, x) if causal else apply_sos_filter(sos, x)
    except (ValueError, TypeError) as e:
        raise click.UsageError(str(e))
    if Path(output).suffix.lower() == ".wav":
        sio.save_data((y, int(sr)), output)
    else:
        sio.save_data(y, output)
    click.echo(f"Filtered signal saved to '{Path(output).name}'.")


EQ_BAND_TYPES = ("peak", "low_shelf", "high_shelf", "notch")


def parse_eq_band(token: str) -> dict:
    """'TYPE:FREQ[:GAIN_DB[:Q]]' -> a stage of apply_parametric_eq ('peak:1000:-6:2', 'notch:50', 'low_shelf:120:3')."""
    parts = [t.strip() for t in token.split(":")]
    form = "write TYPE:FREQ[:GAIN_DB[:Q]] with TYPE one of peak, low_shelf, high_shelf, notch, e.g. peak:1000:-6:1.4"
    if not 2 <= len(parts) <= 4 or parts[0].lower() not in EQ_BAND_TYPES:
        raise click.UsageError(f"--band: cannot read '{token}' ({form}).")
    try:
        nums = [float(v) for v in parts[1:]]
    except ValueError:
        raise click.UsageError(f"--band: cannot read the numbers of '{token}' ({form}).")
    if not all(np.isfinite(nums)):
        raise click.UsageError(f"--band: the numbers of '{token}' must be finite ({form}).")
    stage = {"type": parts[0].lower(), "freq": nums[0]}
    if len(nums) > 1:
        stage["gain_db"] = nums[1]
    if len(nums) > 2:
        stage["q"] = nums[2]
    return stage


@filter_cmd.command("eq")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--band", "bands", multiple=True, required=True,
              help="One EQ stage, TYPE:FREQ[:GAIN_DB[:Q]] (peak, low_shelf, high_shelf, notch); repeatable, applied in order.")
@click.option("--fs", type=float, default=None, help="Sampling frequency (Hz) if the file carries none.")
def filter_eq(input_file, output, bands, fs):
    """Apply a parametric equalizer (a causal cascade of biquads) to a signal or audio file."""
    from ..core.audio.effects import apply_parametric_eq
    stages = [parse_eq_band(tok) for tok in bands]
    x, sr = _load_signal(input_file, fs)
    if sr is None:
        raise click.UsageError("--fs is required: the input file carries no sampling rate.")
    try:
        y = apply_parametric_eq(x, sr, stages)
    except ValueError as e:
        raise click.UsageError(str(e))
    _save_series(y, sr, output)
    click.echo(f"Equalized signal ({len(stages)} stages) saved to '{Path(output).name}'.")


@filter_cmd.command("fir")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False))
@click.option("-o", "--output", required=True, type=click.Path())
@click.option("--numtaps", type=int, required=True, help="Number of taps of the filter.")
@click.option("--cutoff", required=True, help="Cutoff (Hz); comma-separated pair for a band.")
@click.option("--window", default="hamming", show_default=True, help="Window of the design, name[:param].")
@click.option("--pass-zero/--no-pass-zero", "pass_zero", default=True, show_default=True,
              help="Whether the gain at 0 Hz is 1 (low-pass / band-stop) or 0 (high-pass / band-pass).")
@click.option("--fs", type=float, default=None, help="Sampling frequency (Hz) if the file carries none.")
def filter_fir(input_file, output, numtaps, cutoff, window, pass_zero, fs):
    """Apply a windowed FIR filter (scipy.signal.firwin, causal: lfilter(taps, 1, x))."""
    from ..core.filters import apply_fir_filter_batch, design_fir
    try:
        parts = [float(c) for c in str(cutoff).split(",")]
    except ValueError:
        raise click.UsageError(f"--cutoff: cannot read '{cutoff}' as one frequency or a comma-separated pair.")
    if len(parts) not in (1, 2):
        raise click.UsageError(f"--cutoff: cannot read '{cutoff}' as one frequency or a comma-separated pair.")
    w = parse_window_spec(window)
    x, sr = _load_signal(input_file, fs)
    if sr is None:
        raise click.UsageError("--fs is required: the input file carries no sampling rate.")
    try:
        taps = design_fir(numtaps, parts[0] if len(parts) == 1 else parts, sr, window=w, pass_zero=pass_zero)
        y = apply_fir_filter_batch(taps, np.asarray(x, dtype=np.float32)[None, :])[0].cpu().numpy().astype(np.float64)
    except ValueError as e:
        raise click.UsageError(str(e))
    _save_series(y, sr, output)
    click.echo(f"FIR-filtered signal ({numtaps} taps) saved to '{Path(output).name}'.")


# ---------------------------------------------------------------- augment
@click.group("augment")
def augment_cmd():
    """Apply data augmentation techniques to audio signals."""


@augment_cmd.command("add-noise")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False, resolve_path=True))
@click.option("-o", "--output", type=click.Path(resolve_path=True), required=True,
              help="Output file path for the augmented audio.")
@click.option("--snr", type=float, required=True, help="Target Signal-to-Noise Ratio (SNR) in dB.")
@click.option("--noise-type", type=click.Choice(["gaussian", "white", "pink", "brown"], case_sensitive=False),
              default="gaussian", show_default=True, help="Type of noise to add.")
@click.option("--seed", type=int, default=None, help="Random seed for noise generation.")
@click.option("--generator", type=click.Choice(["host", "device"], case_sensitive=False), default="host", show_default=True,
              help="host: the reference's NumPy draw (pink / brown are its white-noise placeholders); "
                   "device: drawn on the GPU, with real pink (1/f) and brown (1/f^2) noise.")
@click.option("--exponent", type=float, default=None,
              help="Spectral exponent in [0, 2] of the noise (density ~ 1/f^exponent); --generator device only.")
def augment_add_noise(input_file, output, snr, noise_type, seed, generator, exponent):
    """Add noise to the audio signal."""
    from ..core.augment import add_noise
    generator = generator.lower()
    if exponent is not None and generator != "device":
        raise click.UsageError("--exponent needs --generator device.")
    if exponent is not None and not 0.0 <= exponent <= 2.0:
        raise click.UsageError(f"--exponent must be in [0, 2] (got {exponent}).")
    x, sr = _load_signal(input_file, None)
    try:
        if generator == "device":
            from ..core.augment import add_noise_device
            y = add_noise_device(x, snr_db=snr, noise_type=noise_type.lower(), seed=seed, exponent=exponent)
        else:
            y = add_noise(x, snr_db=snr, noise_type=noise_type.lower(), seed=seed)
    except ValueError as e:
        raise click.UsageError(f"Error during noise addition: {e}")
    _save_series(y, sr, output)
    click.echo(f"Successfully applied '{noise_type}' noise (SNR={snr} dB) to '{Path(input_file).name}', "
               f"saved to '{Path(output).name}'.")


@augment_cmd.command("time-stretch")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False, resolve_path=True))
@click.option("-o", "--output", type=click.Path(resolve_path=True), required=True,
              help="Output file path for the augmented audio.")
@click.option("--rate", type=float, required=True, help="Factor to stretch time (>1 speeds up, <1 slows down).")
def augment_time_stretch(input_file, output, rate):
    """Stretch the time duration of the audio signal without changing pitch."""
    from ..core.augment import time_stretch
    if rate <= 0:
        raise click.UsageError("Stretch rate must be positive.")
    x, sr = _load_signal(input_file, None)
    try:
        y = time_stretch(x, rate=rate)
    except ValueError as e:
        raise click.UsageError(f"Error during time stretching: {e}")
    _save_series(y, sr, output)
    click.echo(f"Successfully applied time stretch (rate={rate}) to '{Path(input_file).name}', "
               f"saved to '{Path(output).name}'.")


def _mask_value(text: str):
    """--mask-value: 'mean' or a float."""
    if text.strip().lower() == "mean":
        return "mean"
    try:
        return float(text)
    except ValueError:
        raise click.UsageError(f"--mask-value must be 'mean' or a float (got '{text}').")


@augment_cmd.command("spec-augment")
@click.argument("input_file", type=click.Path(exists=True, dir_okay=False, resolve_path=True))
@click.option("-o", "--output", type=click.Path(resolve_path=True), required=True,
              help="Output file path (same layout as the input: .csv or .npz).")
@click.option("--freq-masks", type=click.IntRange(0, 16), default=2, show_default=True, help="Frequency masks.")
@click.option("--freq-width", type=int, default=27, show_default=True, help="Most rows of a frequency mask.")
@click.option("--time-masks", type=click.IntRange(0, 16), default=2, show_default=True, help="Time masks.")
@click.option("--time-width", type=int, default=100, show_default=True, help="Most frames of a time mask.")
@click.option("--time-ratio", type=float, default=1.0, show_default=True,
              help="A time mask is at most this share of the frames, in (0, 1].")
@click.option("--time-warp", type=int, default=0, show_default=True, help="Most frames the warp moves its centre (0: no warp).")
@click.option("--mask-value", default="0", show_default=True, help="What a masked cell holds: a float, or 'mean'.")
@click.option("--seed", type=int, default=None, help="Random seed of the draws (64-bit).")
def augment_spec_augment(input_file, output, freq_masks, freq_width, time_masks, time_width, time_ratio, time_warp, mask_value,
                         seed):
    """SpecAugment on extracted features: every column but `time` is a row."""
    from ..core.augment import spec_augment
    value = _mask_value(mask_value)
    if not 0.0 < time_ratio <= 1.0:
        raise click.UsageError(f"--time-ratio must be in (0, 1] (got {time_ratio}).")
    time, names, x = _post_rows(sio.read_data(Path(input_file)))
    K, T = x.shape
    if not 0 <= freq_width <= K:
        raise click.UsageError(f"--freq-width must be in [0, {K}]: the input has {K} rows (got {freq_width}).")
    try:
        y, used = spec_augment(x, freq_masks, freq_width, time_masks, time_width, time_ratio, time_warp, value, seed=seed,
                               return_seed=True)
    except ValueError as e:
        raise click.UsageError(str(e))
    out = {} if time is None else {"time": np.asarray(time)}
    out.update({n: y[i] for i, n in enumerate(names)})
    sio.save_data(out if Path(output).suffix.lower() == ".npz" else pd.DataFrame(out), Path(output))
    click.echo(f"Applied SpecAugment (seed={used}) to {K} feature rows x {T} frames, saved to '{Path(output).name}'.")


cli.add_command(features_cmd)
cli.add_command(dsp_cmd)
cli.add_command(filter_cmd)
cli.add_command(augment_cmd)

if __name__ == "__main__":
    cli()
