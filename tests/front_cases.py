"""The STFT front-end routing table shared by the host test (tests/test_host_logic.py::test_front_route_is_pinned) and the
device test (tests/test_gpu_front_route.py): every row is one request through a public entry (extract_features_batch,
manager.mel_power_batch, ops.mfcc_batch, cepstral.mfcc); EXPECT pins the route sygnals_amd._front.front_route answers for
it and the library entry points the request then calls, in order.  Both were recorded from the code before the rule had
one home, so that "the same launches as before" stays a checked claim."""
from collections import namedtuple

Case = namedtuple("Case", "entry n_fft hop n_mels power feats mfcc fused sr B L one_launch")

FEATURE_SETS = {
    "M": ["mfcc"],
    "S": ["spectral_centroid", "spectral_rolloff"],
    "C": ["spectral_contrast"],
    "A": ["mfcc", "spectral_centroid", "spectral_contrast"],
    "M3": ["mfcc"],                                   # with dct_type 3: not the standard cepstrum
    "ML": ["mfcc", "spectral_rolloff"],               # with lifter 22
}
MFCC_PARAMS = {"M3": {"dct_type": 3}, "ML": {"lifter": 22}}


def _x(n_fft, feats, n_mels=40, power=2.0, hop=None, sr=22050, one_launch=True):
    """extract_features_batch: 2 ragged clips of three frames and 17 samples."""
    return Case("extract", n_fft, hop or n_fft // 4, n_mels, power, feats, MFCC_PARAMS.get(feats, {}), None, sr, 2,
                3 * n_fft + 17, one_launch)


def _m(n_fft, n_mels=40, power=2.0, hop=None, sr=22050, entry="mel"):
    """manager.mel_power_batch (entry "cepstral": cepstral.mfcc on the first clip)."""
    return Case(entry, n_fft, hop or n_fft // 4, n_mels, power, None, {}, None, sr, 2, 3 * n_fft + 17, True)


def _b(n_fft, n_mels=40, fused=None, sr=22050, B=2, L=None):
    """ops.mfcc_batch(fused=...)."""
    return Case("mfcc_batch", n_fft, n_fft // 4, n_mels, 2.0, None, {}, fused, sr, B, L or 3 * n_fft + 17, True)


CASES = {
    # ---- extract_features_batch, frame length 2048
    "x2048-M": _x(2048, "M"),
    "x2048-S": _x(2048, "S"),
    "x2048-C": _x(2048, "C"),
    "x2048-A": _x(2048, "A"),
    "x2048-M3": _x(2048, "M3"),
    "x2048-ML": _x(2048, "ML"),
    "x2048-M-128": _x(2048, "M", 128),
    "x2048-A-128": _x(2048, "A", 128),
    "x2048-M-300": _x(2048, "M", 300),
    "x2048-A-300": _x(2048, "A", 300),
    "x2048-M-p1": _x(2048, "M", power=1.0),
    "x2048-A-p1": _x(2048, "A", power=1.0),
    "x2048-M-hop1024": _x(2048, "M", hop=1024),
    "x2048-S-hop1024": _x(2048, "S", hop=1024),
    "x2048-C-hop1024": _x(2048, "C", hop=1024),
    "x2048-A-hop1024": _x(2048, "A", hop=1024),
    "x2048-S-hop1024-p1": _x(2048, "S", hop=1024, power=1.0),
    # ... and where ops.settings.one_launch_features decides, with the switch off
    "x2048-M-off": _x(2048, "M", one_launch=False),
    "x2048-A-off": _x(2048, "A", one_launch=False),
    "x2048-ML-off": _x(2048, "ML", one_launch=False),
    "x2048-M-128-off": _x(2048, "M", 128, one_launch=False),
    "x2048-A-128-off": _x(2048, "A", 128, one_launch=False),
    "x2048-M-hop1024-off": _x(2048, "M", hop=1024, one_launch=False),
    "x2048-A-hop1024-off": _x(2048, "A", hop=1024, one_launch=False),
    # ---- frame length 1024
    "x1024-M": _x(1024, "M"),
    "x1024-S": _x(1024, "S"),
    "x1024-A": _x(1024, "A"),
    "x1024-M3": _x(1024, "M3"),
    "x1024-M-128": _x(1024, "M", 128),
    "x1024-A-128": _x(1024, "A", 128),
    "x1024-M-300": _x(1024, "M", 300),
    "x1024-A-300": _x(1024, "A", 300),
    "x1024-M-p1": _x(1024, "M", power=1.0),
    "x1024-A-p1": _x(1024, "A", power=1.0),
    # ---- frame length 4096 (128 bands: a piece table at 22.05 kHz, none at 48 kHz)
    "x4096-M": _x(4096, "M"),
    "x4096-S": _x(4096, "S"),
    "x4096-A": _x(4096, "A"),
    "x4096-A-128": _x(4096, "A", 128),
    "x4096-A-128-48k": _x(4096, "A", 128, sr=48000),
    "x4096-M-p1": _x(4096, "M", power=1.0),
    "x4096-A-p1": _x(4096, "A", power=1.0),
    # ---- frame lengths 512 / 256
    "x512-M": _x(512, "M"),
    "x512-S": _x(512, "S"),
    "x512-A": _x(512, "A"),
    "x512-A-128": _x(512, "A", 128),
    "x512-A-300": _x(512, "A", 300),
    "x512-A-p1": _x(512, "A", power=1.0),
    "x256-M": _x(256, "M"),
    "x256-A": _x(256, "A"),
    "x256-A-128": _x(256, "A", 128),
    "x256-M-p1": _x(256, "M", power=1.0),
    # ---- 128 (the dense power-of-two kernel only), 1000 and 8192 (the generic chain)
    "x128-M": _x(128, "M"),
    "x128-A": _x(128, "A"),
    "x128-M-p1": _x(128, "M", power=1.0),
    "x1000-S": _x(1000, "S"),
    "x1000-A": _x(1000, "A"),
    "x8192-A": _x(8192, "A"),
    # ---- manager.mel_power_batch
    "m2048": _m(2048),
    "m2048-p1": _m(2048, power=1.0),
    "m2048-300": _m(2048, 300),
    "m1024": _m(1024),
    "m1024-128": _m(1024, 128),
    "m1024-p1": _m(1024, power=1.0),
    "m512": _m(512),
    "m256": _m(256),
    "m4096": _m(4096),
    "m4096-128-48k": _m(4096, 128, sr=48000),
    "m128": _m(128),
    "m1000": _m(1000),
    "m8192": _m(8192),
    # ---- cepstral.mfcc (one clip)
    "c2048": _m(2048, entry="cepstral"),
    "c1024-p1": _m(1024, power=1.0, entry="cepstral"),
    "c1000": _m(1000, entry="cepstral"),
    # ---- ops.mfcc_batch: fused = None (its batch-size rule: 128 clips of 4096 samples), True, False
    "b2048": _b(2048),
    "b2048-fused": _b(2048, fused=True),
    "b2048-two": _b(2048, fused=False),
    "b2048-B128": _b(2048, B=128, L=4096),
    "b2048-128-B128": _b(2048, 128, B=128, L=4096),
    "b2048-300": _b(2048, 300),
    "b1024": _b(1024),
    "b1024-128": _b(1024, 128),
    "b1024-fused": _b(1024, fused=True),
    "b1024-two": _b(1024, fused=False),
    "b512": _b(512),
    "b256-128": _b(256, 128),
    "b4096": _b(4096),
    "b4096-two": _b(4096, fused=False),
    "b128": _b(128),
    "b1000": _b(1000),
    "b8192": _b(8192),
}


def wants(c):
    """(rows wanted, mel wanted) of a row."""
    if c.entry != "extract":
        return False, True
    feats = FEATURE_SETS[c.feats]
    return any(f.startswith("spectral") for f in feats), "mfcc" in feats


def run(c, y):
    """The request of row `c` on the clips y [B, L] (float32, host); returns what the entry returns."""
    from sygnals_amd import ops
    from sygnals_amd.core.features import cepstral, manager
    with ops.override(one_launch_features=c.one_launch):
        if c.entry == "extract":
            fp = {"mfcc": dict(c.mfcc, n_mels=c.n_mels, power=c.power)}
            return manager.extract_features_batch(y, c.sr, FEATURE_SETS[c.feats], c.n_fft, c.hop, feature_params=fp)
        if c.entry == "mel":
            return manager.mel_power_batch(ops.to_device_f32(y), c.sr, c.n_fft, c.hop, True, "hann", c.n_mels, 0.0, None, c.power)
        if c.entry == "cepstral":
            return cepstral.mfcc(y[0], c.sr, n_fft=c.n_fft, hop_length=c.hop, n_mels=c.n_mels, power=c.power)
        return ops.mfcc_batch(ops.to_device_f32(y), c.sr, c.n_fft, c.hop, c.n_mels, fused=c.fused)


# case -> (route, entry points called)
EXPECT = {
    "x2048-M": (None, [
        "syg_stft2048_mfcc_tri_f32"]),
    "x2048-S": (('stft2048_stats', None), [
        "syg_stft2048_stats_f32"]),
    "x2048-C": (('stft2048_stats', None), [
        "syg_stft2048_stats_f32",
        "syg_contrast_db_f32"]),
    "x2048-A": (None, [
        "syg_stft2048_features_tri_f32",
        "syg_contrast_db_f32"]),
    "x2048-M3": ((None, 'stft2048_mel'), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32"]),
    "x2048-ML": (('stft2048_mel', None), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32"]),
    "x2048-M-128": (None, [
        "syg_stft2048_mfcc_f32"]),
    "x2048-A-128": (('stft2048_mel', None), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x2048-M-300": ((None, 'generic'), [
        "syg_stft2048_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32"]),
    "x2048-A-300": (('generic', 'generic'), [
        "syg_stft2048_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32",
        "syg_contrast_pv_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x2048-M-p1": ((None, 'generic'), [
        "syg_stft2048_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32"]),
    "x2048-A-p1": (('generic', 'generic'), [
        "syg_stft2048_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32",
        "syg_contrast_pv_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x2048-M-hop1024": (None, [
        "syg_stft2048_mfcc_f32"]),
    "x2048-S-hop1024": (('stft2048_mel', None), [
        "syg_stft2048_mel_f32"]),
    "x2048-C-hop1024": (('stft2048_mel', None), [
        "syg_stft2048_mel_f32",
        "syg_contrast_db_f32"]),
    "x2048-A-hop1024": (('stft2048_mel', None), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x2048-S-hop1024-p1": (('generic', None), [
        "syg_stft2048_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32"]),
    "x2048-M-off": ((None, 'stft2048_mel'), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32"]),
    "x2048-A-off": (('stft2048_mel', None), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x2048-ML-off": (('stft2048_mel', None), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32"]),
    "x2048-M-128-off": ((None, 'stft2048_mel'), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32"]),
    "x2048-A-128-off": (('stft2048_mel', None), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x2048-M-hop1024-off": ((None, 'stft2048_mel'), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32"]),
    "x2048-A-hop1024-off": (('stft2048_mel', None), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x1024-M": ((None, 'stft_mel_w1024_seg'), [
        "syg_stft_mel_w1024_seg_f32",
        "syg_logmel_dct_f32"]),
    "x1024-S": (('stft_rows_w1024', None), [
        "syg_stft_rows_w1024_f32"]),
    "x1024-A": (('stft_rows_w1024', None), [
        "syg_stft_rows_w1024_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x1024-M3": ((None, 'stft_mel_w1024_seg'), [
        "syg_stft_mel_w1024_seg_f32",
        "syg_logmel_dct_f32"]),
    "x1024-M-128": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32",
        "syg_logmel_dct_f32"]),
    "x1024-A-128": (('stft_rows_w1024', 'stft_mel_pow2'), [
        "syg_stft_rows_w1024_f32",
        "syg_stft_mel_pow2_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x1024-M-300": ((None, 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32"]),
    "x1024-A-300": (('generic', 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32",
        "syg_contrast_pv_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x1024-M-p1": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32",
        "syg_logmel_dct_f32"]),
    "x1024-A-p1": (('stft_rows_w1024', 'stft_mel_pow2'), [
        "syg_stft_rows_w1024_f32",
        "syg_stft_mel_pow2_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x4096-M": ((None, 'stft_mel_w4096'), [
        "syg_stft_mel_w4096_f32",
        "syg_logmel_dct_f32"]),
    "x4096-S": (('stft_rows_w4096', None), [
        "syg_stft_rows_w4096_f32"]),
    "x4096-A": (('stft_rows_w4096', None), [
        "syg_stft_rows_w4096_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x4096-A-128": (('stft_rows_w4096', None), [
        "syg_stft_rows_w4096_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x4096-A-128-48k": (('generic', 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32",
        "syg_contrast_pv_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x4096-M-p1": ((None, 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32"]),
    "x4096-A-p1": (('generic', 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32",
        "syg_contrast_pv_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x512-M": ((None, 'stft_mel_wseg_small'), [
        "syg_stft_mel_wseg_small_f32",
        "syg_logmel_dct_f32"]),
    "x512-S": (('stft_rows_wsmall', None), [
        "syg_stft_rows_wsmall_f32"]),
    "x512-A": (('stft_rows_wsmall', 'stft_mel_wseg_small'), [
        "syg_stft_rows_wsmall_f32",
        "syg_stft_mel_wseg_small_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x512-A-128": (('stft_rows_wsmall', 'stft_mel_pow2'), [
        "syg_stft_rows_wsmall_f32",
        "syg_stft_mel_pow2_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x512-A-300": (('generic', 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32",
        "syg_contrast_pv_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x512-A-p1": (('stft_rows_wsmall', 'stft_mel_pow2'), [
        "syg_stft_rows_wsmall_f32",
        "syg_stft_mel_pow2_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x256-M": ((None, 'stft_mel_wseg_small'), [
        "syg_stft_mel_wseg_small_f32",
        "syg_logmel_dct_f32"]),
    "x256-A": (('stft_rows_wsmall', 'stft_mel_wseg_small'), [
        "syg_stft_rows_wsmall_f32",
        "syg_stft_mel_wseg_small_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x256-A-128": (('stft_rows_wsmall', 'stft_mel_pow2'), [
        "syg_stft_rows_wsmall_f32",
        "syg_stft_mel_pow2_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x256-M-p1": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32",
        "syg_logmel_dct_f32"]),
    "x128-M": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32",
        "syg_logmel_dct_f32"]),
    "x128-A": (('generic', 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32",
        "syg_contrast_pv_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x128-M-p1": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32",
        "syg_logmel_dct_f32"]),
    "x1000-S": (('generic', None), [
        "syg_pack_frames_f32",
        "syg_fft_mixed_strided_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32"]),
    "x1000-A": (('generic', 'generic'), [
        "syg_pack_frames_f32",
        "syg_fft_mixed_strided_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32",
        "syg_contrast_pv_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "x8192-A": (('generic', 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_spectral_stats_f32",
        "syg_contrast_pv_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32",
        "syg_contrast_db_f32"]),
    "m2048": ((None, 'stft2048_mel'), [
        "syg_stft2048_mel_f32"]),
    "m2048-p1": ((None, 'generic'), [
        "syg_stft2048_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32"]),
    "m2048-300": ((None, 'generic'), [
        "syg_stft2048_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32"]),
    "m1024": ((None, 'stft_mel_w1024_seg'), [
        "syg_stft_mel_w1024_seg_f32"]),
    "m1024-128": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32"]),
    "m1024-p1": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32"]),
    "m512": ((None, 'stft_mel_wseg_small'), [
        "syg_stft_mel_wseg_small_f32"]),
    "m256": ((None, 'stft_mel_wseg_small'), [
        "syg_stft_mel_wseg_small_f32"]),
    "m4096": ((None, 'stft_mel_w4096'), [
        "syg_stft_mel_w4096_f32"]),
    "m4096-128-48k": ((None, 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32"]),
    "m128": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32"]),
    "m1000": ((None, 'generic'), [
        "syg_pack_frames_f32",
        "syg_fft_mixed_strided_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32"]),
    "m8192": ((None, 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32"]),
    "c2048": ((None, 'stft2048_mel'), [
        "syg_stft2048_mel_f32",
        "syg_logmel_dct_f32"]),
    "c1024-p1": ((None, 'stft_mel_pow2'), [       # (not a recording: the earlier code fails this request -- row stride 0 of the
        "syg_stft_mel_pow2_f32",                    # one clip handed to the entry point -- so m1024-p1's launch + the dB / DCT one)
        "syg_logmel_dct_f32"]),
    "c1000": ((None, 'generic'), [
        "syg_pack_frames_f32",
        "syg_fft_mixed_strided_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_logmel_dct_f32"]),
    "b2048": ((None, 'stft2048_mel'), [
        "syg_stft2048_mel_f32",
        "syg_mel_mfcc_f32"]),
    "b2048-fused": (None, [
        "syg_stft2048_mfcc_tri_f32"]),
    "b2048-two": ((None, 'stft2048_mel'), [
        "syg_stft2048_mel_f32",
        "syg_mel_mfcc_f32"]),
    "b2048-B128": (None, [
        "syg_stft2048_mfcc_tri_f32"]),
    "b2048-128-B128": (None, [
        "syg_stft2048_mfcc_f32"]),
    "b2048-300": ((None, 'generic'), [
        "syg_stft2048_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_mel_mfcc_f32"]),
    "b1024": ((None, 'stft_mel_w1024_seg'), [
        "syg_stft_mel_w1024_seg_f32",
        "syg_mel_mfcc_f32"]),
    "b1024-128": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32",
        "syg_mel_mfcc_f32"]),
    "b1024-fused": (None, [
        "syg_stft_mfcc_pow2_f32"]),
    "b1024-two": ((None, 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_mel_mfcc_f32"]),
    "b512": ((None, 'stft_mel_wseg_small'), [
        "syg_stft_mel_wseg_small_f32",
        "syg_mel_mfcc_f32"]),
    "b256-128": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32",
        "syg_mel_mfcc_f32"]),
    "b4096": ((None, 'stft_mel_w4096'), [
        "syg_stft_mel_w4096_f32",
        "syg_mel_mfcc_f32"]),
    "b4096-two": ((None, 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_mel_mfcc_f32"]),
    "b128": ((None, 'stft_mel_pow2'), [
        "syg_stft_mel_pow2_f32",
        "syg_mel_mfcc_f32"]),
    "b1000": ((None, 'generic'), [
        "syg_pack_frames_f32",
        "syg_fft_mixed_strided_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_mel_mfcc_f32"]),
    "b8192": ((None, 'generic'), [
        "syg_stft_pow2_c2c_f32",
        "syg_cabs_pow_f32",
        "syg_mel_dense_f32",
        "syg_mel_mfcc_f32"]),
}
