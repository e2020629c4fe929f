"""Numpy restatement of the mel analysis (csrc/mel_analysis.h) in a chosen precision: both framings, the filter bank and the
two planes in the kernel's arithmetic order.  Pinned to the reference's own functions (`transform`, `mel_basis`,
`amp_to_db`, `normalize`, `dynamic_range_compression` of larynx/audio.py) by the fixtures tests/golden/analysis/*.npz
(tests/test_emu_analysis.py); the oracle of the HIFIGAN framing, which the reference does not contain, and the source of the
float32 anchors every bound is a multiple of.

`dtype=np.float32` keeps every array and the FFT in single precision: what float32 costs the algorithm itself."""
import numpy as np

FFT, HOP, BINS, PAD = 1024, 256, 513, 384
MAG_EPS = {"hifigan": 1e-9, "reference": 0.0}


def frame_count(framing: str, n: int) -> int:
    if framing == "hifigan":
        return n // HOP if n > PAD else 0
    return -(-(n - FFT) // HOP) if n > FFT else 0


def window(framing: str, dtype=np.float64) -> np.ndarray:
    """Double precision, rounded once: periodic Hann (hifigan) / np.hanning(1024) (reference)."""
    if framing == "hifigan":
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FFT) / FFT)).astype(dtype)
    return np.hanning(FFT).astype(dtype)


def as_float(wav: np.ndarray, dtype=np.float64) -> np.ndarray:
    """int16 -> s / 32768 (exact in float32); float input as it is."""
    wav = np.asarray(wav)
    return (wav.astype(np.float32) * np.float32(1.0 / 32768)).astype(dtype) if wav.dtype == np.int16 else wav.astype(dtype)


def frames_of(wav: np.ndarray, framing: str) -> np.ndarray:
    """[F, 1024] sample frames of one row under the framing's index map."""
    F = frame_count(framing, len(wav))
    if F == 0:
        return np.zeros((0, FFT), wav.dtype)
    idx = HOP * np.arange(F)[:, None] + np.arange(FFT)[None, :]
    if framing == "hifigan":
        idx = idx - PAD
        idx = np.where(idx < 0, -idx, np.where(idx >= len(wav), 2 * (len(wav) - 1) - idx, idx))
    return wav[idx]


def magnitudes(wav: np.ndarray, framing: str, dtype=np.float64, mag_eps=None) -> np.ndarray:
    """[513, F]: sqrt(re^2 + im^2 + mag_eps) of the windowed frames' transforms."""
    eps = MAG_EPS[framing] if mag_eps is None else mag_eps
    spec = np.fft.rfft(frames_of(as_float(wav, dtype), framing) * window(framing, dtype), axis=1)
    re, im = spec.real.astype(dtype), spec.imag.astype(dtype)
    return np.sqrt(re * re + im * im + dtype(eps)).astype(dtype).T


def amplitudes(mag: np.ndarray, basis: np.ndarray, dtype=np.float64) -> np.ndarray:
    """[M, F] = basis @ mag."""
    return (np.asarray(basis, dtype) @ np.asarray(mag, dtype)).astype(dtype)


def normalize(v: np.ndarray, s, dtype=np.float64) -> np.ndarray:
    """AudioSettings.normalize (larynx/audio.py:65-81) in its operation order."""
    ref, mn, mx = dtype(s.ref_level_db), dtype(s.min_level_db), dtype(s.max_norm)
    n = ((v - ref) - mn) / (-mn)
    if s.symmetric_norm:
        n = ((dtype(2) * mx) * n) - mx
        return np.clip(n, -mx, mx) if s.clip_norm else n
    n = mx * n
    return np.clip(n, dtype(0), mx) if s.clip_norm else n


def planes(amp: np.ndarray, s=None, dtype=np.float64):
    """(raw, voc) of amplitudes [M, F] under the audio settings `s` (None: both ln(max(amp, 1e-5)))."""
    amp = np.asarray(amp, dtype)
    ln = np.log(np.maximum(amp, dtype(1e-5)))
    if s is None:
        return ln, ln
    voc = ln if s.do_dynamic_range_compression else amp
    raw = dtype(s.spec_gain) * np.log10(np.maximum(dtype(1e-5), amp)) if s.convert_db_to_amp else voc
    if s.signal_norm:
        raw = normalize(raw, s, dtype)
    return raw.astype(dtype), voc.astype(dtype)


def analyze(wav: np.ndarray, basis: np.ndarray, framing: str, s=None, dtype=np.float64, mag_eps=None):
    """One row: (amp, raw, voc), each [M, F]."""
    amp = amplitudes(magnitudes(wav, framing, dtype, mag_eps), basis, dtype)
    raw, voc = planes(amp, s, dtype)
    return amp, raw, voc


def denormalize_to_voc(raw: np.ndarray, s, dtype=np.float32) -> np.ndarray:
    """The mel transforms of `_sentence_task` (larynx/__init__.py:242-249 -> audio.py:83-108): raw plane -> vocoder plane."""
    v = np.asarray(raw, dtype)
    mn, mx = dtype(s.min_level_db), dtype(s.max_norm)
    if s.signal_norm:
        if s.symmetric_norm:
            if s.clip_norm:
                v = np.clip(v, -mx, mx)
            v = ((v + mx) * -mn / (dtype(2) * mx)) + mn
        else:
            if s.clip_norm:
                v = np.clip(v, dtype(0), mx)
            v = (v * -mn / mx) + mn
        v = v + dtype(s.ref_level_db)
    if s.convert_db_to_amp:
        v = np.power(dtype(10.0), v / dtype(s.spec_gain))
    if s.do_dynamic_range_compression:
        v = np.log(np.maximum(v, dtype(1e-5)))
    return v.astype(dtype)


def designed_signal() -> np.ndarray:
    """10240 samples that REACH the 1e-5 clamp (the golden waveforms never do): 8 hops of digital silence, 12 of a
    0.5-amplitude chirp, 10 of a 1e-3 tone at 9.5 kHz (above mel_fmax), 10 of a 0.8-amplitude 440 Hz tone plus 1e-4
    Gaussian noise from RandomState(5)."""
    sr = 22050.0
    n = np.arange(12 * HOP)
    chirp = 0.5 * np.sin(2.0 * np.pi * (200.0 * n / sr + 0.5 * (6000.0 - 200.0) / (12 * HOP / sr) * (n / sr) ** 2))
    n = np.arange(10 * HOP)
    high = 1e-3 * np.sin(2.0 * np.pi * 9500.0 * n / sr)
    tone = 0.8 * np.sin(2.0 * np.pi * 440.0 * n / sr) + 1e-4 * np.random.RandomState(5).randn(10 * HOP)
    return np.concatenate([np.zeros(8 * HOP), chirp, high, tone]).astype(np.float32)


# ---- the metrics of the tests (an ln-domain maximum over ALL entries is the wrong yardstick: the error is absolute and
# near-empty channels hold amplitudes of 1e-5)
def selection(amp_ref: np.ndarray) -> np.ndarray:
    """Entries with amp_ref >= 1e-3 x their frame's peak amplitude and amp_ref > 2e-5."""
    return (amp_ref >= 1e-3 * amp_ref.max(axis=0, keepdims=True)) & (amp_ref > 2e-5)


def metric_a(voc: np.ndarray, voc_ref: np.ndarray) -> float:
    """max |exp(voc) - exp(voc_ref)| / max exp(voc_ref)."""
    e, r = np.exp(np.asarray(voc, np.float64)), np.exp(np.asarray(voc_ref, np.float64))
    return float(np.abs(e - r).max() / r.max())


def metric_b(x: np.ndarray, ref: np.ndarray, sel: np.ndarray) -> float:
    """max |x - ref| on the selection (the vocoder plane's ln values, or the raw plane's normalised ones)."""
    return float(np.abs(np.asarray(x, np.float64) - np.asarray(ref, np.float64))[sel].max())
