"""Vectorised numpy restatement of the reference's Griffin-Lim vocoder (`larynx/griffin_lim.py:40-76` on the STFT
helpers of `larynx/audio.py:232-306`), in a chosen precision.  Pinned to the reference by the fixtures
tests/golden/griffin_lim/*.npz (tests/test_emu_griffin_lim.py); the oracle for shapes without a fixture.

Conventions, all the reference's: 1024-point frames every 256 samples at range(0, len - 1024, 256), symmetric
np.hanning(1024) on analysis and synthesis, no window-sum normalisation, the last mel frame dropped, the spectrum
rebuilt as mag * (cos(angle), sin(angle)) with angle = arctan2(im, re).  `dtype=np.float32` keeps EVERY array and
transform in single precision (numpy >= 2 runs float32 FFTs natively): what float32 arithmetic costs the algorithm."""
import numpy as np

FFT, HOP, BINS = 1024, 256, 513


def initial_phase(seed: int, frames: int) -> np.ndarray:
    """The reference's draw (`np.angle(np.exp(2j * np.pi * np.random.rand(...)))`, griffin_lim.py:68-69) from a fixed
    RandomState: [513, frames] float32."""
    u = np.random.RandomState(seed).rand(BINS, frames)
    return np.angle(np.exp(2j * np.pi * u)).astype(np.float32)


def magnitudes(mel: np.ndarray, basis: np.ndarray, scaling: float = 1000.0, dtype=np.float64) -> np.ndarray:
    """mel [M, F] (ln domain) -> [513, F - 1]: exp(mel).T @ basis * scaling, last frame dropped (griffin_lim.py:50-58)."""
    m = np.exp(np.asarray(mel, dtype)).T @ np.asarray(basis, dtype)
    return (m.T * dtype(scaling))[:, :-1].astype(dtype)


def overlap_add(frames: np.ndarray) -> np.ndarray:
    """[T, 1024] synthesis frames -> [T * 256 + 1024] (`istft`, audio.py:252-269)."""
    T = frames.shape[0]
    sig = np.zeros(T * HOP + FFT, frames.dtype)
    for q in range(FFT // HOP):  # frames q, q + 4, ... do not overlap each other
        sub = frames[q::4]
        sig[q * HOP: q * HOP + sub.size] += sub.reshape(-1)
    return sig


def inverse(mag: np.ndarray, phase: np.ndarray, dtype=np.float64) -> np.ndarray:
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    spec = np.empty(mag.shape, ctype)
    spec.real = mag * np.cos(phase)
    spec.imag = mag * np.sin(phase)
    frames = np.fft.irfft(spec.T, n=FFT, axis=1).astype(dtype) * np.hanning(FFT).astype(dtype)
    return overlap_add(frames)


def transform_phase(sig: np.ndarray, T: int, dtype=np.float64) -> np.ndarray:
    frames = np.lib.stride_tricks.sliding_window_view(sig, FFT)[::HOP][:T]  # starts 0, 256, ... < len - 1024
    spec = np.fft.rfft(frames * np.hanning(FFT).astype(dtype), axis=1)
    return np.arctan2(spec.imag, spec.real).astype(dtype).T


def griffin_lim(mag: np.ndarray, phase0: np.ndarray, n_iters: int = 60, dtype=np.float64, keep=()):
    """[513, T] magnitudes + initial phase -> the signal after `n_iters` iterations; `keep`: iteration counts whose signals
    are returned as a dict as well (0 = the initial inverse)."""
    mag = np.asarray(mag, dtype)
    T = mag.shape[1]
    sig = inverse(mag, np.asarray(phase0, dtype), dtype)
    kept = {0: sig.copy()} if 0 in keep else {}
    for it in range(1, n_iters + 1):
        sig = inverse(mag, transform_phase(sig, T, dtype), dtype)
        if it in keep:
            kept[it] = sig.copy()
    return (sig, kept) if keep else sig


def float_to_int16(audio: np.ndarray) -> np.ndarray:
    """`audio_float_to_int16` (audio.py:118-125)."""
    a = np.asarray(audio, np.float64)
    peak = max(0.01, float(np.max(np.abs(a)))) if a.size else 0.01
    return np.clip(a * (32767.0 / peak), -32767.0, 32767.0).astype(np.int16)


def rel_rms(a: np.ndarray, ref: np.ndarray) -> float:
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((a - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))
