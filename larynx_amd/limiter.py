"""A true-peak meter and a look-ahead limiter for delivered audio on the HIP backend (`mi355tts_limit`, csrc/limiter.h).
`larynx_amd.loudness` delivers a row at ONE gain, capped by ceiling / max|x|: speech has a peak-to-loudness ratio of 13 - 20 dB,
so at -16 LUFS under -1 dBFS the cap often binds and the row comes out under its target.  With a limiter the row takes the full
gain and only the few milliseconds around a peak are turned down (`Loudness.normalize_limited`).  The designs live here — the
interpolator of the true-peak meter (ITU-R BS.1770-4 Annex 2), the smoothing window, the release —; the library takes them as
tables like any other."""
from __future__ import annotations

import math
import typing

import numpy as np

from .engine import Engine
from .resample import design_lowpass

MAX_LOOKAHEAD = 1024  # LM_MAX_LA of csrc/limiter.h


def design_interpolator(oversample: int) -> typing.Tuple[np.ndarray, int]:
    """The interpolation prototype of the true-peak meter at `oversample` times the rate: `design_lowpass(oversample, 1)`
    -> (taps float32 [2 H + 1], H)."""
    return design_lowpass(int(oversample), 1)


def smoothing_window(lookahead: int) -> np.ndarray:
    """The gain curve's smoothing window over `lookahead + 1` samples: a Hann window without its zero end points, normalised to
    sum 1 in float64 and rounded once -> float32 [lookahead + 1] ([1.0] for lookahead 0)."""
    lookahead = int(lookahead)
    if lookahead < 0:
        raise ValueError("lookahead must be >= 0")
    w = np.hanning(lookahead + 3)[1:-1].astype(np.float64)
    return (w / w.sum()).astype(np.float32)


def release_coefficient(fs: float, ms: float) -> float:
    """The depth's decay per sample for a release time constant of `ms` milliseconds at `fs` Hz: exp(-1 / (ms * fs / 1000));
    0 (no memory) for ms = 0."""
    fs, ms = float(fs), float(ms)
    if not fs > 0 or ms < 0:
        raise ValueError("fs must be positive and ms >= 0")
    return math.exp(-1.0 / (ms * fs / 1000.0)) if ms > 0 else 0.0


class Limiter:
    """`Limiter(engine, sample_rate)`: a true-peak meter and limiter for audio at that rate.  `true_peak` reads each row's true
    peak; `limit` delivers the rows under a true-peak ceiling."""

    def __init__(self, engine: Engine, sample_rate: int, lookahead_ms: float = 1.5, release_ms: float = 50.0, oversample: int = 4):
        self.engine = engine
        self.sample_rate = int(sample_rate)
        if self.sample_rate < 1:
            raise ValueError(f"sample rate must be positive, got {sample_rate}")
        self.oversample = int(oversample)
        self.lookahead = int(round(float(lookahead_ms) * self.sample_rate / 1000.0))
        if not 0 <= self.lookahead <= MAX_LOOKAHEAD:
            raise ValueError(f"a lookahead of {lookahead_ms} ms is {self.lookahead} samples at {self.sample_rate} Hz: more than {MAX_LOOKAHEAD}")
        self.release = float(np.float32(release_coefficient(self.sample_rate, release_ms)))
        self.taps = design_interpolator(self.oversample)[0] if self.oversample > 1 else None
        self.window = smoothing_window(self.lookahead)
        self.model_id = engine.load_limiter(self.taps, self.window, self.oversample, self.release)

    def true_peak(self, audio: np.ndarray, samples=None) -> np.ndarray:
        """float32 or int16, [N] or [B, N] (row b valid for `samples[b]` entries) -> the true peak, linear, float32 [B]."""
        return self.engine.limit(self.model_id, audio, samples)["true_peak"]

    def limit(self, audio: np.ndarray, gain=None, ceiling: float = 10 ** (-1 / 20), int16: bool = True, samples=None) -> np.ndarray:
        """The rows times `gain` (one per row; default 1), turned down around every true peak that would pass `ceiling` (-1 dBFS
        by default).  int16 out (clamp(rint(y * 32768))), or float32 with `int16=False`; rows are zero-filled behind their
        samples."""
        out = self.engine.limit(self.model_id, audio, samples, gain=gain, ceiling=ceiling, want_float=not int16, want_int16=int16)
        return out["i16"] if int16 else out["f32"]


def get_limiter(engine: Engine, sample_rate: int) -> Limiter:
    """One `Limiter` per (engine, rate), made on first use (the sentence path's `limiter=True`) and kept ON the engine, like
    `get_loudness`."""
    return engine.kept("limiter", int(sample_rate), lambda: Limiter(engine, int(sample_rate)))
