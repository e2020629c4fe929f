"""Pitch of delivered audio, or of any recording, on the HIP backend (`mi355tts_pitch`, csrc/pitch.h): a YIN tracker (de
Cheveigne & Kawahara 2002, steps 1-5) that gives the fundamental frequency, the periodicity and the level of every frame in one
launch, and their summary per phoneme.  Timing (`phoneme_spans`) and level (`larynx_amd.loudness`) could be read before; this is
the third part of prosody.  The reference has no such step.  The definition is in include/mi355tts.h."""
from __future__ import annotations

import dataclasses
import math
import typing

import numpy as np

from .engine import Engine

MAX_WINDOW = 2048  # what the library accepts


@dataclasses.dataclass
class PitchTrack:
    """float32 [F] ([B, F] for a batch): `f0` in Hz, 0 where the frame is unvoiced; `periodicity` in [0, 1]; `level_db`, the mean
    square of the frame's window in dB (-100 for silence).  Frame t is centred on sample t * hop of the audio it was read from."""

    f0: np.ndarray
    periodicity: np.ndarray
    level_db: np.ndarray
    hop: int
    sample_rate: int


class PitchTracker:
    """`PitchTracker(engine, sample_rate, fmin, fmax)`: lags tau_min = ceil(sr / fmax) .. tau_max = floor(sr / fmin); `hop`
    defaults to round(256 sr / 22050), the vocoders' frame at the voice's rate; `window` to the smallest multiple of 64 that
    holds two of the longest periods, at most 2048."""

    def __init__(self, engine: Engine, sample_rate: int, fmin: float = 50.0, fmax: float = 500.0, hop: typing.Optional[int] = None,
                 window: typing.Optional[int] = None, threshold: float = 0.15, interpolate: bool = True):
        sample_rate = int(sample_rate)
        if sample_rate < 1 or not 0 < fmin <= fmax:
            raise ValueError(f"need a positive sample rate and 0 < fmin <= fmax, got {sample_rate}, {fmin}, {fmax}")
        self.engine = engine
        self.sample_rate = sample_rate
        self.tau_min = max(1, math.ceil(sample_rate / fmax))
        self.tau_max = math.floor(sample_rate / fmin)
        self.hop = int(hop) if hop is not None else round(256 * sample_rate / 22050)
        self.window = int(window) if window is not None else min(MAX_WINDOW, -(-2 * self.tau_max // 64) * 64)
        self.threshold, self.interpolate = float(threshold), bool(interpolate)
        self.model_id = engine.load_pitch(sample_rate, self.hop, self.window, self.tau_min, self.tau_max, self.threshold, self.interpolate)

    def frames(self, n: int) -> int:
        """Frames of a row of `n` samples: floor(n / hop)."""
        return int(n) // self.hop

    def track(self, audio: np.ndarray, samples=None) -> PitchTrack:
        """float32 or int16, [N] or [B, N] (row b valid for `samples[b]` entries) -> the `PitchTrack` of the rows, zero-filled
        behind their `frames(samples[b])` frames."""
        r = self.engine.pitch(self.model_id, audio, samples)
        return PitchTrack(r["f0"], r["periodicity"], r["level_db"], self.hop, self.sample_rate)


def get_pitch_tracker(engine: Engine, sample_rate: int) -> PitchTracker:
    """One default `PitchTracker` per (engine, rate), made on first use (the sentence path's `pitch=True`) and kept ON the engine
    (`Engine.kept`)."""
    return engine.kept("pitch", int(sample_rate), lambda: PitchTracker(engine, sample_rate))


def pitch_per_span(track: PitchTrack, spans: np.ndarray) -> np.ndarray:
    """float32 [P, 2] for spans int64 [P, 2] (start and end sample, `phoneme_spans`) over a one-row track: the median f0 of the
    voiced frames whose centre t * hop lies in [start, end) (0 where there is none) and the voiced share of the span's frames
    (0 for a span that holds no frame centre).  On the host: it is tiny."""
    f0 = np.asarray(track.f0, np.float32)
    if f0.ndim != 1:
        raise ValueError("pitch_per_span: one row at a time")
    spans = np.asarray(spans, np.int64).reshape(-1, 2)
    centre = np.arange(len(f0), dtype=np.int64) * int(track.hop)
    out = np.zeros((len(spans), 2), np.float32)
    for i, (a, b) in enumerate(spans):
        inside = f0[(centre >= a) & (centre < b)]
        if inside.size:
            voiced = inside[inside > 0]
            out[i] = (np.median(voiced) if voiced.size else 0.0, voiced.size / inside.size)
    return out
