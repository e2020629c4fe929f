"""Pitch shift and tempo of delivered audio, or of any recording, on the HIP backend (`mi355tts_shift`, csrc/shift.h).  Timing
and level could be set before; this sets the third part of prosody.  A shift by `up / down` is a period-synchronous overlap-add
stretch by `up / down` (every frame's read position moved by whole local pitch periods, read from the YIN track of the same row)
played back through the resampler by `down / up`: same duration, pitch times `up / down`.  Without the resampler it is a tempo
change.  This is resampling, not PSOLA: the formants move with the pitch, so it is meant for about +-4 semitones.  The reference
has no such step.  The definition is in include/mi355tts.h."""
from __future__ import annotations

import math
import typing

import numpy as np

from .engine import Engine
from .pitch import PitchTracker
from .resample import Resampler

MAX_FACTOR = 64            # up, down: what the library accepts
MAX_SEMITONES = 12.0       # what the sentence path accepts


def semitone_ratio(semitones: float) -> typing.Tuple[int, int]:
    """(up, down), coprime and both <= 64: the fraction nearest to 2 ** (semitones / 12); of two equally near ones, the one with
    the smaller denominator.  0 -> (1, 1), +12 -> (2, 1), +2 -> (55, 49)."""
    target = 2.0 ** (float(semitones) / 12.0)
    best = None
    for down in range(1, MAX_FACTOR + 1):
        centre = target * down
        for up in {math.floor(centre), math.ceil(centre)}:
            if 1 <= up <= MAX_FACTOR and math.gcd(up, down) == 1:
                key = (abs(up / down - target), down)
                if best is None or key < best[0]:
                    best = (key, up, down)
    if best is None:
        raise ValueError(f"no ratio up / down with both <= {MAX_FACTOR} near 2 ** ({semitones} / 12)")
    return best[1], best[2]


def check_semitones(semitones) -> float:
    """`semitones` as a float in [-12, 12], or a ValueError."""
    st = float(semitones)
    if not -MAX_SEMITONES <= st <= MAX_SEMITONES:
        raise ValueError(f"pitch_shift: {semitones} semitones is outside [-12, 12]")
    return st


def ola_window(N: int) -> np.ndarray:
    """float32 [N]: the periodic Hann window 0.5 - 0.5 cos(2 pi i / N), computed in float64 and rounded once; its second half is
    then SET to 1 - w[i] of the first (float32), so that the two windows over every output sample sum to 1 exactly."""
    N = int(N)
    if N < 2 or N % 2:
        raise ValueError("ola_window: an even length")
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)
    w[N // 2:] = np.float32(1.0) - w[:N // 2]
    return w


class PitchShifter:
    """`PitchShifter(engine, sample_rate, semitones=..)` or `(.., ratio=(up, down))`: exactly one of the two.  It builds its
    `PitchTracker` (the defaults at `sample_rate`) and — unless `tempo` — its `Resampler` by down / up, and keeps them.
    `tempo=True`: the stretch itself is delivered, ceil(n up / down) samples at the input's pitch.  `N`: the overlap-add window."""

    def __init__(self, engine: Engine, sample_rate: int, semitones: typing.Optional[float] = None,
                 ratio: typing.Optional[typing.Tuple[int, int]] = None, tempo: bool = False, N: int = 1024):
        if (semitones is None) == (ratio is None):
            raise ValueError("PitchShifter: exactly one of semitones / ratio")
        up, down = semitone_ratio(semitones) if ratio is None else (int(ratio[0]), int(ratio[1]))
        if up < 1 or down < 1:
            raise ValueError(f"ratio {up} / {down}: both must be positive")
        g = math.gcd(up, down)
        self.engine = engine
        self.sample_rate = int(sample_rate)
        self.up, self.down = up // g, down // g
        self.tempo = bool(tempo)
        self.N = int(N)
        self.window = ola_window(self.N)
        self.tracker = PitchTracker(engine, self.sample_rate)
        # (a ratio of 1 leaves nothing to resample: the plain overlap-add, which returns its input)
        self.resampler = None if self.tempo or self.up == self.down else Resampler(engine, self.up, self.down)
        self.model_id = engine.load_shift(self.up, self.down, self.window, self.tracker.model_id,
                                          self.resampler.model_id if self.resampler is not None else 0)

    def length(self, n: int) -> int:
        """Samples delivered for `n` samples in: n, or ceil(n * up / down) with `tempo`."""
        return -((-int(n) * self.up) // self.down) if self.resampler is None else int(n)

    def shift(self, audio: np.ndarray, samples=None, normalize: bool = False) -> np.ndarray:
        """float32 or int16, [N] or [B, N] (row b valid for `samples[b]` entries) -> the shifted rows, zero-filled behind their
        `length(samples[b])` samples.  `normalize=False`: float32 out.  `normalize=True`: int16 out, each row scaled so that
        its peak lands on 32767 (the reference's `audio_float_to_int16` applied AFTER the shift)."""
        r = self.engine.shift(self.model_id, audio, samples, want_float=not normalize, want_int16=normalize, normalize=normalize)
        return r["i16"] if normalize else r["f32"]


def get_pitch_shifter(engine: Engine, sample_rate: int, semitones: float) -> PitchShifter:
    """One `PitchShifter` per (engine, rate, semitones), made on first use (the sentence path's `pitch_shift=`) and kept ON the
    engine (`Engine.kept`)."""
    st = check_semitones(semitones)
    return engine.kept("shift", (int(sample_rate), st), lambda: PitchShifter(engine, sample_rate, semitones=st))
