"""Sample-rate conversion of delivered audio on the HIP backend (`mi355tts_resample`, csrc/resample.h): every voice produces
22 050 Hz audio, telephony and ASR loops want 8 or 16 kHz, web audio and mixing desks 24 or 48 kHz, files 44.1 kHz.  The
reference has no such step (`larynx/server.py:211-217` writes whatever `AudioSettings.sample_rate` says).  The filter design
lives here; the library takes the taps like any other table."""
from __future__ import annotations

import math
import typing

import numpy as np

from .engine import Engine

MAX_FACTOR = 1024        # up, down: what the library accepts
MAX_TAPS_PER_PHASE = 128


def design_lowpass(up: int, down: int, zero_crossings: int = 16, beta: float = 9.0) -> typing.Tuple[np.ndarray, int]:
    """Kaiser-windowed sinc prototype for resampling by `up / down`, given at the up-sampled rate: with W = max(up, down) and
    H = zero_crossings * W, taps[j + H] = (up / W) * sinc(j / W) * kaiser(2 H + 1, beta)[j + H] for j in [-H, H].  Computed in
    float64 and rounded once -> (taps float32 [2 H + 1], H).  The cutoff is the lower of the two Nyquist frequencies; 16 zero
    crossings at beta 9 give a transition band of about +-0.7 kHz around it at 22 050 -> 8 000 / 16 000 and a stop band
    below -90 dB."""
    up, down, zero_crossings = int(up), int(down), int(zero_crossings)
    if up < 1 or down < 1 or zero_crossings < 1:
        raise ValueError("up, down and zero_crossings must be >= 1")
    W = max(up, down)
    H = zero_crossings * W
    j = np.arange(-H, H + 1, dtype=np.float64)
    taps = (up / W) * np.sinc(j / W) * np.kaiser(2 * H + 1, float(beta))
    return taps.astype(np.float32), H


class Resampler:
    """`Resampler(engine, rate_in, rate_out)`: the ratio is reduced by the gcd (22 050 -> 16 000 is 320 / 441) and the
    prototype designed by `design_lowpass`.  Ratios the library refuses (`up` or `down` above 1024, more than 128 taps per
    phase) are refused here.  `rate_in == rate_out` is the identity: no model is loaded and `resample` returns its input."""

    def __init__(self, engine: Engine, rate_in: int, rate_out: int, zero_crossings: int = 16, beta: float = 9.0):
        rate_in, rate_out = int(rate_in), int(rate_out)
        if rate_in < 1 or rate_out < 1:
            raise ValueError(f"sample rates must be positive, got {rate_in} -> {rate_out}")
        g = math.gcd(rate_in, rate_out)
        self.engine = engine
        self.rate_in, self.rate_out = rate_in, rate_out
        self.up, self.down = rate_out // g, rate_in // g
        self.model_id: typing.Optional[int] = None
        self.taps: typing.Optional[np.ndarray] = None
        if self.up == self.down:
            return
        if self.up > MAX_FACTOR or self.down > MAX_FACTOR:
            raise ValueError(f"{rate_in} -> {rate_out} Hz is {self.up} / {self.down}: factors above {MAX_FACTOR} are not supported")
        self.taps, half_len = design_lowpass(self.up, self.down, zero_crossings, beta)
        if -(-(2 * half_len + 1) // self.up) > MAX_TAPS_PER_PHASE:
            raise ValueError(f"{rate_in} -> {rate_out} Hz with {zero_crossings} zero crossings needs more than "
                             f"{MAX_TAPS_PER_PHASE} taps per phase")
        self.model_id = engine.load_resampler(self.taps, self.up, self.down)

    def length(self, n: int) -> int:
        """Samples out for `n` samples in: ceil(n * up / down)."""
        return -((-int(n) * self.up) // self.down)

    def resample(self, audio: np.ndarray, samples=None, normalize: bool = False) -> np.ndarray:
        """float32 or int16, [N] or [B, N] (row b valid for `samples[b]` entries) -> the rows at the new rate, zero-filled behind
        their `length(samples[b])` samples.  `normalize=False`: float32 out.  `normalize=True`: int16 out, each row scaled
        so that its peak lands on 32767 at the new rate (the reference's `audio_float_to_int16` applied AFTER the
        conversion: nothing clips)."""
        if self.model_id is None:
            return audio
        f32, i16, _ = self.engine.resample(self.model_id, audio, samples, want_float=not normalize, want_int16=normalize,
                                           normalize=normalize)
        return i16 if normalize else f32


def get_resampler(engine: Engine, rate_in: int, rate_out: int) -> Resampler:
    """One `Resampler` per (engine, rate pair), made on first use (the sentence path's `sample_rate=`) and kept ON the engine
    (`Engine.kept`): it lives and dies with the context its model id belongs to."""
    return engine.kept("resampler", (int(rate_in), int(rate_out)), lambda: Resampler(engine, rate_in, rate_out))
