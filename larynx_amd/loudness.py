"""A loudness target for delivered audio on the HIP backend (`mi355tts_loudness`, csrc/loudness.h): the ITU-R BS.1770-4
integrated loudness (mono) of each row, measured where the samples already are, and the row delivered at a target level under
a sample-peak ceiling.  The default delivery stays the reference's: every sentence's peak on 32767
(`larynx/audio.py:118-125`), which lets the level of a document jump from sentence to sentence.  The K-weighting design lives
here; the library takes its ten coefficients like any other table."""
from __future__ import annotations

import math
import typing

import numpy as np

from .engine import Engine


def k_weighting(fs: float) -> typing.Dict[str, np.ndarray]:
    """The two K-weighting biquads at sample rate `fs`, float64: {"shelf_b": [3], "shelf_a": [2], "hp_b": [3], "hp_a": [2]}
    (a0 = 1 is not stored).  The usual re-derivation of the standard's 48 kHz filters: the analogue prototypes behind the
    published table, taken through the bilinear transform at `fs`.  At 48 000 Hz it reproduces the table to 1e-15."""
    fs = float(fs)
    if not fs > 0:
        raise ValueError("fs must be positive")
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf_b = np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K]) / a0
    shelf_a = np.array([2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp_b = np.array([1.0, -2.0, 1.0])
    hp_a = np.array([2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return {"shelf_b": shelf_b, "shelf_a": shelf_a, "hp_b": hp_b, "hp_a": hp_a}


def block_and_hop(fs: float) -> typing.Tuple[int, int]:
    """The 400 ms gating block and its 100 ms hop (75 % overlap) in samples: 8820 and 2205 at 22 050 Hz."""
    return int(round(0.4 * float(fs))), int(round(0.1 * float(fs)))


class Loudness:
    """`Loudness(engine, sample_rate)`: a meter for audio at that rate.  `measure` reads the integrated loudness of each row
    (-inf for a row with nothing above -70 LUFS); `normalize` delivers the rows at a target level."""

    def __init__(self, engine: Engine, sample_rate: int):
        self.engine = engine
        self.sample_rate = int(sample_rate)
        if self.sample_rate < 1:
            raise ValueError(f"sample rate must be positive, got {sample_rate}")
        self.coefficients = {k: v.astype(np.float32) for k, v in k_weighting(self.sample_rate).items()}
        self.block, self.hop = block_and_hop(self.sample_rate)
        self.model_id = engine.load_loudness(block=self.block, hop=self.hop, **self.coefficients)

    def measure(self, audio: np.ndarray, samples=None) -> np.ndarray:
        """float32 or int16, [N] or [B, N] (row b valid for `samples[b]` entries) -> LUFS, float32 [B]."""
        return self.engine.loudness(self.model_id, audio, samples)["lufs"]

    def normalize(self, audio: np.ndarray, target: float = -16.0, ceiling: float = 10 ** (-1 / 20), max_gain_db: float = 30.0,
                  int16: bool = True, samples=None) -> np.ndarray:
        """The rows scaled to `target` LUFS, each by ONE gain: never more than `max_gain_db`, and never so much that a sample
        passes `ceiling` (-1 dBFS by default; the sample peak, not the true peak).  int16 out (clamp(rint(y * 32768))), or
        float32 with `int16=False`; rows are zero-filled behind their samples."""
        out = self.engine.loudness(self.model_id, audio, samples, target=target, ceiling=ceiling, max_gain_db=max_gain_db,
                                   want_float=not int16, want_int16=int16)
        return out["i16"] if int16 else out["f32"]

    def normalize_limited(self, audio: np.ndarray, target: float = -16.0, limiter=None, ceiling: float = 10 ** (-1 / 20),
                          max_gain_db: float = 30.0, int16: bool = True, samples=None) -> np.ndarray:
        """The rows at `target` LUFS through `limiter` (a `larynx_amd.limiter.Limiter` at this rate): each row takes the gain
        its level asks for, G = min(10^((target - L) / 20), 10^(max_gain_db / 20)) (f64, rounded once; 1 for L = -inf), and the
        limiter turns down what would pass the true-peak `ceiling`.  Limiting costs a little level, so the delivered float row
        is measured again on the device, and where it reads more than `LEVEL_TOLERANCE` under the target with G below its cap,
        ONE correction pass limits the row again with G raised by the deficit.  Rows that need no limiting equal `normalize`'s."""
        if limiter is None:
            raise ValueError("normalize_limited needs a Limiter")
        target = float(np.float32(target))
        cap = 10.0 ** (float(np.float32(max_gain_db)) / 20.0)

        def gains(lufs, base):
            with np.errstate(over="ignore"):
                g = np.where(np.isfinite(lufs), np.minimum(base * 10.0 ** ((target - lufs.astype(np.float64)) / 20.0), cap), 1.0)
            return g

        lufs = self.measure(audio, samples)
        g64 = gains(lufs, 1.0)
        out = self.engine.limit(limiter.model_id, audio, samples, gain=g64.astype(np.float32), ceiling=ceiling, want_float=True,
                                want_int16=int16)
        after = self.measure(out["f32"], samples)
        short = np.isfinite(lufs) & np.isfinite(after) & (after.astype(np.float64) < target - LEVEL_TOLERANCE) & (g64 < cap)
        if short.any():
            g64 = np.where(short, gains(after, g64), g64)
            out = self.engine.limit(limiter.model_id, audio, samples, gain=g64.astype(np.float32), ceiling=ceiling,
                                    want_float=not int16, want_int16=int16)
        return out["i16"] if int16 else out["f32"]


LEVEL_TOLERANCE = 0.1  # LU: the meter tolerance of EBU Tech 3341, the project's bound on a delivered level

def get_loudness(engine: Engine, sample_rate: int) -> Loudness:
    """One `Loudness` per (engine, rate), made on first use (the sentence path's `loudness=`) and kept ON the engine
    (`Engine.kept`): it lives and dies with the context its model id belongs to."""
    return engine.kept("loudness", int(sample_rate), lambda: Loudness(engine, int(sample_rate)))
