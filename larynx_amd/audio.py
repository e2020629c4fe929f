"""Audio settings of a voice, as the HIP path needs them.

`AudioSettings` accepts exactly the keys a voice's `config.json["audio"]` carries, so
`AudioSettings(**config["audio"])` (rhasspy/larynx `larynx/__init__.py:352-356`) keeps
working, and defaults match the reference's record (`larynx/audio.py:26-50`).  Unlike the
reference class it has no numpy methods: the three mel transforms `_sentence_task`
applies between the two networks (`larynx/__init__.py:242-249`) run inside the HIP path
(kernel `mel_finalize`, csrc/small_kernels.h); this record only carries their parameters
across the C ABI (`mi355tts_audio_settings`).
"""
from __future__ import annotations

import dataclasses
import typing

# (name, type, default) — STFT geometry first, then the normalisation switches the
# kernel reads.  Only the second group influences the arithmetic.
_STFT_FIELDS = (
    ("filter_length", int, 1024), ("hop_length", int, 256), ("win_length", int, 256),
    ("mel_channels", int, 80), ("sample_rate", int, 22050), ("sample_bytes", int, 2), ("channels", int, 1),
    ("mel_fmin", float, 0.0), ("mel_fmax", typing.Optional[float], 8000.0),
)
_NORM_FIELDS = (
    ("ref_level_db", float, 20.0), ("spec_gain", float, 1.0), ("signal_norm", bool, False),
    ("min_level_db", float, -100.0), ("max_norm", float, 4.0), ("clip_norm", bool, True),
    ("symmetric_norm", bool, True), ("do_dynamic_range_compression", bool, True), ("convert_db_to_amp", bool, True),
)

import numpy as np

AudioSettings = dataclasses.make_dataclass(
    "AudioSettings",
    [(n, t, dataclasses.field(default=d)) for n, t, d in _STFT_FIELDS + _NORM_FIELDS],
    namespace={"__doc__": "Mel (de)normalisation parameters of a voice; see the module docstring."},
)
AudioSettings.__module__ = __name__


def ljspeech_audio_settings() -> "AudioSettings":
    """The `audio` block of `local/en-us/ljspeech-glow_tts/config.json` (thorsten's is identical)."""
    return AudioSettings(win_length=1024, signal_norm=True, max_norm=1.0)


# ---- Slaney mel filter bank (the Griffin-Lim vocoder's magnitudes: exp(mel) @ mel_basis) -------------------------------
# Auditory Toolbox (Slaney 1998) mel scale, as librosa's default `htk=False` filters use it and the reference builds them
# (`larynx/audio.py:131-161`): linear below 1 kHz at 200/3 Hz per mel, logarithmic above with 27 mels per factor of 6.4;
# triangular filters between consecutive band edges, each scaled by 2 / (its width in Hz) ("constant energy per channel").
_MEL_HZ_PER_MEL = 200.0 / 3.0
_MEL_BREAK_HZ = 1000.0
_MEL_BREAK = _MEL_BREAK_HZ / _MEL_HZ_PER_MEL
_MEL_LOGSTEP = np.log(6.4) / 27.0


def _hz_to_mel(hz):
    hz = np.asarray(hz, np.float64)
    return np.where(hz >= _MEL_BREAK_HZ, _MEL_BREAK + np.log(np.maximum(hz, _MEL_BREAK_HZ) / _MEL_BREAK_HZ) / _MEL_LOGSTEP,
                    hz / _MEL_HZ_PER_MEL)


def _mel_to_hz(mel):
    mel = np.asarray(mel, np.float64)
    return np.where(mel >= _MEL_BREAK, _MEL_BREAK_HZ * np.exp(_MEL_LOGSTEP * (np.maximum(mel, _MEL_BREAK) - _MEL_BREAK)),
                    mel * _MEL_HZ_PER_MEL)


def mel_basis(sample_rate: int, num_fft: int, num_mels: int = 80, fmin: float = 0.0,
              fmax: typing.Optional[float] = None) -> np.ndarray:
    """[num_mels, 1 + num_fft // 2] float32 filter bank; computed in float64 and rounded once per entry."""
    if fmax is None:
        fmax = sample_rate / 2.0
    bins = np.linspace(0.0, sample_rate / 2.0, 1 + num_fft // 2)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), int(num_mels) + 2))
    lo, mid, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    rising = (bins[None, :] - lo) / (mid - lo)
    falling = (hi - bins[None, :]) / (hi - mid)
    tri = np.maximum(0.0, np.minimum(rising, falling))
    return (tri.astype(np.float32) * (2.0 / (hi - lo)).astype(np.float64)).astype(np.float32)
