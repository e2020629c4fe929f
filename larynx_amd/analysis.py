"""Mel analysis on the HIP backend: a recording into a voice's own mel domain (`mi355tts_mel_from_audio`, one launch), the
direction the reference's inference path never takes — it carries `amp_to_db`, `normalize`, `dynamic_range_compression`
and `stft` (`larynx/audio.py:55-108, 232-249`) and calls none of them."""
from __future__ import annotations

import typing

import numpy as np

from . import ffi
from .audio import AudioSettings, mel_basis
from .engine import Engine, MelBatch


class MelAnalyzer:
    """`MelAnalyzer(engine, audio_settings, framing="hifigan")`: the filter bank comes from the settings (`sample_rate`,
    `mel_channels`, `mel_fmin`, `mel_fmax`), the two planes of the result from their normalisation switches.

    `framing` names the convention, and the choice is the caller's — which one a released voice was trained with is not
    recorded anywhere this library can read:
    "hifigan"    the published HiFi-GAN training convention (not part of the reference): reflect padding by 384 samples, periodic
                 Hann, sqrt(re^2 + im^2 + 1e-9); N samples give N // 256 frames, frame t centred on hop t;
    "reference"  the reference's own `stft`: no padding, symmetric `np.hanning(1024)`; ceil((N - 1024) / 256) frames.

    The STFT is 1024-point frames every 256 samples, as in the Griffin-Lim wrapper: other settings are rejected."""

    def __init__(self, engine: Engine, audio_settings: AudioSettings, framing: str = "hifigan",
                 mag_eps: typing.Optional[float] = None):
        if int(audio_settings.filter_length) != 1024 or int(audio_settings.hop_length) != 256:
            raise ValueError(f"the analysis is 1024-point frames every 256 samples, got filter_length="
                             f"{audio_settings.filter_length}, hop_length={audio_settings.hop_length}")
        if framing not in ffi.FRAMINGS:
            raise ValueError(f"framing must be one of {sorted(ffi.FRAMINGS)}, got {framing!r}")
        self.engine = engine
        self.audio_settings = audio_settings
        self.framing = framing
        self.mel_basis = mel_basis(audio_settings.sample_rate, 1024, audio_settings.mel_channels, audio_settings.mel_fmin,
                                   audio_settings.mel_fmax)
        self.model_id = engine.load_analysis(self.mel_basis, framing, mag_eps)

    def audio_to_mels(self, audio: np.ndarray, samples=None) -> MelBatch:
        """float32 in [-1, 1] or int16, [N] or [B, N] (row b valid for `samples[b]` entries) -> `MelBatch`."""
        return self.engine.mel_from_audio(self.model_id, audio, samples, self.audio_settings)
