"""Griffin-Lim vocoder on the HIP backend — drop-in for
`larynx.griffin_lim.GriffinLimVocoder` (`larynx/griffin_lim.py:22-76`): mel to
waveform with no weights, so a voice directory without a generator checkpoint can
still be heard."""
from __future__ import annotations

import typing

import numpy as np

from .audio import mel_basis
from .constants import ARRAY_OR_TENSOR, InferenceBackend, SettingsType, VocoderModel, VocoderModelConfig
from .engine import MelBatch
from .runtime import get_engine


class HipGriffinLimVocoder(VocoderModel):
    """The reference's constructor keywords (`sample_rate, num_fft, num_mels, mel_fmin, mel_fmax, mel_scaling,
    iterations`) plus `device`, `library_path` and `seed`.

    The reference hard-wires 1024-point frames every 256 samples in its STFT helpers (`larynx/audio.py:284,297`)
    whatever `num_fft` says; `num_fft` only sizes the mel filter bank, which must have 513 columns to multiply the
    spectrum — so anything but 1024 is rejected here instead of failing inside numpy.

    The initial phase is drawn on the device.  `seed=None` (default) draws a fresh 64-bit seed per call from numpy's
    global generator — as irreproducible as the reference's `np.random.rand`, and like it controlled by
    `np.random.seed`; an int seed (here or as `settings["seed"]`) makes a call reproducible.  `settings` may also carry
    `iterations`.

    All arithmetic is float32: a mel that is not in the ln domain (magnitudes beyond ~1e30) is out of scope."""

    def __init__(self, config: VocoderModelConfig, sample_rate: int = 22050, num_fft: int = 1024, num_mels: int = 80,
                 mel_fmin: float = 0.0, mel_fmax: float = 8000, mel_scaling: float = 1000.0, iterations: int = 60,
                 device: int = 0, library_path=None, seed: typing.Optional[int] = None):
        super().__init__(config)
        if config.backend not in (None, InferenceBackend.HIP):
            raise ValueError(f"Unknown backend: {config.backend}")
        if int(num_fft) != 1024:
            raise ValueError(f"num_fft must be 1024 (the STFT is 1024-point frames every 256 samples), got {num_fft}")
        self.engine = get_engine(device, library_path)
        self.mel_basis = mel_basis(sample_rate, num_fft, num_mels, mel_fmin, mel_fmax)
        self.mel_channels = int(num_mels)
        self.mel_scaling = float(mel_scaling)
        self.iterations = int(iterations)
        self.seed = seed
        self.model_id = self.engine.load_griffin_lim(self.mel_basis, self.mel_scaling, self.iterations)

    def _batch(self, mels: ARRAY_OR_TENSOR) -> MelBatch:
        if isinstance(mels, MelBatch):
            return mels
        if not isinstance(mels, np.ndarray) and hasattr(mels, "cpu"):  # a torch tensor, as the reference accepts
            mels = mels.detach().cpu().numpy()
        return self.engine.mel_from_numpy(np.asarray(mels, np.float32))

    def _run(self, mels, settings, want_float, want_int16, phase0=None):
        iterations, seed = self.iterations, self.seed
        if settings:
            iterations = int(settings.get("iterations", iterations))
            seed = settings.get("seed", seed)
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        batch = self._batch(mels)
        f32, i16, _ = self.engine.griffin_lim_infer(self.model_id, batch, phase0=phase0, seed=int(seed), iterations=iterations,
                                                    want_float=want_float, want_int16=want_int16)
        out = f32 if want_float else i16
        if batch.batch != 1:
            return out
        T = max(int(batch.frames[0]) - 1, 0)
        return out[0, : T * 256 + 1024 if T else 0]

    def mels_to_audio(self, mels: ARRAY_OR_TENSOR, settings: typing.Optional[SettingsType] = None) -> np.ndarray:
        """`[1, 80, F]` (numpy / torch) or a device-resident `MelBatch` -> the float signal `[(F - 1) * 256 + 1024]`
        (`griffin_lim_iter(spec[:, :, :-1]).squeeze(0)`, griffin_lim.py:56-60).  The reference returns float64; this
        returns float32.  A batch of more than one row returns `[B, N]`, short rows zero-filled."""
        return self._run(mels, settings, True, False)

    def mels_to_int16(self, mels: ARRAY_OR_TENSOR, settings: typing.Optional[SettingsType] = None) -> np.ndarray:
        """`audio_float_to_int16(mels_to_audio(...))` (`larynx/audio.py:118-125`), computed on the device."""
        return self._run(mels, settings, False, True)

    def mels_to_audio_with_phase(self, mels: ARRAY_OR_TENSOR, phase0: np.ndarray,
                                 settings: typing.Optional[SettingsType] = None) -> np.ndarray:
        """`mels_to_audio` from an injected initial phase `[513, F - 1]` (what parity with the reference is defined on)."""
        return self._run(mels, settings, True, False, phase0=np.asarray(phase0, np.float32))
