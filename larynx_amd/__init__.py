"""larynx_amd — the MI355X-native forward path of Larynx TTS.

phoneme ids -> GlowTTS -> mel transform -> HiFi-GAN -> waveform as hand-written
gfx950 HIP kernels behind a C ABI (`include/mi355tts.h`), wrapped in the
reference's own model interface.  Text handling (gruut, SSML), the CLI and the
HTTP server stay in Larynx; see INTEGRATION.md for the two edit points.
"""
from __future__ import annotations

import functools
import logging
import time
import typing
from concurrent.futures import Executor, ThreadPoolExecutor
from pathlib import Path

import numpy as np

from .audio import AudioSettings
from .constants import (
    InferenceBackend,
    SettingsType,
    TextToSpeechModel,
    TextToSpeechModelConfig,
    TextToSpeechResult,
    TextToSpeechType,
    VocoderModel,
    VocoderModelConfig,
    VocoderQuality,
    VocoderType,
)

_LOGGER = logging.getLogger("larynx_amd")

__all__ = [
    "AudioSettings", "InferenceBackend", "TextToSpeechResult", "load_tts_model", "load_vocoder_model",
    "sentence_task", "sentence_task_aligned", "sentence_task_at_rate", "sentence_task_leveled", "sentence_task_limited",
    "sentence_task_shifted", "phonemes_to_speech",
]


def load_tts_model(model_type, model_path, backend=InferenceBackend.HIP, no_optimizations: bool = False,
                   use_cuda: bool = True, half: bool = False, **kwargs) -> TextToSpeechModel:
    """Same signature as `larynx.load_tts_model` (`larynx/__init__.py:379-407`)."""
    config = TextToSpeechModelConfig(model_path=Path(model_path), use_cuda=use_cuda, half=half, backend=backend)
    if model_type == TextToSpeechType.GLOW_TTS:
        from .glow_tts import HipGlowTextToSpeech

        return HipGlowTextToSpeech(config, **kwargs)
    raise ValueError(f"Unknown text to speech model type: {model_type}")


def load_vocoder_model(model_type, model_path, backend=InferenceBackend.HIP, no_optimizations: bool = False,
                       use_cuda: bool = True, half: bool = False, denoiser_strength: float = 0.0,
                       executor: typing.Optional[Executor] = None, **kwargs) -> VocoderModel:
    """Same signature as `larynx.load_vocoder_model` (`larynx/__init__.py:472-508`)."""
    config = VocoderModelConfig(model_path=Path(model_path), use_cuda=use_cuda, half=half,
                                denoiser_strength=denoiser_strength, backend=backend)
    if model_type == VocoderType.HIFI_GAN:
        from .hifi_gan import HipHiFiGanVocoder

        return HipHiFiGanVocoder(config, executor=executor, **kwargs)
    if model_type == VocoderType.GRIFFIN_LIM:
        # no weights: `model_path` is ignored, as in the reference (`larynx/__init__.py:498-501`)
        from .griffin_lim import HipGriffinLimVocoder

        return HipGriffinLimVocoder(config, **kwargs)
    raise ValueError(f"Unknown vocoder model type: {model_type}")


def sentence_task(text: str, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                  pause_before_ms: int = 0, pause_after_ms: int = 0) -> np.ndarray:
    """The per-sentence hot loop, argument for argument the reference's
    `_sentence_task` (`larynx/__init__.py:214-285`): GlowTTS, the mel transforms
    (numpy here only if the model did not already fuse them), the vocoder, the
    three debug log lines and the SSML pause padding."""
    return _sentence(text, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                     pause_before_ms, pause_after_ms)[0]


def sentence_task_at_rate(text: str, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                          pause_before_ms: int = 0, pause_after_ms: int = 0, sample_rate: typing.Optional[int] = None) -> np.ndarray:
    """`sentence_task` delivered at `sample_rate` Hz: the vocoder's FLOAT row, SSML pauses included, is resampled on the
    device and normalised to int16 afterwards (`larynx_amd.resample`; the peak lands on 32767 at the new rate), n samples
    becoming ceil(n * up / down).  `None`, or the voice's own rate, is `sentence_task`."""
    return _sentence(text, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                     pause_before_ms, pause_after_ms, sample_rate)[0]


def sentence_task_leveled(text: str, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                          pause_before_ms: int = 0, pause_after_ms: int = 0, sample_rate: typing.Optional[int] = None,
                          loudness: typing.Optional[float] = None) -> np.ndarray:
    """`sentence_task` delivered at `loudness` LUFS: the vocoder's FLOAT row, SSML pauses included (and resampled first when
    `sample_rate` asks for another rate), is measured on the device (BS.1770 integrated loudness at the delivered rate) and
    becomes int16 there at ONE gain, under a -1 dBFS sample-peak ceiling (`larynx_amd.loudness`).  This replaces the peak
    normalisation for this call only; `loudness=None` is `sentence_task_at_rate`."""
    return _sentence(text, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                     pause_before_ms, pause_after_ms, sample_rate, loudness)[0]


def sentence_task_limited(text: str, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                          pause_before_ms: int = 0, pause_after_ms: int = 0, sample_rate: typing.Optional[int] = None,
                          loudness: typing.Optional[float] = None) -> np.ndarray:
    """`sentence_task_leveled` through the true-peak limiter: the float row takes the gain its level asks for, whatever its
    peaks, and the limiter turns down only what would pass the -1 dBFS TRUE-peak ceiling, on the device
    (`Loudness.normalize_limited`, `larynx_amd.limiter`): the row reaches `loudness` LUFS where the single gain of
    `sentence_task_leveled` stops at the ceiling.  `loudness` is required."""
    if loudness is None:
        raise ValueError("limiter: valid only together with loudness")
    return _sentence(text, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                     pause_before_ms, pause_after_ms, sample_rate, loudness, True)[0]


def sentence_task_aligned(text: str, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                          pause_before_ms: int = 0, pause_after_ms: int = 0, sample_rate: typing.Optional[int] = None,
                          loudness: typing.Optional[float] = None, limiter: typing.Optional[bool] = None) -> typing.Tuple[np.ndarray, np.ndarray]:
    """`sentence_task` that also returns where every phoneme id sounds: `(audio, spans)`, spans int64 [P, 2] in samples
    of `audio`, leading pause included (`larynx_amd.alignment.phoneme_spans`).  The TTS model must be one whose mels
    carry durations (`HipGlowTextToSpeech`); the audio is what `sentence_task` gives for the same settings.  With a
    Griffin-Lim vocoder the spans are nominal frame positions (hop 256), see `phoneme_spans`.  With `sample_rate` (see
    `sentence_task_at_rate`) the spans are positions in the delivered audio: both ends scaled by (s * up) // down.  `loudness`
    (see `sentence_task_leveled`; with `limiter`, `sentence_task_limited`) changes the level of the audio, not the spans."""
    return _aligned(text, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings, pause_before_ms,
                    pause_after_ms, sample_rate, loudness, limiter)


def sentence_task_shifted(text: str, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                          pause_before_ms: int = 0, pause_after_ms: int = 0, sample_rate: typing.Optional[int] = None,
                          loudness: typing.Optional[float] = None, limiter: typing.Optional[bool] = None,
                          pitch_shift: typing.Optional[float] = None, alignment: bool = False):
    """`sentence_task` with the voice's pitch moved by `pitch_shift` semitones (in [-12, 12]; meant for about +-4: the formants
    move with the pitch): the vocoder's FLOAT row, SSML pauses included, goes through the period-synchronous pitch shifter on
    the device at the voice's rate (`larynx_amd.shift`) BEFORE `sample_rate`, `loudness` and `limiter` act on it as in the
    other tasks; with none of them the shifter's own normalised int16 is delivered (the peak lands on 32767 after the shift).
    The duration is unchanged.  `alignment`: `(audio, spans)` as `sentence_task_aligned` gives them, the spans unchanged by
    the shift.  `None` or 0 semitones is the task the other arguments name."""
    shifter = _shifter_for(vocoder_model, audio_settings, pitch_shift)
    if alignment:
        return _aligned(text, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings, pause_before_ms,
                        pause_after_ms, sample_rate, loudness, limiter, shifter)
    if limiter and loudness is None:
        raise ValueError("limiter: valid only together with loudness")
    return _sentence(text, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings,
                     pause_before_ms, pause_after_ms, sample_rate, loudness, bool(limiter), shifter)[0]


def _aligned(text, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings, pause_before_ms,
             pause_after_ms, sample_rate, loudness, limiter, shifter=None):
    if limiter and loudness is None:
        raise ValueError("limiter: valid only together with loudness")
    settings = dict(tts_settings or {})
    settings["alignment"] = True
    audio, mels, before, resampler = _sentence(text, phoneme_ids, audio_settings, tts_model, settings, vocoder_model,
                                               vocoder_settings, pause_before_ms, pause_after_ms, sample_rate, loudness, bool(limiter),
                                               shifter)
    from .alignment import phoneme_spans, scale_spans

    durations = getattr(mels, "durations", None)
    if durations is None:
        raise ValueError("the text-to-speech model's mels carry no per-phoneme durations")
    hparams = getattr(vocoder_model, "hparams", None)
    hop = int(hparams.hop) if hparams is not None else 256  # Griffin-Lim: hard-wired 256 (larynx/audio.py:284,297)
    spans = phoneme_spans(durations[0], hop, pad_before=before)
    return audio, (spans if resampler is None else scale_spans(spans, resampler.up, resampler.down))


def _resampler_for(vocoder_model, audio_settings, sample_rate):
    """The cached `Resampler` from the voice's rate to `sample_rate`, or None where the voice's own rate is delivered."""
    voice_rate = audio_settings.sample_rate if audio_settings is not None else 22050
    if sample_rate is None or int(sample_rate) == int(voice_rate):
        return None
    engine = getattr(vocoder_model, "engine", None)
    if engine is None:
        raise ValueError("sample_rate: the vocoder has no HIP engine to resample on")
    from .resample import get_resampler

    return get_resampler(engine, voice_rate, sample_rate)


def _shifter_for(vocoder_model, audio_settings, pitch_shift):
    """The cached `PitchShifter` at the voice's rate for `pitch_shift` semitones, or None for None / 0; outside [-12, 12]: a
    ValueError."""
    if pitch_shift is None:
        return None
    from .shift import check_semitones, get_pitch_shifter

    if check_semitones(pitch_shift) == 0.0:
        return None
    engine = getattr(vocoder_model, "engine", None)
    if engine is None:
        raise ValueError("pitch_shift: the vocoder has no HIP engine to shift on")
    return get_pitch_shifter(engine, audio_settings.sample_rate if audio_settings is not None else 22050, pitch_shift)


def _float_row(vocoder_model, mels, vocoder_settings, before, after) -> np.ndarray:
    """The vocoder's float signal with the SSML pauses in it: what is resampled BEFORE the int16 normalisation."""
    padded = getattr(vocoder_model, "mels_to_float_padded", None)
    if padded is not None:
        return padded(mels, vocoder_settings, before, after)
    audio = np.asarray(vocoder_model.mels_to_audio(mels, settings=vocoder_settings))
    if audio.dtype.kind != "f":
        raise ValueError("sample_rate: the vocoder delivers no float signal to resample")
    return np.pad(audio.astype(np.float32, copy=False), pad_width=(before, after), constant_values=0)


def _sentence(text, phoneme_ids, audio_settings, tts_model, tts_settings, vocoder_model, vocoder_settings, pause_before_ms,
              pause_after_ms, deliver_rate=None, deliver_lufs=None, limited=False, shifter=None):
    """-> (audio, the mels the vocoder consumed, leading pause in samples at the voice's rate, the `Resampler` the audio went
    through or None).  `shifter` (a `PitchShifter` at the voice's rate): the float row goes through it first."""
    t0 = time.perf_counter()
    mels = tts_model.phonemes_to_mels(phoneme_ids, settings=tts_settings)
    tts_mels = mels
    t1 = time.perf_counter()
    _LOGGER.debug("Got mels in %s second(s) (shape=%s, text='%s')", t1 - t0, getattr(mels, "shape", None), text)
    if audio_settings is not None and (audio_settings.signal_norm or audio_settings.convert_db_to_amp
                                       or audio_settings.do_dynamic_range_compression):
        # a non-fused TextToSpeechModel (e.g. the reference's own GlowTextToSpeech feeding the HIP
        # vocoder): the three transforms still run in-kernel, applied while wrapping the array
        from .glow_tts import mels_as_numpy

        mels = vocoder_model.engine.mel_from_numpy(mels_as_numpy(mels), audio_settings=audio_settings)
    sample_rate = audio_settings.sample_rate if audio_settings is not None else 22050
    before = max(0, (pause_before_ms * sample_rate) // 1000)
    after = max(0, (pause_after_ms * sample_rate) // 1000)
    lead = before
    t2 = time.perf_counter()
    resampler = _resampler_for(vocoder_model, audio_settings, deliver_rate)
    padded = getattr(vocoder_model, "mels_to_audio_padded", None)
    shifted = None
    if shifter is not None:
        # the float row, pauses included, shifted at the voice's rate: what the delivery stages below then take, or — with none
        # of them — the shifter's own normalised int16
        shifted = shifter.shift(_float_row(vocoder_model, mels, vocoder_settings, before, after),
                                normalize=deliver_lufs is None and resampler is None)
    if shifted is not None and deliver_lufs is None and resampler is None:
        audio = shifted
        before = after = 0
    elif deliver_lufs is not None:
        # a level target: the float row, pauses included, at the delivered rate; measured, scaled and made int16 on the device
        engine = getattr(vocoder_model, "engine", None)
        if engine is None:
            raise ValueError("loudness: the vocoder has no HIP engine to measure on")
        from .loudness import get_loudness

        row = shifted if shifted is not None else _float_row(vocoder_model, mels, vocoder_settings, before, after)
        if resampler is not None:
            row = resampler.resample(row)
            sample_rate = resampler.rate_out
        if limited:  # the full gain, and the true-peak limiter in place of the single gain's cap
            from .limiter import get_limiter

            audio = get_loudness(engine, sample_rate).normalize_limited(row, target=float(deliver_lufs), limiter=get_limiter(engine, sample_rate))
        else:
            audio = get_loudness(engine, sample_rate).normalize(row, target=float(deliver_lufs))
        before = after = 0
    elif resampler is not None:
        # another rate: the float row, pauses included, resampled on the device and normalised to int16 there
        row = shifted if shifted is not None else _float_row(vocoder_model, mels, vocoder_settings, before, after)
        audio = resampler.resample(row, normalize=True)
        sample_rate = resampler.rate_out
        before = after = 0
    elif padded is not None and (before or after):
        # SSML pauses written by the device's int16 kernel instead of np.pad (same samples)
        audio = padded(mels, vocoder_settings, before, after)
        before = after = 0
    else:
        audio = vocoder_model.mels_to_audio(mels, settings=vocoder_settings)
    t3 = time.perf_counter()
    _LOGGER.debug("Got audio in %s second(s) (shape=%s, text='%s')", t3 - t2, audio.shape, text)
    dur = audio.shape[-1] / sample_rate
    _LOGGER.debug("Real-time factor: %0.2f (infer=%0.2f sec, audio=%0.2f sec)", (t3 - t0) / dur if dur > 0 else 0.0, t3 - t0, dur)
    if before or after:
        audio = np.pad(audio, pad_width=(before, after), constant_values=0)
    return audio, tts_mels, lead, resampler


def _with_pitch(task, engine, sample_rate, aligned, *args):
    """`task(*args)` with the YIN track of the audio it delivered (at `sample_rate`, pauses included) behind it, in the same pool
    thread: (audio, spans or None, track, per-phoneme pitch or None)."""
    from .pitch import get_pitch_tracker, pitch_per_span

    audio, spans = task(*args) if aligned else (task(*args), None)
    track = get_pitch_tracker(engine, sample_rate).track(np.ascontiguousarray(audio))
    return audio, spans, track, (pitch_per_span(track, spans) if aligned else None)


def _ensure_pool_workers(executor, *models):
    """One worker per pool thread (+ a spare) on the models' engine before the first sentence is submitted: the engine then knows
    which worker streams share a hardware queue and spreads the sentences' calls evenly (Engine.ensure_workers)."""
    n = getattr(executor, "_max_workers", None)
    if not isinstance(n, int) or n < 2:
        return
    for m in models:
        eng = getattr(m, "engine", None)
        if eng is not None and hasattr(eng, "ensure_workers"):
            eng.ensure_workers(min(n, 32) + 1)


def phonemes_to_speech(sentences: typing.Iterable[typing.Tuple[str, typing.Sequence[int]]], tts_model, vocoder_model,
                       tts_settings: typing.Optional[SettingsType] = None,
                       vocoder_settings: typing.Optional[SettingsType] = None,
                       executor: typing.Optional[Executor] = None, alignment: bool = False,
                       sample_rate: typing.Optional[int] = None,
                       loudness: typing.Optional[float] = None,
                       limiter: typing.Optional[bool] = None, pitch: bool = False,
                       pitch_shift: typing.Optional[float] = None) -> typing.Iterable[TextToSpeechResult]:
    """`text_to_speech` (`larynx/__init__.py:47-190`) from the point where gruut /
    phonemes2ids have produced ids: one task per sentence on an executor, results
    yielded in submission order.  `alignment`: every result also carries `phoneme_spans`, the start and end sample
    of each phoneme id in its audio (`sentence_task_aligned`); the audio is the same either way.  `sample_rate`: deliver
    the audio at that rate instead of the voice's own (`sentence_task_at_rate`: resampled on the device, int16 of
    ceil(n * up / down) samples, spans scaled to match); `None` or the voice's rate changes nothing.  `loudness`: deliver
    every sentence at that many LUFS instead of with its peak on 32767 (`sentence_task_leveled`); `None` changes nothing.
    `limiter=True` (only together with `loudness`): through the true-peak limiter, so that the level is reached whatever the
    sentence's peaks (`sentence_task_limited`); `None` or `False` changes nothing.  `pitch=True`: every result also carries
    `pitch`, the YIN track of its delivered audio at the delivered rate, pauses included (`larynx_amd.pitch`), and, together
    with `alignment`, `phoneme_pitch`, the median f0 and voiced share of every phoneme; the audio is the same either way.
    `pitch_shift`: move the voice's pitch by that many semitones, in [-12, 12] (`sentence_task_shifted`: the float row is
    shifted on the device at the voice's rate before `sample_rate`, `loudness` and `limiter` act; duration and `phoneme_spans`
    unchanged; `pitch=True` then reads the shifted pitch); `None` or 0 changes nothing and runs nothing new."""
    if limiter and loudness is None:
        raise ValueError("limiter: valid only together with loudness")
    shifting = _shifter_for(vocoder_model, getattr(tts_model, "audio_settings", None), pitch_shift) is not None  # (made here, once)
    if pitch and getattr(vocoder_model, "engine", None) is None:
        raise ValueError("pitch: the vocoder has no HIP engine to track on")
    own = executor is None
    executor = executor or ThreadPoolExecutor()
    _ensure_pool_workers(executor, tts_model, vocoder_model)
    try:
        audio_settings = getattr(tts_model, "audio_settings", None)
        sr = audio_settings.sample_rate if audio_settings is not None else 22050
        task = sentence_task_aligned if alignment else sentence_task
        if _resampler_for(vocoder_model, audio_settings, sample_rate) is not None:  # (made here, once, before the pool needs it)
            sr = int(sample_rate)
            task = functools.partial(sentence_task_aligned if alignment else sentence_task_at_rate, sample_rate=sr)
        if loudness is not None:  # (the voice's own rate as `sample_rate` is no resampling)
            task = functools.partial(sentence_task_aligned if alignment else sentence_task_leveled, sample_rate=sr, loudness=float(loudness))
            if limiter:
                task = (functools.partial(sentence_task_aligned, sample_rate=sr, loudness=float(loudness), limiter=True) if alignment
                        else functools.partial(sentence_task_limited, sample_rate=sr, loudness=float(loudness)))
        if shifting:  # (the one task that takes every other switch)
            task = functools.partial(sentence_task_shifted, sample_rate=sr, loudness=None if loudness is None else float(loudness),
                                     limiter=bool(limiter), pitch_shift=float(pitch_shift), alignment=alignment)
        if pitch:  # (a wrapper around whichever task the other switches chose; made here, once, before the pool needs it)
            from .pitch import get_pitch_tracker

            get_pitch_tracker(vocoder_model.engine, sr)
            task = functools.partial(_with_pitch, task, vocoder_model.engine, sr, alignment)
        futures = []
        for text, ids in sentences:
            fut = executor.submit(task, text, np.asarray(ids, np.int64), audio_settings, tts_model, tts_settings,
                                  vocoder_model, vocoder_settings)
            futures.append((text, fut))
        for text, fut in futures:
            if pitch:
                audio, spans, track, per_phoneme = fut.result()
                yield TextToSpeechResult(text=text, audio=audio, sample_rate=sr, phoneme_spans=spans, pitch=track, phoneme_pitch=per_phoneme)
                continue
            audio, spans = fut.result() if alignment else (fut.result(), None)
            yield TextToSpeechResult(text=text, audio=audio, sample_rate=sr, phoneme_spans=spans)
    finally:
        if own:
            executor.shutdown(wait=True)
