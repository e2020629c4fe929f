"""Phoneme timings: from the frames every phoneme id occupies (`MelBatch.durations`, the reference's
`attn.sum(-1)`, glow_tts/models.py:350-354) to sample positions in the delivered audio; `align_spans` does the same for a
mel that already exists (forced alignment, `HipGlowTextToSpeech.align`), `align_audio_spans` for a recording, `scale_spans`
moves spans to another sample rate."""
from __future__ import annotations

import numpy as np


def phoneme_spans(durations, hop: int, pad_before: int = 0) -> np.ndarray:
    """`durations` [P] (frames per id) -> int64 [P, 2]: id t sounds in samples [start, end) of the audio, with
    start = pad_before + hop * (frames before t) and end = pad_before + hop * (frames up to and including t).
    `pad_before` is the leading pause in samples (`_sentence_task`'s pause_before_ms).  An id without frames has
    an empty span (start == end) at its position; the last end is pad_before + F * hop.

    With the HiFi-GAN vocoder these are exact: frame j becomes samples [j * hop, (j + 1) * hop).  Griffin-Lim audio
    has (F - 1) * 256 + 1024 samples (overlapping 1024-sample frames every 256): the spans there are NOMINAL frame
    positions, hop 256 — the last ends can lie past the middle of the final frame's window."""
    d = np.asarray(durations, np.int64).reshape(-1)
    if np.any(d < 0):
        raise ValueError("durations must be >= 0")
    end = np.cumsum(d)
    spans = np.stack([end - d, end], axis=1) * int(hop) + int(pad_before)
    return spans.astype(np.int64)


def align_spans(tts_model, phoneme_ids, mels, hop: int, pad_before: int = 0, settings=None) -> np.ndarray:
    """The `phoneme_spans` of an existing mel: `tts_model.align(phoneme_ids, mels, settings)` (the best monotonic path of the
    ids through the mel under the voice's own likelihood) -> int64 [P, 2] sample positions."""
    return phoneme_spans(tts_model.align(phoneme_ids, mels, settings), hop, pad_before)


def align_audio_spans(tts_model, phoneme_ids, audio, hop: int = 256, pad_before: int = 0, settings=None,
                      framing: str = "hifigan") -> np.ndarray:
    """The `phoneme_spans` of a recording: `tts_model.align_audio(phoneme_ids, audio, settings, framing)` -> int64 [P, 2]
    sample positions in `audio`.  Under the "hifigan" framing frame j is centred on samples [j * hop, (j + 1) * hop), the
    relation `phoneme_spans` relies on; under "reference" frame j covers [j * hop, j * hop + 1024)."""
    return phoneme_spans(tts_model.align_audio(phoneme_ids, audio, settings, framing), hop, pad_before)


def scale_spans(spans, up: int, down: int) -> np.ndarray:
    """Sample positions at the voice's rate -> positions in audio resampled by `up / down` (`larynx_amd.resample`): both ends
    of every span become (s * up) // down, so contiguous spans stay contiguous and no end lies past the ceil(n * up / down)
    delivered samples."""
    return (np.asarray(spans, np.int64) * int(up)) // int(down)
