"""The true-peak meter and look-ahead limiter (csrc/limiter.h) on the MI355X: the check functions of tests/test_emu_limiter.py
under the same rules — bit equality with the float32 restatement without release, the curve within 16 x the restatement's own
error of the float64 oracle with it, the limiter property, batch rows and int16 input bit for bit —, the launches by kernel name,
device pointers as torch tensors, and what only the device has: a golden utterance end to end.  Every test prints what it measured."""
from pathlib import Path

import numpy as np
import pytest

from larynx_amd import synthetic
from tests.test_emu_limiter import (CEILING, FS, GAIN, LIMIT_KERNELS, LONG, METER_KERNELS, TILE, check_device_pointers, check_exact,
                                    check_int16_input, check_intersample, check_passthrough, check_ragged_batch, check_refusals, check_release,
                                    check_schedule, check_sentence_path, check_the_point, config, row)
from tests.test_emu_resample import torch_alloc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def leave_no_counts(request):
    yield
    if "gpu_engine" in request.fixturenames:
        request.getfixturevalue("gpu_engine").profile_reset()


def test_exact_without_release(gpu_engine):
    check_exact(gpu_engine)


def test_release_against_the_oracle(gpu_engine):
    check_release(gpu_engine)


def test_rows_under_the_ceiling_pass_unchanged(gpu_engine):
    check_passthrough(gpu_engine)


def test_ragged_batch(gpu_engine):
    check_ragged_batch(gpu_engine)


def test_int16_input(gpu_engine):
    check_int16_input(gpu_engine)


def test_intersample_peak(gpu_engine):
    check_intersample(gpu_engine)


def test_schedule_by_kernel_name(gpu_engine):
    """Two launches meter and six limit, under their names, for a short row and the long row; nothing else is counted."""
    check_schedule(gpu_engine)
    gpu_engine.profile_reset()
    cfg = config(gpu_engine)
    for n in (TILE + 1, LONG):
        gpu_engine.limit(cfg.model_id, row(n))
        gpu_engine.limit(cfg.model_id, row(n), gain=GAIN, ceiling=CEILING, want_int16=True)
    counts = {k: v for k, v in gpu_engine.kernel_counts().items() if v}
    print(counts)
    assert counts == {k: 2 * (v + METER_KERNELS.get(k, 0)) for k, v in LIMIT_KERNELS.items()}


def test_refusals_and_unload(gpu_engine):
    check_refusals(gpu_engine)


def test_the_target_is_reached(gpu_engine):
    check_the_point(gpu_engine)


def test_device_pointers(gpu_engine):
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE with torch tensors: tests/test_emu_limiter.py's check on the device's own memory."""
    pytest.importorskip("torch")
    check_device_pointers(gpu_engine, torch_alloc)


def test_sentence_path(gpu_engine):
    from tests.test_emu_analysis import tiny_voice
    from tests.test_emu_resample import vocoder

    check_sentence_path(tiny_voice(), vocoder())


def test_golden_utterance_end_to_end(gpu_engine):
    """The `echo` utterance of the golden set through `sentence_task_limited` at the full-size 'low' models: what
    `normalize_limited` gives for its float row, within 0.1 LU of the target, under the ceiling."""
    import larynx_amd
    from larynx_amd.audio import ljspeech_audio_settings
    from larynx_amd.constants import TextToSpeechModelConfig, VocoderModelConfig
    from larynx_amd.glow_tts import HipGlowTextToSpeech
    from larynx_amd.hifi_gan import HipHiFiGanVocoder
    from larynx_amd.limiter import get_limiter
    from larynx_amd.loudness import get_loudness
    from tests.golden_util import load_case

    c = load_case("ljspeech_low_echo")
    cfg = c["glow_hp"].to_config()
    cfg["audio"].update({k: v for k, v in vars(ljspeech_audio_settings()).items() if k != "mel_channels"})  # (the voice fuses the mel transforms)
    tts = HipGlowTextToSpeech(TextToSpeechModelConfig(model_path=Path("unused")), state_dict=synthetic.make_glow_state_dict(c["glow_hp"], seed=1234),
                              model_config=cfg)
    voc = HipHiFiGanVocoder(VocoderModelConfig(model_path=Path("unused")), state_dict=synthetic.make_hifigan_state_dict(c["voc_hp"], seed=1234),
                            model_config=c["voc_hp"].to_config())
    settings = {"seed": 5}
    s = tts.audio_settings
    assert s is not None and s.sample_rate == FS
    m, lim = get_loudness(voc.engine, FS), get_limiter(voc.engine, FS)
    fr = voc.mels_to_float_padded(tts.phonemes_to_mels(c["ids"], settings=settings), None, 0, 0)
    before = float(m.measure(fr)[0])
    for target in (-16.0, -8.0):  # the second asks for more than the row's peaks allow: the limiter works
        audio = larynx_amd.sentence_task_limited("echo", c["ids"], s, tts, settings, voc, None, 0, 0, None, target)
        exp = m.normalize_limited(fr, target=target, limiter=lim)
        single = float(m.measure(m.normalize(fr, target=target))[0])
        lufs, tp = float(m.measure(audio)[0]), float(lim.true_peak(audio)[0])
        print(f"echo: {audio.size} samples, float row {before:.2f} LUFS, peak {np.abs(fr).max():.3f}; target {target}: delivered {lufs:.3f} LUFS "
              f"(one gain: {single:.3f}), int16 peak {np.abs(audio.astype(np.int32)).max()}, true peak {tp:.5f}")
        assert audio.dtype == np.int16 and np.array_equal(audio, exp)
        assert np.abs(audio.astype(np.int32)).max() <= round(CEILING * 32768)
        if target == -16.0:
            assert abs(lufs - target) <= 0.1
