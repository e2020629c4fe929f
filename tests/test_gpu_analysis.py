"""Mel analysis (csrc/mel_analysis.h) on the MI355X: the parity cases of tests/test_emu_analysis.py under the same rule — the
device may lie 16 x as far from the float64 oracle as the float32 restatement does, never above 1e-5 (A) or 1e-3 (B, raw) —,
the ragged batch, the int16 path, device pointers, the schedule, and the two consumers of the result: copy-synthesis through
HiFi-GAN and forced alignment from the device plane.  Every test prints what it measured."""
import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from tests.test_emu_analysis import (CASES, FRAMINGS, RAGGED, SETTINGS, SWITCHES, analysis_models, check_align_audio, check_edges,
                                     check_inverse, check_int16, check_parity, check_plain, check_ragged, check_refusals,
                                     check_schedule, check_switches, ragged_batch, tiny_voice, wave)
from tests.test_gpu_parity import models

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("framing", FRAMINGS)
@pytest.mark.parametrize("case", CASES)
def test_parity(gpu_engine, case, framing):
    check_parity(gpu_engine, case, framing)


@pytest.mark.parametrize("framing", FRAMINGS)
def test_ragged_batch_rows_equal_their_batch1_calls(gpu_engine, framing):
    check_ragged(gpu_engine, framing)


def test_frame_count_edges(gpu_engine):
    check_edges(gpu_engine)


@pytest.mark.parametrize("framing", FRAMINGS)
def test_int16_input_and_no_settings(gpu_engine, framing):
    check_int16(gpu_engine, framing)
    check_plain(gpu_engine, framing)


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_normalisation_switches(gpu_engine, name):
    for framing in FRAMINGS:
        check_switches(gpu_engine, framing, name)


@pytest.mark.parametrize("framing", FRAMINGS)
def test_inverse_consistency_and_schedule(gpu_engine, framing):
    check_inverse(gpu_engine, framing)
    check_schedule(gpu_engine, framing)


def test_refusals(gpu_engine):
    check_refusals(gpu_engine)


def test_device_pointers(gpu_engine):
    """MI355TTS_IN_DEVICE: torch tensors (float32 and int16, row stride past the rows' samples) give the host call's bits."""
    torch = pytest.importorskip("torch")
    _, batch = ragged_batch()
    model = analysis_models(gpu_engine)["hifigan"]
    host = gpu_engine.mel_from_audio(model, batch, samples=RAGGED, audio_settings=SETTINGS)
    dev = torch.from_numpy(batch).cuda().contiguous()
    torch.cuda.synchronize()
    mel = gpu_engine.mel_from_audio_raw(model, dev.data_ptr(), None, RAGGED, batch.shape[1], SETTINGS, flags=ffi.IN_DEVICE)
    assert list(mel.frames) == list(host.frames)
    for which in ("raw", "voc"):
        assert np.array_equal(mel.numpy(which), host.numpy(which))
    i16 = np.round(batch * 32767).astype(np.int16)
    host16 = gpu_engine.mel_from_audio(model, i16, samples=RAGGED, audio_settings=SETTINGS)
    dev16 = torch.from_numpy(i16).cuda().contiguous()
    torch.cuda.synchronize()
    mel16 = gpu_engine.mel_from_audio_raw(model, None, dev16.data_ptr(), RAGGED, i16.shape[1], SETTINGS, flags=ffi.IN_DEVICE)
    for which in ("raw", "voc"):
        assert np.array_equal(mel16.numpy(which), host16.numpy(which))


def test_copy_synthesis_plumbing(gpu_engine):
    """wav -> mel -> HiFi-GAN: the analysis `MelBatch` feeds the vocoder exactly like its host copy wrapped again."""
    _, (_, v) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_MEDIUM)
    mel = gpu_engine.mel_from_audio(analysis_models(gpu_engine)["hifigan"], wave("ljspeech_high_short5"), audio_settings=SETTINGS)
    direct, direct16 = gpu_engine.hifigan_infer(v, mel)
    again, again16 = gpu_engine.hifigan_infer(v, gpu_engine.mel_from_numpy(mel.numpy("voc")))
    assert direct.shape == (1, 42 * HP.HIFIGAN_MEDIUM.hop) and np.isfinite(direct).all() and np.abs(direct).max() > 0
    assert np.array_equal(direct, again) and np.array_equal(direct16, again16)


def test_glow_align_from_the_device_plane(gpu_engine):
    """`glow_align` on the `MelBatch` (its raw plane where it lies) equals `glow_align` on its host copy."""
    from larynx_amd import synthetic

    (_, g), _ = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_MEDIUM)
    ids = [synthetic.synthetic_phoneme_ids(np.random.default_rng(7 + b), n, HP.LJSPEECH.num_symbols) for b, n in enumerate((9, 31))]
    wav = np.zeros((2, 34304), np.float32)
    wav[0, :10752], wav[1] = wave("ljspeech_high_short5"), wave("ljspeech_high_echo")
    mel = gpu_engine.mel_from_audio(analysis_models(gpu_engine)["hifigan"], wav, samples=(10752, 34304), audio_settings=SETTINGS)
    assert list(mel.frames) == [42, 134]
    dur, score, z = gpu_engine.glow_align(g, ids, mel, want_latent=True)
    hdur, hscore, hz = gpu_engine.glow_align(g, ids, mel.numpy("raw"), frames=mel.frames, want_latent=True)
    assert np.array_equal(dur, hdur) and np.array_equal(score, hscore) and np.array_equal(z, hz)
    assert list(dur.sum(axis=1)) == [42, 134] and dur[0, :9].min() >= 1 and dur[1].min() >= 1


def test_align_audio(gpu_engine):
    tts = tiny_voice()
    for framing in FRAMINGS:
        check_align_audio(tts, framing)
