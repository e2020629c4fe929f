"""The Griffin-Lim vocoder (csrc/griffin_lim.h) on the CPU emulator: registry dispatch, parity with the reference's
fixtures (tests/golden/griffin_lim/*.npz, made by tools/make_golden_griffin_lim.py from the reference's own functions),
the mel filter bank, `sentence_task`, the degenerate inputs, and the numpy restatement the device tests use as their
oracle for shapes without a fixture."""
import importlib.util
import json
import os
from pathlib import Path

import numpy as np
import pytest

import larynx_amd
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.audio import ljspeech_audio_settings, mel_basis
from larynx_amd.constants import InferenceBackend, TextToSpeechType, VocoderType
from larynx_amd.griffin_lim import HipGriffinLimVocoder
from tests import griffin_lim_np as G
from tests.golden_util import GOLDEN, reference_has

FIXTURES = ("ljspeech_high_short5", "ljspeech_high_echo")
REF = Path(os.environ.get("LARYNX_REFERENCE", "/root/reference"))


def load_fixture(case):
    z = np.load(GOLDEN / "griffin_lim" / f"{case}.npz")
    fx = {k: z[k] for k in z.files}
    mel = np.load(GOLDEN / f"{case}.npz")["mel_voc"].astype(np.float32)
    fx["mel"] = mel if mel.ndim == 3 else mel[None]
    fx["phase0"] = G.initial_phase(int(fx["phase_seed"]), fx["mel"].shape[2] - 1)
    return fx


def parity_bound(fx, iters):
    """16 x what float32 arithmetic costs the reference's own algorithm on this case, never above 1e-4."""
    return min(16.0 * float(fx[f"ref_f32_rel_rms_{iters}"]), 1e-4)


@pytest.fixture(scope="module")
def vocoder(emu_library_path):
    return larynx_amd.load_vocoder_model(VocoderType.GRIFFIN_LIM, "no-such-directory", backend=InferenceBackend.HIP,
                                         library_path=emu_library_path)


def test_registry_dispatches_griffin_lim(vocoder, emu_library_path):
    assert isinstance(vocoder, HipGriffinLimVocoder)
    assert vocoder.mel_basis.shape == (80, 513) and vocoder.iterations == 60 and vocoder.mel_scaling == 1000.0
    with pytest.raises(ValueError):
        larynx_amd.load_vocoder_model(VocoderType.GRIFFIN_LIM, "x", library_path=emu_library_path, num_fft=2048)


def test_mel_basis_matches_the_reference():
    fx = load_fixture(FIXTURES[0])
    ours = mel_basis(22050, 1024, 80, 0.0, 8000)
    ref = fx["mel_basis"]
    assert ours.shape == ref.shape == (80, 513) and ours.dtype == np.float32
    assert np.array_equal(ours == 0, ref == 0)  # the same support
    nz = ref != 0
    assert np.max(np.abs(ours[nz] - ref[nz]) / np.abs(ref[nz])) <= 1e-6
    np.testing.assert_allclose(ours.reshape(-1)[fx["mel_basis_sample_index"]], fx["mel_basis_sample"], rtol=1e-6, atol=0)


@pytest.mark.parametrize("case", FIXTURES)
def test_parity_with_the_reference(vocoder, case):
    fx = load_fixture(case)
    eng = vocoder.engine
    mel = eng.mel_from_numpy(fx["mel"])
    T = fx["mel"].shape[2] - 1
    for iters in (1, 60):
        f32, i16, ph = eng.griffin_lim_infer(vocoder.model_id, mel, phase0=fx["phase0"], iterations=iters, want_int16=True, want_phase=True)
        ref = fx[f"signal_{iters}"]
        assert f32.shape == (1, T * 256 + 1024) and f32.shape[1] == ref.shape[0]
        assert np.isfinite(f32).all() and np.array_equal(ph[0], fx["phase0"])
        err = G.rel_rms(f32[0], ref)
        print(f"{case} iterations={iters}: rel rms {err:.3e} (bound {parity_bound(fx, iters):.3e})")
        assert err <= parity_bound(fx, iters)
        if iters == 60:
            assert np.abs(i16[0].astype(np.int32) - fx["int16_60"].astype(np.int32)).max() <= 1
    # the class interface: float32 [N] from a reference-style array, int16 through the device's conversion
    audio = vocoder.mels_to_audio_with_phase(fx["mel"], fx["phase0"])
    assert audio.dtype == np.float32 and audio.shape == fx["signal_60"].shape
    assert np.array_equal(audio, f32[0])


def test_seeded_mode_and_settings(vocoder):
    fx = load_fixture(FIXTURES[0])
    a = vocoder.mels_to_audio(fx["mel"], {"seed": 11, "iterations": 2})
    b = vocoder.mels_to_audio(fx["mel"], {"seed": 11, "iterations": 2})
    c = vocoder.mels_to_audio(fx["mel"], {"seed": 12, "iterations": 2})
    assert a.dtype == np.float32 and np.array_equal(a, b) and not np.array_equal(a, c)
    eng = vocoder.engine
    mel = eng.mel_from_numpy(fx["mel"])
    f1, _, ph = eng.griffin_lim_infer(vocoder.model_id, mel, seed=11, iterations=2, want_phase=True)
    f2, _, _ = eng.griffin_lim_infer(vocoder.model_id, mel, phase0=ph, iterations=2)
    assert np.array_equal(f1[0], a) and np.array_equal(f1, f2)
    assert -np.pi < float(ph.min()) and float(ph.max()) <= np.pi and abs(float(ph.mean())) < 0.1
    i16 = vocoder.mels_to_int16(fx["mel"], {"seed": 11, "iterations": 2})
    assert i16.dtype == np.int16 and np.abs(i16.astype(np.int32) - G.float_to_int16(a).astype(np.int32)).max() <= 1
    counts0 = eng.kernel_counts()
    vocoder.mels_to_audio(fx["mel"], {"seed": 1, "iterations": 5})
    counts1 = eng.kernel_counts()
    assert counts1["griffin_lim_iter_kernel"] - counts0["griffin_lim_iter_kernel"] == 5
    assert counts1["griffin_lim_init_kernel"] - counts0["griffin_lim_init_kernel"] == 1


def test_ragged_batch_rows_equal_their_batch1_results(vocoder):
    fx = load_fixture(FIXTURES[1])
    eng = vocoder.engine
    lens = (12, 30, 2, 1)
    mel = np.zeros((len(lens), 80, max(lens)), np.float32)
    for b, n in enumerate(lens):
        mel[b, :, :n] = fx["mel"][0, :, 10 * b: 10 * b + n]
    ph = np.random.default_rng(3).uniform(-3.0, 3.0, (len(lens), 513, max(lens) - 1)).astype(np.float32)
    f32, i16, _ = eng.griffin_lim_infer(vocoder.model_id, eng.mel_from_numpy(mel, frames=lens), phase0=ph, iterations=3, want_int16=True)
    assert np.isfinite(f32).all()
    for b, n in enumerate(lens):
        N = (n - 1) * 256 + 1024 if n > 1 else 0
        assert np.all(f32[b, N:] == 0) and np.all(i16[b, N:] == 0)
        if n < 2:
            continue
        one, one16, _ = eng.griffin_lim_infer(vocoder.model_id, eng.mel_from_numpy(mel[b:b + 1, :, :n]), phase0=ph[b:b + 1, :, : n - 1],
                                              iterations=3, want_int16=True)
        assert np.array_equal(one[0], f32[b, :N]) and np.array_equal(one16[0], i16[b, :N])
        assert np.abs(f32[b, :N]).max() > 0


def test_degenerate_inputs(vocoder):
    eng = vocoder.engine
    # one frame: no STFT frame, an empty signal
    one = np.zeros((1, 80, 1), np.float32)
    f32, i16, ph = eng.griffin_lim_infer(vocoder.model_id, eng.mel_from_numpy(one), seed=1, want_int16=True, want_phase=True)
    assert f32.shape == (1, 0) and i16.shape == (1, 0) and ph.shape == (1, 513, 0)
    assert vocoder.mels_to_audio(one).shape == (0,)
    # exp(-200) underflows to 0 in float32: zero magnitudes, so from the second transform on every |S| is 0 — the
    # (mag, 0) rule instead of 0 / 0.  Silent frames next to loud ones must stay finite too.
    mel = np.full((1, 80, 9), -200.0, np.float32)
    f32, i16, _ = eng.griffin_lim_infer(vocoder.model_id, eng.mel_from_numpy(mel), seed=2, iterations=3, want_int16=True)
    assert f32.shape == (1, 8 * 256 + 1024) and np.all(f32 == 0) and np.all(i16 == 0)
    mel[0, :, :3] = 1.0
    f32, _, _ = eng.griffin_lim_infer(vocoder.model_id, eng.mel_from_numpy(mel), seed=2, iterations=3)
    assert np.isfinite(f32).all() and np.abs(f32).max() > 0
    with pytest.raises(larynx_amd.ffi.Mi355ttsError):  # 40 channels into an 80-channel vocoder
        eng.griffin_lim_infer(vocoder.model_id, eng.mel_from_numpy(np.zeros((1, 40, 5), np.float32)))


def test_model_is_unloaded_like_the_others(emu_engine):
    m = emu_engine.load_griffin_lim(mel_basis(22050, 1024, 80, 0.0, 8000))
    emu_engine.unload(m)
    with pytest.raises(larynx_amd.ffi.Mi355ttsError):
        emu_engine.griffin_lim_infer(m, emu_engine.mel_from_numpy(np.zeros((1, 80, 4), np.float32)))
    with pytest.raises(larynx_amd.ffi.Mi355ttsError):
        emu_engine.load_griffin_lim(np.zeros((300, 513), np.float32))


def test_sentence_task_with_a_glow_tts_model(emu_library_path, tmp_path):
    gdir = tmp_path / "tiny-glow_tts"
    gdir.mkdir()
    cfg = HP.TINY_GLOW.to_config()
    cfg["audio"].update({k: v for k, v in vars(ljspeech_audio_settings()).items() if k != "mel_channels"})
    (gdir / "config.json").write_text(json.dumps(cfg))
    np.savez(gdir / "generator.npz", **synthetic.make_glow_state_dict(HP.TINY_GLOW, seed=3))
    tts = larynx_amd.load_tts_model(TextToSpeechType.GLOW_TTS, gdir, library_path=emu_library_path)
    voc = larynx_amd.load_vocoder_model(VocoderType.GRIFFIN_LIM, tmp_path, library_path=emu_library_path,
                                        num_mels=HP.TINY_GLOW.mel_channels, iterations=4, seed=7)
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(2), 13, HP.TINY_GLOW.num_symbols)
    setattr(tts, "audio_settings", ljspeech_audio_settings())  # the registry attaches it after construction
    frames = np.asarray(tts.phonemes_to_mels(ids, {"noise_scale": 0.0})).shape[2]
    audio = larynx_amd.sentence_task("hello", ids, getattr(tts, "audio_settings"), tts, {"noise_scale": 0.0}, voc, None,
                                     pause_before_ms=10, pause_after_ms=20)
    assert audio.dtype == np.float32 and audio.shape == (220 + (frames - 1) * 256 + 1024 + 441,)
    assert np.isfinite(audio).all() and np.all(audio[:220] == 0) and np.all(audio[-441:] == 0) and np.abs(audio).max() > 0


@pytest.mark.parametrize("case", FIXTURES)
def test_numpy_restatement_against_the_fixtures(case):
    """float64: the reference itself stores its spectrum as complex64 (audio.py:279), which costs it ~2e-7 against exact
    arithmetic at every iteration count (no amplification), so 1e-6 holds with room.  float32: reproduces the stored figure."""
    fx = load_fixture(case)
    mag = G.magnitudes(fx["mel"][0], fx["mel_basis"], 1000.0, np.float64)
    _, kept = G.griffin_lim(mag, fx["phase0"], 60, np.float64, keep=(1, 60))
    for iters in (1, 60):
        assert kept[iters].shape == fx[f"signal_{iters}"].shape
        assert G.rel_rms(kept[iters], fx[f"signal_{iters}"]) <= 1e-6
    assert np.abs(G.float_to_int16(kept[60]).astype(np.int32) - fx["int16_60"].astype(np.int32)).max() <= 1
    mag32 = G.magnitudes(fx["mel"][0], fx["mel_basis"], 1000.0, np.float32)
    _, kept32 = G.griffin_lim(mag32, fx["phase0"], 60, np.float32, keep=(1, 60))
    for iters in (1, 60):
        assert kept32[iters].dtype == np.float32
        assert G.rel_rms(kept32[iters], fx[f"signal_{iters}"]) == pytest.approx(float(fx[f"ref_f32_rel_rms_{iters}"]), rel=0.05)


@pytest.mark.skipif(not reference_has(REF / "larynx" / "griffin_lim.py"), reason="needs the reference checkout")
def test_numpy_restatement_against_the_reference_functions():
    """The reference's own `inverse` / `transform` (loaded by file path: `import larynx` needs gruut) on a shape without a
    fixture, iteration by iteration."""
    spec = importlib.util.spec_from_file_location("_ref_larynx_audio", REF / "larynx" / "audio.py")
    audio = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(audio)
    rng = np.random.default_rng(5)
    T = 23
    mag = (np.exp(rng.normal(0.0, 1.5, (513, T))) * 1000.0).astype(np.float32)
    phase0 = G.initial_phase(9, T)
    np.testing.assert_allclose(mel_basis(22050, 1024, 80, 0.0, 8000), audio.mel_basis(22050, 1024, 80, 0.0, 8000), rtol=1e-6, atol=0)
    sig = audio.inverse(mag[None], phase0[None])
    _, kept = G.griffin_lim(mag, phase0, 6, np.float64, keep=tuple(range(7)))
    for it in range(7):
        assert G.rel_rms(kept[it], sig[0]) <= 1e-6, it
        _, ang = audio.transform(sig)
        sig = audio.inverse(mag[None], ang)
