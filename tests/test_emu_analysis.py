"""Mel analysis (csrc/mel_analysis.h: waveform -> mi355tts_mel in one launch) on the CPU emulator.

Oracles.  REFERENCE framing: the fixtures tests/golden/analysis/*.npz, made by tools/make_golden_analysis.py from the reference's
own `transform` / `mel_basis` / `amp_to_db` / `normalize` / `dynamic_range_compression` in float64.  HIFIGAN framing (not in the
reference): the float64 restatement tests/analysis_np.py, pinned to those fixtures here through the REFERENCE framing.

Metrics (analysis_np): A = max |exp(voc) - exp(ref)| / max exp(ref); B = max |voc - ref| over the entries with amp_ref >= 1e-3 x
their frame's peak and amp_ref > 2e-5 (an ln-domain maximum over ALL entries is the wrong yardstick: the error is absolute, and
on the designed signal the float32 restatement itself lies 2e-3 from float64 where amplitudes are 1e-5); raw plane: B's
selection, in the normalised domain.  The selection must cover 100 % of the golden waveforms and >= 25 % of the designed signal.

Bound: the yardstick is what float32 costs the algorithm itself — the float32 restatement's deviation from the float64 one (the
anchor: stored in the fixture, computed here for inputs without one).  The device or emulator may lie 16 x as far (another FFT
factorisation, its logf / sqrtf), never above 1e-5 (A) or 1e-3 (B, raw).  The check functions are shared with
tests/test_gpu_analysis.py."""
import ctypes as C
import dataclasses
from pathlib import Path

import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.alignment import align_audio_spans, phoneme_spans
from larynx_amd.analysis import MelAnalyzer
from larynx_amd.audio import ljspeech_audio_settings, mel_basis
from tests import analysis_np as A
from tests.golden_util import GOLDEN

CASES = ("ljspeech_high_short5", "ljspeech_high_echo", "designed")
FRAMINGS = ("reference", "hifigan")
SETTINGS = ljspeech_audio_settings()
BASIS = mel_basis(22050, 1024, 80, 0.0, 8000)
RAGGED = (385, 10752, 34304, 10240)
_cache = {}


def wave(case):
    if case not in _cache:
        _cache[case] = A.designed_signal() if case == "designed" else np.load(GOLDEN / f"{case}.npz")["wav"].astype(np.float32)
    return _cache[case]


def fixture(case):
    z = np.load(GOLDEN / "analysis" / f"{case}.npz")
    return {k: z[k] for k in z.files}


def oracle(case, framing, settings=SETTINGS):
    """(amp, raw, voc) in float64 and the float32 anchors (a, b, raw) of a case; computed once."""
    key = (case, framing, id(settings))
    if key not in _cache:
        amp, raw, voc = A.analyze(wave(case), BASIS, framing, settings, np.float64)
        if settings is SETTINGS:
            fx = fixture(case)
            anchors = tuple(float(fx[f"f32_{framing}_{k}"]) for k in ("a", "b", "raw"))
            if framing == "reference":  # the reference's own chain, not the restatement
                amp, raw, voc = fx["ref_amp"], fx["ref_raw"], fx["ref_voc"]
        else:
            _, raw32, voc32 = A.analyze(wave(case), BASIS, framing, settings, np.float32)
            sel = A.selection(amp)
            anchors = (A.metric_a(voc32, voc), A.metric_b(voc32, voc, sel), A.metric_b(raw32, raw, sel))
        _cache[key] = (amp, raw, voc, anchors)
    return _cache[key]


def analysis_models(eng):
    key = ("models", id(eng))
    if key not in _cache:
        _cache[key] = {f: eng.load_analysis(BASIS, f) for f in FRAMINGS}
    return _cache[key]


def bounds(anchors):
    return min(16.0 * anchors[0], 1e-5), min(16.0 * anchors[1], 1e-3), min(16.0 * anchors[2], 1e-3)


def compare(tag, raw, voc, amp_ref, raw_ref, voc_ref, anchors, min_share):
    assert raw.shape == voc.shape == voc_ref.shape, (raw.shape, voc_ref.shape)
    assert np.isfinite(raw).all() and np.isfinite(voc).all()
    sel = A.selection(amp_ref)
    a, b, r = A.metric_a(voc, voc_ref), A.metric_b(voc, voc_ref, sel), A.metric_b(raw, raw_ref, sel)
    ba, bb, br = bounds(anchors)
    print(f"{tag}: A {a:.2e} (float32 restatement {anchors[0]:.2e}, bound {ba:.2e})  B {b:.2e} ({anchors[1]:.2e}, {bb:.2e})  "
          f"raw {r:.2e} ({anchors[2]:.2e}, {br:.2e})  selected {100 * sel.mean():.1f} %")
    assert sel.mean() >= min_share
    assert a <= ba and b <= bb and r <= br


def check_parity(eng, case, framing):
    mel = eng.mel_from_audio(analysis_models(eng)[framing], wave(case), audio_settings=SETTINGS)
    F = A.frame_count(framing, len(wave(case)))
    assert mel.shape == (1, 80, F) and list(mel.frames) == [F]
    with pytest.raises(ValueError):
        mel.durations  # like a wrapped buffer
    amp, raw, voc, anchors = oracle(case, framing)
    compare(f"{case} {framing}", mel.numpy("raw")[0], mel.numpy("voc")[0], amp, raw, voc, anchors, 0.25 if case == "designed" else 1.0)


def ragged_batch():
    rows = [wave("ljspeech_high_echo")[3000: 3000 + 385], wave("ljspeech_high_short5"), wave("ljspeech_high_echo"), wave("designed")]
    assert tuple(len(r) for r in rows) == RAGGED
    batch = np.full((len(rows), max(RAGGED)), 0.25, np.float32)  # what lies past a row's samples must not be read
    for b, r in enumerate(rows):
        batch[b, : len(r)] = r
    return rows, batch


def check_ragged(eng, framing):
    """Every row equals its batch-1 call bit for bit, tails are zero; 42 and 134 (38, 130) frames are no multiples of the 4
    frames a workgroup takes, the 385-sample row has one frame (none under the reference framing)."""
    rows, batch = ragged_batch()
    model = analysis_models(eng)[framing]
    mel = eng.mel_from_audio(model, batch, samples=RAGGED, audio_settings=SETTINGS)
    frames = [A.frame_count(framing, n) for n in RAGGED]
    assert list(mel.frames) == frames and mel.max_frames == max(frames)
    ptr, ld = mel.plane("voc")
    assert ptr and ld == (max(frames) + 3) // 4 * 4
    for which in ("raw", "voc"):
        got = mel.numpy(which)
        for b, r in enumerate(rows):
            assert np.all(got[b, :, frames[b]:] == 0)
            one = eng.mel_from_audio(model, r, audio_settings=SETTINGS)
            assert one.shape == (1, 80, frames[b])
            assert np.array_equal(one.numpy(which)[0], got[b, :, : frames[b]]), (which, b)
            if frames[b]:
                assert np.abs(got[b, :, : frames[b]]).max() > 0


def check_edges(eng):
    """Frame counts at the edges of both framings, one batched call each, every row against the float64 restatement."""
    src = wave("ljspeech_high_echo")[3000:]
    for framing, sizes, frames in (("hifigan", (0, 384, 385, 511, 512), (0, 0, 1, 1, 2)), ("reference", (1024, 1025, 1280, 1281), (0, 1, 1, 2))):
        model = analysis_models(eng)[framing]
        batch = np.stack([src[: max(sizes)]] * len(sizes))
        mel = eng.mel_from_audio(model, batch, samples=sizes, audio_settings=SETTINGS)
        assert tuple(mel.frames) == frames == tuple(A.frame_count(framing, n) for n in sizes)
        voc, raw = mel.numpy("voc"), mel.numpy("raw")
        for b, n in enumerate(sizes):
            one = eng.mel_from_audio(model, src[:n], audio_settings=SETTINGS)
            assert one.shape == (1, 80, frames[b]) and np.array_equal(one.numpy("voc")[0], voc[b, :, : frames[b]])
            if not frames[b]:
                assert one.max_frames == 0 and one.numpy("raw").shape == (1, 80, 0)
                continue
            amp64, raw64, voc64 = A.analyze(src[:n], BASIS, framing, SETTINGS, np.float64)
            _, raw32, voc32 = A.analyze(src[:n], BASIS, framing, SETTINGS, np.float32)
            sel = A.selection(amp64)
            anchors = (A.metric_a(voc32, voc64), A.metric_b(voc32, voc64, sel), A.metric_b(raw32, raw64, sel))
            compare(f"{framing} N={n}", raw[b, :, : frames[b]], voc[b, :, : frames[b]], amp64, raw64, voc64, anchors, 0.25)


def check_int16(eng, framing):
    """int16 samples are converted as s / 32768 inside the launch: the float call on that array gives the same bits."""
    i16 = np.load(GOLDEN / "ljspeech_high_short5.npz")["wav_i16"]
    assert i16.dtype == np.int16 and np.abs(i16).max() > 1000
    model = analysis_models(eng)[framing]
    a = eng.mel_from_audio(model, i16, audio_settings=SETTINGS)
    b = eng.mel_from_audio(model, A.as_float(i16, np.float32), audio_settings=SETTINGS)
    assert a.max_frames == A.frame_count(framing, len(i16)) > 0
    for which in ("raw", "voc"):
        assert np.array_equal(a.numpy(which), b.numpy(which))


def check_plain(eng, framing):
    """audio == NULL: both planes ln(max(amp, 1e-5)), the vocoder plane of a call with the ljspeech settings."""
    model = analysis_models(eng)[framing]
    plain = eng.mel_from_audio(model, wave("designed"))
    with_settings = eng.mel_from_audio(model, wave("designed"), audio_settings=SETTINGS)
    assert np.array_equal(plain.numpy("raw"), plain.numpy("voc")) and np.array_equal(plain.numpy("voc"), with_settings.numpy("voc"))
    assert abs(float(plain.numpy("voc").min()) - np.log(1e-5)) < 1e-5  # the designed signal reaches the clamp


# clipping starts at amp < 1e-3 with these levels (the ljspeech ones never clip): reached by selected entries of the designed signal
CLIPPING = dataclasses.replace(SETTINGS, min_level_db=-3.0, ref_level_db=0.0, max_norm=4.0)
SWITCHES = {"asymmetric": dataclasses.replace(CLIPPING, symmetric_norm=False), "no-clip": dataclasses.replace(CLIPPING, clip_norm=False),
            "no-db": dataclasses.replace(CLIPPING, convert_db_to_amp=False)}


def check_switches(eng, framing, name):
    s = SWITCHES[name]
    mel = eng.mel_from_audio(analysis_models(eng)[framing], wave("designed"), audio_settings=s)
    amp, raw, voc, anchors = oracle("designed", framing, s)
    got = mel.numpy("raw")[0]
    compare(f"designed {framing} {name}", got, mel.numpy("voc")[0], amp, raw, voc, anchors, 0.25)
    sel = A.selection(amp)
    lo = 0.0 if name == "asymmetric" else -4.0
    if name == "no-clip":
        assert got[sel].min() < lo and raw[sel].min() < lo
    else:
        assert got.min() == lo and (got[sel] == lo).any() and (raw[sel] == lo).any()  # selected entries sit at the limit
        assert got.max() <= 4.0


def check_inverse(eng, framing):
    """The raw plane through the mel transforms (`mel_from_numpy(raw, audio_settings)`) reproduces the vocoder plane on B's
    selection, within 16 x what the float32 numpy round trip of the same data shows."""
    mel = eng.mel_from_audio(analysis_models(eng)[framing], wave("designed"), audio_settings=SETTINGS)
    raw, voc = mel.numpy("raw"), mel.numpy("voc")
    sel = A.selection(oracle("designed", framing)[0])
    back = eng.mel_from_numpy(raw, audio_settings=SETTINGS).numpy("voc")
    d_np = A.metric_b(A.denormalize_to_voc(raw[0], SETTINGS, np.float32), voc[0], sel)
    d = A.metric_b(back[0], voc[0], sel)
    print(f"inverse {framing}: round trip {d:.2e} (float32 numpy round trip {d_np:.2e}, bound {16 * d_np:.2e})")
    assert 0 < d_np < 1e-3 and d <= 16.0 * d_np


def check_schedule(eng, framing):
    """One launch per call, and nothing else."""
    model = analysis_models(eng)[framing]
    eng.profile_reset()
    eng.mel_from_audio(model, ragged_batch()[1], samples=RAGGED, audio_settings=SETTINGS)
    counts = eng.kernel_counts()
    assert counts["mel_analysis_kernel"] == 1
    assert all(v == 0 for k, v in counts.items() if k != "mel_analysis_kernel"), counts


def _refused(fn, what):
    with pytest.raises(ffi.Mi355ttsError) as e:
        fn()
    assert e.value.code == -1 and what in str(e.value), str(e.value)


def check_refusals(eng):
    model = analysis_models(eng)["hifigan"]
    wav = np.ascontiguousarray(wave("ljspeech_high_short5"))
    i16 = np.zeros(len(wav), np.int16)
    for kw, what in ((dict(framing=2), "unknown framing"), (dict(mag_eps=-1.0), "mag_eps"), (dict(mag_eps=float("nan")), "mag_eps"),
                     (dict(mag_eps=float("inf")), "mag_eps")):
        _refused(lambda: eng.load_analysis(BASIS, **kw), what)
    lib, out, mid = eng.lib, C.c_void_p(), C.c_int()
    n = np.array([len(wav)], np.int64)
    n_p = n.ctypes.data_as(C.POINTER(C.c_int64))
    for num_mels in (0, 257):
        p = ffi.AnalysisParamsC(num_mels, 0, 0.0)
        _refused(lambda: ffi.check(lib, lib.mi355tts_load_analysis(eng._ctx, C.byref(p), BASIS.ctypes.data, C.byref(mid))), "num_mels")
    p = ffi.AnalysisParamsC(80, 0, 0.0)
    _refused(lambda: ffi.check(lib, lib.mi355tts_load_analysis(eng._ctx, C.byref(p), None, C.byref(mid))), "null")
    _refused(lambda: ffi.check(lib, lib.mi355tts_load_analysis(eng._ctx, None, BASIS.ctypes.data, C.byref(mid))), "null")

    def call(f32, s16, samples, out_p=C.byref(out)):
        return lambda: ffi.check(lib, lib.mi355tts_mel_from_audio(eng._ctx, model, f32, s16, samples, 1, len(wav), None, 0, out_p))

    _refused(call(wav.ctypes.data, i16.ctypes.data, n_p), "exactly one")
    _refused(call(None, None, n_p), "exactly one")
    _refused(call(wav.ctypes.data, None, None), "null")
    _refused(call(wav.ctypes.data, None, n_p, None), "null")
    for bad in (-1, len(wav) + 1):
        m = np.array([bad], np.int64)
        _refused(call(wav.ctypes.data, None, m.ctypes.data_as(C.POINTER(C.c_int64))), "samples[0]")
    with pytest.raises(ffi.Mi355ttsError) as e:
        eng.mel_from_audio(10 ** 6, wav)
    assert e.value.code == -5
    mel = eng.mel_from_audio(model, wav)  # the context still works
    ptr, ld = C.c_void_p(), C.c_int()
    _refused(lambda: ffi.check(lib, lib.mi355tts_mel_plane(mel.handle, 2, C.byref(ptr), C.byref(ld))), "which")
    assert mel.max_frames == 42 and np.isfinite(mel.numpy("voc")).all()


def tiny_voice(library_path=None):
    """A 16-channel voice with the ljspeech audio block: its own mel domain for `align_audio`."""
    from larynx_amd.constants import TextToSpeechModelConfig
    from larynx_amd.glow_tts import HipGlowTextToSpeech

    cfg = HP.TINY_GLOW.to_config()
    cfg["audio"].update({k: v for k, v in vars(SETTINGS).items() if k != "mel_channels"})
    return HipGlowTextToSpeech(TextToSpeechModelConfig(model_path=Path("unused")), library_path=library_path,
                               state_dict=synthetic.make_glow_state_dict(HP.TINY_GLOW, seed=3), model_config=cfg)


def check_align_audio(tts, framing):
    """A recording plus ids: exactly the durations of `align` on the host copy of the analysis' raw plane."""
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(4), 11, HP.TINY_GLOW.num_symbols)
    wav = wave("designed")
    dur = tts.align_audio(ids, wav, framing=framing)
    analyzer = tts._analyzers[framing]
    assert isinstance(analyzer, MelAnalyzer) and analyzer.mel_basis.shape == (16, 513)
    assert np.array_equal(tts.align_audio(ids, wav, framing=framing), dur) and tts._analyzers[framing] is analyzer  # one per framing, cached
    mel = analyzer.audio_to_mels(wav)
    F = A.frame_count(framing, len(wav))
    assert mel.shape == (1, 16, F)
    host = tts.align(ids, mel.numpy("raw"))
    assert dur.dtype == np.int32 and dur.shape == (len(ids),) and np.array_equal(dur, host) and np.array_equal(dur, tts.align(ids, mel))
    assert dur.min() >= 1 and dur.sum() == F // HP.TINY_GLOW.n_sqz * HP.TINY_GLOW.n_sqz
    assert np.array_equal(align_audio_spans(tts, ids, wav, 256, 7, framing=framing), phoneme_spans(host, 256, 7))


# ---------------------------------------------------------------- the emulator's runs
@pytest.mark.parametrize("case", CASES)
def test_restatement_against_the_reference_fixtures(case):
    """float64: the restatement IS the reference's chain (same operations in the same order: at most round-off apart).
    float32: reproduces the stored anchors (another FFT or BLAS build may move a maximum a little: within a factor 2)."""
    fx = fixture(case)
    assert int(fx["samples"]) == len(wave(case)) and fx["ref_amp"].dtype == np.float64
    amp, raw, voc = A.analyze(wave(case), BASIS, "reference", SETTINGS, np.float64)
    sel = A.selection(fx["ref_amp"])
    assert A.metric_a(voc, fx["ref_voc"]) <= 1e-12 and A.metric_b(voc, fx["ref_voc"], sel) <= 1e-10
    assert A.metric_b(raw, fx["ref_raw"], sel) <= 1e-10 and np.abs(amp - fx["ref_amp"]).max() <= 1e-10 * fx["ref_amp"].max()
    at_clamp = float((fx["ref_amp"] <= 1e-5).mean())
    assert (0.35 < at_clamp < 0.5) if case == "designed" else at_clamp == 0.0
    for framing in FRAMINGS:
        amp64, raw64, voc64 = A.analyze(wave(case), BASIS, framing, SETTINGS, np.float64)
        amp32, raw32, voc32 = A.analyze(wave(case), BASIS, framing, SETTINGS, np.float32)
        assert voc32.dtype == np.float32 and raw32.dtype == np.float32
        s64 = A.selection(amp64)
        assert float(fx[f"share_{framing}"]) == pytest.approx(s64.mean())
        assert not np.any((amp64 <= 1e-5) != (amp32 <= 1e-5))  # no entry changes clamp side between the precisions
        for key, got in (("a", A.metric_a(voc32, voc64)), ("b", A.metric_b(voc32, voc64, s64)), ("raw", A.metric_b(raw32, raw64, s64))):
            anchor = float(fx[f"f32_{framing}_{key}"])
            print(f"{case} {framing} float32 restatement {key}: {got:.2e} (stored {anchor:.2e})")
            assert 0.5 * anchor <= got <= 2.0 * anchor


@pytest.mark.parametrize("framing", FRAMINGS)
@pytest.mark.parametrize("case", CASES)
def test_parity(emu_engine, case, framing):
    check_parity(emu_engine, case, framing)


@pytest.mark.parametrize("framing", FRAMINGS)
def test_ragged_batch_rows_equal_their_batch1_calls(emu_engine, framing):
    check_ragged(emu_engine, framing)


def test_frame_count_edges(emu_engine):
    check_edges(emu_engine)


@pytest.mark.parametrize("framing", FRAMINGS)
def test_int16_input_and_no_settings(emu_engine, framing):
    check_int16(emu_engine, framing)
    check_plain(emu_engine, framing)


@pytest.mark.parametrize("name", sorted(SWITCHES))
@pytest.mark.parametrize("framing", FRAMINGS)
def test_normalisation_switches(emu_engine, framing, name):
    check_switches(emu_engine, framing, name)


@pytest.mark.parametrize("framing", FRAMINGS)
def test_inverse_consistency_and_schedule(emu_engine, framing):
    check_inverse(emu_engine, framing)
    check_schedule(emu_engine, framing)


def test_refusals_and_unload(emu_engine):
    check_refusals(emu_engine)
    m = emu_engine.load_analysis(BASIS, "reference")
    emu_engine.unload(m)
    with pytest.raises(ffi.Mi355ttsError):
        emu_engine.mel_from_audio(m, wave("designed"))
    with pytest.raises(ValueError):
        MelAnalyzer(emu_engine, dataclasses.replace(SETTINGS, hop_length=128))
    with pytest.raises(ValueError):
        MelAnalyzer(emu_engine, SETTINGS, framing="librosa")


def test_align_audio(emu_library):
    tts = tiny_voice(emu_library)
    for framing in FRAMINGS:
        check_align_audio(tts, framing)
