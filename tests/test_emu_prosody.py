"""Phoneme timings out, per-phoneme duration control in (`mi355tts_prosody`) on the CPU emulator build: scaled durations
against the oracle, the round trip durations_out -> durations_in, ragged batches, the error returns and the Python surface.
The `check_*` functions take the engine, so tests/test_gpu_prosody.py runs them on the device as well."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.alignment import phoneme_spans
from larynx_amd.audio import ljspeech_audio_settings
from oracle import glow_tts_np

F32 = np.float32
SCALE_SET = np.array([0.0, 0.5, 0.75, 1.0, 1.5, 2.0], F32)
MARGIN = 1e-5  # every scaled duration's distance from an integer, relative: the device's logw sits ~1e-6 from the oracle's


@pytest.fixture(scope="module")
def tiny(emu_engine):
    gsd = synthetic.make_glow_state_dict(HP.TINY_GLOW, seed=7)
    vsd = synthetic.make_hifigan_state_dict(HP.TINY_HIFIGAN, seed=7)
    return dict(gsd=gsd, vsd=vsd, g=emu_engine.load_glow(HP.TINY_GLOW, gsd), v=emu_engine.load_hifigan(HP.TINY_HIFIGAN, vsd))


# ---------------------------------------------------------------- expected values (numpy, float32 like the kernel)
def scaled_w(logw, length_scale, scales=None):
    """w = (exp(logw) * length_scale) * scale in float32 and in this order (what ceil sees)."""
    w = (np.exp(np.asarray(logw, F32)).astype(F32) * F32(length_scale)).astype(F32)
    return w if scales is None else (w * np.asarray(scales, F32)).astype(F32)


def clears_margin(w, margin=MARGIN):
    """True when no w > 0 lies within `margin` (relative) of an integer; w == 0 (a zero scale) is exact."""
    w = np.asarray(w, np.float64)
    w = w[w > 0]
    return bool(np.all(np.abs(w - np.round(w)) > margin * w))


def attn_durations(d, n_sqz):
    """-> (what the reference's attn[b, 0, t, :].sum() is for durations d, the row's frame count F)"""
    cum = np.cumsum(np.asarray(d, np.int64))
    F = (max(int(cum[-1]), 1) // n_sqz) * n_sqz
    return np.diff(np.minimum(cum, F), prepend=0).astype(np.int32), F


def draw_scales(n, seed, logw=None, length_scale=1.0):
    """Seeded scales from SCALE_SET with at least one 0 and one non-unit value; with `logw`, the first seed at or after
    `seed` whose scaled durations clear MARGIN (a choice made on the CPU from the oracle's logw, never from the device)."""
    for s in range(seed, seed + 1000):
        sc = np.random.default_rng(s).choice(SCALE_SET, size=n).astype(F32)
        if n >= 2 and (not np.any(sc == 0) or not np.any((sc != 0) & (sc != 1))):
            continue
        if logw is None or clears_margin(scaled_w(logw, length_scale, sc)):
            return sc
    raise AssertionError("no seed found")


def oracle_with_durations(sd, hp, ids, d, noise, noise_scale, speaker_id=None):
    """text_encoder -> expansion by the durations d -> + noise * noise_scale -> flow_decoder_reverse"""
    g = glow_tts_np.speaker_vector(sd, hp, speaker_id)
    x_m, _ = glow_tts_np.text_encoder(sd, np.asarray(ids, np.int64), hp, None, g)
    cum = np.cumsum(np.asarray(d, np.int64))
    _, F = attn_durations(d, hp.n_sqz)
    if F == 0:
        return np.zeros((hp.mel_channels, 0), F32)
    idx = np.minimum(np.searchsorted(cum, np.arange(F), side="right"), len(ids) - 1)
    z = x_m[:, idx]
    if noise is not None and noise_scale != 0.0:
        z = z + np.asarray(noise, F32)[:, :F] * F32(noise_scale)
    return glow_tts_np.flow_decoder_reverse(sd, z.astype(F32), hp, None, g)


def oracle_logw(sd, hp, ids, speaker_id=None):
    g = glow_tts_np.speaker_vector(sd, hp, speaker_id)
    return np.asarray(glow_tts_np.text_encoder(sd, np.asarray(ids, np.int64), hp, None, g)[1], F32).reshape(-1)


# ---------------------------------------------------------------- checks shared with the device suite
def check_scaled_against_oracle(eng, g, sd, hp, ids, logw, length_scale, noise_scale, seed, atol, rtol):
    """Durations exact, mel within (atol, rtol) of the oracle run with the expected durations."""
    sc = draw_scales(len(ids), seed, logw, length_scale)
    w = scaled_w(logw, length_scale, sc)
    assert clears_margin(w)  # precondition on the fixture
    assert np.any(sc == 0) and np.any((sc != 0) & (sc != 1))
    d = np.ceil(w).astype(np.int64)
    exp_d, F = attn_durations(d, hp.n_sqz)
    noise = np.random.default_rng(seed + 1).standard_normal((hp.mel_channels, int(d.sum()) + 8)).astype(F32)
    mel = eng.glow_infer(g, ids, noise_scale, length_scale, noise=noise, id_scales=sc)
    got_d = mel.durations
    assert got_d.dtype == np.int32 and got_d.shape == (1, len(ids))
    assert np.array_equal(got_d[0], exp_d), (got_d[0], exp_d)
    assert int(mel.frames[0]) == F == int(got_d.sum())
    ref = oracle_with_durations(sd, hp, ids, d, noise, noise_scale)
    np.testing.assert_allclose(mel.numpy("raw")[0], ref, atol=atol, rtol=rtol)
    return sc


def check_round_trip(eng, g, ids, length_scale=1.0, seed=11, scales=None):
    """durations_out fed back as durations_in reproduces the raw mel bit for bit (same seed, then same noise);
    id_scales all 1.0 is bit-identical to no prosody."""
    plain = eng.glow_infer(g, ids, 0.667, length_scale, seed=seed)
    a = eng.glow_infer(g, ids, 0.667, length_scale, seed=seed, want_durations=True, id_scales=scales)
    if scales is None:
        assert np.array_equal(a.frames, plain.frames) and np.array_equal(a.numpy("raw"), plain.numpy("raw"))
    ones = eng.glow_infer(g, ids, 0.667, length_scale, seed=seed, id_scales=np.ones(len(ids), F32))
    assert np.array_equal(ones.frames, plain.frames) and np.array_equal(ones.numpy("raw"), plain.numpy("raw"))
    assert np.array_equal(ones.numpy("vocoder"), plain.numpy("vocoder"))
    d = a.durations
    assert int(d.sum()) == int(a.frames[0])
    # (length_scale is not read for the durations: any value must do)
    b = eng.glow_infer(g, ids, 0.667, 3.0 * length_scale, seed=seed, durations=d[0])
    assert np.array_equal(b.frames, a.frames) and np.array_equal(b.durations, d)
    assert np.array_equal(b.numpy("raw"), a.numpy("raw"))
    M = a.channels
    noise = np.random.default_rng(seed).standard_normal((M, int(a.frames[0]) + 4)).astype(F32)
    c1 = eng.glow_infer(g, ids, 0.667, length_scale, noise=noise, id_scales=scales, want_durations=True)
    c2 = eng.glow_infer(g, ids, 0.667, length_scale, noise=noise, durations=c1.durations[0])
    assert np.array_equal(c1.durations, d) and np.array_equal(c2.durations, d)
    assert np.array_equal(c1.numpy("raw"), c2.numpy("raw"))


def check_ragged_batch(eng, g, num_symbols, lens=(9, 30, 17), seed=5, atol=2e-5, rtol=1e-4):
    """A ragged batch with a scale vector per row equals its rows run alone with the same row seeds: durations
    exact, mel within the bar of test_glow_variable_length_batch_equals_rowwise, entries past a row's length 0."""
    rng = np.random.default_rng(seed)
    rows = [synthetic.synthetic_phoneme_ids(rng, n, num_symbols) for n in lens]
    scales = [draw_scales(n, seed + 10 * b) for b, n in enumerate(lens)]
    seeds = [900 + 7 * b for b in range(len(lens))]
    mel = eng.glow_infer(g, rows, 0.5, 1.1, row_seeds=seeds, id_scales=scales)
    d = mel.durations
    assert d.shape == (len(lens), max(lens)) and d.dtype == np.int32
    got = mel.numpy("raw")
    for b, ids in enumerate(rows):
        solo = eng.glow_infer(g, ids, 0.5, 1.1, row_seeds=[seeds[b]], id_scales=scales[b])
        F = int(solo.frames[0])
        assert int(mel.frames[b]) == F
        assert np.array_equal(d[b, : lens[b]], solo.durations[0]) and np.all(d[b, lens[b]:] == 0)
        assert int(d[b].sum()) == F
        assert np.all(d[b, : lens[b]][scales[b] == 0] == 0)
        np.testing.assert_allclose(got[b, :, :F], solo.numpy("raw")[0], atol=atol, rtol=rtol)
        assert np.all(got[b, :, F:] == 0)


# ---------------------------------------------------------------- emulator tests
def test_scaled_durations_against_the_oracle(emu_engine, tiny):
    hp = HP.TINY_GLOW
    for n, ls, seed in ((23, 1.0, 3), (40, 0.8, 4), (5, 1.3, 6)):
        ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(seed), n, hp.num_symbols)
        logw = oracle_logw(tiny["gsd"], hp, ids)
        check_scaled_against_oracle(emu_engine, tiny["g"], tiny["gsd"], hp, ids, logw, ls, 0.667, seed, atol=2e-5, rtol=1e-4)


def test_plain_durations_are_the_references_attention_sums(emu_engine, tiny):
    """Want_durations alone: expected = diff(min(cumsum(ceil(exp(logw) ls)), F)), the truncated last id included."""
    hp = HP.TINY_GLOW
    odd = 0
    for seed in range(20, 32):
        ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(seed), 10 + seed % 7, hp.num_symbols)
        w = scaled_w(oracle_logw(tiny["gsd"], hp, ids), 1.0)
        if not clears_margin(w):
            continue
        d = np.ceil(w).astype(np.int64)
        exp_d, F = attn_durations(d, hp.n_sqz)
        odd += int(d.sum()) != F
        mel = emu_engine.glow_infer(tiny["g"], ids, 0.3, 1.0, seed=seed, want_durations=True)
        assert np.array_equal(mel.durations[0], exp_d) and int(mel.frames[0]) == F
    assert hp.n_sqz == 1 or odd > 0  # the truncation rule was exercised


def test_round_trip(emu_engine, tiny):
    hp = HP.TINY_GLOW
    for n, seed in ((23, 11), (64, 12), (130, 13), (1, 14)):
        ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(seed), n, hp.num_symbols)
        check_round_trip(emu_engine, tiny["g"], ids, 1.0, seed)
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(15), 31, hp.num_symbols)
    check_round_trip(emu_engine, tiny["g"], ids, 0.9, 15, scales=draw_scales(31, 15))


def test_ragged_batch_equals_rows_alone(emu_engine, tiny):
    check_ragged_batch(emu_engine, tiny["g"], HP.TINY_GLOW.num_symbols)


def check_fused_call(eng, g, v, ids, hop, seed=21):
    """The fused call with durations_out only = the two-call path's durations; frames and int16 samples = those
    of the plain fused call with the same seed, bit for bit."""
    s = ljspeech_audio_settings()
    two = eng.glow_infer(g, ids, 0.667, 1.0, seed=seed, audio_settings=s, want_durations=True)
    f0, _, i0 = eng.synthesize(g, v, ids, 0.667, 1.0, seed=seed, audio_settings=s, pad_before=3, pad_after=4)
    f1, _, i1, d1 = eng.synthesize(g, v, ids, 0.667, 1.0, seed=seed, audio_settings=s, pad_before=3, pad_after=4, return_durations=True)
    assert np.array_equal(d1, two.durations) and d1.dtype == np.int32
    assert np.array_equal(f0, f1) and np.array_equal(f1, two.frames) and np.array_equal(i0, i1)
    # durations in through the fused call: the same audio again
    f2, _, i2, d2 = eng.synthesize(g, v, ids, 0.667, 1.0, seed=seed, audio_settings=s, pad_before=3, pad_after=4, durations=d1[0],
                                   return_durations=True)
    assert np.array_equal(f2, f1) and np.array_equal(i2, i1) and np.array_equal(d2, d1)
    assert i1.shape[1] == 3 + int(f1[0]) * hop + 4


def test_fused_call(emu_engine, tiny):
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(21), 19, HP.TINY_GLOW.num_symbols)
    check_fused_call(emu_engine, tiny["g"], tiny["v"], ids, HP.TINY_HIFIGAN.hop)


def test_fused_call_fills_durations_when_the_buffer_is_too_small(emu_engine, tiny):
    """MI355TTS_ERR_TOO_SMALL: durations_out is filled like frames_out."""
    lib = emu_engine.lib
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(22), 12, HP.TINY_GLOW.num_symbols)
    want = emu_engine.glow_infer(tiny["g"], ids, 0.667, 1.0, seed=5, want_durations=True)
    lens = np.array([12], np.int32)
    dout = np.full((1, 12), -1, np.int32)
    p = ffi.ProsodyC(None, None, dout.ctypes.data_as(C.POINTER(C.c_int32)), 12)
    frames = np.zeros(1, np.int32)
    i16 = np.zeros((1, 8), np.int16)
    rc = lib.mi355tts_synthesize_prosody(emu_engine._ctx, tiny["g"], tiny["v"], ids.ctypes.data, lens.ctypes.data_as(C.POINTER(C.c_int32)),
                                         1, 12, 0.667, 1.0, None, 0, 5, None, None, 0.0, 0, 0,
                                         frames.ctypes.data_as(C.POINTER(C.c_int32)), None, i16.ctypes.data, 8, 0, C.byref(p))
    assert rc == -4
    assert np.array_equal(frames, want.frames) and np.array_equal(dout, want.durations)


def _infer_rc(eng, g, ids, prosody, out):
    lens = np.array([len(ids)], np.int32)
    return eng.lib.mi355tts_glow_infer_prosody(eng._ctx, g, ids.ctypes.data, lens.ctypes.data_as(C.POINTER(C.c_int32)), 1, len(ids),
                                               0.667, 1.0, None, 0, 1, None, None, None, 0, C.byref(prosody), C.byref(out))


def test_errors(emu_engine, tiny):
    """MI355TTS_ERR_INVALID (-1), a message, and the process goes on."""
    lib, g = emu_engine.lib, tiny["g"]
    n = 9
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(30), n, HP.TINY_GLOW.num_symbols)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def invalid(p, what):
        out = C.c_void_p()
        rc = _infer_rc(emu_engine, g, ids, p, out)
        msg = lib.mi355tts_last_error().decode()
        assert rc == -1 and msg and not out.value, (rc, msg)
        assert what in msg, msg

    for bad in (np.nan, np.inf, -0.5):
        sc = np.ones((1, n), F32)
        sc[0, 4] = bad
        invalid(ffi.ProsodyC(sc.ctypes.data_as(fp), None, None, n), "id_scales[0][4]")
    d = np.full((1, n), 2, np.int32)
    d[0, 7] = -1
    invalid(ffi.ProsodyC(None, d.ctypes.data_as(ip), None, n), "durations_in[0][7]")
    d[0, 7] = (1 << 28) + 1
    invalid(ffi.ProsodyC(None, d.ctypes.data_as(ip), None, n), "durations_in[0][7]")
    d[0, 7] = 2
    sc = np.ones((1, n), F32)
    invalid(ffi.ProsodyC(sc.ctypes.data_as(fp), d.ctypes.data_as(ip), None, n), "exclude")
    invalid(ffi.ProsodyC(sc.ctypes.data_as(fp), None, None, n - 1), "id_lens[0]")
    invalid(ffi.ProsodyC(None, None, None, n - 1), "ld")
    # a wrapped mel has no durations
    mb = emu_engine.mel_from_numpy(np.zeros((1, HP.TINY_GLOW.mel_channels, 6), F32))
    buf = np.zeros((1, n), np.int32)
    assert lib.mi355tts_mel_durations(mb.handle, buf.ctypes.data_as(ip), n) == -1 and lib.mi355tts_last_error()
    with pytest.raises(ValueError):
        mb.durations
    # ... and so has the mel of a call that did not ask
    with pytest.raises(ValueError):
        emu_engine.glow_infer(g, ids, 0.667, 1.0, seed=1).durations
    # the Python wrapper raises the library's error
    with pytest.raises(ffi.Mi355ttsError):
        emu_engine.glow_infer(g, ids, id_scales=np.full(n, -1.0, F32))
    with pytest.raises(ValueError):
        emu_engine.glow_infer(g, ids, id_scales=np.ones(n + 1, F32))
    # the process goes on
    ok = emu_engine.glow_infer(g, ids, 0.667, 1.0, seed=1, want_durations=True)
    assert int(ok.durations.sum()) == int(ok.frames[0])


def test_all_zero_durations_give_an_empty_mel(emu_engine, tiny):
    hp = HP.TINY_GLOW
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(31), 6, hp.num_symbols)
    mel = emu_engine.glow_infer(tiny["g"], ids, 0.667, 1.0, seed=2, durations=np.zeros(6, np.int32))
    F = 0 if hp.n_sqz > 1 else 1
    assert int(mel.frames[0]) == F and mel.numpy("raw").shape == (1, hp.mel_channels, F)
    assert np.all(mel.durations == 0)
    z = emu_engine.glow_infer(tiny["g"], ids, 0.667, 1.0, seed=2, id_scales=np.zeros(6, F32))
    assert int(z.frames[0]) == F and np.all(z.durations == 0)
    frames, _, i16, d = emu_engine.synthesize(tiny["g"], tiny["v"], ids, seed=2, durations=np.zeros(6, np.int32), return_durations=True)
    assert int(frames[0]) == F and i16.shape[1] == F * HP.TINY_HIFIGAN.hop and np.all(d == 0)


def test_prosody_calls_never_join_a_coalesced_pass(emu_engine, tiny):
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(32), 14, HP.TINY_GLOW.num_symbols)
    emu_engine.set_option("call_coalesce", 2)
    try:
        p0, r0 = emu_engine.coalesce_stats()
        emu_engine.synthesize(tiny["g"], tiny["v"], ids, seed=3)
        p1, r1 = emu_engine.coalesce_stats()
        assert r1 - r0 == 1  # the plain call rides the coalescer ...
        emu_engine.synthesize(tiny["g"], tiny["v"], ids, seed=3, return_durations=True)
        emu_engine.synthesize(tiny["g"], tiny["v"], ids, seed=3, id_scales=np.ones(14, F32))
        assert emu_engine.coalesce_stats() == (p1, r1)  # ... a prosody call never does
    finally:
        emu_engine.set_option("call_coalesce", emu_engine.get_call_coalesce_default())


# ---------------------------------------------------------------- Python surface
def test_phoneme_spans():
    sp = phoneme_spans([3, 0, 2, 0], 8, pad_before=5)
    assert sp.dtype == np.int64 and sp.shape == (4, 2)
    assert sp.tolist() == [[5, 29], [29, 29], [29, 45], [45, 45]]
    assert phoneme_spans([3, 0, 2, 0], 8)[-1, 1] == 5 * 8
    assert phoneme_spans(np.zeros(0, np.int32), 8).shape == (0, 2)
    with pytest.raises(ValueError):
        phoneme_spans([1, -1], 8)


@pytest.fixture(scope="module")
def host_models(emu_library):
    from larynx_amd.constants import TextToSpeechModelConfig, VocoderModelConfig
    from larynx_amd.glow_tts import HipGlowTextToSpeech
    from larynx_amd.hifi_gan import HipHiFiGanVocoder

    gsd = synthetic.make_glow_state_dict(HP.TINY_GLOW, seed=3)
    vsd = synthetic.make_hifigan_state_dict(HP.TINY_HIFIGAN, seed=3)
    tts = HipGlowTextToSpeech(TextToSpeechModelConfig(model_path=Path("unused")), library_path=emu_library, state_dict=gsd,
                              model_config=HP.TINY_GLOW.to_config())
    tts.audio_settings = ljspeech_audio_settings()
    voc = HipHiFiGanVocoder(VocoderModelConfig(model_path=Path("unused")), library_path=emu_library, state_dict=vsd,
                            model_config=HP.TINY_HIFIGAN.to_config())
    return tts, voc, gsd


def test_settings_keys_of_the_model_object(host_models):
    tts, _, gsd = host_models
    hp = HP.TINY_GLOW
    n = 17
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(40), n, hp.num_symbols)
    logw = oracle_logw(gsd, hp, ids)
    sc = draw_scales(n, 40, logw, 1.0)
    exp_d, F = attn_durations(np.ceil(scaled_w(logw, 1.0, sc)).astype(np.int64), hp.n_sqz)
    mel = tts.phonemes_to_mels(ids, {"id_length_scales": list(map(float, sc)), "seed": 9})
    assert mel.durations.shape == (1, n) and mel.durations.dtype == np.int32
    assert np.array_equal(mel.durations[0], exp_d) and int(mel.frames[0]) == F
    again = tts.phonemes_to_mels(ids, {"durations": [int(x) for x in mel.durations[0]], "seed": 9})
    assert np.array_equal(again.durations, mel.durations) and np.array_equal(np.asarray(again), np.asarray(mel))
    plain = tts.phonemes_to_mels(ids, {"seed": 9})
    with pytest.raises(ValueError):
        plain.durations
    timed = tts.phonemes_to_mels(ids, {"seed": 9, "alignment": True})
    assert np.array_equal(np.asarray(timed), np.asarray(plain)) and int(timed.durations.sum()) == int(plain.frames[0])


def test_phonemes_to_speech_alignment(host_models):
    import larynx_amd

    tts, voc, _ = host_models
    hop = HP.TINY_HIFIGAN.hop
    rng = np.random.default_rng(41)
    sents = [(f"s{i}", synthetic.synthetic_phoneme_ids(rng, n, HP.TINY_GLOW.num_symbols)) for i, n in enumerate((11, 4, 26))]
    on = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings={"seed": 77}, alignment=True))
    off = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings={"seed": 77}))
    for (text, ids), a, b in zip(sents, on, off):
        assert b.phoneme_spans is None and a.text == b.text == text
        assert np.array_equal(a.audio, b.audio)
        sp = a.phoneme_spans
        assert sp.shape == (len(ids), 2) and sp.dtype == np.int64
        assert sp[0, 0] == 0 and sp[-1, 1] == a.audio.size and np.all(sp[1:, 0] == sp[:-1, 1]) and np.all(sp % hop == 0)
    # with pauses: the spans start after the leading pad and end before the trailing one
    text, ids = sents[0]
    s = tts.audio_settings
    audio, sp = larynx_amd.sentence_task_aligned(text, ids, s, tts, {"seed": 77}, voc, None, pause_before_ms=10, pause_after_ms=20)
    plain = larynx_amd.sentence_task(text, ids, s, tts, {"seed": 77}, voc, None, pause_before_ms=10, pause_after_ms=20)
    assert np.array_equal(audio, plain)
    assert sp[0, 0] == 220 and sp[-1, 1] == audio.size - 441
    assert np.array_equal(sp - 220, on[0].phoneme_spans)
