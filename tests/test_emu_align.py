"""Forced alignment (`mi355tts_glow_align`, `mi355tts_op_maximum_path`) on the CPU emulator build, on the small test
geometry: the path operator against tests/align_np.py (exact), the round trip with synthesis, batches, truncation, the
refusals, the schedule and the Python surface.  The `check_*` functions take the engine, so tests/test_gpu_align.py runs
them on the device as well."""
from pathlib import Path

import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.alignment import align_spans, phoneme_spans
from oracle import glow_tts_np
from tests import align_np

F32 = np.float32
# shapes (P, F) of the path operator: one id; the forced diagonal; the lane seam (64 ids = one id per lane), the chunk seams
# (65, 130: 2 and 4 ids per lane)
PATH_SHAPES = [(1, 1), (1, 7), (5, 5), (2, 3), (33, 64), (64, 65), (65, 200), (130, 131)]
# direction bits past the kernel's LDS budget (24576 words; 2 words per frame at <= 64 ids): staged back from global memory
PATH_SPILL = (3, 12400)


# ---------------------------------------------------------------- checks shared with the device suite
def check_path(eng, value, id_lens=None, frames=None):
    """durations identical and score bit-identical to tests/align_np.py, row by row"""
    value = np.asarray(value, F32)
    v3 = value if value.ndim == 3 else value[None]
    dur, score = eng.maximum_path(value, id_lens, frames)
    assert dur.dtype == np.int32 and dur.shape == v3.shape[:2] and score.dtype == F32
    for b in range(v3.shape[0]):
        P = v3.shape[1] if id_lens is None else int(id_lens[b])
        F = v3.shape[2] if frames is None else int(frames[b])
        d_ref, s_ref, _ = align_np.maximum_path(v3[b, :P, :F])
        assert np.array_equal(dur[b, :P], d_ref), (b, P, F, np.flatnonzero(dur[b, :P] != d_ref)[:8])
        assert not dur[b, P:].any()
        assert score[b].tobytes() == s_ref.tobytes(), (b, P, F, float(score[b]), float(s_ref))
        assert dur[b, :P].min() >= 1 and int(dur[b].sum()) == F


def check_path_ties(eng, P, F, seed):
    """small integers: ties everywhere, the `stay` rule decides"""
    check_path(eng, np.random.default_rng(seed).integers(-2, 3, (P, F)).astype(F32))
    check_path(eng, np.zeros((P, F), F32))


def check_path_ragged(eng, seed):
    rng = np.random.default_rng(seed)
    value = rng.standard_normal((3, 70, 150)).astype(F32)
    check_path(eng, value, id_lens=np.array([70, 1, 33], np.int32), frames=np.array([149, 150, 33], np.int32))


def check_round_trip(eng, g, ids, length_scale=1.0, speaker=None):
    """noise_scale = 0: aligning the synthesised mel returns the call's durations exactly, and feeding them back reproduces
    the mel bit for bit"""
    mel = eng.glow_infer(g, ids, 0.0, length_scale, want_durations=True, speaker_ids=speaker)
    dur, score = eng.glow_align(g, ids, mel, speaker_ids=speaker)
    print("P", len(ids), "F", int(mel.frames[0]), "mismatches", int(np.sum(dur[0] != mel.durations[0])), "score", float(score[0]))
    assert dur.dtype == np.int32 and dur.shape == (1, len(ids))
    assert np.array_equal(dur, mel.durations)
    assert np.isfinite(score[0])
    again = eng.glow_infer(g, ids, 0.0, length_scale, durations=dur[0], speaker_ids=speaker)
    assert np.array_equal(again.frames, mel.frames) and np.array_equal(again.numpy("raw"), mel.numpy("raw"))
    return mel, dur


def check_batch_rows(eng, g, rows, mels, z_tol):
    """a ragged batch returns each row's solo durations, zeros past P, and z within f32 round-off of the solo z"""
    solo = [eng.glow_align(g, r, m, want_latent=True) for r, m in zip(rows, mels)]
    Fmax = max(m.shape[-1] for m in mels)
    batch = np.zeros((len(rows), mels[0].shape[0], Fmax), F32)
    for b, m in enumerate(mels):
        batch[b, :, : m.shape[1]] = m
    frames = np.array([m.shape[1] for m in mels], np.int32)
    dur, score, z = eng.glow_align(g, rows, batch, frames=frames, want_latent=True)
    for b, (d1, s1, z1) in enumerate(solo):
        P, F = len(rows[b]), int(frames[b])
        assert np.array_equal(dur[b, :P], d1[0]) and not dur[b, P:].any()
        assert abs(float(score[b]) - float(s1[0])) <= 1e-4 * abs(float(s1[0]))
        err = float(np.abs(z[b, :, :F] - z1[0]).max())
        print("row", b, "batch z vs solo z max-abs", err)
        assert err <= z_tol and not z[b, :, F // 2 * 2:].any()


def check_truncation(eng, g, ids, mel, speaker=None):
    """one more frame appended (F_in odd at n_sqz = 2): the durations of the even case"""
    assert mel.shape[1] % 2 == 0
    even, _ = eng.glow_align(g, ids, mel, speaker_ids=speaker)
    odd, _ = eng.glow_align(g, ids, np.concatenate([mel, mel[:, -1:] + 1.0], axis=1), speaker_ids=speaker)
    assert np.array_equal(odd, even)


def _refused(fn, what):
    with pytest.raises(ffi.Mi355ttsError) as e:
        fn()
    assert e.value.code == -1 and what in str(e.value), str(e.value)


def check_refusals(eng, g_single, g_multi, hp):
    import ctypes as C

    M = hp.mel_channels
    ids = np.arange(1, 9, dtype=np.int64) % hp.num_symbols
    mel = np.zeros((M, 20), F32)
    _refused(lambda: eng.glow_align(g_single, ids, mel[:, :6]), "frames")  # F < P
    _refused(lambda: eng.glow_align(g_single, np.append(ids, 1), mel[:, :9]), "frames")  # 9 frames count as 8 at n_sqz = 2
    _refused(lambda: eng.glow_align(g_multi, ids, mel), "speaker")
    _refused(lambda: eng.glow_align(g_single, ids, mel, speaker_ids=0), "speaker")
    big = np.ones(2049, np.int64)
    _refused(lambda: eng.glow_align(g_single, big, np.zeros((M, 2050), F32)), "2048")
    # the C entry: null pointers, dur_ld < P
    lens = np.array([len(ids)], np.int32)
    fr = np.array([20], np.int32)
    dur = np.zeros((1, 8), np.int32)
    i32 = C.POINTER(C.c_int32)

    def call(ids_p, mel_p, dur_p, dur_ld):
        return eng.lib.mi355tts_glow_align(eng._ctx, g_single, ids_p, lens.ctypes.data_as(i32), 1, len(ids), mel_p, fr.ctypes.data_as(i32), 20,
                                           None, 0, dur_p, dur_ld, None, None)

    d_p = dur.ctypes.data_as(i32)
    assert call(ids.ctypes.data, mel.ctypes.data, d_p, 8) == 0
    assert call(None, mel.ctypes.data, d_p, 8) == -1 and b"null" in eng.lib.mi355tts_last_error()
    assert call(ids.ctypes.data, None, d_p, 8) == -1 and b"null" in eng.lib.mi355tts_last_error()
    assert call(ids.ctypes.data, mel.ctypes.data, None, 8) == -1 and b"null" in eng.lib.mi355tts_last_error()
    assert call(ids.ctypes.data, mel.ctypes.data, d_p, 7) == -1 and b"dur_ld" in eng.lib.mi355tts_last_error()
    val = np.zeros((1, 4, 3), F32)
    _refused(lambda: eng.maximum_path(val), "frames")


def check_schedule(eng, g, hp, ids):
    """by kernel name and by class: the forward decoder takes no more launches than the reverse one (+ squeeze-in and
    unsqueeze-out, which stand where expansion and mel_finalize stand), one score and one path launch per call, and a
    synthesis call before and after shows the same counts"""
    def counted(fn):
        eng.set_profiling(True)
        eng.profile_reset()
        out = fn()
        prof, names = eng.profile(), eng.kernel_counts()
        eng.set_profiling(False)
        return out, prof, {k: v for k, v in names.items() if v}

    try:
        mel = eng.glow_infer(g, ids, 0.0, 1.0)
        eng.glow_align(g, ids, mel)  # workspaces sized outside the counted calls
        mel, p_inf, n_inf = counted(lambda: eng.glow_infer(g, ids, 0.0, 1.0))
        _, p_al, n_al = counted(lambda: eng.glow_align(g, ids, mel))
        _, p_inf2, n_inf2 = counted(lambda: eng.glow_infer(g, ids, 0.0, 1.0))
    finally:
        eng.set_profiling(False)
    launches = lambda p: {k: v["launches"] for k, v in p.items() if v["launches"]}
    print("glow_infer:", launches(p_inf), n_inf)
    print("glow_align:", launches(p_al), n_al)
    assert launches(p_inf2) == launches(p_inf) and n_inf2 == n_inf
    assert "glow_fwd_kernel" not in n_inf and "align_path_kernel" not in n_inf
    assert n_al["align_score_kernel"] == 1 and n_al["align_path_kernel"] == 1
    assert n_al["glow_fwd_kernel"] == hp.n_blocks_dec + 1 and n_inf["glow_tail_kernel"] == hp.n_blocks_dec
    assert "glow_tail_kernel" not in n_al
    dec = "conv_mfma.glow_decoder"
    assert p_al[dec]["launches"] <= p_inf[dec]["launches"]
    assert p_al["conv_mfma.glow_encoder"]["launches"] == p_inf["conv_mfma.glow_encoder"]["launches"]
    # elementwise: the encoder's small launches are the same; infer adds durations, expansion, finalize; align adds
    # squeeze, unsqueeze, scores, path
    assert p_al["elementwise"]["launches"] == p_inf["elementwise"]["launches"] + 1


def check_dropin(tts, hop, ids, settings=None):
    s = dict(settings or {}, noise_scale=0.0, alignment=True)
    mel = tts.phonemes_to_mels(ids, s)
    a = tts.align(ids, mel, settings)
    b = tts.align(ids, mel.numpy("raw"), settings)
    assert a.dtype == np.int32 and a.shape == (len(ids),) and np.array_equal(a, b)
    assert np.array_equal(a, mel.durations[0])
    assert np.array_equal(align_spans(tts, ids, mel, hop, 100, settings), phoneme_spans(mel.durations[0], hop, 100))
    again = tts.phonemes_to_mels(ids, dict(s, durations=a))  # the timing of one take onto another
    assert np.array_equal(again.numpy("raw"), mel.numpy("raw"))


# ---------------------------------------------------------------- the emulator's runs
TINY_MULTI = None


@pytest.fixture(scope="module")
def tiny(emu_engine):
    import dataclasses

    hp, mhp = HP.TINY_GLOW, dataclasses.replace(HP.TINY_GLOW, n_speakers=3, gin_channels=8)
    gsd, msd = synthetic.make_glow_state_dict(hp, seed=7), synthetic.make_glow_state_dict(mhp, seed=9)
    return dict(hp=hp, mhp=mhp, gsd=gsd, msd=msd, g=emu_engine.load_glow(hp, gsd), gm=emu_engine.load_glow(mhp, msd))


def _ids(n, seed, hp=HP.TINY_GLOW):
    return synthetic.synthetic_phoneme_ids(np.random.default_rng(seed), n, hp.num_symbols)


@pytest.mark.parametrize("P,F", PATH_SHAPES + [PATH_SPILL])
def test_path_operator_exact(emu_engine, P, F):
    check_path(emu_engine, np.random.default_rng(P * 1000 + F).standard_normal((P, F)).astype(F32) * 3)


def test_path_operator_ties_and_ragged_batch(emu_engine):
    check_path_ties(emu_engine, 9, 30, 1)
    check_path_ties(emu_engine, 70, 75, 2)
    check_path_ragged(emu_engine, 3)


def test_restated_path_is_the_forced_diagonal_and_prefers_to_stay():
    d, s, _ = align_np.maximum_path(np.arange(25, dtype=F32).reshape(5, 5))
    assert np.array_equal(d, np.ones(5, np.int32)) and s == F32(0 + 6 + 12 + 18 + 24)
    d, _, _ = align_np.maximum_path(np.zeros((2, 5), F32))  # all ties: every step stays, the move comes as early as it can
    assert np.array_equal(d, [1, 4])


@pytest.mark.parametrize("fuse", [1, 0])
def test_round_trip_and_latent(emu_engine, tiny, fuse):
    """fused and un-fused forward flow; z at noise_scale 0 is the expanded x_m (models.py:336-348), from the oracle's encoder"""
    hp = tiny["hp"]
    emu_engine.set_option("glow_fuse", fuse)
    try:
        for n, seed in ((9, 3), (23, 4)):
            ids = _ids(n, seed)
            mel, dur = check_round_trip(emu_engine, tiny["g"], ids)
            _, _, z = emu_engine.glow_align(tiny["g"], ids, mel, want_latent=True)
            x_m, _ = glow_tts_np.text_encoder(tiny["gsd"], np.asarray(ids, np.int64), hp, None, None)
            err = float(np.abs(z[0] - np.repeat(x_m, dur[0], axis=1)).max())
            print("fuse", fuse, "P", n, "z vs expanded x_m max-abs", err)
            assert err <= 2e-4
    finally:
        emu_engine.set_option("glow_fuse", 1)


def test_fused_and_unfused_flows_agree(emu_engine, tiny):
    ids = _ids(17, 5)
    mel = emu_engine.glow_infer(tiny["g"], ids, 0.667, 1.0, seed=5).numpy("raw")[0]
    a = emu_engine.glow_align(tiny["g"], ids, mel, want_latent=True)
    emu_engine.set_option("glow_fuse", 0)
    try:
        b = emu_engine.glow_align(tiny["g"], ids, mel, want_latent=True)
    finally:
        emu_engine.set_option("glow_fuse", 1)
    assert np.array_equal(a[0], b[0]) and float(np.abs(a[2] - b[2]).max()) <= 2e-5


def test_multispeaker_round_trip(emu_engine, tiny):
    check_round_trip(emu_engine, tiny["gm"], _ids(12, 8, tiny["mhp"]), speaker=2)


def test_batch_rows_and_truncation(emu_engine, tiny):
    rows = [_ids(5, 11), _ids(19, 12), _ids(9, 13)]
    mels = [emu_engine.glow_infer(tiny["g"], r, 0.0, 1.0).numpy("raw")[0] for r in rows]
    check_batch_rows(emu_engine, tiny["g"], rows, mels, z_tol=2e-5)
    check_truncation(emu_engine, tiny["g"], rows[1], mels[1])


def test_refusals(emu_engine, tiny):
    check_refusals(emu_engine, tiny["g"], tiny["gm"], tiny["hp"])


def test_schedule(emu_engine, tiny):
    check_schedule(emu_engine, tiny["g"], tiny["hp"], _ids(21, 14))


def test_the_half_switch_does_not_change_an_alignment(emu_engine):
    hp = HP.TINY_GLOW
    g = emu_engine.load_glow(hp, synthetic.make_glow_state_dict(hp, seed=7))
    try:
        ids = _ids(15, 15)
        mel = emu_engine.glow_infer(g, ids, 0.5, 1.0, seed=2).numpy("raw")[0]
        a = emu_engine.glow_align(g, ids, mel, want_latent=True)
        emu_engine.set_precision(g, ffi.PRECISION_F16)
        b = emu_engine.glow_align(g, ids, mel, want_latent=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[1][0] == b[1][0]
    finally:
        emu_engine.unload(g)


def test_dropin(emu_library):
    from larynx_amd.constants import TextToSpeechModelConfig
    from larynx_amd.glow_tts import HipGlowTextToSpeech

    tts = HipGlowTextToSpeech(TextToSpeechModelConfig(model_path=Path("unused")), library_path=emu_library,
                              state_dict=synthetic.make_glow_state_dict(HP.TINY_GLOW, seed=3), model_config=HP.TINY_GLOW.to_config())
    check_dropin(tts, HP.TINY_HIFIGAN.hop, _ids(14, 16))
