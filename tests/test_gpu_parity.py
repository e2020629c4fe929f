"""Parity of the HIP path (through the C ABI, on a real MI355X) against the
golden vectors produced by the reference's torch modules and against the CPU
oracle.  Tolerances are north_star's: mel +-1e-3 max-abs, waveform 1e-4 RMS,
identical frame counts, int16 within 1 LSB."""
import numpy as np
import pytest

from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.audio import ljspeech_audio_settings
from oracle import audio_np, glow_tts_np, hifi_gan_np, nn_np
from tests.golden_util import CASES, load_case
from tests.test_emu_conv import CASES as CONV_CASES

pytestmark = pytest.mark.gpu

MEL_TOL = 1e-3
WAV_RMS_TOL = 1e-4

_models = {}


def models(eng, ghp, vhp):
    if ("g", ghp) not in _models:
        sd = synthetic.make_glow_state_dict(ghp, seed=1234)
        _models[("g", ghp)] = (sd, eng.load_glow(ghp, sd))
    if ("v", vhp) not in _models:
        sd = synthetic.make_hifigan_state_dict(vhp, seed=1234)
        _models[("v", vhp)] = (sd, eng.load_hifigan(vhp, sd))
    return _models[("g", ghp)], _models[("v", vhp)]


@pytest.mark.parametrize("Cin,Cout,K,dil,L,B,slope,act", CONV_CASES + [(256, 256, 11, 5, 4992, 1, 0.1, 0), (32, 32, 3, 1, 159744, 1, 0.1, 0)])
def test_conv1d_kernel(gpu_engine, Cin, Cout, K, dil, L, B, slope, act):
    rng = np.random.default_rng(Cin * 1000 + Cout + K)
    x = rng.standard_normal((B, Cin, L)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, K)) / np.sqrt(Cin * K)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    lens = np.array([L] + [L - 37] * (B - 1), np.int32)
    y = gpu_engine.conv1d(x, w, b, dilation=dil, in_slope=slope, out_act=act, lens=lens)
    for i in range(B):
        n = lens[i]
        ref = nn_np.conv1d(nn_np.leaky_relu(x[i, :, :n], slope), w, b, dilation=dil, padding=(K * dil - dil) // 2)
        if act == 1:
            ref = np.maximum(ref, 0)
        elif act == 2:
            ref = np.tanh(ref)
        np.testing.assert_allclose(y[i, :, :n], ref, rtol=1e-4, atol=5e-5)
        assert np.all(y[i, :, n:] == 0)


@pytest.mark.parametrize("shape", [0, 1, 2, 3])
@pytest.mark.parametrize("Cin,Cout,K,dil,L", [(128, 128, 11, 5, 3000), (192, 384, 5, 1, 478), (64, 64, 7, 3, 9000), (80, 512, 7, 1, 700), (32, 32, 3, 5, 20000), (192, 80, 1, 1, 120)])
def test_conv1d_every_tile_shape(gpu_engine, monkeypatch, shape, Cin, Cout, K, dil, L):
    monkeypatch.setenv("MI355TTS_FORCE_TILE_DYNAMIC", str(shape))
    rng = np.random.default_rng(shape * 7 + K)
    x = rng.standard_normal((1, Cin, L)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, K)) / np.sqrt(Cin * K)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    y = gpu_engine.conv1d(x, w, b, dilation=dil, in_slope=0.1)
    ref = nn_np.conv1d(nn_np.leaky_relu(x[0], 0.1), w, b, dilation=dil, padding=(K * dil - dil) // 2)
    np.testing.assert_allclose(y[0], ref, rtol=1e-4, atol=5e-5)


def test_conv1d_random_shapes_full_size(gpu_engine):
    """The emulator suite's randomised conv check (tests/test_emu_random.py) at real
    channel counts and lengths, on the device."""
    from hypothesis import HealthCheck, given, settings
    from hypothesis import strategies as st

    from tests.test_emu_random import TAPS, check_conv1d

    @settings(max_examples=40, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
    @given(taps=TAPS, cin=st.integers(1, 300), cout=st.integers(1, 300), L=st.integers(1, 6000), B=st.integers(1, 3),
           shape=st.sampled_from([-1, 0, 1, 2, 3]), slope=st.sampled_from([1.0, 0.1]), act=st.sampled_from([0, 1, 2]),
           seed=st.integers(0, 2 ** 16))
    def run(taps, cin, cout, L, B, shape, slope, act, seed):
        check_conv1d(gpu_engine, taps, cin, cout, L, B, shape, slope, act, seed)

    run()


@pytest.mark.parametrize("Cin,Cout,K,u,L", [(16, 8, 16, 8, 50), (512, 256, 16, 8, 624), (64, 32, 4, 2, 5000)])
def test_conv_transpose1d_kernel(gpu_engine, Cin, Cout, K, u, L):
    rng = np.random.default_rng(K * 100 + u)
    x = rng.standard_normal((1, Cin, L)).astype(np.float32)
    w = (rng.standard_normal((Cin, Cout, K)) / np.sqrt(Cin * 2)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    y = gpu_engine.conv_transpose1d(x, w, b, stride=u, in_slope=0.1)
    ref = nn_np.conv_transpose1d(nn_np.leaky_relu(x[0], 0.1), w, b, stride=u, padding=(K - u) // 2)
    np.testing.assert_allclose(y[0], ref, rtol=1e-4, atol=5e-5)


@pytest.mark.parametrize("name", CASES)
def test_golden_reference_parity(gpu_engine, name):
    """HIP path vs outputs of the reference's own torch implementation."""
    c = load_case(name)
    (gsd, g), (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    s = ljspeech_audio_settings()
    mel = gpu_engine.glow_infer(g, c["ids"], float(c["noise_scale"]), float(c["length_scale"]), noise=c["noise"], audio_settings=s)
    assert int(mel.frames[0]) == c["mel"].shape[1]
    raw = mel.numpy("raw")[0]
    assert np.abs(raw - c["mel"]).max() <= MEL_TOL
    # tighter than north_star: the path is exact f32 MFMA, expect f32 round-off only
    assert np.abs(raw - c["mel"]).max() <= 5e-5
    # the vocoder-input mel crosses the 1e-5 clamp and the log of the M1 transforms: the numpy oracle sits at <= 1.4e-4 from the
    # reference on this tensor (tests/golden/oracle_vs_reference.json), so a `mel_finalize` regression shows HERE, not first
    # in the waveform check downstream
    assert np.abs(mel.numpy("vocoder")[0] - c["mel_voc"]).max() <= 5e-4
    wav, i16 = gpu_engine.hifigan_infer(v, mel)
    assert int(c["wav_stride"]) == 1 and wav.shape[1] == c["wav"].shape[0]  # every sample is compared
    rms = np.sqrt(np.mean((wav[0] - c["wav"]) ** 2))
    assert rms <= WAV_RMS_TOL, rms
    assert np.abs(i16[0].astype(np.int32) - c["wav_i16"].astype(np.int32)).max() <= 1  # +-1 LSB
    # the fused one-call entry point gives the same bits as the two calls
    frames, f1, i1 = gpu_engine.synthesize(g, v, c["ids"], float(c["noise_scale"]), float(c["length_scale"]), noise=c["noise"],
                                           audio_settings=s, want_float=True)
    assert int(frames[0]) == c["mel"].shape[1] and np.array_equal(f1, wav) and np.array_equal(i1, i16)


def test_serial_branch_schedule_matches_reference(gpu_engine):
    c = load_case("ljspeech_low_echo")
    _, (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    mb = gpu_engine.mel_from_numpy(c["mel_voc"])
    gpu_engine.set_option("serial_branches", 1)
    try:
        wav, _ = gpu_engine.hifigan_infer(v, mb)
    finally:
        gpu_engine.set_option("serial_branches", 0)
    assert np.sqrt(np.mean((wav[0] - c["wav"]) ** 2)) <= 2e-5


def test_denoiser_matches_reference(gpu_engine):
    """`denoiser_strength > 0` (CLI/server default path, larynx/hifi_gan.py:152-203)
    against the reference's own numpy STFT helpers run on the reference generator."""
    c = load_case("ljspeech_medium_dave_ls12")
    _, (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    mb = gpu_engine.mel_from_numpy(c["mel_voc"])
    wav, i16 = gpu_engine.hifigan_infer(v, mb, denoiser_strength=float(c["denoiser_strength"]))
    assert int(c["wav_denoised_stride"]) == 1
    assert wav.shape[1] == c["mel_voc"].shape[1] * 256 == c["wav_denoised"].shape[0]
    assert np.sqrt(np.mean((wav[0] - c["wav_denoised"]) ** 2)) <= 1e-4
    assert np.abs(i16[0].astype(np.int32) - c["wav_denoised_i16"].astype(np.int32)).max() <= 1
    plain, _ = gpu_engine.hifigan_infer(v, mb)
    assert np.sqrt(np.mean((plain[0] - wav[0]) ** 2)) > 1e-3  # the denoiser did something


def test_denoise_kernels(gpu_engine):
    from oracle import denoise_np

    rng = np.random.default_rng(21)
    wav = (rng.standard_normal((2, 256 * 300)) * 0.3).astype(np.float32)
    bias = np.abs(rng.standard_normal(513)).astype(np.float32)
    got = gpu_engine.denoise(wav, bias, 0.4)
    for b in range(2):
        assert np.abs(got[b] - denoise_np.denoise(wav[b], bias, 0.4)).max() < 5e-5


def test_vocoder_alone_on_reference_mel(gpu_engine):
    """`mels_to_audio` drop-in: host mel (already transformed) in, int16 out."""
    c = load_case("ljspeech_high_echo")
    _, (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    mb = gpu_engine.mel_from_numpy(c["mel_voc"])
    wav, i16 = gpu_engine.hifigan_infer(v, mb)
    assert np.sqrt(np.mean((wav[0] - c["wav"]) ** 2)) <= 2e-5
    assert np.abs(i16[0].astype(np.int32) - c["wav_i16"].astype(np.int32)).max() <= 1


def test_config4_batch_rows_equal_the_reference(gpu_engine):
    """BASELINE config 4: thorsten + 'medium', B = 8 variable length (P = 19 ... 120) in ONE
    padded batch.  EVERY row's mel, float waveform and int16 against the golden row the
    reference itself produced at B = 1 (the reference never batches; each row
    must equal its own un-batched result), padded tails exactly 0."""
    from tests.golden_util import load_batch8

    c = load_batch8()
    ghp, vhp = c["glow_hp"], c["voc_hp"]
    (gsd, g), (vsd, v) = models(gpu_engine, ghp, vhp)
    s = ljspeech_audio_settings()
    mel = gpu_engine.glow_infer(g, c["ids"], c["noise_scale"], c["length_scale"], noise=c["noise"], audio_settings=s)
    wav, i16 = gpu_engine.hifigan_infer(v, mel)
    raw = mel.numpy("raw")
    hop = vhp.hop
    for b in range(8):
        F = c["mel"][b].shape[1]
        assert int(mel.frames[b]) == F
        assert np.abs(raw[b, :, :F] - c["mel"][b]).max() <= 5e-5
        assert np.all(raw[b, :, F:] == 0)
        n = F * hop
        assert n == c["wav"][b].shape[0]
        rms = np.sqrt(np.mean((wav[b, :n] - c["wav"][b]) ** 2))
        assert rms <= WAV_RMS_TOL, (b, rms)
        ref16 = audio_np.audio_float_to_int16(c["wav"][b])  # larynx/audio.py:118-125 on the reference's float waveform
        assert np.abs(i16[b, :n].astype(np.int32) - ref16.astype(np.int32)).max() <= 1
        assert np.all(wav[b, n:] == 0) and np.all(i16[b, n:] == 0)
    # and a row on its own gives the same bits as inside the batch
    for b in (0, 5, 7):
        one = gpu_engine.glow_infer(g, c["ids"][b], c["noise_scale"], c["length_scale"], noise=c["noise"][b], audio_settings=s)
        F = int(one.frames[0])
        np.testing.assert_allclose(raw[b, :, :F], one.numpy("raw")[0], atol=1e-5)
        w1, _ = gpu_engine.hifigan_infer(v, one)
        assert np.sqrt(np.mean((wav[b, : F * hop] - w1[0]) ** 2)) <= 1e-5


def test_device_noise_is_standard_normal(gpu_engine):
    """The production noise mode (bench.py times it): 2 x 80 x 8192 = 1.3e6 draws."""
    from tests.noise_check import check_gauss_noise

    n = 2 * 80 * 8192
    check_gauss_noise(gpu_engine, 2, 80, 8192, ks_bound=1.95 / np.sqrt(n))


def test_host_feature_checks_on_the_device(gpu_engine):
    """The emulator suite's host-runtime checks (fused call, pause padding, schedule
    invariance under load) on the real build at full model sizes."""
    import torch

    from tests.test_emu_host_features import check_empty_vocoder_call, check_schedule_invariance, check_synthesize_equals_two_calls

    (gsd, g), (vsd, v) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_MEDIUM)
    check_synthesize_equals_two_calls(gpu_engine, g, v, HP.LJSPEECH.num_symbols, HP.HIFIGAN_MEDIUM.hop, lens=(40, 17, 63))

    def torch_buffer(shape, dtype):
        t = torch.full(shape, 7, dtype=torch.float32 if dtype == np.float32 else torch.int16, device="cuda")
        torch.cuda.synchronize()
        return t.data_ptr(), lambda: t.cpu().numpy()

    check_empty_vocoder_call(gpu_engine, g, v, HP.LJSPEECH.num_symbols, HP.HIFIGAN_MEDIUM.num_mels, device_buffer=torch_buffer)
    _, (_, vh) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_HIGH)
    check_schedule_invariance(gpu_engine, vh, 80, frames=150, threads=6)
    from larynx_amd import ffi

    gpu_engine.set_precision(vh, ffi.PRECISION_BF16X3)  # the split-bf16 kernels (k-split tile, fused pairs) under the same schedules
    try:
        check_schedule_invariance(gpu_engine, vh, 80, frames=150, threads=6)
    finally:
        gpu_engine.set_precision(vh, ffi.PRECISION_F32)
    gpu_engine.reserve(4, g, vh, max_batch=1, max_ids=128, max_frames=1024, denoiser=True, max_pad_samples=22050)


def test_counted_launches_are_timed_under_the_same_name_on_the_device(gpu_engine):
    """`kernel_counts` and `profile_kernels` agree name for name on the real build (the emulator suite's check): the fused call
    and the vocoder at `test_host_feature_checks_on_the_device`'s shapes, then 'high' at 150 frames — the smallest input of
    this file that reaches the grouped and the fused-pair runners."""
    from tests.test_emu_host_features import check_counted_means_timed

    (_, g), (_, v) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_MEDIUM)
    check_counted_means_timed(gpu_engine, g, v, HP.LJSPEECH.num_symbols, HP.HIFIGAN_MEDIUM.num_mels, lens=(40, 40, 17, 63), frames=150)
    _, (_, vh) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_HIGH)
    check_counted_means_timed(gpu_engine, g, vh, HP.LJSPEECH.num_symbols, HP.HIFIGAN_HIGH.num_mels, lens=(40, 40, 17, 63), frames=150)
    names = gpu_engine.kernel_counts()  # (the last call of the check: the batch-1 fused call, profiling off)
    assert names["rb_group_kernel"] + names["rb_group_kernel.snake"] + names["conv_group_kernel"] > 0, names
    assert names["rb_pair_group_kernel"] + names["pair_group_kernel"] > 0, names


def test_dispatch_selfcheck_is_neither_counted_nor_timed():
    """The self-check's own grouped launches (a `quiet` worker) on a context that profiles: the check runs with the first
    'high'-class load, and no kernel name is counted and no class has a timed launch afterwards."""
    from larynx_amd.engine import Engine

    eng = Engine(device=0)
    try:
        eng.set_profiling(True)
        eng.profile_reset()
        eng.load_hifigan(HP.HIFIGAN_HIGH, synthetic.make_hifigan_state_dict(HP.HIFIGAN_HIGH, seed=1234))
        r = eng.dispatch_selfcheck()
        assert r["state"] in ("snake order kept", "snake order switched off"), r
        assert not any(eng.kernel_counts().values()), eng.kernel_counts()
        assert all(acc["launches"] == 0 for acc in eng.profile().values()) and eng.profile_kernels() == {}
    finally:
        eng.close()


def test_standard_utterance_properties(gpu_engine):
    """BASELINE config 2 at full size (P=120): size-independent checks — frame
    count equals the duration sum, bounded tanh output, int16 peak-normalised,
    determinism, and noise_scale=0 equals noise=None."""
    ghp, vhp = HP.LJSPEECH, HP.HIFIGAN_HIGH
    (gsd, g), (vsd, v) = models(gpu_engine, ghp, vhp)
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(1234), 120, ghp.num_symbols)
    s = ljspeech_audio_settings()
    taps = {}
    glow_tts_np.text_encoder(gsd, ids, ghp, taps)
    w_ceil, F, _ = glow_tts_np.durations_to_frames(taps["logw"], 1.0, 2)
    noise = np.random.default_rng(1234).standard_normal((80, 1400)).astype(np.float32)
    mel = gpu_engine.glow_infer(g, ids, 0.667, 1.0, noise=noise, audio_settings=s)
    assert int(mel.frames[0]) == F
    wav, i16 = gpu_engine.hifigan_infer(v, mel)
    assert wav.shape[1] == F * 256 and np.all(np.abs(wav) < 1.0) and np.isfinite(wav).all()
    # peak-normalised: the peak sample is peak * fl(32767 / peak), which float32 rounding leaves at 32767 or a hair
    # under it (truncated: 32766) — exactly what the reference's astype does, so pin it to the oracle on the same wav
    assert np.abs(i16).max() >= 32766 or np.abs(wav).max() < 0.01
    assert np.abs(i16[0].astype(np.int32) - audio_np.audio_float_to_int16(wav[0]).astype(np.int32)).max() <= 1
    mel2 = gpu_engine.glow_infer(g, ids, 0.667, 1.0, noise=noise, audio_settings=s)
    wav2, _ = gpu_engine.hifigan_infer(v, mel2)
    assert np.array_equal(wav, wav2)
    a = gpu_engine.glow_infer(g, ids, 0.0, 1.0, noise=noise).numpy()
    b = gpu_engine.glow_infer(g, ids, 0.0, 1.0).numpy()
    assert np.array_equal(a, b)
    # device RNG: different seeds differ, same seed repeats
    r1 = gpu_engine.glow_infer(g, ids, 0.667, 1.0, seed=1).numpy()
    r2 = gpu_engine.glow_infer(g, ids, 0.667, 1.0, seed=1).numpy()
    r3 = gpu_engine.glow_infer(g, ids, 0.667, 1.0, seed=2).numpy()
    assert np.array_equal(r1, r2) and not np.array_equal(r1, r3)


def test_threads_share_one_engine(gpu_engine):
    """The reference calls its models from a ThreadPoolExecutor (larynx/__init__.py:146)."""
    from concurrent.futures import ThreadPoolExecutor

    ghp, vhp = HP.LJSPEECH, HP.HIFIGAN_MEDIUM
    (gsd, g), (vsd, v) = models(gpu_engine, ghp, vhp)
    rng = np.random.default_rng(5)
    rows = [synthetic.synthetic_phoneme_ids(rng, n, ghp.num_symbols) for n in (20, 35, 50, 28, 41, 33)]
    s = ljspeech_audio_settings()

    def run(ids):
        m = gpu_engine.glow_infer(g, ids, 0.0, 1.0, audio_settings=s)
        return gpu_engine.hifigan_infer(v, m)[0][0]

    serial = [run(r) for r in rows]
    with ThreadPoolExecutor(4) as ex:
        par = list(ex.map(run, rows))
    for a, b in zip(serial, par):
        assert np.array_equal(a, b)


def test_coalesced_calls_equal_their_solitary_results(gpu_engine):
    """csrc/host_join.h on the device (option `call_coalesce`): eight threads' batch-1 fused calls (ragged lengths on both sides
    of the 16- and 32-column tile seams, the device RNG on, a pause before / after some rows, device AND host outputs) ride fused
    padded calls, and every caller gets its solitary call's result to f32 round-off — frames identical, float waveform RMS <=
    1e-5, int16 within 1 LSB — in f32 and in the split-bf16 mode; a lone caller gets the same BITS as with the option off."""
    import threading

    from larynx_amd import ffi

    (gsd, g), (vsd, v) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_HIGH)
    s = ljspeech_audio_settings()
    rng = np.random.default_rng(77)
    lens = (120, 33, 64, 97, 120, 15, 81, 50)
    pads = ((0, 0), (220, 0), (0, 441), (0, 0), (100, 100), (0, 0), (0, 0), (7, 3))
    ids = [synthetic.synthetic_phoneme_ids(rng, n, HP.LJSPEECH.num_symbols) for n in lens]

    def call(i):
        # (a generous buffer guess: a row whose buffer is too small sends its whole pass to the solitary path — tested on the emulator)
        return gpu_engine.synthesize(g, v, ids[i], 0.667, 0.65, seed=500 + i, audio_settings=s, want_float=True, pad_before=pads[i][0],
                                     pad_after=pads[i][1], frames_per_id_guess=20.0)

    for precision in (ffi.PRECISION_F32, ffi.PRECISION_BF16X3):
        gpu_engine.set_precision(v, precision)
        try:
            gpu_engine.set_option("call_coalesce", 0)
            solo = [call(i) for i in range(len(ids))]
            for lanes in (1, 2, 3):
                gpu_engine.set_option("call_coalesce", lanes)
                p0, r0 = gpu_engine.coalesce_stats()
                for rep in range(3):
                    out = [None] * len(ids)
                    bar = threading.Barrier(len(ids))

                    def work(i):
                        bar.wait()
                        out[i] = call(i)

                    th = [threading.Thread(target=work, args=(i,)) for i in range(len(ids))]
                    for t in th:
                        t.start()
                    for t in th:
                        t.join()
                    for (fa, wa, ia), (fb, wb, ib) in zip(solo, out):
                        assert np.array_equal(fa, fb) and ia.shape == ib.shape
                        assert np.abs(ia.astype(np.int32) - ib.astype(np.int32)).max() <= 1
                        assert np.sqrt(np.mean((wa - wb) ** 2)) <= 1e-5
                p1, r1 = gpu_engine.coalesce_stats()
                assert r1 - r0 == 3 * len(ids) and p1 - p0 < r1 - r0, (p1 - p0, r1 - r0)  # passes were shared
                lone = call(3)
                assert np.array_equal(lone[1], solo[3][1]) and np.array_equal(lone[2], solo[3][2])
        finally:
            gpu_engine.set_option("call_coalesce", gpu_engine.get_call_coalesce_default())
            gpu_engine.set_precision(v, ffi.PRECISION_F32)


def test_seeded_path_equals_injected_noise(gpu_engine):
    """`glow_infer(seed = s)` (what bench.py times) == `glow_infer(noise = gauss_noise(s, ...))` (how every parity test feeds the
    reference's recorded `randn_like` draw, glow_tts/models.py:348), bit for bit at ljspeech size: batch 1 and a ragged batch
    of 3 (row b draws the stream s + b)."""
    from tests.test_emu_host_features import check_seeded_path_equals_injected_noise

    (gsd, g), _ = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_HIGH)
    hp = HP.LJSPEECH
    check_seeded_path_equals_injected_noise(gpu_engine, g, hp.num_symbols, hp.mel_channels, lens=(120,))
    check_seeded_path_equals_injected_noise(gpu_engine, g, hp.num_symbols, hp.mel_channels, lens=(120, 47, 90), seed=99)


def test_workspace_growth_keeps_live_buffers():
    from larynx_amd.engine import Engine
    from tests.test_emu_host_features import check_workspace_growth_keeps_live_buffers

    check_workspace_growth_keeps_live_buffers(lambda: Engine(device=0))


def _torch_device_blob(blob):
    import torch

    t = torch.from_numpy(blob).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


def test_load_from_device_blob(gpu_engine):
    """Both loaders from a blob in device memory (a torch tensor's `data_ptr()`) against the same blob from the host."""
    from tests.test_emu_host_features import check_load_from_device_blob

    check_load_from_device_blob(gpu_engine, _torch_device_blob)


def test_load_rejects_bad_blob(gpu_engine):
    """Wrong blob sizes are refused before a device blob is copied: the probe is a 4-byte allocation, which a copy of the
    claimed size could not come from."""
    from tests.test_emu_host_features import check_load_rejects_bad_blob

    ptr, keep = _torch_device_blob(np.zeros(1, np.float32))
    check_load_rejects_bad_blob(gpu_engine, ptr)
    del keep


def test_glowtts_launch_counts_on_the_device(gpu_engine):
    """The fused GlowTTS schedule is the one that runs for the released voices' shape: 97 decoder launches (1 start + 12 x (4
    gate convs + 3 res_skip + 1 tail)), 31 encoder conv launches, 12 small kernels per utterance — a shape check that silently
    fell back to the separate launches (122 / 32 / 23) would still pass the value checks."""
    (gsd, g), _ = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_HIGH)
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(3), 120, HP.LJSPEECH.num_symbols)
    gpu_engine.glow_infer(g, ids, 0.667, 0.65, seed=1).free()
    gpu_engine.set_profiling(True)
    try:
        gpu_engine.profile_reset()
        gpu_engine.glow_infer(g, ids, 0.667, 0.65, seed=1).free()
        prof = gpu_engine.profile()
    finally:
        gpu_engine.set_profiling(False)
        names = gpu_engine.kernel_counts()
    hp = HP.LJSPEECH
    # by kernel name: the 16-row gate tile, the block tails and conv_o + LayerNorm as column owners; no generic-tile fallback
    assert names["gate16_kernel"] == hp.n_blocks_dec * hp.n_block_layers and names["glow_tail_kernel"] == hp.n_blocks_dec
    assert names["oproj_ln_kernel"] == hp.n_layers_enc
    assert names["lin16_kernel"] + names["lin16_kernel.ln"] >= hp.n_blocks_dec * (hp.n_block_layers - 1) + 2 * hp.n_layers_enc
    assert prof["conv_mfma.glow_decoder"]["launches"] == 1 + hp.n_blocks_dec * (2 * hp.n_block_layers)
    assert prof["conv_mfma.glow_encoder"]["launches"] == 4 + hp.n_layers_enc * 4 + 3
    assert prof["elementwise"]["launches"] == 1 + hp.n_layers_enc + 5


VOC_KERNELS = {
    # 'high' at 617 frames, batch 1: the 256-channel stage's six launches are the PROMOTED ones (128-row tile, snake dispatch
    # order), the 128-channel stage's six keep the plain longest-first order (more workgroups than resident slots; a call that
    # shares the context with another one runs them on 128-column tiles: test_busy_context_takes_128_column_tiles), the 64- and
    # 32-channel stages run the four-wave fused pair; nothing falls back to the chunked tile or the k-split pair
    "high": {"rb_group_kernel.snake": 6, "rb_group_kernel": 6, "rb_group_kernel.nb4": 0, "rb_pair_group_kernel": 6, "conv_group_kernel": 0, "pair_group_kernel": 0,
             "mrf_small_kernel": 0, "mrf8_kernel": 0},
    # 'medium': 42 / 161 tiles per member in its 64- / 32-channel stages -> the 8-wave k-split pair (plan_pair's rule); the 16-
    # and 8-channel stages are one launch each
    "medium": {"pair_group_kernel": 6, "rb_pair_group_kernel": 0, "rb_group_kernel": 0, "rb_group_kernel.snake": 0, "conv_group_kernel": 0,
               "mrf_small_kernel": 1, "mrf8_kernel": 1},
}


@pytest.mark.parametrize("quality,resblock,narrow", [("high", 18, 0), ("medium", 6, 2)])
def test_vocoder_launch_counts_on_the_device(gpu_engine, quality, resblock, narrow):
    """The fused vocoder schedule is the one that runs at the released shapes, by launch CLASS ('high' = 18 grouped ResBlock
    launches, 'medium' = 6 fused-pair launches + one launch per narrow stage) and by kernel NAME (`kernel_counts`): the class
    counts cannot tell `rb_group_kernel` from `conv_group_kernel` or `rb_pair_group_kernel` from `pair_group_kernel` — same
    launch count, and the first pair computes the same bits by design — so a tile rule that misfired would pass every value
    check and the class counts."""
    vhp = HP.VOCODER_QUALITY[quality]
    _, (vsd, v) = models(gpu_engine, HP.LJSPEECH, vhp)
    rng = np.random.default_rng(5)
    mel = (0.57 + 0.06 * rng.standard_normal((1, 80, 617))).astype(np.float32)
    mb = gpu_engine.mel_from_numpy(mel[0])
    gpu_engine.hifigan_infer(v, mb)
    gpu_engine.set_profiling(True)
    try:
        gpu_engine.profile_reset()
        gpu_engine.hifigan_infer(v, mb)
        prof = gpu_engine.profile()
        names = gpu_engine.kernel_counts()
    finally:
        gpu_engine.set_profiling(False)
    assert prof["conv_mfma.hifigan_resblock"]["launches"] == resblock, prof
    assert prof.get("mrf_small.hifigan_narrow_stage", {"launches": 0})["launches"] == narrow, prof
    assert prof["conv_mfma.hifigan_upsample"]["launches"] == 4 and prof["conv_mfma.hifigan_pre_post"]["launches"] == 2, prof
    for k, n in VOC_KERNELS[quality].items():
        assert names[k] == n, (k, names)


def test_busy_context_takes_128_column_tiles(gpu_engine):
    """`rb_group_kernel<11, 7, 3, 4>` (host_launch.h, run_group): the 128-channel stage's grouped launches of a call that shares the
    context with another call run on 128-column tiles (927 of them at 617 frames: more than the chip holds) — the same bits as the lone
    call's 64-column tiles.  Two threads synthesise the same mel concurrently; every result equals the lone call's, and the
    128-column launches were taken (by some of the calls: a call that happens to find the context idle keeps the 64-column ones)."""
    import threading

    vhp = HP.VOCODER_QUALITY["high"]
    _, (vsd, v) = models(gpu_engine, HP.LJSPEECH, vhp)
    mel = (0.57 + 0.06 * np.random.default_rng(5).standard_normal((1, 80, 617))).astype(np.float32)
    lone, _ = gpu_engine.hifigan_infer(v, gpu_engine.mel_from_numpy(mel[0]))
    gpu_engine.profile_reset()
    out = [None] * 12
    errs = []

    def work(t):
        try:
            for i in range(t, len(out), 3):
                out[i], _ = gpu_engine.hifigan_infer(v, gpu_engine.mel_from_numpy(mel[0]))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(t,)) for t in range(3)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    names = gpu_engine.kernel_counts()
    assert names.get("rb_group_kernel.nb4", 0) > 0, names  # (read per launch: a call may mix the two tiles)
    assert names.get("rb_group_kernel.nb4", 0) + names.get("rb_group_kernel", 0) == 6 * len(out), names
    for w in out:
        np.testing.assert_array_equal(w, lone)


def test_worker_streams_are_grouped_by_hardware_queue(gpu_engine):
    """`mi355tts_reserve` measures which worker streams share a hardware queue (the runtime has 4 — GPU_MAX_HW_QUEUES — and deals
    them to streams as they are first used; two streams of one queue run their kernels one after the other) and a call takes the
    free worker whose queue carries the fewest calls.  With 9 workers: every worker probed, between 2 and 8 groups numbered from
    0, no group empty, and at least one group with two streams (9 streams cannot have 4 queues to themselves).  Results do not
    depend on which worker a call gets: eight concurrent callers, every waveform equal to the lone call's."""
    import threading

    vhp = HP.VOCODER_QUALITY["medium"]
    _, (vsd, v) = models(gpu_engine, HP.LJSPEECH, vhp)
    gpu_engine.reserve(9, 0, v, max_batch=1, max_frames=256)
    groups = gpu_engine.worker_queue_groups()
    probed = [g for g in groups if g >= 0]
    assert len(probed) >= 9, groups
    n = max(probed) + 1
    assert 2 <= n <= 8 and set(probed) == set(range(n)), groups
    assert max(probed.count(g) for g in range(n)) >= 2, groups
    mel = (0.57 + 0.06 * np.random.default_rng(6).standard_normal((1, 80, 200))).astype(np.float32)
    lone, _ = gpu_engine.hifigan_infer(v, gpu_engine.mel_from_numpy(mel[0]))
    out, errs = [None] * 24, []

    def work(t):
        try:
            for i in range(t, len(out), 8):
                out[i], _ = gpu_engine.hifigan_infer(v, gpu_engine.mel_from_numpy(mel[0]))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for w in out:
        np.testing.assert_array_equal(w, lone)


def test_dispatch_order_selfcheck_on_the_device(gpu_engine):
    """`mi355tts_dispatch_selfcheck`: the dispatcher rule behind the snake order of fully resident grouped launches (and the
    promotion of the 256-channel stage that relies on it) is MEASURED on the device the library runs on — on an MI355X the snake
    order must win (profiles/r04_rb_diag_snake_order.txt: 121 us against 133 for the plain order), and the options stay on."""
    models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_HIGH)  # the first 'high'-class load runs the check by itself
    r = gpu_engine.dispatch_selfcheck()
    assert r["state"] == "snake order kept", r
    assert 50.0 < r["snake_us"] <= 1.02 * r["plain_us"] < 400.0, r


def test_promoted_stage_really_runs_on_the_device(gpu_engine):
    """The 256-channel stage of 'high' at batch 1 takes the 128-row tile in snake order (`promote_group_plans`; the golden parity
    tests above run through it).  Option "group_promote" = 0 sends the same step to the 64 x 32 k-split tile — another summation
    order — so: the two settings give different bits (the promotion is live on this device, not a silent fallback), both within
    the waveform bar of the reference's output, and the launch count of the class is the same 18."""
    c = load_case("ljspeech_high_S120")
    (gsd, g), (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    mb = gpu_engine.mel_from_numpy(c["mel_voc"][None])
    gpu_engine.set_profiling(True)
    gpu_engine.profile_reset()
    on, _ = gpu_engine.hifigan_infer(v, mb)
    n_on = gpu_engine.profile()["conv_mfma.hifigan_resblock"]["launches"]
    gpu_engine.set_option("group_promote", 0)
    try:
        gpu_engine.profile_reset()
        off, _ = gpu_engine.hifigan_infer(v, mb)
        n_off = gpu_engine.profile()["conv_mfma.hifigan_resblock"]["launches"]
    finally:
        gpu_engine.set_option("group_promote", 1)
        gpu_engine.set_profiling(False)
    n = c["wav"].shape[0]
    assert n_on == n_off == 18
    assert not np.array_equal(on, off)
    for wav in (on, off):
        assert np.sqrt(np.mean((wav[0, :n] - c["wav"]) ** 2)) <= WAV_RMS_TOL
    assert np.abs(on - off).max() <= 1e-5


def test_long_utterance_and_three_resident_voices(gpu_engine):
    """BASELINE config 5 shape: three voices (en V=46, de V=54, fr V=42) resident at
    once, interleaved calls; plus a long (400-id) sentence at 'low' quality:
    frame count = duration sum, every sample finite, per-voice results unaffected by
    what else is loaded."""
    s = ljspeech_audio_settings()
    voices = {}
    for name, ghp in (("en", HP.LJSPEECH), ("de", HP.THORSTEN), ("fr", HP.SIWIS)):
        sd = synthetic.make_glow_state_dict(ghp, seed=1234 + len(name) * 7 + ord(name[0]))
        voices[name] = (ghp, sd, gpu_engine.load_glow(ghp, sd))
    _, (vsd, v) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_LOW)
    rng = np.random.default_rng(3)
    first = {}
    for rnd in range(2):
        for name, (ghp, sd, g) in voices.items():
            ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(ord(name[0])), 40, ghp.num_symbols)
            mel = gpu_engine.glow_infer(g, ids, 0.0, 1.0, audio_settings=s)
            wav, _ = gpu_engine.hifigan_infer(v, mel)
            if rnd == 0:
                first[name] = wav.copy()
                ref = glow_tts_np.glow_tts_infer(sd, ghp, ids, None, 0.0, 1.0)
                assert int(mel.frames[0]) == ref.shape[1]
                assert np.abs(mel.numpy("raw")[0] - ref).max() <= 5e-5
            else:
                assert np.array_equal(first[name], wav)
    ghp, sd, g = voices["en"]
    ids = synthetic.synthetic_phoneme_ids(rng, 400, ghp.num_symbols)
    taps = {}
    glow_tts_np.text_encoder(sd, ids, ghp, taps)
    _, F, _ = glow_tts_np.durations_to_frames(taps["logw"], 1.0, 2)
    mel = gpu_engine.glow_infer(g, ids, 0.667, 1.0, seed=5, audio_settings=s)
    assert int(mel.frames[0]) == F
    wav, i16 = gpu_engine.hifigan_infer(v, mel)
    assert wav.shape[1] == F * 256 and np.isfinite(wav).all() and np.abs(wav).max() < 1.0
    for name, (_, _, g) in voices.items():
        gpu_engine.unload(g)


def test_device_resident_mel_input(gpu_engine):
    """`mi355tts_mel_from_buffer` with MI355TTS_IN_DEVICE: a mel produced elsewhere on the GPU
    (here a torch tensor — north_star: "PyTorch-ROCm tensors for I/O only") goes to the vocoder
    without a host round trip and gives the same waveform as the host-array path, including the
    fused mel transforms; and MI355TTS_OUT_DEVICE writes the waveform into a torch tensor."""
    import torch

    from larynx_amd import ffi

    _, (vsd, v) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_LOW)
    s = ljspeech_audio_settings()
    rng = np.random.default_rng(17)
    raw = (0.57 + 0.2 * rng.standard_normal((2, 80, 96))).astype(np.float32)
    frames = np.array([96, 70], np.int32)
    host = gpu_engine.mel_from_numpy(raw, frames=frames, audio_settings=s)
    w_host, i_host = gpu_engine.hifigan_infer(v, host)
    t = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    dev = gpu_engine.mel_from_device(t.data_ptr(), frames, 80, 96, audio_settings=s)
    w_dev, i_dev = gpu_engine.hifigan_infer(v, dev)
    n = 96 * 256
    out_f = torch.full((2, n + 8), 7.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((2, n + 8), 7, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    gpu_engine.hifigan_infer_raw(v, dev, out_f.data_ptr(), out_i.data_ptr(), n + 8, flags=ffi.OUT_DEVICE)
    dev.free()
    assert np.array_equal(w_host, w_dev) and np.array_equal(i_host, i_dev)
    assert np.array_equal(out_f.cpu().numpy()[:, :n], w_host) and np.array_equal(out_i.cpu().numpy()[:, :n], i_host)
    assert np.all(out_f.cpu().numpy()[:, n:] == 0) and np.all(out_i.cpu().numpy()[:, n:] == 0)  # tail up to wav_ld zero-filled
    ref = hifi_gan_np.hifigan_infer(vsd, HP.HIFIGAN_LOW, audio_np.mel_to_vocoder_input(raw[1, :, :70], s))
    assert np.sqrt(np.mean((w_dev[1, : 70 * 256] - ref) ** 2)) <= 2e-5 and np.all(w_dev[1, 70 * 256 :] == 0)


def test_fallback_kernels_for_unusual_hparams(gpu_engine):
    from tests.test_emu_pipeline import check_fallback_kernels

    check_fallback_kernels(gpu_engine)


def test_bad_ids_are_rejected(gpu_engine):
    from larynx_amd.ffi import Mi355ttsError

    (gsd, g), _ = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_MEDIUM)
    with pytest.raises(Mi355ttsError):
        gpu_engine.glow_infer(g, np.array([3, 46, 2]))
    with pytest.raises(Mi355ttsError):
        gpu_engine.glow_infer(g, np.array([3, -1, 2]))


@pytest.mark.parametrize("n_ids", [1, 2, 9])
def test_shortest_utterances_full_size_models(gpu_engine, n_ids):
    (gsd, g), (vsd, v) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_MEDIUM)
    ids = np.array([3, 8, 4, 14, 3, 35, 3, 26, 2][:n_ids], np.int64)
    s = ljspeech_audio_settings()
    ref = glow_tts_np.glow_tts_infer(gsd, HP.LJSPEECH, ids, None, 0.0, 1.0)
    mel = gpu_engine.glow_infer(g, ids, 0.0, 1.0, audio_settings=s)
    assert int(mel.frames[0]) == ref.shape[1]
    assert np.abs(mel.numpy("raw")[0] - ref).max() <= 5e-5
    wav, _ = gpu_engine.hifigan_infer(v, mel)
    refw = hifi_gan_np.hifigan_infer(vsd, HP.HIFIGAN_MEDIUM, audio_np.mel_to_vocoder_input(ref, s))
    assert np.sqrt(np.mean((wav[0] - refw) ** 2)) <= 1e-4
    # the same ids with the decoder's WaveNets in fp16 (wn_f16.h: a one-tile launch with most of the tile past the sequence's end):
    # same frame count, the mel inside the half-precision band the golden cases are held to (the reference's decoder under .half():
    # 1.5-1.7e-3)
    from larynx_amd import ffi

    assert gpu_engine.set_precision(g, ffi.PRECISION_F16) == 0
    try:
        mel16 = gpu_engine.glow_infer(g, ids, 0.0, 1.0)
    finally:
        gpu_engine.set_precision(g, ffi.PRECISION_F32)
    assert int(mel16.frames[0]) == ref.shape[1]
    e16 = float(np.abs(mel16.numpy("raw")[0] - ref).max())
    assert 0 < e16 <= 1.5e-3, e16


@pytest.mark.parametrize("name", ["ljspeech_high_echo", "ljspeech_high_S120", "ljspeech_medium_dave_ls12", "ljspeech_low_echo"])
def test_bf16x3_mode_against_the_reference(gpu_engine, name):
    """The reference's `half` switch on this backend = split-bf16 ResBlock convs (conv_bf16.h).  Documented
    tolerance vs the reference's f32 output: waveform RMS <= 1e-4 (north_star's f32 bar still holds — the
    split keeps 16 mantissa bits per operand and accumulates in f32), int16 within 1 LSB (measured on every golden:
    RMS 0.5-1.7e-6, 1 LSB — the bound bench.py / README / DESIGN quote is the one asserted here); the exact mode is
    untouched by switching back and forth."""
    from larynx_amd import ffi

    c = load_case(name)
    _, (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    mb = gpu_engine.mel_from_numpy(c["mel_voc"])
    exact, _ = gpu_engine.hifigan_infer(v, mb)
    gpu_engine.set_precision(v, ffi.PRECISION_BF16X3)
    try:
        wav, i16 = gpu_engine.hifigan_infer(v, mb)
    finally:
        gpu_engine.set_precision(v, ffi.PRECISION_F32)
    again, _ = gpu_engine.hifigan_infer(v, mb)
    assert np.array_equal(exact, again)
    rms = float(np.sqrt(np.mean((wav[0] - c["wav"]) ** 2)))
    mx = float(np.abs(wav[0] - c["wav"]).max())
    d16 = int(np.abs(i16[0].astype(np.int32) - c["wav_i16"].astype(np.int32)).max())
    print(f"bf16x3 {name}: rms {rms:.3e} max {mx:.3e} int16 {d16} LSB")
    if c["voc_hp"].upsample_initial_channel >= 128:
        assert not np.array_equal(exact, wav)  # the mode ran (stages with >= 64 channels exist)
    assert rms <= WAV_RMS_TOL and d16 <= 1, (rms, mx, d16)


@pytest.mark.parametrize("name", ["ljspeech_high_S120", "ljspeech_medium_dave_ls12"])
def test_bf16x3_fused_call_against_the_reference(gpu_engine, name):
    """The path `half=True` really takes — ids -> ONE fused `mi355tts_synthesize` call with the vocoder in split-bf16
    mode (what bench.py's half_mode leg times) — against the reference's f32 golden: frames identical, waveform RMS
    within north_star's 1e-4, int16 within 1 LSB."""
    from larynx_amd import ffi

    c = load_case(name)
    (gsd, g), (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    s = ljspeech_audio_settings()
    gpu_engine.set_precision(v, ffi.PRECISION_BF16X3)
    gpu_engine.set_precision(g, ffi.PRECISION_BF16X3)
    try:
        frames, wav, i16 = gpu_engine.synthesize(g, v, c["ids"], float(c["noise_scale"]), float(c["length_scale"]), noise=c["noise"],
                                                 audio_settings=s, want_float=True)
    finally:
        gpu_engine.set_precision(v, ffi.PRECISION_F32)
        gpu_engine.set_precision(g, ffi.PRECISION_F32)
    assert int(frames[0]) == c["mel"].shape[1]
    n = c["wav"].shape[0]
    rms = float(np.sqrt(np.mean((wav[0, :n] - c["wav"]) ** 2)))
    d16 = int(np.abs(i16[0, :n].astype(np.int32) - c["wav_i16"].astype(np.int32)).max())
    print(f"bf16x3 fused {name}: rms {rms:.3e} int16 {d16} LSB")
    assert rms <= WAV_RMS_TOL and d16 <= 1, (rms, d16)


def test_plain_bf16_mode_documented_tolerance(gpu_engine):
    """MI355TTS_PRECISION_BF16 (one bf16 MFMA per product): the plain `half`-style precision.  Documented tolerance vs
    the reference's f32 waveform: RMS <= 1e-2 (measured ~1e-3 on amplitude ~0.18 waveforms) — two to three orders
    coarser than the split mode, which is what `half=True` selects."""
    from larynx_amd import ffi

    c = load_case("ljspeech_high_S120")
    _, (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    mb = gpu_engine.mel_from_numpy(c["mel_voc"])
    out = {}
    for name, prec in (("bf16", ffi.PRECISION_BF16), ("bf16x3", ffi.PRECISION_BF16X3)):
        gpu_engine.set_precision(v, prec)
        try:
            wav, _ = gpu_engine.hifigan_infer(v, mb)
        finally:
            gpu_engine.set_precision(v, ffi.PRECISION_F32)
        out[name] = float(np.sqrt(np.mean((wav[0] - c["wav"]) ** 2)))
    print("plain bf16 rms", out["bf16"], "split rms", out["bf16x3"])
    assert out["bf16"] <= 1e-2 and out["bf16x3"] <= 1e-4 and out["bf16"] > 20 * out["bf16x3"]


F16_CASES = ["ljspeech_high_echo", "ljspeech_high_S120", "ljspeech_high_P200", "ljspeech_high_short5", "ljspeech_medium_dave_ls12", "ljspeech_low_echo",
             "thorsten_medium_veg"]


@pytest.mark.parametrize("name", F16_CASES)
def test_f16_mode_against_the_reference(gpu_engine, name):
    """The reference's `half` switch = `.half()` on the generator (larynx/hifi_gan.py:96-97).  Here: the native fp16 vocoder
    (csrc/conv_f16.h).  The tolerance is anchored on the reference itself: oracle/make_golden.py ran the reference's OWN
    generator under .half() on this case's vocoder input and stored its RMS / max error against its own f32 waveform
    (`ref_half_rms`, `ref_half_max`); the HIP mode must be no worse — on the float waveform and on the int16 samples.  Every
    layer honours the switch (no f32 / bf16 vocoder kernel launches), and the exact mode is untouched by switching back."""
    from larynx_amd import ffi

    c = load_case(name)
    _, (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    mb = gpu_engine.mel_from_numpy(c["mel_voc"])
    exact, _ = gpu_engine.hifigan_infer(v, mb)
    assert gpu_engine.set_precision(v, ffi.PRECISION_F16) == 0
    try:
        gpu_engine.profile_reset()
        wav, i16 = gpu_engine.hifigan_infer(v, mb)
        counts = gpu_engine.kernel_counts()
    finally:
        gpu_engine.set_precision(v, ffi.PRECISION_F32)
    again, _ = gpu_engine.hifigan_infer(v, mb)
    assert np.array_equal(exact, again)
    vh = c["voc_hp"]
    steps = len(vh.upsample_rates) * len(vh.resblock_dilation_sizes[0])
    if vh.resblock == "1":  # one fused conv1 + conv2 launch per dilation step (pair_f16.h) up to 128 channels, two grouped launches above
        wide = sum(1 for i in range(len(vh.upsample_rates)) if vh.stage_channels(i) > 128) * len(vh.resblock_dilation_sizes[0])
        assert counts.get("pair_f16_group_kernel", 0) == steps - wide and counts.get("conv_f16_group_kernel", 0) == 2 * wide
    else:
        assert counts.get("conv_f16_group_kernel", 0) == steps and counts.get("pair_f16_group_kernel", 0) == 0
    assert counts.get("conv_f16_kernel", 0) == 1 + len(vh.upsample_rates) and counts.get("post_f16_kernel", 0) == 1
    for k in ("conv_mfma_kernel", "conv_mfma_kernel.m128", "rb_group_kernel", "rb_group_kernel.snake", "rb_pair_group_kernel", "conv_bf16_group_kernel",
              "pair_bf16_group_kernel", "mrf_small_kernel", "mrf8_kernel", "post_conv_kernel"):
        assert counts.get(k, 0) == 0, k
    rms = float(np.sqrt(np.mean((wav[0] - c["wav"]) ** 2)))
    mx = float(np.abs(wav[0] - c["wav"]).max())
    d16 = int(np.abs(i16[0].astype(np.int32) - c["wav_i16"].astype(np.int32)).max())
    print(f"f16 {name}: rms {rms:.3e} (reference .half(): {float(c['ref_half_rms']):.3e})  max {mx:.3e} ({float(c['ref_half_max']):.3e})  "
          f"int16 {d16} LSB ({int(c['ref_half_i16'])})")
    assert rms <= float(c["ref_half_rms"]) and mx <= 1.5 * float(c["ref_half_max"]) and d16 <= 1.5 * int(c["ref_half_i16"]), (rms, mx, d16)
    assert not np.array_equal(exact, wav)


@pytest.mark.parametrize("name", CASES)
def test_f16_acoustic_mode_against_the_reference(gpu_engine, name):
    """The acoustic model's share of the reference's `half` switch (`.half()` on the FlowGenerator, larynx/glow_tts.py:90-91): the
    decoder's WaveNets in fp16, ONE launch per coupling block (csrc/wn_f16.h).  The tolerance is anchored on the reference itself:
    oracle/make_golden_glow_half.py ran the reference's OWN FlowGenerator with its decoder under .half() on this case and stored
    the mel's max / RMS deviation from its f32 mel (tests/golden/glow_half_reference.json); the HIP mode must be no worse.  The
    frame count is the f32 model's (encoder and durations stay f32), and switching back restores the exact chain bit for bit."""
    from larynx_amd import ffi
    from tests.golden_util import load_glow_half_reference

    c = load_case(name)
    anchor = load_glow_half_reference()[name]
    (gsd, g), _ = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    ns, ls = float(c["noise_scale"]), float(c["length_scale"])
    exact = gpu_engine.glow_infer(g, c["ids"], ns, ls, noise=c["noise"]).numpy("raw")[0]
    assert gpu_engine.set_precision(g, ffi.PRECISION_F16) == 0
    try:
        gpu_engine.profile_reset()
        mel = gpu_engine.glow_infer(g, c["ids"], ns, ls, noise=c["noise"])
        counts = gpu_engine.kernel_counts()
    finally:
        assert gpu_engine.set_precision(g, ffi.PRECISION_F32) == 0
    nb = c["glow_hp"].n_blocks_dec
    assert counts.get("wn_f16_kernel", 0) == nb and counts.get("glow_tail_kernel", 0) == nb
    assert counts.get("gate16_kernel", 0) == 0 and counts.get("gate16_kernel.wide", 0) == 0
    F = int(mel.frames[0])
    assert F == c["mel"].shape[1]
    got = mel.numpy("raw")[0][:, :F]
    mx = float(np.abs(got - c["mel"]).max())
    rms = float(np.sqrt(np.mean((got - c["mel"]) ** 2)))
    print(f"f16 acoustic {name}: mel max {mx:.3e} (reference decoder .half(): {anchor['dec_half_max']:.3e})  rms {rms:.3e} ({anchor['dec_half_rms']:.3e})")
    assert mx <= anchor["dec_half_max"] and rms <= anchor["dec_half_rms"], (mx, rms)
    assert not np.array_equal(got, exact[:, :F])
    again = gpu_engine.glow_infer(g, c["ids"], ns, ls, noise=c["noise"]).numpy("raw")[0]
    assert np.array_equal(exact, again)


@pytest.mark.parametrize("acoustic", ["f32", "f16"])
@pytest.mark.parametrize("name", ["ljspeech_high_S120", "ljspeech_medium_dave_ls12"])
def test_f16_fused_call_against_the_reference(gpu_engine, name, acoustic):
    """The path `half=True` really takes — ids -> ONE fused `mi355tts_synthesize` call (what bench.py's half_mode leg times):
    frames identical to the reference's.  Vocoder in fp16 and the acoustic model left in f32: waveform within the reference's own
    generator-under-.half() error against the f32 golden.  BOTH models in fp16 (what `half=True` selects on both classes): within
    what the reference's own two models under .half() cost on this case at the f32 model's frame count
    (tests/golden/glow_half_reference.json: both_half_wav_rms, both_half_i16)."""
    from larynx_amd import ffi
    from tests.golden_util import load_glow_half_reference

    c = load_case(name)
    (gsd, g), (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    s = ljspeech_audio_settings()
    gpu_engine.set_precision(v, ffi.PRECISION_F16)
    if acoustic == "f16":
        assert gpu_engine.set_precision(g, ffi.PRECISION_F16) == 0
    try:
        gpu_engine.profile_reset()
        frames, wav, i16 = gpu_engine.synthesize(g, v, c["ids"], float(c["noise_scale"]), float(c["length_scale"]), noise=c["noise"],
                                                 audio_settings=s, want_float=True)
        counts = gpu_engine.kernel_counts()
    finally:
        gpu_engine.set_precision(v, ffi.PRECISION_F32)
        gpu_engine.set_precision(g, ffi.PRECISION_F32)
    assert counts.get("wn_f16_kernel", 0) == (c["glow_hp"].n_blocks_dec if acoustic == "f16" else 0)
    assert int(frames[0]) == c["mel"].shape[1]
    n = int(frames[0]) * c["voc_hp"].hop
    rms = float(np.sqrt(np.mean((wav[0, :n] - c["wav"]) ** 2)))
    d16 = int(np.abs(i16[0, :n].astype(np.int32) - c["wav_i16"].astype(np.int32)).max())
    if acoustic == "f32":
        bar_rms, bar_i16 = float(c["ref_half_rms"]), 1.5 * int(c["ref_half_i16"])
    else:
        a = load_glow_half_reference()[name]
        bar_rms, bar_i16 = a["both_half_wav_rms"], a["both_half_i16"]
    print(f"f16 fused {name} (acoustic model {acoustic}): rms {rms:.3e} (reference .half(): {bar_rms:.3e}) int16 {d16} LSB ({bar_i16})")
    assert rms <= bar_rms and d16 <= bar_i16, (rms, d16)


def test_f16_acoustic_config4_batch_rows(gpu_engine):
    """BASELINE config 4's ragged batch of 8 (thorsten) with the acoustic model's decoder WaveNets in fp16: every row's frame count
    the reference's, every row's mel within the reference's own decoder-under-.half() figures (the single-utterance thorsten case of
    tests/golden/glow_half_reference.json: the same voice), padded tails exactly 0, and a row inside the batch equal to its solitary
    call within a tenth of that figure (not bit for bit at this size: the f32 launches around the fp16 one pick other tiles for a
    padded batch — another f32 summation order —, and the rounding of `h` to fp16 turns a last-bit difference into half an fp16 ulp
    here and there; on the emulator's shapes, where the tiles coincide, rows equal their solitary calls exactly)."""
    from larynx_amd import ffi
    from tests.golden_util import load_batch8, load_glow_half_reference

    c = load_batch8()
    anchor = load_glow_half_reference()["thorsten_medium_veg"]
    (gsd, g), _ = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    assert gpu_engine.set_precision(g, ffi.PRECISION_F16) == 0
    try:
        gpu_engine.profile_reset()
        mel = gpu_engine.glow_infer(g, c["ids"], c["noise_scale"], c["length_scale"], noise=c["noise"])
        assert gpu_engine.kernel_counts().get("wn_f16_kernel", 0) == c["glow_hp"].n_blocks_dec
        raw = mel.numpy("raw")
        for b in range(8):
            F = c["mel"][b].shape[1]
            assert int(mel.frames[b]) == F
            d = raw[b][:, :F] - c["mel"][b]
            assert float(np.abs(d).max()) <= anchor["dec_half_max"] and float(np.sqrt(np.mean(d ** 2))) <= anchor["dec_half_rms"], (b, float(np.abs(d).max()))
            assert np.all(raw[b][:, F:] == 0)
        for b in (0, 6):
            one = gpu_engine.glow_infer(g, c["ids"][b], c["noise_scale"], c["length_scale"], noise=c["noise"][b])
            F = int(one.frames[0])
            assert float(np.abs(one.numpy("raw")[0][:, :F] - raw[b][:, :F]).max()) <= 0.1 * anchor["dec_half_max"]
    finally:
        gpu_engine.set_precision(g, ffi.PRECISION_F32)


def test_f16_config4_batch_rows(gpu_engine):
    """BASELINE config 4 (thorsten + 'medium', B = 8 ragged) with the vocoder in fp16: every row within the reference's own
    .half() error for THAT row, padded tails exactly 0, and a row inside the batch equal to its solitary call bit for bit
    (the ragged grid deals a row its own tiles: same tiles, same summation order)."""
    from larynx_amd import ffi
    from tests.golden_util import load_batch8

    c = load_batch8()
    ghp, vhp = c["glow_hp"], c["voc_hp"]
    (gsd, g), (vsd, v) = models(gpu_engine, ghp, vhp)
    s = ljspeech_audio_settings()
    mel = gpu_engine.glow_infer(g, c["ids"], c["noise_scale"], c["length_scale"], noise=c["noise"], audio_settings=s)
    hop = vhp.hop
    gpu_engine.set_precision(v, ffi.PRECISION_F16)
    try:
        wav, i16 = gpu_engine.hifigan_infer(v, mel)
        for b in range(8):
            n = c["mel"][b].shape[1] * hop
            rms = float(np.sqrt(np.mean((wav[b, :n] - c["wav"][b]) ** 2)))
            assert rms <= c["ref_half_rms"][b], (b, rms, c["ref_half_rms"][b])
            assert np.all(wav[b, n:] == 0) and np.all(i16[b, n:] == 0)
        for b in (0, 5):
            one = gpu_engine.glow_infer(g, c["ids"][b], c["noise_scale"], c["length_scale"], noise=c["noise"][b], audio_settings=s)
            w1, _ = gpu_engine.hifigan_infer(v, one)
            n = int(one.frames[0]) * hop
            if np.array_equal(one.numpy("vocoder")[0], mel.numpy("vocoder")[b, :, : int(one.frames[0])]):  # same mel bits in -> same bits out
                np.testing.assert_array_equal(wav[b, :n], w1[0, :n])
            else:
                assert np.sqrt(np.mean((wav[b, :n] - w1[0, :n]) ** 2)) <= 2 * c["ref_half_rms"][b]
    finally:
        gpu_engine.set_precision(v, ffi.PRECISION_F32)


def test_f16_denoiser_uses_the_half_models_own_bias(gpu_engine):
    """`denoiser_strength > 0` with the vocoder in fp16: the bias spectrum comes from the generator AS IT RUNS (the reference
    derives it from the half model, larynx/hifi_gan.py:181-203) — cached per arithmetic, so switching modes never mixes them —
    and the denoised waveform equals the oracle's STFT denoiser applied to the mode's own waveform with the mode's own bias."""
    from larynx_amd import ffi
    from oracle import denoise_np

    c = load_case("ljspeech_medium_dave_ls12")
    _, (vsd, v) = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    mb = gpu_engine.mel_from_numpy(c["mel_voc"])
    strength = 0.1
    f32_den, _ = gpu_engine.hifigan_infer(v, mb, denoiser_strength=strength)  # the f32 bias exists first
    gpu_engine.set_precision(v, ffi.PRECISION_F16)
    try:
        plain, _ = gpu_engine.hifigan_infer(v, mb)
        den, _ = gpu_engine.hifigan_infer(v, mb, denoiser_strength=strength)
        bias = denoise_np.bias_spectrum(lambda m: gpu_engine.hifigan_infer(v, gpu_engine.mel_from_numpy(np.asarray(m, np.float32)[None]))[0][0])
    finally:
        gpu_engine.set_precision(v, ffi.PRECISION_F32)
    want = denoise_np.denoise(plain[0], bias, strength)
    assert np.sqrt(np.mean((den[0] - want) ** 2)) <= 1e-5
    assert np.sqrt(np.mean((den[0] - c["wav_denoised"]) ** 2)) <= 2 * float(c["ref_half_rms"])  # and near the reference's f32 result
    again, _ = gpu_engine.hifigan_infer(v, mb, denoiser_strength=strength)
    assert np.array_equal(again, f32_den)  # the f32 mode kept its own bias


def test_f16_coalesced_calls(gpu_engine):
    """Whole-call coalescing with the vocoder in fp16: eight threads' ragged batch-1 calls ride fused padded calls; frames identical
    to the solitary calls.  A padded batch's acoustic pass differs from the solitary one at f32 round-off; in fp16 that is enough to
    send roundings of the mel and of every later plane the other way, so the two waveforms are two draws of the mode's rounding
    noise: each within the reference's own .half() deviation from the f32 truth (3.3e-4 RMS on 'high', tests/golden), their
    difference within 1.5 x that (measured 2.7e-4)."""
    import threading

    from larynx_amd import ffi

    (gsd, g), (vsd, v) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_HIGH)
    s = ljspeech_audio_settings()
    rng = np.random.default_rng(78)
    lens = (120, 33, 64, 97, 120, 15, 81, 50)
    ids = [synthetic.synthetic_phoneme_ids(rng, n, HP.LJSPEECH.num_symbols) for n in lens]

    def call(i):
        return gpu_engine.synthesize(g, v, ids[i], 0.667, 0.65, seed=900 + i, audio_settings=s, want_float=True, pad_before=11 * i,
                                     frames_per_id_guess=20.0)

    gpu_engine.set_precision(v, ffi.PRECISION_F16)
    try:
        gpu_engine.set_option("call_coalesce", 0)
        solo = [call(i) for i in range(len(ids))]
        gpu_engine.set_option("call_coalesce", 2)
        p0, r0 = gpu_engine.coalesce_stats()
        out = [None] * len(ids)
        bar = threading.Barrier(len(ids))

        def work(i):
            bar.wait()
            out[i] = call(i)

        th = [threading.Thread(target=work, args=(i,)) for i in range(len(ids))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        p1, r1 = gpu_engine.coalesce_stats()
        assert r1 - r0 == len(ids) and p1 - p0 < r1 - r0
        for (fa, wa, ia), (fb, wb, ib) in zip(solo, out):
            assert np.array_equal(fa, fb) and ia.shape == ib.shape
            assert np.sqrt(np.mean((wa - wb) ** 2)) <= 1.5 * 3.3e-4
    finally:
        gpu_engine.set_option("call_coalesce", gpu_engine.get_call_coalesce_default())
        gpu_engine.set_precision(v, ffi.PRECISION_F32)


def test_broadcast_weights_over_a_callers_rccl_communicator(gpu_engine):
    """`mi355tts_broadcast_weights`: the caller owns an RCCL communicator — here a one-rank
    one made with ctypes on the system's librccl —, the folded weight blob sits in device memory, the library
    broadcasts it in place and loads the model from the device buffer."""
    import ctypes

    import torch

    from larynx_amd import ffi

    path = "/opt/rocm/lib/librccl.so"
    try:
        rccl = ctypes.CDLL(path)
    except OSError:
        pytest.skip("no system RCCL library")

    class UniqueId(ctypes.Structure):
        _fields_ = [("internal", ctypes.c_char * 128)]

    uid = UniqueId()
    rccl.ncclGetUniqueId.argtypes = [ctypes.POINTER(UniqueId)]
    rccl.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, UniqueId, ctypes.c_int]
    rccl.ncclCommDestroy.argtypes = [ctypes.c_void_p]
    assert rccl.ncclGetUniqueId(ctypes.byref(uid)) == 0
    comm = ctypes.c_void_p()
    assert rccl.ncclCommInitRank(ctypes.byref(comm), 1, uid, 0) == 0
    try:
        hp = HP.HIFIGAN_LOW
        sd = synthetic.make_hifigan_state_dict(hp, seed=1234)
        blob = gpu_engine.hifigan_blob(hp, sd)
        t = torch.from_numpy(blob).cuda()
        torch.cuda.synchronize()
        gpu_engine.broadcast_weights(comm.value, 0, t.data_ptr(), blob.size, rccl_library=path)
        assert np.array_equal(t.cpu().numpy(), blob)
        v_dev = gpu_engine.load_hifigan(hp, device_ptr=t.data_ptr())
        _, (_, v_host) = models(gpu_engine, HP.LJSPEECH, hp)
        melin = (np.random.default_rng(3).standard_normal((1, 80, 40)) * 2).astype(np.float32)
        a, _ = gpu_engine.hifigan_infer(v_dev, gpu_engine.mel_from_numpy(melin))
        b, _ = gpu_engine.hifigan_infer(v_host, gpu_engine.mel_from_numpy(melin))
        assert np.array_equal(a, b)
        gpu_engine.unload(v_dev)
        with pytest.raises(ffi.Mi355ttsError):
            gpu_engine.broadcast_weights(0, 0, t.data_ptr(), blob.size)
    finally:
        rccl.ncclCommDestroy(comm)


def test_refused_calls_leave_the_worker_clean_on_the_device():
    """A context with ONE worker, so that every call runs on the worker the call before it gave back: the three refusals that
    arrive behind queued work (conv1d with K = 9, a fused call into a row that is too small, explicit noise of too few
    columns) are plain INVALID / TOO_SMALL returns, and conv1d (B = 1, 32 -> 32 channels, K = 3, L = 64) and a 13-id
    `synthesize` behind each of them give the bits they gave before (the emulator suite's check, tiny models)."""
    from larynx_amd.engine import Engine
    from tests.test_emu_host_features import check_refusals_leave_the_worker_clean

    eng = Engine(device=0)
    try:
        g = eng.load_glow(HP.TINY_GLOW, synthetic.make_glow_state_dict(HP.TINY_GLOW, seed=7))
        v = eng.load_hifigan(HP.TINY_HIFIGAN, synthetic.make_hifigan_state_dict(HP.TINY_HIFIGAN, seed=7))
        eng.reserve(1, g, v, max_batch=1, max_ids=16, max_frames=256)
        assert len(eng.worker_queue_groups()) == 1
        y, frames, f32, i16 = check_refusals_leave_the_worker_clean(eng, g, v, HP.TINY_GLOW.num_symbols, HP.TINY_HIFIGAN.num_mels)
        assert int(frames[0]) > 0 and np.any(i16) and np.all(np.isfinite(f32)) and np.any(y)
        assert len(eng.worker_queue_groups()) == 1  # no call ever found the worker taken
    finally:
        eng.close()
