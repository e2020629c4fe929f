"""The Griffin-Lim vocoder (csrc/griffin_lim.h) on the MI355X against the reference's fixtures
(tests/golden/griffin_lim/*.npz) and, for shapes without one, the numpy restatement tests/griffin_lim_np.py (itself
pinned to the fixtures by tests/test_emu_griffin_lim.py).

The parity bound.  The anchor is what float32 arithmetic costs the reference's OWN algorithm: the relative RMS
deviation of the all-float32 numpy restatement from the reference (stored per fixture and iteration count; computed
here for the shape without a fixture).  The kernel may lie 16 x as far — a different FFT factorisation, the device's
division and square root — and never above 1e-4."""
import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd.audio import mel_basis
from tests import griffin_lim_np as G
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("ljspeech_high_short5", "ljspeech_high_echo")


def golden_mel(case):
    mel = np.load(GOLDEN / f"{case}.npz")["mel_voc"].astype(np.float32)
    return mel if mel.ndim == 3 else mel[None]


def load_fixture(case):
    z = np.load(GOLDEN / "griffin_lim" / f"{case}.npz")
    fx = {k: z[k] for k in z.files}
    fx["mel"] = golden_mel(case)
    fx["phase0"] = G.initial_phase(int(fx["phase_seed"]), fx["mel"].shape[2] - 1)
    return fx


@pytest.fixture(scope="module")
def basis():
    return mel_basis(22050, 1024, 80, 0.0, 8000)


@pytest.fixture(scope="module")
def model(gpu_engine, basis):
    m = gpu_engine.load_griffin_lim(basis, 1000.0, 60)
    yield m
    gpu_engine.unload(m)


@pytest.mark.parametrize("case", FIXTURES)
def test_parity_with_the_reference(gpu_engine, model, case):
    fx = load_fixture(case)
    mel = gpu_engine.mel_from_numpy(fx["mel"])
    T = fx["mel"].shape[2] - 1
    for iters in (1, 60):
        f32, i16, ph = gpu_engine.griffin_lim_infer(model, mel, phase0=fx["phase0"], iterations=iters, want_int16=True, want_phase=True)
        ref = fx[f"signal_{iters}"]
        assert f32.shape == (1, T * 256 + 1024) and f32.shape[1] == ref.shape[0]
        assert np.isfinite(f32).all() and np.array_equal(ph[0], fx["phase0"])
        err = G.rel_rms(f32[0], ref)
        bound = min(16.0 * float(fx[f"ref_f32_rel_rms_{iters}"]), 1e-4)
        print(f"{case} iterations={iters}: rel rms {err:.3e} (bound {bound:.3e}, float32 restatement {float(fx[f'ref_f32_rel_rms_{iters}']):.3e})")
        assert err <= bound
        if iters == 60:
            d = np.abs(i16[0].astype(np.int32) - fx["int16_60"].astype(np.int32)).max()
            print(f"{case}: int16 max difference {d} LSB")
            assert d <= 1


def test_a_shape_without_a_fixture(gpu_engine, model, basis):
    """`S120` (596 mel frames, 595 STFT frames) against the float64 restatement, under the same 16 x rule with this
    case's own float32-restatement deviation."""
    mel = golden_mel("ljspeech_high_S120")
    T = mel.shape[2] - 1
    assert T == 595
    phase0 = G.initial_phase(1, T)
    _, ref = G.griffin_lim(G.magnitudes(mel[0], basis, 1000.0, np.float64), phase0, 60, np.float64, keep=(1, 60))
    _, r32 = G.griffin_lim(G.magnitudes(mel[0], basis, 1000.0, np.float32), phase0, 60, np.float32, keep=(1, 60))
    batch = gpu_engine.mel_from_numpy(mel)
    for iters in (1, 60):
        f32, i16, _ = gpu_engine.griffin_lim_infer(model, batch, phase0=phase0, iterations=iters, want_int16=True)
        assert f32.shape == (1, ref[iters].shape[0]) and np.isfinite(f32).all()
        anchor = G.rel_rms(r32[iters], ref[iters])
        err = G.rel_rms(f32[0], ref[iters])
        bound = min(16.0 * anchor, 1e-4)
        print(f"S120 iterations={iters}: rel rms {err:.3e} (bound {bound:.3e}, float32 restatement {anchor:.3e})")
        assert err <= bound
        assert np.abs(i16[0].astype(np.int32) - G.float_to_int16(ref[iters]).astype(np.int32)).max() <= 1


def test_ragged_batch(gpu_engine, model):
    """Three rows of 41, 134 and 75 frames: each bit-identical to its batch-1 result, zero beyond its length."""
    rows = [golden_mel("ljspeech_high_short5")[0][:, :41], golden_mel("ljspeech_high_echo")[0], golden_mel("ljspeech_high_S120")[0][:, 200:275]]
    lens = [r.shape[1] for r in rows]
    assert lens == [41, 134, 75]
    mel = np.zeros((3, 80, 134), np.float32)
    for b, r in enumerate(rows):
        mel[b, :, : lens[b]] = r
    ph = np.stack([np.pad(G.initial_phase(20 + b, lens[b] - 1), ((0, 0), (0, 133 - (lens[b] - 1)))) for b in range(3)])
    f32, i16, _ = gpu_engine.griffin_lim_infer(model, gpu_engine.mel_from_numpy(mel, frames=lens), phase0=ph, iterations=60, want_int16=True)
    assert np.isfinite(f32).all()
    for b, n in enumerate(lens):
        N = (n - 1) * 256 + 1024
        one, one16, _ = gpu_engine.griffin_lim_infer(model, gpu_engine.mel_from_numpy(rows[b][None]), phase0=ph[b:b + 1, :, : n - 1],
                                                     iterations=60, want_int16=True)
        assert one.shape == (1, N)
        assert np.array_equal(one[0], f32[b, :N]) and np.array_equal(one16[0], i16[b, :N])
        assert np.all(f32[b, N:] == 0) and np.all(i16[b, N:] == 0)


def test_seeded_mode(gpu_engine, model):
    mel = gpu_engine.mel_from_numpy(golden_mel("ljspeech_high_echo"))
    a, a16, ph = gpu_engine.griffin_lim_infer(model, mel, seed=77, want_int16=True, want_phase=True)
    b, b16, _ = gpu_engine.griffin_lim_infer(model, mel, seed=77, want_int16=True)
    c, _, ph_c = gpu_engine.griffin_lim_infer(model, mel, seed=78, want_phase=True)
    d, d16, _ = gpu_engine.griffin_lim_infer(model, mel, phase0=ph, want_int16=True)
    assert np.isfinite(a).all() and np.isfinite(c).all()
    assert np.array_equal(a, b) and np.array_equal(a16, b16)
    assert np.array_equal(a, d) and np.array_equal(a16, d16)
    assert not np.array_equal(a, c) and not np.array_equal(ph, ph_c)
    assert ph.shape == (1, 513, 133) and -np.pi < float(ph.min()) and float(ph.max()) <= np.pi
    # uniform on the circle: mean 0 +- 5 sigma of pi / sqrt(3 n), both half circles in use
    assert abs(float(ph.mean())) < 5 * np.pi / np.sqrt(3 * ph.size) and 0.49 < float((ph > 0).mean()) < 0.51


def test_device_pointers(gpu_engine, model):
    """MI355TTS_IN_DEVICE / MI355TTS_OUT_DEVICE: torch tensors in and out give the host call's bits, tails zeroed."""
    torch = pytest.importorskip("torch")
    fx = load_fixture("ljspeech_high_short5")
    mel = gpu_engine.mel_from_numpy(fx["mel"])
    T = fx["mel"].shape[2] - 1
    N = T * 256 + 1024
    host, host16, _ = gpu_engine.griffin_lim_infer(model, mel, phase0=fx["phase0"], iterations=3, want_int16=True)
    ph = torch.from_numpy(fx["phase0"][None]).cuda().contiguous()
    ld = N + 100
    wav = torch.full((1, ld), 7.0, dtype=torch.float32, device="cuda")
    w16 = torch.full((1, ld), 7, dtype=torch.int16, device="cuda")
    pho = torch.zeros((1, 513, T), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu_engine.griffin_lim_infer_raw(model, mel, ph.data_ptr(), 0, pho.data_ptr(), wav.data_ptr(), w16.data_ptr(), ld, iterations=3,
                                     flags=ffi.IN_DEVICE | ffi.OUT_DEVICE)
    assert np.array_equal(wav.cpu().numpy()[0, :N], host[0]) and np.array_equal(w16.cpu().numpy()[0, :N], host16[0])
    assert np.all(wav.cpu().numpy()[0, N:] == 0) and np.all(w16.cpu().numpy()[0, N:] == 0)
    assert np.array_equal(pho.cpu().numpy()[0], fx["phase0"])


def test_degenerate_rows(gpu_engine, model):
    one = np.zeros((1, 80, 1), np.float32)
    f32, i16, ph = gpu_engine.griffin_lim_infer(model, gpu_engine.mel_from_numpy(one), seed=1, want_int16=True, want_phase=True)
    assert f32.shape == (1, 0) and i16.shape == (1, 0) and ph.shape == (1, 513, 0)
    # zero magnitudes (exp(-200) underflows in float32): every |S| is 0 from the first transform on — the (mag, 0) rule, no 0 / 0
    mel = np.full((2, 80, 9), -200.0, np.float32)
    mel[1, :, :3] = 1.0
    f32, i16, _ = gpu_engine.griffin_lim_infer(model, gpu_engine.mel_from_numpy(mel, frames=[9, 1]), seed=2, iterations=3, want_int16=True)
    assert np.all(f32 == 0) and np.all(i16 == 0)  # row 0 silent, row 1 a single frame: empty
    f32, _, _ = gpu_engine.griffin_lim_infer(model, gpu_engine.mel_from_numpy(mel), seed=2, iterations=3)
    assert np.isfinite(f32).all() and np.all(f32[0] == 0) and np.abs(f32[1]).max() > 0


def test_kernel_counts(gpu_engine, model):
    mel = gpu_engine.mel_from_numpy(golden_mel("ljspeech_high_short5"))
    gpu_engine.profile_reset()
    gpu_engine.griffin_lim_infer(model, mel, seed=3, iterations=60, want_int16=True)
    counts = gpu_engine.kernel_counts()
    assert counts["griffin_lim_iter_kernel"] == 60
    assert counts["griffin_lim_mag_kernel"] == 1 and counts["griffin_lim_init_kernel"] == 1
    assert counts["griffin_lim_out_kernel"] == 1 and counts["griffin_lim_int16_kernel"] == 1
    assert counts.get("stft_denoise_kernel", 0) == 0 and counts.get("overlap_add_kernel", 0) == 0
    assert all(v == 0 for k, v in counts.items() if not k.startswith("griffin_lim_"))
    gpu_engine.profile_reset()
    gpu_engine.griffin_lim_infer(model, mel, seed=3)  # the model's own count
    assert gpu_engine.kernel_counts()["griffin_lim_iter_kernel"] == 60
