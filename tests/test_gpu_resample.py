"""Resampling (csrc/resample.h) on the MI355X: the check functions of tests/test_emu_resample.py under the same rules — impulses
bit for bit, the device within 16 x the float32 restatement's own error and under the a-priori bound —, plus what only the device
has: device pointers, and a row long enough that n * down passes 2^31.  Every test prints what it measured."""
import numpy as np
import pytest

from larynx_amd import ffi
from tests import resample_np as R
from tests.test_emu_resample import (RATES, bits, check_direct_path, check_impulses, check_int16_input, check_int16_output,
                                     check_lengths, check_parity, check_ragged, check_refusals, check_schedule, check_sentence_path,
                                     check_sentence_path_griffin_lim,
                                     model, prototype, vocoder)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ratio", [(3, 2), (320, 441), (160, 441), (320, 147)])
def test_impulses_are_exact(gpu_engine, ratio):
    check_impulses(gpu_engine, *ratio)


def test_lengths_and_edges(gpu_engine):
    check_lengths(gpu_engine)


@pytest.mark.parametrize("n", (257, 700, 1500))
@pytest.mark.parametrize("rate", RATES)
def test_parity(gpu_engine, rate, n):
    check_parity(gpu_engine, rate, n)


@pytest.mark.parametrize("ratio", [(320, 441), (320, 147)])
def test_ragged_batch_rows_equal_their_batch1_calls(gpu_engine, ratio):
    check_ragged(gpu_engine, *ratio)


@pytest.mark.parametrize("ratio", [(160, 441), (320, 147)])
def test_int16_input_and_output(gpu_engine, ratio):
    check_int16_input(gpu_engine, *ratio)
    check_int16_output(gpu_engine, *ratio)


def test_schedule(gpu_engine):
    check_schedule(gpu_engine, 320, 441)


def test_refusals_and_unload(gpu_engine):
    check_refusals(gpu_engine)


def test_unstaged_path(gpu_engine):
    check_direct_path(gpu_engine)


def test_device_pointers(gpu_engine):
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE: torch tensors (float32 and int16 in, all three output forms, row strides past the
    rows' samples, outputs pre-filled) give the host call's bits and zero tails up to out_ld."""
    torch = pytest.importorskip("torch")
    up, down = 320, 441
    m = model(gpu_engine, up, down)
    samples = (700, 0, 257)
    batch = np.full((3, 768), 0.25, np.float32)
    for b, n in enumerate(samples):
        batch[b, :n] = R.tone_noise(n, 10 + b)
    i16 = np.round(batch * 32767).astype(np.int16)
    ld = R.out_length(700, up, down) + 21
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE
    for src in (batch, i16):
        host_f, host_sat, n_out = gpu_engine.resample(m, src, samples, want_int16=True)
        _, host_nrm, _ = gpu_engine.resample(m, src, samples, want_float=False, want_int16=True, normalize=True)
        dev = torch.from_numpy(src).cuda().contiguous()
        ptrs = (None, dev.data_ptr()) if src.dtype == np.int16 else (dev.data_ptr(), None)
        for mode, host_i, with_float in ((ffi.PCM_SATURATE, host_sat, True), (ffi.PCM_NORMALIZE, host_nrm, True), (ffi.PCM_NORMALIZE, host_nrm, False)):
            of = torch.full((3, ld), 7.0, dtype=torch.float32, device="cuda")
            oi = torch.full((3, ld), 7, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            got = gpu_engine.resample_raw(m, ptrs[0], ptrs[1], samples, 768, of.data_ptr() if with_float else None, oi.data_ptr(), ld, mode, flags)
            torch.cuda.synchronize()
            assert list(got) == list(n_out)
            f, i = of.cpu().numpy(), oi.cpu().numpy()
            w = host_f.shape[1]
            if with_float:
                assert np.array_equal(bits(f[:, :w]), bits(host_f)) and not f[:, w:].any()
            else:
                assert np.all(f == 7.0)
            assert np.array_equal(i[:, :w], host_i) and not i[:, w:].any()


def test_positions_past_2_to_31(gpu_engine):
    """The longest row the library takes (2^24 samples, int16) at 160 / 441: n * down reaches 2.7e9.  The outputs around the
    point where n * down passes 2^31 and at the row's end against the float64 definition, under the a-priori bound."""
    up, down = 160, 441
    taps, H = prototype(up, down)
    t64 = taps.astype(np.float64)
    N = 1 << 24
    x = np.random.default_rng(5).integers(-32768, 32768, N, dtype=np.int16)
    y, _, n_out = gpu_engine.resample(model(gpu_engine, up, down), x)
    total = R.out_length(N, up, down)
    assert n_out[0] == len(y) == total and (total - 1) * down > 2 ** 31
    cross = 2 ** 31 // down
    worst = 0.0
    for n in list(range(cross - 300, cross + 300)) + list(range(total - 300, total)):
        c = n * down + H
        i = np.arange(max(0, -((2 * H - c) // up)), min(N - 1, c // up) + 1)
        ref = float(np.dot(x[i].astype(np.float64) / 32768.0, t64[c - i * up]))
        worst = max(worst, abs(float(y[n]) - ref))
    bound = R.a_priori_bound(taps, up, 1.0)
    print(f"2^24 samples -> {total} outputs: max error {worst:.2e} over 900 outputs around n * down = 2^31 and at the end (bound {bound:.2e})")
    assert np.abs(y[cross - 300: cross + 300]).max() > 0.05 and worst <= bound


def test_sentence_path(gpu_engine):
    from tests.test_emu_analysis import tiny_voice

    tts = tiny_voice()
    check_sentence_path(tts, vocoder())
    check_sentence_path_griffin_lim(tts)
