"""Resampling (csrc/resample.h) on the MI355X: the check functions of tests/test_emu_resample.py under the same rules — impulses
bit for bit, the device within 16 x the float32 restatement's own error and under the a-priori bound, device pointers
as torch tensors —, plus what only the device has: a row long enough that n * down passes 2^31.  Every test prints what it measured."""
import numpy as np
import pytest

from tests import resample_np as R
from tests.test_emu_resample import (RATES, check_device_pointers, check_direct_path, check_impulses, check_int16_input,
                                     check_int16_output, check_lengths, check_parity, check_ragged, check_refusals, check_schedule,
                                     check_sentence_path, check_sentence_path_griffin_lim, model, prototype, torch_alloc, vocoder)

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
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE with torch tensors: tests/test_emu_resample.py's check on the device's own memory."""
    pytest.importorskip("torch")
    check_device_pointers(gpu_engine, torch_alloc)


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
