"""The YIN pitch tracker (csrc/pitch.h) on the MI355X: the check functions of tests/test_emu_pitch.py under the same rules — exact
periods bit for bit; the designed signal and two golden utterances against the float64 oracle on the decided frames, within 16 x
the float32 restatement's own error; edges, a ragged batch, int16 input and device pointers (torch tensors) bit for bit; every
limit refused; one launch per call under the kernel's name.  The largest input is 2.4 s of audio.  Every test prints what it
measured."""
import pytest

from tests.test_emu_pitch import (check_designed, check_device_pointers, check_edges, check_exact_periods, check_golden, check_int16_input,
                                  check_ragged_batch, check_refusals, check_schedule)
from tests.test_emu_resample import torch_alloc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def leave_no_counts(request):
    yield
    if "gpu_engine" in request.fixturenames:
        request.getfixturevalue("gpu_engine").profile_reset()


def test_exact_periods(gpu_engine):
    check_exact_periods(gpu_engine)


def test_designed_signal(gpu_engine):
    check_designed(gpu_engine)


@pytest.mark.parametrize("case", ("ljspeech_high_short5", "ljspeech_high_echo"))
def test_golden_utterances(gpu_engine, case):
    check_golden(gpu_engine, case)


def test_edges_and_silence(gpu_engine):
    check_edges(gpu_engine)


def test_ragged_batch(gpu_engine):
    check_ragged_batch(gpu_engine)


def test_int16_input(gpu_engine):
    check_int16_input(gpu_engine)


def test_device_pointers(gpu_engine):
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE with torch tensors: tests/test_emu_pitch.py's check on the device's own memory."""
    pytest.importorskip("torch")
    check_device_pointers(gpu_engine, torch_alloc)


def test_schedule_by_kernel_name(gpu_engine):
    check_schedule(gpu_engine)


def test_refusals_and_unload(gpu_engine):
    check_refusals(gpu_engine)
