"""The pitch shifter (csrc/shift.h) on the MI355X: the check functions of tests/test_emu_shift.py under the same rules — exact
periods without tolerance; positions and the overlap-add bit for bit against numpy; the resampled row within 16 x the float32
restatement's own error; the pitch of the delivered row read back with the float64 YIN oracle; edges, a ragged batch, int16
input and device pointers (torch tensors) bit for bit; the launches by kernel name; every limit refused; the Python object.  The
largest input is 2.4 s of audio.  Every test prints what it measured."""
import pytest

from tests.test_emu_pitch import designed
from tests.test_emu_resample import torch_alloc
from tests.test_emu_shift import (PITCH_RATIOS, check_batch_forms, check_chain, check_exact_periods, check_identity_and_edges,
                                  check_injected_positions, check_positions, check_refusals, check_schedule, check_shifter_object)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def leave_no_counts(request):
    yield
    if "gpu_engine" in request.fixturenames:
        request.getfixturevalue("gpu_engine").profile_reset()


def test_exact_periods(gpu_engine):
    check_exact_periods(gpu_engine)


def test_positions_bit_for_bit(gpu_engine):
    check_positions(gpu_engine)


def test_injected_positions(gpu_engine):
    check_injected_positions(gpu_engine)


@pytest.mark.parametrize("ratio", PITCH_RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
def test_chain_and_claim(gpu_engine, ratio):
    assert designed().size == 52920
    check_chain(gpu_engine, ratio)


def test_identity_and_edges(gpu_engine):
    check_identity_and_edges(gpu_engine)


def test_batch_int16_and_device_pointers(gpu_engine):
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE with torch tensors: tests/test_emu_shift.py's check on the device's own memory."""
    pytest.importorskip("torch")
    check_batch_forms(gpu_engine, torch_alloc)


def test_schedule_by_kernel_name(gpu_engine):
    check_schedule(gpu_engine)


def test_refusals_and_unload(gpu_engine):
    check_refusals(gpu_engine)


def test_shifter_object(gpu_engine):
    check_shifter_object(gpu_engine)
