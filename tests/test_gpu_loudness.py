"""Loudness (csrc/loudness.h) on the MI355X: the check functions of tests/test_emu_loudness.py under the same rules — every
K-weighted sample and the integrated value within 16 x the float32 restatement's own error of the float64 oracle, seams,
linearity, delivery and batch rows bit for bit —, the launches by kernel name, and device pointers as torch tensors.
Every test prints what it measured."""
import pytest

from tests.test_emu_loudness import (BLOCK, LONG, check_calibration, check_device_pointers, check_gain, check_gating,
                                     check_int16_input, check_linearity, check_refusals, check_row_lengths, check_schedule, check_seams,
                                     check_sentence_path, meter, row)
from tests.test_emu_resample import torch_alloc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def leave_no_counts(request):
    yield
    if "gpu_engine" in request.fixturenames:
        request.getfixturevalue("gpu_engine").profile_reset()


def test_calibration_tone(gpu_engine):
    check_calibration(gpu_engine)


def test_row_lengths_and_ragged_batch(gpu_engine):
    check_row_lengths(gpu_engine)


def test_seams(gpu_engine):
    check_seams(gpu_engine)


def test_linearity_is_bit_exact(gpu_engine):
    check_linearity(gpu_engine)


def test_gating(gpu_engine):
    check_gating(gpu_engine)


def test_gain_and_delivery(gpu_engine):
    check_gain(gpu_engine)


def test_int16_input(gpu_engine):
    check_int16_input(gpu_engine)


def test_schedule_by_kernel_name(gpu_engine):
    """The six kernels run under their names, five launches to measure and a sixth to deliver, for N = block and the long row."""
    check_schedule(gpu_engine)
    gpu_engine.profile_reset()
    m = meter(gpu_engine)
    for n in (BLOCK, LONG):
        gpu_engine.loudness(m.model_id, row(n), target=-16.0, want_int16=True)
    counts = {k: v for k, v in gpu_engine.kernel_counts().items() if v}
    print(counts)
    assert counts == {f"loudness_{k}_kernel": 2 for k in ("chunk", "carry", "weight", "segment", "gate", "apply")}


def test_refusals_and_unload(gpu_engine):
    check_refusals(gpu_engine)


def test_device_pointers(gpu_engine):
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE with torch tensors: tests/test_emu_loudness.py's check on the device's own memory."""
    pytest.importorskip("torch")
    check_device_pointers(gpu_engine, torch_alloc)


def test_sentence_path(gpu_engine):
    from tests.test_emu_analysis import tiny_voice
    from tests.test_emu_resample import vocoder

    check_sentence_path(tiny_voice(), vocoder())
