"""Loudness (csrc/loudness.h) on the MI355X: the check functions of tests/test_emu_loudness.py under the same rules — every
K-weighted sample and the integrated value within 16 x the float32 restatement's own error of the float64 oracle, seams,
linearity, delivery and batch rows bit for bit —, the launches by kernel name, and what only the device has: device pointers.
Every test prints what it measured."""
import numpy as np
import pytest

from larynx_amd import ffi
from tests.test_emu_loudness import (BLOCK, CEILING, LONG, RAGGED, bits, check_calibration, check_gain, check_gating, check_int16_input,
                                     check_linearity, check_refusals, check_row_lengths, check_schedule, check_seams, check_sentence_path,
                                     meter, row)

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
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE: torch tensors (float32 and int16 in, both delivered forms and the weighted rows
    out, row strides past the rows' samples, outputs pre-filled) give the host call's bits and zero tails up to the strides."""
    torch = pytest.importorskip("torch")
    m = meter(gpu_engine).model_id
    batch = np.full((len(RAGGED), LONG + 40), 0.25, np.float32)
    for b, n in enumerate(RAGGED):
        batch[b, :n] = row(n)
    i16 = np.round(batch * 32767).astype(np.int16)
    in_ld, out_ld = batch.shape[1], LONG + 61
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE
    for src in (batch, i16):
        host = gpu_engine.loudness(m, src, RAGGED, target=-20.0, ceiling=CEILING, want_float=True, want_int16=True, want_weighted=True)
        dev = torch.from_numpy(src).cuda().contiguous()
        ptrs = (None, dev.data_ptr()) if src.dtype == np.int16 else (dev.data_ptr(), None)
        of = torch.full((len(RAGGED), out_ld), 7.0, dtype=torch.float32, device="cuda")
        oi = torch.full((len(RAGGED), out_ld), 7, dtype=torch.int16, device="cuda")
        ow = torch.full((len(RAGGED), in_ld), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        lufs, gain, peak = gpu_engine.loudness_raw(m, ptrs[0], ptrs[1], RAGGED, in_ld, -20.0, CEILING, 30.0, of.data_ptr(), oi.data_ptr(), out_ld,
                                                   ow.data_ptr(), flags)
        torch.cuda.synchronize()
        f, i, w = of.cpu().numpy(), oi.cpu().numpy(), ow.cpu().numpy()
        for got, k in ((lufs, "lufs"), (gain, "gain"), (peak, "peak")):
            assert np.array_equal(bits(got), bits(host[k])), k
        assert np.array_equal(bits(f[:, :in_ld]), bits(host["f32"])) and not f[:, in_ld:].any()
        assert np.array_equal(i[:, :in_ld], host["i16"]) and not i[:, in_ld:].any()
        assert np.array_equal(bits(w), bits(host["weighted"]))
        for b, n in enumerate(RAGGED):
            assert not f[b, n:].any() and not i[b, n:].any() and not w[b, n:].any()
        # measuring only, from device memory
        lufs2, gain2, _ = gpu_engine.loudness_raw(m, ptrs[0], ptrs[1], RAGGED, in_ld, float("nan"), 1.0, 30.0, flags=ffi.IN_DEVICE)
        assert np.array_equal(bits(lufs2), bits(lufs)) and np.all(gain2 == 1.0)


def test_sentence_path(gpu_engine):
    from tests.test_emu_analysis import tiny_voice
    from tests.test_emu_resample import vocoder

    check_sentence_path(tiny_voice(), vocoder())
