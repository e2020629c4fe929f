"""Emulator: the ResBlock kernels compiled for a step's dilation (rb_group_dil_kernel, rbp_dil_group_kernel; option rb_dil) give
the bits of the run-time-dilation kernels — host dispatch and the compile-time offsets of rb_tile / rbp_phase, on small rows.
(The device tests, test_gpu_rb_dil.py, walk every channel count and length.)"""
import pytest

from tests import rb_dil_check as R


@pytest.mark.parametrize("channels, nb4, kernels", [(128, False, R.GROUP_KERNELS), (128, True, R.GROUP_KERNELS), (64, False, R.PAIR_KERNELS),
                                                      (32, False, R.PAIR_KERNELS)])
def test_fixed_dilation_kernels_equal_the_runtime_dilation_kernels(emu_engine, monkeypatch, channels, nb4, kernels):
    R.set_knobs(monkeypatch, nb4)
    v = R.load_one_stage(emu_engine, channels)
    try:
        for frames in ([65], list(R.RAGGED)) if not nb4 else ([129],):
            R.compare(emu_engine, v, frames, kernels)
            if nb4:
                assert emu_engine.kernel_counts().get("rb_group_kernel.nb4", 0) == 6
    finally:
        emu_engine.unload(v)


def test_other_dilations_take_the_runtime_kernel(emu_engine, monkeypatch):
    """A model whose steps have a dilation without an instantiation (2) or members that differ still runs — on the kernels that
    read the dilation from their arguments — and option rb_dil changes nothing for it."""
    from larynx_amd import hparams as HP
    from larynx_amd import synthetic

    R.set_knobs(monkeypatch, False)
    hp = HP.HifiGanHParams(upsample_rates=(1,), upsample_kernel_sizes=(3,), upsample_initial_channel=256,
                           resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 2), (1, 2), (3, 2)), num_mels=R.NUM_MELS)
    v = emu_engine.load_hifigan(hp, synthetic.make_hifigan_state_dict(hp, seed=77))
    try:
        R.compare(emu_engine, v, [70], R.GROUP_KERNELS, steps=2)
    finally:
        emu_engine.unload(v)
