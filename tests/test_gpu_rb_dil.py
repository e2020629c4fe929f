"""Device: every ResBlock kernel compiled for a dilation (rb_group_dil_kernel<11, 7, 3, NB, 1 / 3 / 5>, rbp_dil_group_kernel<11, 7, 3,
CB, 1 / 3 / 5>) against the kernel that reads the dilation from its arguments, every output word equal.  One inference of a
one-stage vocoder (rb_dil_check.py) runs k = 3 / 7 / 11 x d = 1 / 3 / 5 (conv1) and d = 1 (conv2) at one channel count."""
import pytest

from tests import rb_dil_check as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vocoders(gpu_engine):
    loaded = {c: R.load_one_stage(gpu_engine, c) for c in (256, 128, 64, 32)}
    yield loaded
    for v in loaded.values():
        gpu_engine.unload(v)


@pytest.mark.parametrize("nb4", [False, True], ids=["nb2", "nb4"])
@pytest.mark.parametrize("channels", [128, 256])
def test_group_kernels_per_dilation_equal_the_runtime_kernel(gpu_engine, vocoders, monkeypatch, channels, nb4):
    R.set_knobs(monkeypatch, nb4)
    for frames in R.LENGTHS:
        R.compare(gpu_engine, vocoders[channels], [frames], R.GROUP_KERNELS)
        assert gpu_engine.kernel_counts().get("rb_group_kernel.nb4", 0) == (6 if nb4 else 0), frames
    if not nb4:  # a batch of rows runs the 64-column tiles (run_group)
        R.compare(gpu_engine, vocoders[channels], R.RAGGED, R.GROUP_KERNELS)


@pytest.mark.parametrize("channels", [64, 32])
def test_pair_kernels_per_dilation_equal_the_runtime_kernel(gpu_engine, vocoders, monkeypatch, channels):
    R.set_knobs(monkeypatch, False)
    for frames in R.LENGTHS:
        R.compare(gpu_engine, vocoders[channels], [frames], R.PAIR_KERNELS)
    R.compare(gpu_engine, vocoders[channels], R.RAGGED, R.PAIR_KERNELS)
