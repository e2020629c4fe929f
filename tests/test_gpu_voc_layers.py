"""Every launch of the shipped vocoders' reduced-precision schedules against a float64 reference computed from that launch's own
input plane (tests/workload_check.py: check_layers, tests/voc_layers_np.py), on the device.  This bounds what the hop-periodicity
check cannot see (W.blind_tiles: the fp16 HPOST_TW and 256-column conv tile, the bf16 POST_TW and 128-column tile of the last
stage, and any error all tiles share).  The emulator twin is tests/test_emu_voc_layers.py.

The frame count is the smallest that puts two interior seams of every tile of W.vocoder_tiles inside a row, with a ragged last
tile wherever a frame count can make one (W.layer_frames): 33 for 'high' and 'low', 64 / 65 for 'medium'.  conv_pre's and the
first upsampler's tiles (not in vocoder_tiles) have no seam inside a row at these lengths: one longer call on 'low' compares
those two launches alone (test_pre_and_first_upsampler_seams)."""
import time

import pytest

from larynx_amd import hparams as HP
from larynx_amd import synthetic
from tests import workload_check as W
from tests.test_emu_vocoder_period import TILE_CLASS

pytestmark = pytest.mark.gpu

FRAMES = {("high", "f16"): 33, ("high", "bf16"): 33, ("medium", "f16"): 64, ("medium", "bf16"): 65, ("low", "f16"): 33, ("low", "bf16"): 33}
MRF_OFF = {"mrf_small": (0, 1)}  # the one-launch narrow stages write no plane of a single conv or pair (W.LAYER_BLIND_KERNELS)
# NOTES' "Kernels seen inside a periodic check" for the three reduced modes: each must be some tap's `kernel`
NEED = {
    ("high", "f16"): ("conv_f16_group_kernel", "pair_f16_group_kernel", "conv_f16_kernel", "post_f16_kernel", "pack_octets_kernel"),
    ("high", "bf16x3"): ("conv_bf16_group_kernel", "pair_bf16_group_kernel", "conv_bf16_kernel"),
    ("high", "bf16"): ("conv_bf16_group_kernel", "pair_bf16_group_kernel", "conv_bf16_kernel"),
    ("medium", "f16"): ("pair_f16_group_kernel",),
    ("medium", "bf16x3"): ("pair_bf16_group_kernel",),
    ("medium", "bf16"): ("pair_bf16_group_kernel",),
    ("low", "f16"): ("conv_f16_group_kernel",),
    ("low", "bf16x3"): ("conv_bf16_group_kernel",),
    ("low", "bf16"): ("conv_bf16_group_kernel",),
}
_models = {}


def _model(eng, quality):
    vhp = HP.VOCODER_QUALITY[quality]
    if quality not in _models:
        sd = synthetic.make_hifigan_state_dict(vhp, seed=1234)
        _models[quality] = (sd, eng.load_hifigan(vhp, sd))
    return (vhp,) + _models[quality]


@pytest.mark.parametrize("batch", ["lone", "ragged"])
@pytest.mark.parametrize("precision", ["f16", "bf16x3", "bf16"])
@pytest.mark.parametrize("quality", ["high", "medium", "low"])
def test_every_layer_against_float64(gpu_engine, quality, precision, batch):
    vhp, sd, v = _model(gpu_engine, quality)
    tile_class = TILE_CLASS[precision]
    F = W.layer_frames(vhp, tile_class)
    assert F == FRAMES[(quality, tile_class)], (quality, precision, F)
    rows = (F,) if batch == "lone" else (F, 9, max(F - 37, 5))
    t = time.perf_counter()
    report, kernels = W.check_layers(gpu_engine, vhp, precision, rows, {} if precision == "f16" else MRF_OFF, v=v, sd=sd, label=quality)
    print(f"{quality} {precision} rows {rows}: {len(report)} layers, {time.perf_counter() - t:.2f} s")
    for k in NEED[(quality, precision)]:
        assert k in kernels, (quality, precision, k, sorted(kernels))


def test_f32_call_has_its_taps(gpu_engine):
    vhp, sd, v = _model(gpu_engine, "medium")
    report, kernels = W.check_layers(gpu_engine, vhp, "f32", (64, 9, 27), {}, v=v, sd=sd, label="medium")
    assert report == [] and "post_conv_kernel" in kernels


@pytest.mark.parametrize("precision", ["f16", "bf16x3", "bf16"])
def test_pre_and_first_upsampler_seams(gpu_engine, precision):
    """conv_pre and the first upsampler run along the mel's frames: their widest tile is 128 columns (256 for the f32 conv_pre of
    the bf16 modes), so F = 2 * width + 5 puts two interior seams and a ragged last tile of both inside the row.  'low', one
    row: the planes of one call at this length stay under the seam's 256 MB.  Only these two launches are compared with float64."""
    vhp, sd, v = _model(gpu_engine, "low")
    F = 2 * (128 if precision == "f16" else 256) + 5
    t = time.perf_counter()
    report, kernels = W.check_layers(gpu_engine, vhp, precision, (F,), {} if precision == "f16" else MRF_OFF, v=v, sd=sd, label="low long",
                                     only=("pre", "up0"))
    print(f"low {precision} F={F}, pre and up0 alone: {time.perf_counter() - t:.2f} s")
    assert [r["name"] for r in report] == ["pre", "up0"]
