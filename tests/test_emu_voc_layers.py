"""Every launch of the vocoder's reduced-precision schedules against a float64 reference computed from that launch's own input
plane (tests/workload_check.py: check_layers, tests/voc_layers_np.py), on the CPU emulator with the tiny geometries.  The bounds
are derived (the f32 sum's forward error, half an fp16 ulp) or calibrated on the reference alone (the flip share): an index slip
inside ONE layer — a wrong tap, column, slab or chain — leaves them at that layer.  The device twin is
tests/test_gpu_voc_layers.py."""
import time

import numpy as np
import pytest

from larynx_amd import hparams as HP
from larynx_amd import synthetic
from tests import workload_check as W
from tests.test_emu_f16 import CASES as F16_CASES

# the six geometries of tests/test_emu_f16.py (SLIM, MID and WIDE tiles, both grouped tap sets, the pair kernel at 16 / 8 / 64 / 128
# channels) and one with a 256-channel stage: steps above 128 channels take two grouped launches
WIDE_256 = HP.HifiGanHParams(upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=512, num_mels=16)
# fp16 refuses more than 64 channels into conv_post: the same 256-channel stage with one more upsampler behind it (256 / 128 / 64)
WIDE_256_F16 = HP.HifiGanHParams(upsample_rates=(2, 2, 2), upsample_kernel_sizes=(4, 4, 4), upsample_initial_channel=512, num_mels=16)
GEOMETRIES = dict(F16_CASES, stage_256=WIDE_256, stage_256_f16=WIDE_256_F16)
CASES = sorted(F16_CASES) + ["stage_256"]
F = 70
ROWS = {"lone": (F,), "ragged": (F, 9, F - 37)}
MRF_OFF = {"mrf_small": (0, 1)}  # the one-launch narrow stages write no plane of a single conv or pair (W.LAYER_BLIND_KERNELS)

# kernel names a case must show in some tap's `kernel` field: what every case of the mode shows, and what its geometry adds
# (together: conv_f16_kernel, conv_f16_group_kernel, pair_f16_group_kernel, post_f16_kernel, pack_octets_kernel; conv_bf16_kernel,
# conv_bf16_group_kernel, pair_bf16_group_kernel, pair_bf16_kernel)
NEED_ALWAYS = {"f16": ("conv_f16_kernel", "post_f16_kernel", "pack_octets_kernel"), "bf16": ("conv_bf16_kernel",)}
NEED = {
    ("grouped_11_7_3", "f16"): ("pair_f16_group_kernel",),
    ("pairs_128_64", "f16"): ("pair_f16_group_kernel",),
    ("grouped_7_5_3", "f16"): ("conv_f16_group_kernel",),
    ("stage_256", "f16"): ("conv_f16_group_kernel", "pair_f16_group_kernel"),
    ("pairs_128_64", "bf16"): ("conv_bf16_group_kernel", "pair_bf16_group_kernel"),
    ("stage_256", "bf16"): ("conv_bf16_group_kernel",),
    ("wide_and_mid_tiles", "bf16"): ("pair_bf16_kernel",),
}
_models = {}


def _model(eng, geometry):
    hp = GEOMETRIES[geometry]
    if geometry not in _models:
        sd = synthetic.make_hifigan_state_dict(hp, seed=21)
        _models[geometry] = (sd, eng.load_hifigan(hp, sd))
    return (hp,) + _models[geometry]


def run_case(eng, model, precision, rows, options, label):
    hp, sd, v = model
    t = time.perf_counter()
    report, kernels = W.check_layers(eng, hp, precision, rows, options, v=v, sd=sd, label=label)
    print(f"{label} {precision} rows {rows}: {len(report)} layers, {time.perf_counter() - t:.2f} s")
    return report, kernels


@pytest.mark.parametrize("batch", sorted(ROWS))
@pytest.mark.parametrize("precision", ["f16", "bf16x3", "bf16"])
@pytest.mark.parametrize("geometry", CASES)
def test_every_layer_against_float64(emu_engine, geometry, precision, batch):
    model = _model(emu_engine, "stage_256_f16" if (geometry, precision) == ("stage_256", "f16") else geometry)
    report, kernels = run_case(emu_engine, model, precision, ROWS[batch], {} if precision == "f16" else MRF_OFF, geometry)
    mode = "f16" if precision == "f16" else "bf16"
    for k in NEED_ALWAYS[mode] + NEED.get((geometry, mode), ()):
        assert k in kernels, (geometry, precision, k, sorted(kernels))


@pytest.mark.parametrize("geometry", ["grouped_11_7_3", "pairs_128_64"])
def test_two_launch_form_of_the_fused_pairs(emu_engine, geometry):
    """"rb_pair" = 0: conv1's stored output is a tap of its own ("rb{i}.{j}.{d}.t") and conv2 is checked from it."""
    report, kernels = run_case(emu_engine, _model(emu_engine, geometry), "f16", ROWS["ragged"], {"rb_pair": (0, 1)}, geometry + " rb_pair=0")
    assert "pair_f16_group_kernel" not in kernels and any(r["name"].endswith(".t") for r in report)


def test_f32_call_has_its_taps(emu_engine):
    """The f32 schedule: the taps exist and `wav` is the returned rows (check_layers asserts both and stops there)."""
    report, kernels = run_case(emu_engine, _model(emu_engine, "pairs_128_64"), "f32", ROWS["ragged"], {}, "pairs_128_64")
    assert report == [] and "post_conv_kernel" in kernels


def _tap_names(eng, geometry, options):
    hp, sd, v = _model(eng, geometry)
    mb = eng.mel_from_numpy(W.layer_mel(hp.num_mels, [24, 9]), np.array([24, 9], np.int32))
    for k, (val, _) in options.items():
        eng.set_option(k, val)
    try:
        wav, taps = eng.hifigan_infer_taps(v, mb)
    finally:
        for k, (_, default) in options.items():
            eng.set_option(k, default)
        mb.free()
    return hp, taps


def test_stages_without_single_planes_are_named(emu_engine):
    """What stays outside the layer walk is visible in the tap list: the one-launch narrow stages leave their two partial sums
    ("stage{i}.sum{m}", counted under W.LAYER_BLIND_KERNELS), the serial form leaves the stage's average ("stage{i}") in place
    of its chains' last steps.  A reduced-precision walk over either is refused by check_layers."""
    hp, taps = _tap_names(emu_engine, "grouped_11_7_3", {})
    names = [t["name"] for t in taps]
    sums = [t for t in taps if ".sum" in t["name"]]
    assert [t["name"] for t in sums] == ["stage0.sum0", "stage0.sum1", "stage1.sum0", "stage1.sum1"], names
    assert {t["kernel"] for t in sums} == set(W.LAYER_BLIND_KERNELS) and not any(n.startswith("rb") for n in names)
    for t in sums:
        i = int(t["name"][5])
        mul = int(np.prod(hp.upsample_rates[: i + 1]))
        assert t["channels"] == hp.stage_channels(i) and t["len"] == [24 * mul, 9 * mul] and t["x"].shape == (2, t["channels"], t["ld"]), t["name"]
    hp, taps = _tap_names(emu_engine, "grouped_11_7_3", {"serial_branches": (1, 0), "mrf_small": (0, 1)})
    names = [t["name"] for t in taps]
    nd = len(hp.resblock_dilation_sizes[0])
    assert "stage0" in names and "stage1" in names and not any(n.endswith(f".{nd - 1}") for n in names if n.startswith("rb")), names
    assert names.index("stage0") < names.index("up1") and f"rb0.0.{nd - 2}" in names
    hp, sd, v = _model(emu_engine, "grouped_11_7_3")
    with pytest.raises(AssertionError, match="switch this fusion off"):
        W.check_layers(emu_engine, hp, "bf16", (24,), {}, v=v, sd=sd)


def test_forked_schedule_is_refused_with_a_reason(emu_engine):
    from larynx_amd import ffi

    hp, sd, v = _model(emu_engine, "pairs_128_64")
    mb = emu_engine.mel_from_numpy(W.layer_mel(hp.num_mels, [12]))
    emu_engine.set_option("mrf_group", 0)
    try:
        with pytest.raises(ffi.Mi355ttsError, match="side streams"):
            emu_engine.hifigan_infer_taps(v, mb)
    finally:
        emu_engine.set_option("mrf_group", 1)
        mb.free()
