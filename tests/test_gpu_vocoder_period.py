"""A constant mel gives a hop-periodic waveform (tests/workload_check.py: check_hop_periodic) on the device: the shipped vocoders in
every precision, at the lengths around the launch-rule switches, under the schedule options and with the denoiser.  Samples t and
t + hop of the interior are compared for equality: no oracle, no golden, no tolerance — a case is a handful of vocoder calls and
one array compare per row.  The emulator twin is tests/test_emu_vocoder_period.py."""
import time

import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from tests import workload_check as W
from tests.test_emu_vocoder_period import BLIND, PRECISIONS, TILE_CLASS

pytestmark = pytest.mark.gpu

# 'high' changes kernels at F = 472 (the 64-channel stage's pairs move to the 4-wave tile), 492 (the 32-channel stage's) and 511
# (the 128-channel stage's 128-row tile) — tests/test_gpu_config3.py: 471 | 472 | 492 | 511 puts one length on each side of each
# switch.  Plus the shortest length with three stage-0 tiles inside the interior (W.short_frames) and 1100.
SWITCHES = (471, 472, 492, 511)
LONG = 1100
# the ragged batch of 8: the lengths above and two more, unsorted
RAGGED = (492, 1100, 471, 300, 511, 200, 472)

# kernels that must have run inside a periodic check, per vocoder and precision
NEED = {
    ("high", "f32"): ("rb_group_kernel", "rb_group_kernel.snake", "conv_group_kernel", "rb_pair_group_kernel", "pair_group_kernel"),
    ("high", "bf16x3"): ("conv_bf16_group_kernel", "pair_bf16_group_kernel"),
    ("high", "bf16"): ("conv_bf16_group_kernel", "pair_bf16_group_kernel"),
    ("high", "f16"): ("conv_f16_group_kernel", "pair_f16_group_kernel"),
    ("medium", "f32"): ("mrf_small_kernel", "mrf8_kernel"),
    ("medium", "bf16x3"): ("pair_bf16_group_kernel", "mrf_small_kernel", "mrf8_kernel"),
    ("medium", "bf16"): ("pair_bf16_group_kernel", "mrf_small_kernel", "mrf8_kernel"),
    ("medium", "f16"): ("pair_f16_group_kernel",),
    ("low", "f32"): ("conv_group_kernel",),
    ("low", "bf16x3"): ("conv_bf16_group_kernel",),
    ("low", "bf16"): ("conv_bf16_group_kernel",),
    ("low", "f16"): ("conv_f16_group_kernel",),
}

_models = {}


def _model(eng, quality):
    vhp = HP.VOCODER_QUALITY[quality]
    if quality not in _models:
        _models[quality] = eng.load_hifigan(vhp, synthetic.make_hifigan_state_dict(vhp, seed=1234))
    return vhp, _models[quality]


def _report(label, ran, need):
    print(f"{label}: ran {sorted(ran)}")
    for k in need:
        assert k in ran, (label, k, sorted(ran))


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("quality", ["high", "medium", "low"])
def test_constant_mel_is_hop_periodic(gpu_engine, quality, prec):
    """Six lone calls (the short length, one on each side of each launch-rule switch, 1100) and one ragged batch of 8."""
    eng = gpu_engine
    vhp, v = _model(eng, quality)
    blind = W.blind_tiles(vhp, TILE_CLASS[prec])
    print(f"{quality} {prec}: seams this check cannot see (tile width divides the hop): {blind}")
    assert blind == BLIND[(quality, TILE_CLASS[prec])]
    t = time.perf_counter()
    try:
        eng.set_precision(v, PRECISIONS[prec])
    except ffi.Mi355ttsError as e:
        print(f"{quality} {prec}: skipped, the library refuses the mode: {e}")
        return
    ran = set()
    try:
        short = W.short_frames(vhp, TILE_CLASS[prec])
        Fs = (short,) + SWITCHES + (LONG,)
        print(f"{quality} {prec}: lengths {Fs}, ragged batch {(short,) + RAGGED}")
        for F in Fs:
            sig = W.check_hop_periodic(eng, v, vhp, F, label=f"{quality} {prec}")
            print(f"{quality} {prec} F={F}: {sorted(sig)}")
            ran |= sig
        ran |= W.check_hop_periodic(eng, v, vhp, 0, rows=(short,) + RAGGED, label=f"{quality} {prec}")
    finally:
        eng.set_precision(v, ffi.PRECISION_F32)
    print(f"{quality} {prec}: {time.perf_counter() - t:.2f} s")
    _report(f"{quality} {prec}", ran, NEED[(quality, prec)])


def test_128_column_resblock_tiles_keep_the_period(gpu_engine, monkeypatch):
    """`rb_group_kernel<11, 7, 3, 4>` (128-column tiles: 512 samples at the 128-channel stage, two seams per three periods) runs only
    while another call is in flight; MI355TTS_RB_NB4_MIN_TILES = 1 gives it to a lone call."""
    vhp, v = _model(gpu_engine, "high")
    monkeypatch.setenv("MI355TTS_RB_NB4_MIN_TILES", "1")
    ran = set()
    for F in (511, LONG):
        ran |= W.check_hop_periodic(gpu_engine, v, vhp, F, label="high f32 nb4")
    _report("high f32 nb4", ran, ("rb_group_kernel.nb4",))


# option, value, default, kernels that must run under it at F = 511 of 'high'
SCHEDULES = [
    ("serial_branches", 1, 0, ()),
    ("mrf_group", 0, 1, ("conv_mfma_kernel.m128",)),
    ("rb_pair", 0, 1, ("pair_group_kernel",)),
    ("rb_conv", 0, 1, ("conv_group_kernel",)),
    ("voc_out", 0, 1, ("rb_group_kernel",)),
    ("adaptive_schedule", 1, 0, ("rb_group_kernel",)),
]


@pytest.mark.parametrize("option", [s[0] for s in SCHEDULES])
def test_schedule_options_keep_the_period(gpu_engine, option):
    _, value, default, need = next(s for s in SCHEDULES if s[0] == option)
    vhp, v = _model(gpu_engine, "high")
    gpu_engine.set_option(option, value)
    try:
        ran = W.check_hop_periodic(gpu_engine, v, vhp, 511, label=f"high f32 {option}={value}")
    finally:
        gpu_engine.set_option(option, default)
    _report(f"high f32 {option}={value}", ran, need)
    if option == "voc_out":
        assert not (ran & {"post_conv_kernel", "wave_out_kernel"}), sorted(ran)


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_denoised_waveform_keeps_the_period(gpu_engine, prec):
    """The denoiser's STFT hop is the vocoders' hop: the same comparison, with one STFT window and hop more of reach."""
    vhp, v = _model(gpu_engine, "medium")
    try:
        assert gpu_engine.set_precision(v, PRECISIONS[prec]) == 0
        ran = W.check_hop_periodic(gpu_engine, v, vhp, 472, denoise=0.01, label=f"medium {prec} denoised")
    finally:
        gpu_engine.set_precision(v, ffi.PRECISION_F32)
    _report(f"medium {prec} denoised", ran, NEED[("medium", prec)])
