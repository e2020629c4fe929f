"""A constant mel gives a hop-periodic waveform (tests/workload_check.py: check_hop_periodic), on the CPU emulator: the vocoder's
bound-free seam check in every precision, schedule and forced tile shape the tiny geometries reach.  Samples t and t + hop of the
interior are the same arithmetic whichever tile computes them, so they are compared for equality — no oracle, no tolerance.  The
device twin is tests/test_gpu_vocoder_period.py."""
import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from tests import workload_check as W

GEOMETRIES = {
    "tiny": HP.TINY_HIFIGAN,            # ResBlock1, two chains, 16 / 8 channels
    "rb2": HP.TINY_HIFIGAN_RB2,         # ResBlock2, hop 16
    "pair": HP.TINY_HIFIGAN_PAIR,       # 64- and 32-channel stages: the fused pairs
    "narrow": HP.TINY_HIFIGAN_NARROW,   # the shipped chains on 16 / 8 channels: the one-launch MRF stages, the fp16 pairs
}
# 128- and 64-channel stages with the shipped tap set (tests/test_emu_host_features.py): the grouped 128-row launches
WIDE = HP.HifiGanHParams(upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=256,
                         resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 5), (1, 3), (1, 5)), num_mels=16)
PRECISIONS = {"f32": ffi.PRECISION_F32, "bf16x3": ffi.PRECISION_BF16X3, "bf16": ffi.PRECISION_BF16, "f16": ffi.PRECISION_F16}
TILE_CLASS = {"f32": "f32", "bf16x3": "bf16", "bf16": "bf16", "f16": "f16"}  # workload_check.vocoder_tiles' precision per mode
# What the check cannot see in the shipped vocoders (workload_check.blind_tiles: the tile's width in samples divides the hop, so
# its seams fall on the same phase of every period), pinned: a tile change that moves a seam into this set fails here instead of
# passing unseen.  The last stage's 256-column tiles (one tile per period), and on the 128-channel stage of 'high' the 32- and
# 64-column f32 conv tiles (4 samples a column: 128 / 256 samples) — the f32 ones are bounded per sample against the oracle by
# the tile-edge sweep (tests/test_gpu_config3.py), the fp16 last-stage ones stay as open as they were.  No stage-0 tile, no pair
# tile (T - (K - 1) columns never divide a power of two), no 128-column tile of a wide stage.
BLIND = {
    ("high", "f32"): [("conv_mfma T_T=32", 1, 32), ("conv_mfma T_T=64", 1, 64), ("POST_TW", 3, 256)],
    ("high", "bf16"): [("POST_TW", 3, 256)],
    ("high", "f16"): [("HPOST_TW", 3, 256)],
    ("medium", "f32"): [("POST_TW", 3, 256), ("mrf_small T", 3, 256)],
    ("medium", "bf16"): [("POST_TW", 3, 256), ("mrf_small T", 3, 256)],
    ("medium", "f16"): [("HPOST_TW", 3, 256)],
    ("low", "f32"): [("conv_mfma T_T=32", 1, 32), ("conv_mfma T_T=64", 1, 64), ("conv_mfma T_T=32", 2, 32), ("conv_mfma T_T=64", 2, 64),
                     ("conv_mfma T_T=128", 2, 128), ("POST_TW", 2, 256), ("conv_mfma T_T=256", 2, 256)],
    ("low", "bf16"): [("conv_bf16 128 columns", 2, 128), ("POST_TW", 2, 256)],
    ("low", "f16"): [("HPOST_TW", 2, 256), ("f16 h_tile_dims", 2, 256)],
}
F = 300  # 1200 ... 4800 samples: every stage has several tiles of every width (32 ... 256 columns) inside the interior
RAGGED = [300, 131, 217]
F_WIDE, RAGGED_WIDE = 200, [200, 150]  # (128 channels cost the emulator ten times the tiny stages)

TAIL32 = {"post_conv_kernel", "wave_out_kernel"}
TAIL16 = {"conv_f16_kernel", "post_f16_kernel", "pack_octets_kernel", "wave_out_kernel"}
# the kernels a lone call of F frames must have run, per geometry and precision
NEED = {
    ("tiny", "f32"): TAIL32 | {"conv_mfma_kernel"},
    ("rb2", "f32"): TAIL32 | {"conv_mfma_kernel"},
    ("pair", "f32"): TAIL32 | {"conv_mfma_kernel", "resblock_pair_kernel"},
    ("narrow", "f32"): TAIL32 | {"conv_mfma_kernel", "mrf_small_kernel", "mrf8_kernel"},
    ("tiny", "bf16"): TAIL32 | {"conv_bf16_kernel"},
    ("rb2", "bf16"): TAIL32 | {"conv_bf16_kernel"},
    ("pair", "bf16"): TAIL32 | {"conv_bf16_kernel", "pair_bf16_kernel"},
    ("narrow", "bf16"): TAIL32 | {"conv_bf16_kernel", "mrf_small_kernel", "mrf8_kernel"},
    ("tiny", "f16"): TAIL16,
    ("rb2", "f16"): TAIL16,
    ("pair", "f16"): TAIL16,
    ("narrow", "f16"): TAIL16 | {"pair_f16_group_kernel"},
}

_models = {}


def _model(eng, name, hp=None):
    hp = hp or GEOMETRIES[name]
    if name not in _models:
        _models[name] = eng.load_hifigan(hp, synthetic.make_hifigan_state_dict(hp, seed=1234))
    return hp, _models[name]


def _need(sig, need, label):
    print(f"{label}: {sorted(sig)}")
    assert need <= sig, (label, sorted(need - sig), sorted(sig))


def test_reach_and_blind_set_of_the_geometries():
    """vocoder_reach from the hparams alone (the emulator showed the last differing sample 56 ... 193 from an end); the tiles
    whose seams the check cannot see: none at these hops, and for the shipped vocoders exactly the lists the device test pins."""
    assert [W.vocoder_reach(hp) for hp in GEOMETRIES.values()] == [72, 161, 144, 204]
    assert W.vocoder_reach(HP.HIFIGAN_HIGH) == 3552 == W.vocoder_reach(HP.HIFIGAN_MEDIUM) and W.vocoder_reach(HP.HIFIGAN_HIGH, True) == 3552 + 1280
    for name, hp in GEOMETRIES.items():
        for prec in ("f32", "bf16", "f16"):
            assert W.vocoder_tiles(hp, prec), (name, prec)
            assert W.blind_tiles(hp, prec) == [], (name, prec)
    for (quality, prec), want in BLIND.items():
        hp = HP.VOCODER_QUALITY[quality]
        got = W.blind_tiles(hp, prec)
        print(f"{quality} {prec}: blind {got}")
        assert got == want, (quality, prec, got)
        assert not [t for t in got if t[1] == 0 or "pair" in t[0]], (quality, prec, got)
        assert any("pair" in t[0] for t in W.vocoder_tiles(hp, prec)) == (hp.resblock == "1"), (quality, prec)  # (the pair tiles are listed)
    assert [W.short_frames(HP.HIFIGAN_HIGH, p) for p in ("f32", "bf16", "f16")] == [142, 78, 78]
    with pytest.raises(ValueError, match="fewer than 8 periods"):
        W.check_hop_periodic(None, 0, HP.HIFIGAN_HIGH, 35)  # 2 x 14 frames of reach + 7 periods: refused before any call


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_constant_mel_is_hop_periodic(emu_engine, name, prec):
    hp, v = _model(emu_engine, name)
    try:
        assert emu_engine.set_precision(v, PRECISIONS[prec]) == 0
        sig = W.check_hop_periodic(emu_engine, v, hp, F, label=f"{name} {prec}")
    finally:
        emu_engine.set_precision(v, ffi.PRECISION_F32)
    _need(sig, NEED[(name, "bf16" if prec == "bf16x3" else prec)], f"{name} {prec}")
    other = {"conv_f16_kernel", "pair_f16_group_kernel"} if prec != "f16" else {"conv_mfma_kernel", "conv_bf16_kernel", "post_conv_kernel"}
    assert not (sig & other), (name, prec, sorted(sig & other))


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_ragged_batch_is_hop_periodic_per_row(emu_engine, name):
    """Three rows of different lengths, each its own column: every row periodic over its own interior, its tail 0 — in f32, in
    split bf16 and in fp16 (the ragged grids deal a row its own tiles)."""
    hp, v = _model(emu_engine, name)
    try:
        for prec in ("f32", "bf16x3", "f16"):
            assert emu_engine.set_precision(v, PRECISIONS[prec]) == 0
            sig = W.check_hop_periodic(emu_engine, v, hp, 0, rows=RAGGED, label=f"{name} {prec} ragged")
            _need(sig, NEED[(name, "bf16" if prec == "bf16x3" else prec)], f"{name} {prec} ragged")
    finally:
        emu_engine.set_precision(v, ffi.PRECISION_F32)


# option, value, default, the geometry whose launches it moves, kernels that must (not) run under it
SCHEDULES = [
    ("serial_branches", 1, 0, "narrow", {"conv_mfma_kernel"}, {"mrf_small_kernel", "mrf8_kernel"}),
    ("mrf_group", 0, 1, "wide", {"conv_mfma_kernel.m128", "rb_pair_kernel"}, {"rb_group_kernel", "rb_group_kernel.snake", "pair_group_kernel"}),
    ("rb_pair", 0, 1, "wide", {"pair_group_kernel"}, {"rb_pair_group_kernel", "rb_pair_kernel"}),
    ("rb_conv", 0, 1, "wide", {"conv_group_kernel"}, {"rb_group_kernel", "rb_group_kernel.snake", "rb_conv_kernel"}),
    ("voc_out", 0, 1, "pair", {"conv_mfma_kernel", "resblock_pair_kernel"}, TAIL32),
    ("adaptive_schedule", 1, 0, "wide", set(), set()),
]


@pytest.mark.parametrize("option", [s[0] for s in SCHEDULES])
def test_schedule_options_keep_the_period(emu_engine, monkeypatch, option):
    """One run under each schedule option that moves launches between kernels (or between streams)."""
    _, value, default, name, need, absent = next(s for s in SCHEDULES if s[0] == option)
    if name == "wide":  # the thresholds of the 128-row tile and the 4-wave pair tile at emulator sizes
        monkeypatch.setenv("MI355TTS_M128_MIN_TILES", "1")
        monkeypatch.setenv("MI355TTS_RB_PAIR_MIN_TILES", "1")
    hp, v = _model(emu_engine, name, WIDE if name == "wide" else None)
    emu_engine.set_option(option, value)
    try:
        sig = W.check_hop_periodic(emu_engine, v, hp, F_WIDE if name == "wide" else F, label=f"{name} {option}={value}")
    finally:
        emu_engine.set_option(option, default)
    _need(sig, need, f"{name} {option}={value}")
    assert not (sig & absent), (option, sorted(sig & absent))


@pytest.mark.parametrize("shape", [0, 1, 2, 3])
def test_forced_tile_shapes_keep_the_period(emu_engine, monkeypatch, shape):
    """MI355TTS_FORCE_TILE_DYNAMIC pins conv_mfma's tile: 64, 128, 256 and 32 columns on every f32 conv of the four geometries."""
    monkeypatch.setenv("MI355TTS_FORCE_TILE_DYNAMIC", str(shape))
    for name in GEOMETRIES:
        hp, v = _model(emu_engine, name)
        sig = W.check_hop_periodic(emu_engine, v, hp, F, label=f"{name} tile shape {shape}")
        _need(sig, {"conv_mfma_kernel"}, f"{name} tile shape {shape}")


def test_grouped_128_row_tiles_keep_the_period(emu_engine, monkeypatch):
    """The grouped launches of a 128-channel stage: the continuous-stream tile in its 64-column form (dealt as a snake and in
    the plain order) and, through MI355TTS_RB_NB4_MIN_TILES, in its 128-column form; the 4-wave pair tile on the 64-channel
    stage; then the bf16 and fp16 grouped tiles of the same geometry."""
    monkeypatch.setenv("MI355TTS_M128_MIN_TILES", "1")
    monkeypatch.setenv("MI355TTS_RB_PAIR_MIN_TILES", "1")
    hp, v = _model(emu_engine, "wide", WIDE)
    monkeypatch.setenv("MI355TTS_GROUP_NCU", "8")  # 7 + 7 + 7 workgroups on "8 CUs": more than one round, all resident: the snake
    sig = W.check_hop_periodic(emu_engine, v, hp, F_WIDE, label="wide snake")
    _need(sig, {"rb_group_kernel.snake", "rb_pair_group_kernel", "rb_conv_kernel"}, "wide snake")
    monkeypatch.setenv("MI355TTS_GROUP_NCU", "4")
    sig = W.check_hop_periodic(emu_engine, v, hp, F_WIDE, label="wide plain order")
    _need(sig, {"rb_group_kernel", "rb_pair_group_kernel"}, "wide plain order")
    monkeypatch.setenv("MI355TTS_RB_NB4_MIN_TILES", "1")
    sig = W.check_hop_periodic(emu_engine, v, hp, F_WIDE, label="wide nb4")
    _need(sig, {"rb_group_kernel.nb4"}, "wide nb4")
    assert not (sig & {"rb_group_kernel", "rb_group_kernel.snake"}), sorted(sig)
    sig = W.check_hop_periodic(emu_engine, v, hp, 0, rows=RAGGED_WIDE, label="wide nb4 ragged")
    print("wide nb4 ragged:", sorted(sig))
    monkeypatch.delenv("MI355TTS_RB_NB4_MIN_TILES")
    try:
        for prec, need in (("bf16x3", {"conv_bf16_group_kernel", "pair_bf16_group_kernel"}), ("bf16", {"conv_bf16_group_kernel", "pair_bf16_group_kernel"}),
                           ("f16", {"pair_f16_group_kernel", "conv_f16_kernel"})):
            assert emu_engine.set_precision(v, PRECISIONS[prec]) == 0
            sig = W.check_hop_periodic(emu_engine, v, hp, F_WIDE, label=f"wide {prec}")
            _need(sig, need, f"wide {prec}")
    finally:
        emu_engine.set_precision(v, ffi.PRECISION_F32)


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_denoised_waveform_has_the_stft_period(emu_engine, prec):
    """With the denoiser the waveform goes through an STFT of hop 256: TINY_HIFIGAN_RB2 (hop 16) is periodic with period 256 —
    and, as a check of the check, not with period 16 any more."""
    hp, v = _model(emu_engine, "rb2")
    Fd = 320  # 2 x (161 + 1280) samples of reach and 8 periods of 256: from 310 frames
    try:
        assert emu_engine.set_precision(v, PRECISIONS[prec]) == 0
        with pytest.raises(ValueError, match="fewer than 8 periods"):
            W.check_hop_periodic(emu_engine, v, hp, 256, denoise=0.5, label=f"rb2 {prec} denoised")
        sig = W.check_hop_periodic(emu_engine, v, hp, Fd, denoise=0.5, label=f"rb2 {prec} denoised")
        _need(sig, NEED[("rb2", prec)], f"rb2 {prec} denoised")
        mb = emu_engine.mel_from_numpy(W.constant_mel(hp, [Fd]))
        wav, _ = emu_engine.hifigan_infer(v, mb, denoiser_strength=0.5)
        mb.free()
    finally:
        emu_engine.set_precision(v, ffi.PRECISION_F32)
    R = -(-W.vocoder_reach(hp, True) // hp.hop) * hp.hop
    n = Fd * hp.hop
    assert np.array_equal(wav[0, R : n - R - 256], wav[0, R + 256 : n - R])
    assert not np.array_equal(wav[0, R : n - R - hp.hop], wav[0, R + hp.hop : n - R])
