"""Shared by test_emu_rb_dil.py and test_gpu_rb_dil.py: a one-stage HiFi-GAN per channel count (upsampling rate 1, so a mel of
F frames gives the ResBlock convs rows of exactly F columns).  Its three ResBlock steps (the three MRF chains of a step are ONE
launch: k = 3 / 7 / 11 side by side, d = 1 / 3 / 5 step by step) are the grouped launches of rb_conv.h (128 / 256 channels) or
rb_pair.h (64 / 32 channels).  Every inference runs once on the kernels compiled for the step's dilation (option rb_dil = 1, the
default) and once on the run-time-dilation kernels (rb_dil = 0): every output word must be equal."""
import numpy as np

from larynx_amd import hparams as HP
from larynx_amd import synthetic

# columns of a row: a row shorter than one halo, a last partial tile, exactly one tile, a tile + 1, three 64-column tiles + 5
# (first tile with left padding, interior tiles, partial last tile), two 128-column tiles + 1 (the NB = 4 edge)
LENGTHS = (1, 63, 64, 65, 64 * 3 + 5, 128 * 2 + 1)
RAGGED = (5, 129, 64)
NUM_MELS = 16

GROUP_KERNELS = ("rb_group_kernel", "rb_group_kernel.snake", "rb_group_kernel.nb4")
PAIR_KERNELS = ("rb_pair_group_kernel",)


def one_stage_hparams(channels):
    return HP.HifiGanHParams(upsample_rates=(1,), upsample_kernel_sizes=(3,), upsample_initial_channel=2 * channels,
                             resblock_kernel_sizes=(3, 7, 11), resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)),
                             num_mels=NUM_MELS)


def load_one_stage(engine, channels):
    hp = one_stage_hparams(channels)
    return engine.load_hifigan(hp, synthetic.make_hifigan_state_dict(hp, seed=400 + channels))


def set_knobs(monkeypatch, nb4):
    """Every launch of these small shapes on the tiles the headline runs: the 128-row tile and the 4-wave pair from one
    tile up, 128-column tiles (NB = 4) always or never."""
    monkeypatch.setenv("MI355TTS_M128_MIN_TILES", "1")
    monkeypatch.setenv("MI355TTS_RB_PAIR_MIN_TILES", "1")
    monkeypatch.setenv("MI355TTS_RB_NB4_MIN_TILES", "1" if nb4 else "0")


def compare(engine, vocoder, frames, expect_kernels, steps=3):
    """One inference per setting of rb_dil on rows of `frames` columns; returns the waveform after the asserts."""
    frames = list(frames)
    rng = np.random.default_rng(1000 + sum(frames))
    mel = (0.5 + 0.1 * rng.standard_normal((len(frames), NUM_MELS, max(frames)))).astype(np.float32)
    mb = engine.mel_from_numpy(mel, np.array(frames, np.int32))
    engine.profile_reset()
    fixed, _ = engine.hifigan_infer(vocoder, mb)
    names = engine.kernel_counts()
    # conv1 and conv2 of a step are two grouped launches on the 128-row tile, one fused launch on the pair tile
    want = steps if expect_kernels is PAIR_KERNELS else 2 * steps
    assert sum(names.get(k, 0) for k in expect_kernels) == want, (frames, names)
    engine.set_option("rb_dil", 0)
    try:
        engine.profile_reset()
        runtime, _ = engine.hifigan_infer(vocoder, mb)
        names0 = engine.kernel_counts()
    finally:
        engine.set_option("rb_dil", 1)
    assert {k: names0.get(k, 0) for k in expect_kernels} == {k: names.get(k, 0) for k in expect_kernels}, (names, names0)
    fixed, runtime = np.asarray(fixed), np.asarray(runtime)
    assert fixed.shape == runtime.shape and fixed.tobytes() == runtime.tobytes(), (frames, np.abs(fixed - runtime).max())
    assert np.isfinite(fixed).all() and np.abs(fixed).max() > 1e-4, frames
    return fixed
