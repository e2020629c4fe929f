"""Every launch of the acoustic model against a float64 reference computed from the planes that launch read
(tests/workload_check.py: check_glow_layers, tests/glow_layers_np.py), on the device at the released shape (HP.LJSPEECH: H = 192,
2 heads, six encoder layers, twelve flow blocks of four WaveNet layers; the synthetic state dict of seed 1234, as the sweep uses).
About 150 launches per call, each judged on its own: nothing is amplified through the layers behind it and every bound is derived
(gate_fast's E alone is measured, against float64 on a grid of biases: glow_layers_np.E_GATE_FAST).
The end-to-end bars (5e-5 on the f32 mel, the reference's own .half() deviation in fp16: tests/test_gpu_glow_sweep.py) have a
hundred-fold and a thirty-fold slack; this file bounds what they and the bound-free seam check cannot see: an error every column
shares.  The emulator twin, where the float32 restatement of every launch kind passes the same bounds, is
tests/test_emu_glow_layers.py.

The lengths come from the tile table (W.GLOW_TILE_WIDTHS through W.glow_layer_lengths): at least three tiles of every listed
kind inside a row, the last one ragged.  Every case runs as a lone call and as one ragged three-row batch (full, 1, mid)."""
import dataclasses
import time

import pytest

from larynx_amd import hparams as HP
from larynx_amd import synthetic
from tests import workload_check as W
from tests.test_gpu_parity import models

pytestmark = pytest.mark.gpu

ATTENTION = ("attention_mfma_kernel", "attention_mfma_kernel.p768", "attention_kernel")
FUSE_OFF = {"glow_fuse": (0, 1)}
ENC_TILES = ("attention_mfma 32", "oproj_ln", "lin16")
DEC_TILES = ("gate16", "lin16", "glow_tail")
H32 = HP.GlowHParams(num_symbols=30, hidden_channels=32, filter_channels=32, filter_channels_dp=32, n_blocks_dec=2, n_layers_enc=2,
                     n_block_layers=4, mel_channels=8)  # tests/test_emu_glow_f16.py's geometry: the other wn_f16_kernel instantiation
SPLIT8 = dataclasses.replace(H32, n_layers_enc=1, n_block_layers=2, n_split=8)  # tests/test_emu_glow_coltile.py's: no fused InvConvNear
TINY_MULTI = dataclasses.replace(HP.TINY_GLOW, n_speakers=3, gin_channels=20)  # tests/test_multispeaker.py

# case -> (model, precision, axis, tile kinds, smallest length, options, kernels that must run, kernels that must not)
CASES = {
    "encoder-256": ("ljspeech", "f32", "P", ENC_TILES, 1, {}, (ATTENTION[0], "oproj_ln_kernel", "lin16_kernel", "lin16_kernel.ln"), ATTENTION[1:]),
    "encoder-p768": ("ljspeech", "f32", "P", ENC_TILES, 257, {}, (ATTENTION[1], "oproj_ln_kernel", "lin16_kernel.ln"), (ATTENTION[0], ATTENTION[2])),
    "encoder-valu": ("ljspeech", "f32", "P", ("attention ATT_ROWS",), 769, {}, (ATTENTION[2],), ATTENTION[:2]),
    "decoder-f32": ("ljspeech", "f32", "F2", DEC_TILES, 1, {}, ("gate16_kernel", "lin16_kernel", "glow_tail_kernel", "conv_mfma_kernel"), ("wn_f16_kernel",)),
    "decoder-f16": ("ljspeech", "f16", "F2", ("wn_f16",), 1, {}, ("wn_f16_kernel", "glow_tail_kernel"), ("gate16_kernel", "gate16_kernel.wide")),
    "decoder-f16-f32-length": ("ljspeech", "f16", "F2", DEC_TILES, 1, {}, ("wn_f16_kernel", "glow_tail_kernel"), ("gate16_kernel",)),
    # ("glow_fuse" = 0 also sends the plain convs back to the generic tile: conv_mfma_kernel's linear, gate-less and coupling epilogues)
    "fallback-encoder-256": ("ljspeech", "f32", "P", ENC_TILES, 1, FUSE_OFF, (ATTENTION[0], "conv_mfma_kernel"),
                             ("oproj_ln_kernel", "lin16_kernel", "lin16_kernel.ln", "glow_tail_kernel")),
    "fallback-decoder-f32": ("ljspeech", "f32", "F2", DEC_TILES, 1, FUSE_OFF, ("gate16_kernel", "conv_mfma_kernel"),
                             ("oproj_ln_kernel", "lin16_kernel", "lin16_kernel.ln", "glow_tail_kernel")),
    "narrow-f16": ("h32", "f16", "F2", ("wn_f16",), 1, {}, ("wn_f16_kernel", "glow_tail_kernel"), ("gate16_kernel",)),
    "multi-speaker": ("multi", "f32", "P", ("oproj_ln",), 1, {}, ("gate16_kernel", "glow_tail_kernel"), ()),
    # n_split = 8 has no fused mix: conv_mfma_kernel's coupling epilogue without it (`blk{b}.zc`), then invconv_actnorm_kernel
    "eight-way-split": ("split8", "f32", "P", ("attention_mfma 32", "oproj_ln"), 1, {}, ("conv_mfma_kernel",), ("glow_tail_kernel",)),
    "fallback-eight-way-split": ("split8", "f32", "P", ("attention_mfma 32", "oproj_ln"), 1, FUSE_OFF, ("conv_mfma_kernel",), ("glow_tail_kernel", "oproj_ln_kernel")),
}
WIDE = ("gate16_kernel.wide", "lin16_kernel.wide")
_models = {}


def _model(eng, which):
    if which == "ljspeech":
        (gsd, g), _ = models(eng, HP.LJSPEECH, HP.HIFIGAN_HIGH)  # synthetic state dict, seed 1234
        return HP.LJSPEECH, gsd, g
    hp, seed = {"h32": (H32, 70), "multi": (TINY_MULTI, 21), "split8": (SPLIT8, 72)}[which]
    if which not in _models:
        sd = synthetic.make_glow_state_dict(hp, seed=seed)
        _models[which] = (sd, eng.load_glow(hp, sd))
    return (hp,) + _models[which]


def test_every_named_kernel_is_some_case_s():
    """Every kernel name a GlowTTS call can be counted under is required by at least one case below."""
    need = set(WIDE) | {k for c in CASES.values() for k in c[6]}
    assert set(W.GLOW_NAMED_KERNELS) <= need, sorted(set(W.GLOW_NAMED_KERNELS) - need)
    assert "conv_mfma_kernel" in need  # (and the generic tile; its shape variants are counted as conv_mfma_kernel.*)


def _run(eng, which, precision, rows, options, need, absent, label, speaker_ids=None):
    hp, sd, g = _model(eng, which)
    t = time.perf_counter()
    report, kernels, counts = W.check_glow_layers(eng, hp, precision, rows, options, g=g, sd=sd, label=label, speaker_ids=speaker_ids)
    worst = max(report, key=lambda r: r["ratio"])
    print(f"{label} {precision} {rows!r}: {len(report)} planes, worst err / bound {worst['ratio']:.3f} ({worst['name']}, {worst['kernel']}), "
          f"{time.perf_counter() - t:.2f} s")
    ran = {k.split(".")[0] if k.startswith("conv_mfma_kernel") else k for k, c in counts.items() if c > 0}
    for k in need:
        assert k in ran, (label, k, sorted(ran))
    for k in absent:
        assert k not in ran, (label, k, sorted(ran))
    return report


@pytest.mark.parametrize("batch", ["lone", "ragged"])
@pytest.mark.parametrize("case", list(CASES))
def test_every_launch_against_float64(gpu_engine, case, batch):
    which, precision, axis, kinds, lo, options, need, absent = CASES[case]
    hp = _model(gpu_engine, which)[0]
    n = W.glow_layer_lengths(hp, precision, axis, kinds, lo)
    # past 256 ids the case is about the encoder: 32 of its ids get frames, so that the decoder pass behind it stays short (and the
    # three rows' planes under the seam's 256 MB)
    kw = dict(frames_for=32) if axis == "P" and n > 256 else {}
    rows = [W.GlowCase(hp, axis, n, **kw)]
    if batch == "ragged":
        rows += [W.GlowCase(hp, axis, 1), W.GlowCase(hp, axis, n // 2 + 1, **kw)]
    spk = None if which != "multi" else ([2] if batch == "lone" else [2, 0, 1])
    report = _run(gpu_engine, which, precision, rows, options, need, absent, f"{case} {axis}={n}", spk)
    if which == "split8":
        by = {r["name"]: r["kernel"] for r in report}
        assert all(by[f"blk{b}.zc"].startswith("conv_mfma_kernel") and by[f"blk{b}.z"] == "-" for b in range(hp.n_blocks_dec)), by


def test_wide_tiles_through_the_batch(gpu_engine):
    """`gate16_kernel.wide` / `lin16_kernel.wide` through the batch, not the length (the sweep's batch-rules (a)): 8 rows of F2 <= 100
    are 4 * 24 * 8 = 768 16-row tiles; here the longest row has 97 columns and most are short: the tile count is the padded pass's."""
    hp = HP.LJSPEECH
    rows = [W.GlowCase(hp, "F2", n) for n in (97, 1, 33, 2, 17, 3, 65, 5)]  # (the longest row sets the pass's tiles)
    _run(gpu_engine, "ljspeech", "f32", rows, {}, WIDE + ("glow_tail_kernel",), (), "decoder-f32 wide")


@pytest.mark.parametrize("precision", ["f16", "f32"])
@pytest.mark.parametrize("which", ["h32", "h192"])
def test_gate_epilogue_alone_on_a_grid_of_biases(gpu_engine, which, precision):
    """W.gate_grid_state_dict: every block's last gate conv has zero weights, so its `acts` plane is the epilogue of its biases alone
    — gate_fast (two v_exp_f32, one v_rcp_f32, the +-15 clamp) in both wn_f16_kernel instantiations, tanhf / expf in f32 — against
    float64 tanh(a) sigmoid(b) under the epilogue's own E, nothing carried."""
    hp = H32 if which == "h32" else dataclasses.replace(H32, hidden_channels=192, n_layers_enc=1)
    key = which + "-grid"
    if key not in _models:
        sd = W.gate_grid_state_dict(synthetic.make_glow_state_dict(hp, seed=70), hp)
        _models[key] = (sd, gpu_engine.load_glow(hp, sd))
    sd, g = _models[key]
    report, kernels, counts = W.check_glow_layers(gpu_engine, hp, precision, [W.GlowCase(hp, "F2", 97)], {}, g=g, sd=sd, label=key)
    last = [r for r in report if r["name"].endswith(f".acts{hp.n_block_layers - 1}")]
    assert len(last) == hp.n_blocks_dec and counts.get("wn_f16_kernel" if precision == "f16" else "gate16_kernel", 0) > 0, counts
    print(f"{key} {precision}: the gate epilogue alone, worst err / bound {max(r['ratio'] for r in last):.3f}, worst |err| {max(r['abs'] for r in last):.3e}")
