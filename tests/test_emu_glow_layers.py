"""Every launch of the acoustic model against a float64 reference computed from the planes that launch read
(tests/workload_check.py: check_glow_layers, tests/glow_layers_np.py), on the CPU emulator with the tiny geometries of
tests/test_emu_glow_*.py: H = 32 and the released width H = 192 at short lengths, the three attention kernels, both `glow_fuse`
forms, f32 and the fp16 WaveNet launch, a multi-speaker voice.  Every bound is derived (glow_layers_np's rule; gate_fast's E is measured on a grid of biases) and the float32
chain restatement of each launch kind passes the same assertion here.  An error that every column shares — a wrong tap weight,
LayerNorm's epsilon, a clamp, an attention window off by one — leaves the bound at the launch that made it; the end-to-end mel
bounds (5e-5 in f32, the reference's own .half() deviation in fp16) have a hundred-fold slack for it.  The device twin is
tests/test_gpu_glow_layers.py."""
import dataclasses
import time

import numpy as np
import pytest

from larynx_amd import hparams as HP
from larynx_amd import synthetic
from tests import glow_layers_np as G
from tests import voc_layers_np as V
from tests import workload_check as W

ATTENTION = ("attention_mfma_kernel", "attention_mfma_kernel.p768", "attention_kernel")
FUSE_OFF = {"glow_fuse": (0, 1)}


def _hp(hidden, enc=2, blocks=2, layers=2, mel=8, **kw):
    return HP.GlowHParams(num_symbols=30, hidden_channels=hidden, filter_channels=kw.pop("filter_channels", 32), filter_channels_dp=32,
                          n_blocks_dec=blocks, n_layers_enc=enc, n_block_layers=layers, mel_channels=mel, **kw)


GEOMETRIES = {
    "h32": (_hp(32, layers=4), 70),                                                       # the H = 32 wn_f16_kernel instantiation
    "h64": (_hp(64, enc=1, blocks=1), 68),                                                # the long-P attention kernels, affordably
    "h192": (_hp(192, enc=2, blocks=2, layers=4, mel=80, filter_channels=768), 71),      # the released voices' instantiations
    "multi": (dataclasses.replace(HP.TINY_GLOW, n_speakers=3, gin_channels=20), 21),
    "split8": (_hp(32, enc=1, n_split=8), 72),                                            # no fused mix: invconv_actnorm_kernel
}
_models = {}


def _model(eng, geometry):
    hp, seed = GEOMETRIES[geometry]
    if geometry not in _models:
        sd = synthetic.make_glow_state_dict(hp, seed=seed)
        _models[geometry] = (sd, eng.load_glow(hp, sd))
    return (hp,) + _models[geometry]


def _rows(hp, axis, n, batch):
    """A lone call of length n, or the ragged three-row batch: full, the smallest legal, mid."""
    if batch == "lone":
        return [W.GlowCase(hp, axis, n)]
    return [W.GlowCase(hp, axis, n), W.GlowCase(hp, axis, 1), W.GlowCase(hp, axis, max(n // 2 + 1, 2))]


def run_case(eng, geometry, precision, rows, options=None, need=(), absent=(), speaker_ids=None, restate=True, model=None):
    hp, sd, g = model or _model(eng, geometry)
    t = time.perf_counter()
    report, kernels, counts = W.check_glow_layers(eng, hp, precision, rows, options, g=g, sd=sd, label=geometry, speaker_ids=speaker_ids,
                                                  restate=restate)
    print(f"{geometry} {precision} {rows!r} {options or ''}: {len(report)} planes, {time.perf_counter() - t:.2f} s")
    for k in need:
        assert counts.get(k, 0) > 0 and k in kernels, (geometry, precision, k, counts)
    for k in absent:
        assert counts.get(k, 0) == 0, (geometry, precision, k, counts)
    return report


# the lengths come from the tile table (W.GLOW_TILE_WIDTHS), not from the workload
def test_lengths_come_from_the_tile_table():
    hp = HP.LJSPEECH
    P = W.glow_layer_lengths(hp, "f32", "P", ("attention_mfma 32", "oproj_ln"))
    assert P == 65 and P > 2 * 32 and P % 32 and P % 16
    assert W.glow_layer_lengths(hp, "f32", "P", ("attention_mfma 32", "oproj_ln"), lo=257) == 257
    assert W.glow_layer_lengths(hp, "f32", "P", ("attention ATT_ROWS",), lo=769) == 769
    assert W.glow_layer_lengths(hp, "f32", "F2", ("gate16", "lin16", "glow_tail")) == 65
    assert W.glow_layer_lengths(hp, "f16", "F2", ("wn_f16",)) == 97  # 2 x 48 + a ragged third


@pytest.mark.parametrize("batch", ["lone", "ragged"])
@pytest.mark.parametrize("fuse", ["fused", "glow_fuse=0"])
@pytest.mark.parametrize("geometry", ["h32", "h192"])
def test_every_launch_against_float64_f32(emu_engine, geometry, fuse, batch):
    hp = GEOMETRIES[geometry][0]
    n = W.glow_layer_lengths(hp, "f32", "P", ("attention_mfma 32", "oproj_ln", "lin16", "gate16", "glow_tail"))  # P ids of 2 frames: F2 = P
    if fuse == "fused":
        need, absent = ("attention_mfma_kernel", "oproj_ln_kernel", "gate16_kernel", "glow_tail_kernel"), ()
        if geometry == "h192":  # (the 16-row tile takes no conv of the H = 32 model)
            need += ("lin16_kernel", "lin16_kernel.ln")
    else:
        need, absent = ("attention_mfma_kernel", "gate16_kernel"), ("oproj_ln_kernel", "lin16_kernel.ln", "glow_tail_kernel")
    report = run_case(emu_engine, geometry, "f32", _rows(hp, "P", n, batch), {} if fuse == "fused" else FUSE_OFF, need, absent)
    names = {r["name"] for r in report}
    if fuse == "fused":
        # (a conv without a 16-row shape keeps its LayerNorm launch in the fused form too: "{name}.ln")
        assert "enc1.x0" in names and "enc0.o" not in names and not any(x.endswith(".zc") or x == "logw.ln" for x in names)
        if geometry == "h192":
            assert {r["kernel"] for r in report if r["name"] in ("enc1.x0", "enc1.qkv")} == {"lin16_kernel.ln"}
    else:
        assert {"enc0.o", "enc1.x0", "pre.1.ln", "dp.2.ln", "logw.ln", f"blk0.skip{hp.n_block_layers - 1}"} <= names


@pytest.mark.parametrize("batch", ["lone", "ragged"])
@pytest.mark.parametrize("geometry", ["h32", "h192"])
def test_every_launch_against_float64_f16(emu_engine, geometry, batch):
    """The fp16 WaveNet launch: 48 written columns per workgroup, 8 recomputed per side; two full tiles and a ragged third."""
    hp = GEOMETRIES[geometry][0]
    n = W.glow_layer_lengths(hp, "f16", "F2", ("wn_f16",))
    report = run_case(emu_engine, geometry, "f16", _rows(hp, "F2", n, batch), {}, ("wn_f16_kernel", "glow_tail_kernel"),
                      ("gate16_kernel", "gate16_kernel.wide"))
    assert {r["kernel"] for r in report if r["name"].startswith("blk") and ".acts" in r["name"]} == {"wn_f16_kernel"}


@pytest.mark.parametrize("P,kernel", [(257 + 8, ATTENTION[1]), (769 + 1, ATTENTION[2])])
def test_long_attention_kernels(emu_engine, P, kernel):
    """The ATTM_MAXP LDS layout (P > 256) and the VALU kernel (P > 768, ATT_ROWS = 4 rows per workgroup: 770 leaves a ragged one, and
    in the batch a padded row next to it: the score scratch's stride), one encoder layer at H = 64."""
    hp = GEOMETRIES["h64"][0]
    run_case(emu_engine, "h64", "f32", [W.GlowCase(hp, "P", P)], {}, (kernel,), tuple(k for k in ATTENTION if k != kernel))
    if kernel == ATTENTION[2]:
        run_case(emu_engine, "h64", "f32", [W.GlowCase(hp, "P", 1), W.GlowCase(hp, "P", P)], {}, (kernel,), restate=False)


@pytest.mark.parametrize("batch", ["lone", "ragged"])
@pytest.mark.parametrize("fuse", ["fused", "glow_fuse=0"])
def test_eight_way_split_has_no_fused_mix(emu_engine, fuse, batch):
    """n_split = 8: neither glow_tail_kernel nor the coupling epilogue's mix takes the block's end, so conv_mfma_kernel's coupling
    epilogue runs WITHOUT the mix (`blk{b}.zc`) and invconv_actnorm_kernel does InvConvNear and ActNorm as a launch of its own
    (`blk{b}.z`, counted under no name) — in both `glow_fuse` forms."""
    hp = GEOMETRIES["split8"][0]
    report = run_case(emu_engine, "split8", "f32", _rows(hp, "P", 65, batch), {} if fuse == "fused" else FUSE_OFF, ("conv_mfma_kernel",),
                      ("glow_tail_kernel",))
    by = {r["name"]: r for r in report}
    for b in range(hp.n_blocks_dec):
        assert by[f"blk{b}.zc"]["kernel"].startswith("conv_mfma_kernel") and by[f"blk{b}.z"]["kernel"] == "-", (by[f"blk{b}.zc"], by[f"blk{b}.z"])
        assert by[f"blk{b}.zc"]["restated"] is not None and by[f"blk{b}.z"]["restated"] is not None


@pytest.mark.parametrize("fuse", ["fused", "glow_fuse=0"])
def test_multi_speaker_voice(emu_engine, fuse):
    """The speaker's offsets into every gate (`cond`) and the duration predictor's speaker plane (speaker_dp_plane_kernel)."""
    hp = GEOMETRIES["multi"][0]
    rows = [W.GlowCase(hp, "P", 37), W.GlowCase(hp, "P", 1), W.GlowCase(hp, "P", 18)]
    report = run_case(emu_engine, "multi", "f32", rows, {} if fuse == "fused" else FUSE_OFF, speaker_ids=[2, 0, 1])
    assert "dp.spk" in {r["name"] for r in report}


@pytest.mark.parametrize("precision", ["f16", "f32"])
@pytest.mark.parametrize("geometry", ["h32", "h192"])
def test_gate_epilogue_alone_on_a_grid_of_biases(emu_engine, geometry, precision):
    """W.gate_grid_state_dict: the last gate conv of every block has zero weights, so its `acts` plane is the epilogue of its biases
    alone — gate_fast in fp16 (both wn_f16_kernel instantiations), tanhf / expf in f32 — and the walk's bound for that plane is the
    epilogue's E and nothing else: the clamp, a wrong constant in an exponent, a reciprocal too coarse show here."""
    hp, seed = GEOMETRIES[geometry]
    key = geometry + "-grid"
    if key not in _models:
        sd = W.gate_grid_state_dict(synthetic.make_glow_state_dict(hp, seed=seed), hp)
        _models[key] = (sd, emu_engine.load_glow(hp, sd))
    need = ("wn_f16_kernel",) if precision == "f16" else ("gate16_kernel",)
    report = run_case(emu_engine, key, precision, [W.GlowCase(hp, "F2", 97)], {}, need, model=(hp,) + _models[key])
    last = [r for r in report if r["name"].endswith(f".acts{hp.n_block_layers - 1}")]
    assert len(last) == hp.n_blocks_dec and all(r["ratio"] <= 1.0 for r in last)
    print(f"{key} {precision}: the gate epilogue alone, worst err / bound {max(r['ratio'] for r in last):.3f}, worst |err| {max(r['abs'] for r in last):.3e}")


def test_gate_fast_against_float64_on_a_grid():
    """The float32 restatement of gate_fast's formula over a grid of pre-activations (both clamps, the sigmoid's overflow side) stays
    inside E_GATE_FAST: a measured E under which the restatement failed would be a wrong measurement."""
    a, b = np.meshgrid(np.linspace(-20, 20, 801), np.linspace(-90, 90, 721))
    a, b = a.astype(np.float32), b.astype(np.float32)
    ref, delta = G.wn_gate(a.astype(np.float64), b.astype(np.float64), 0.0, 0.0)
    err = np.abs(G.wn_gate32(a, b).astype(np.float64) - ref)
    ratio = err / V.bound_f32(ref, delta)
    print(f"gate_fast restated in float32 over {a.size} points: worst err / bound {ratio.max():.3f}, worst |err| {err.max():.3e}")
    assert ratio.max() <= 1.0


def test_the_rows_of_a_tapped_call(emu_engine):
    """The tap list itself: launch order, every plane [B, channels, ld] with the rows' lengths, kernel names from the launch
    accounting ("-" for the launches it counts under no name)."""
    hp, sd, g = _model(emu_engine, "h32")
    c = [W.GlowCase(hp, "P", 9), W.GlowCase(hp, "P", 4)]
    noise = np.zeros((2, hp.mel_channels, 24), np.float32)
    mel, taps = emu_engine.glow_infer_taps(g, [x.ids for x in c], 0.667, 1.0, noise=noise, durations=[x.d for x in c])
    assert [int(f) for f in mel.frames] == [18, 8]
    mel.free()
    names = [t["name"] for t in taps]
    assert names[:2] == ["emb", "pre.0"] and names[-1] == "mel" and names.index("pre.1") < names.index("xm") < names.index("z0") < names.index("blk1.acts0")
    by = {t["name"]: t for t in taps}
    assert by["enc0.qkv"]["channels"] == 3 * hp.hidden_channels and by["enc0.qkv"]["len"] == [9, 4] and by["enc0.qkv"]["ld"] == 12
    assert by["blk1.z"]["channels"] == hp.mel_channels * hp.n_sqz and by["blk1.z"]["len"] == [9, 4]
    assert by["mel"]["len"] == [18, 8] and by["emb"]["kernel"] == "-" and by["enc0.x1"]["kernel"] == "oproj_ln_kernel"
    assert by["blk0.h"]["kernel"] == "glow_tail_kernel" and by["blk1.h"]["kernel"].startswith("conv_mfma_kernel")
    assert all(t["f16"] == 0 and t["x"].shape == (2, t["channels"], t["ld"]) for t in taps)
