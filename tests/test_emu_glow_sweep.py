"""The GlowTTS launch-rule and tile-edge sweep (tests/workload_check.py: scan_glow_signatures, choose_glow_lengths,
check_glow_lengths) on the CPU emulator build, with models the emulator affords.  tests/test_gpu_glow_sweep.py runs the same
helpers on the device at the released shape; here they prove themselves (edge table, scan, choice, comparison) and pin which
attention kernel `kernel_counts()` names at 256 / 257 and 768 / 769 ids."""
import time

import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from tests import workload_check as W

ATTENTION = ("attention_mfma_kernel", "attention_mfma_kernel.p768", "attention_kernel")

_oracle = W.GlowOracle()


def _hp(hidden, enc=2, blocks=2, layers=2, mel=8, **kw):
    return HP.GlowHParams(num_symbols=30, hidden_channels=hidden, filter_channels=kw.pop("filter_channels", 32), filter_channels_dp=32,
                          n_blocks_dec=blocks, n_layers_enc=enc, n_block_layers=layers, mel_channels=mel, **kw)


@pytest.fixture()
def model(emu_engine, request):
    hp, seed = request.param
    sd = synthetic.make_glow_state_dict(hp, seed=seed)
    g = emu_engine.load_glow(hp, sd)
    yield hp, sd, g, f"emu-{hp.hidden_channels}-{seed}"
    emu_engine.set_precision(g, ffi.PRECISION_F32)
    emu_engine.unload(g)


# ---------------------------------------------------------------- the helpers themselves (no engine)
def test_tile_table_and_edges():
    """glow_tiles at the released shape: the widths and halos of the kernels' headers; edge_frames over the two axes; the
    vocoder's callers see the same edges as before the axis function existed."""
    hp = HP.LJSPEECH
    f32 = {(lab, st[0]): (w, h) for lab, st, w, h in W.glow_tiles(hp, "f32")}
    f16 = {(lab, st[0]): (w, h) for lab, st, w, h in W.glow_tiles(hp, "f16")}
    assert f32[("gate16 32 columns", "F2")] == (32, 2) and ("gate16 32 columns", "F2") not in f16
    assert f16[("wn_f16 WN_W - 2 margin", "F2")] == (48, 8) and ("wn_f16 WN_W - 2 margin", "F2") not in f32
    assert f32[("attention_mfma 32 rows / 32 keys", "P")] == (32, 4) and f32[("attention ATT_ROWS", "P")] == (4, 0)
    assert f32[("glow_tail COL_T", "F2")] == (16, 0) and f32[("lin16 TC=16", "P")] == (16, 1)
    for axis in ("P", "F2"):
        assert [f32[(f"conv_mfma T_T={w}", axis)][0] for w in (32, 64, 128, 256)] == [32, 64, 128, 256]
    # the P axis: the VALU attention's tiles exist only past 768 ids, the MFMA attention's only up to there
    e = W.edge_frames(hp, W.glow_tiles(hp, "f32"), 760, 780, W.glow_axis(hp, "P"))
    assert ("attention ATT_ROWS", ("P", 769, None), 4, "one") in e[769] and not any(lab == "attention ATT_ROWS" for lab, *_ in e[768])
    assert any(lab.startswith("attention_mfma") and kind == "full" for lab, _, _, kind in e[768])
    assert not any(lab.startswith("attention_mfma") for lab, *_ in e[769])
    # the F2 axis: F = 2 F2 for the 256-frame kernels; the fp16 tile: full, one column, narrower than its halo
    e = W.edge_frames(hp, W.glow_tiles(hp, "f16"), 90, 130, W.glow_axis(hp, "F2"))
    kinds = {n: {k for lab, _, _, k in e.get(n, ()) if lab.startswith("wn_f16")} for n in (96, 97, 103, 104)}
    assert kinds == {96: {"full"}, 97: {"one"}, 103: {"halo"}, 104: set()}
    assert any(lab.startswith("expand_noise") and k == "full" for lab, _, _, k in e[128])
    cover = W.cover_edges(e)
    left = {(s, w, k) for hits in e.values() for (_, s, w, k) in hits}
    for n in cover:
        left -= {(s, w, k) for (_, s, w, k) in e[n]}
    assert not left and len(cover) <= 6
    assert W.cover_edges(e, have=cover) == [] and len(W.cover_edges(e, cap=2)) == 2
    # the vocoder: the default axis function is the stage length
    vhp = HP.HIFIGAN_HIGH
    tiles = W.vocoder_tiles(vhp, "f32")
    assert W.edge_frames(vhp, tiles, 1, 40) == W.edge_frames(vhp, tiles, 1, 40, W.vocoder_axis(vhp))
    assert all((F * int(np.prod(vhp.upsample_rates[: st + 1]))) % w in (0, 1) or k == "halo"
               for F, hits in W.edge_frames(vhp, tiles, 1, 40).items() for (_, st, w, k) in hits)


def test_forced_durations_and_ids():
    hp = HP.LJSPEECH
    for F2 in list(range(1, 40)) + [673, 1500]:
        d = W.forced_durations(hp, F2)
        assert d.sum() == 2 * F2 and d.min() >= 0 and np.any(d % 2) and len(set(d.tolist())) > 1
        assert W.forced_durations(hp, F2, odd_sum=True).sum() == 2 * F2 + 1
        c = W.GlowCase(hp, "F2", F2, odd_sum=True)
        assert c.F == 2 * F2 and c.exp_d.sum() == c.F and c.exp_d[-1] == c.d[-1] - 1  # the truncated last id
    c = W.GlowCase(hp, "P", 9)
    assert c.F == 18 and np.array_equal(c.exp_d, c.d) and c.noise.shape == (80, 23)
    assert np.array_equal(W.glow_ids(hp, 9), W.GlowCase(hp, "P", 9).ids) and not np.array_equal(W.glow_ids(hp, 9)[:8], W.glow_ids(hp, 8))


# ---------------------------------------------------------------- the sweep on small models
@pytest.mark.parametrize("model", [(_hp(64, blocks=1), 67)], indirect=True)
def test_encoder_sweep(emu_engine, model):
    """P = 1 ... 70 at H = 64 (the test_emu_glow_coltile shape): one signature, the tile-edge lengths of the P axis and the lengths
    around window_size against the oracle, lone and as one ragged batch; the plain call's durations at every compared length."""
    hp, sd, g, key = model
    eng = emu_engine
    t = time.perf_counter()
    sigs = W.scan_glow_signatures(eng, g, hp, "P", 1, 70, label=key)
    t_scan = time.perf_counter() - t
    assert all("attention_mfma_kernel" in s and not s & set(ATTENTION[1:]) for s in sigs.values())
    edges = W.edge_frames(hp, W.glow_tiles(hp, "f32"), 17, 70, W.glow_axis(hp, "P"))
    Ps = W.choose_glow_lengths(sigs, (1, 2, 3, 8, 9, 10), edges, cap=14, label=key)
    assert {1, 2, 3, 8, 9, 10, 64, 65} <= set(Ps)  # 64 / 65: a full and a one-column last tile of every 16- to 64-wide kernel at once
    t = time.perf_counter()
    cases = [W.GlowCase(hp, "P", P) for P in Ps]
    ran, ran_b = W.check_glow_lengths(eng, g, sd, hp, cases, _oracle, key, label=key)
    for P in Ps:
        W.check_plain_durations(eng, g, sd, hp, P, label=key)
    print(f"{key}: scan {t_scan:.1f} s, compare {time.perf_counter() - t:.1f} s (oracle {_oracle.seconds:.1f} s)")
    for k in ("attention_mfma_kernel", "oproj_ln_kernel", "gate16_kernel", "glow_tail_kernel"):
        assert k in ran and k in ran_b, (k, sorted(ran), sorted(ran_b))


@pytest.mark.parametrize("model", [(_hp(64, enc=1, blocks=1), 68)], indirect=True)
def test_attention_names_at_256_and_768(emu_engine, model):
    """A one-layer model at P = 255 ... 258 and 767 ... 770: `kernel_counts()` names the 256-id MFMA layout up to 256 ids, the
    ATTM_MAXP layout up to 768 and the VALU kernel past it, one launch per encoder layer; all eight lengths against the oracle,
    and 1 id next to 769 as a batch (the VALU attention with a padded row)."""
    hp, sd, g, key = model
    eng = emu_engine
    Ps = (255, 256, 257, 258, 767, 768, 769, 770)
    sigs = W.scan_glow_signatures(eng, g, hp, "P", 0, 0, label=key, only=Ps)
    for P in Ps:
        want = ATTENTION[0] if P <= 256 else ATTENTION[1] if P <= 768 else ATTENTION[2]
        assert sigs[P] & set(ATTENTION) == {want}, (P, sorted(sigs[P]))
    assert W.choose_glow_lengths(sigs, label=key) == [255, 256, 257, 768, 769]

    def one_launch(counts, tag):
        assert sum(counts.get(k, 0) for k in ATTENTION) == hp.n_layers_enc, (tag, counts)

    cases = [W.GlowCase(hp, "P", P) for P in Ps]
    ran, _ = W.check_glow_lengths(eng, g, sd, hp, cases, _oracle, key, label=key, batch=0, on_counts=one_launch)
    assert set(ATTENTION) <= ran
    one = W.GlowCase(hp, "P", 1)
    _, ran_b = W.check_glow_lengths(eng, g, sd, hp, [one, cases[6]], _oracle, key, label=key, rows=[one, cases[6]])
    assert "attention_kernel" in ran_b and not ran_b & set(ATTENTION[:2])


@pytest.mark.parametrize("model", [(_hp(64, enc=1), 69)], indirect=True)
def test_decoder_sweep(emu_engine, model):
    """F2 = 1 ... 110 at H = 64 with 8 ids of forced, uneven durations: the F2-axis tile edges, F2 = 1 ... 5 and one odd duration
    sum against the oracle, lone and as one ragged batch."""
    hp, sd, g, key = model
    eng = emu_engine
    sigs = W.scan_glow_signatures(eng, g, hp, "F2", 1, 110, label=key)
    edges = W.edge_frames(hp, W.glow_tiles(hp, "f32"), 17, 110, W.glow_axis(hp, "F2"))
    ns = W.choose_glow_lengths(sigs, (1, 2, 3, 4, 5), edges, cap=14, label=key)
    assert {1, 2, 3, 4, 5, 64, 65} <= set(ns)
    cases = [W.GlowCase(hp, "F2", n) for n in ns] + [W.GlowCase(hp, "F2", 37, odd_sum=True)]
    ran, ran_b = W.check_glow_lengths(eng, g, sd, hp, cases, _oracle, key, label=key)
    for k in ("gate16_kernel", "glow_tail_kernel", "conv_mfma_kernel"):
        assert k in ran and k in ran_b, (k, sorted(ran), sorted(ran_b))
    assert W.check_interior_columns_equal(eng, g, hp, 110, label=key) >= 60  # f32: the gate16 / glow_tail seams


# a half-precision band for these synthetic models, as tests/test_emu_glow_f16.py: the mels are O(1), fp16 has 11 bits: an index
# slip (a wrong tap, tile margin, column) is an O(1) error on some element
F16_BAND = dict(max=2e-2, rms=4e-3)


@pytest.mark.parametrize("model", [(_hp(32, enc=1, blocks=2, layers=4), 70)], indirect=True)
def test_decoder_sweep_f16(emu_engine, model):
    """The fp16 WaveNet launch (wn_f16.h) at H = 32 with four layers: 48 written columns per workgroup, 8 recomputed per side;
    last tile full, one column, narrower than the halo.  On these shapes a row of a padded batch runs the tiles of its lone call:
    bit-equal."""
    hp, sd, g, key = model
    eng = emu_engine
    tiles = [t for t in W.glow_tiles(hp, "f16") if t[0].startswith("wn_f16")]
    assert [(w, h) for _, _, w, h in tiles] == [(48, 8)]
    assert eng.set_precision(g, ffi.PRECISION_F16) == 0
    sigs = W.scan_glow_signatures(eng, g, hp, "F2", 1, 110, label=key)
    assert all("wn_f16_kernel" in s and "gate16_kernel" not in s for s in sigs.values())
    edges = W.edge_frames(hp, tiles, 40, 110, W.glow_axis(hp, "F2"))
    ns = W.choose_glow_lengths(sigs, (1, 7, 8, 9), edges, cap=10, label=key)
    assert {48, 49} <= set(ns) or {96, 97} <= set(ns)

    def launches(counts, tag):
        assert counts.get("wn_f16_kernel", 0) == hp.n_blocks_dec, (tag, counts)
        assert counts.get("gate16_kernel", 0) == 0 and counts.get("gate16_kernel.wide", 0) == 0, (tag, counts)

    cases = [W.GlowCase(hp, "F2", n) for n in ns]
    W.check_glow_lengths(eng, g, sd, hp, cases, _oracle, key, F16_BAND, label=key, solo_tol=0.0, on_counts=launches)
    # the band above is far wider than what one missing halo column costs (an error four layers deep): the exact seam check
    assert W.check_interior_columns_equal(eng, g, hp, 110, label=key) >= 60  # the seam at column 48 lies inside


@pytest.mark.parametrize("model", [(_hp(192, enc=1, blocks=1, layers=4, mel=80, filter_channels=768), 71)], indirect=True)
def test_released_width_short_lengths(emu_engine, model):
    """H = 192, 2 heads (dk = 96), FFN 768, 80 mel channels, one encoder layer and one flow block: the released voices' kernel
    instantiations at short lengths on both sides of the 16- and 32-column seams, f32 and the fp16 WaveNet launch."""
    hp, sd, g, key = model
    eng = emu_engine
    cases = [W.GlowCase(hp, "P", P) for P in (1, 9, 17, 33)] + [W.GlowCase(hp, "F2", 49), W.GlowCase(hp, "F2", 5, odd_sum=True)]
    ran, ran_b = W.check_glow_lengths(eng, g, sd, hp, cases, _oracle, key, label=key)
    for k in ("attention_mfma_kernel", "oproj_ln_kernel", "lin16_kernel", "gate16_kernel", "glow_tail_kernel"):
        assert k in ran, (k, sorted(ran))
    for P in (9, 33):
        W.check_plain_durations(eng, g, sd, hp, P, label=key)
    assert eng.set_precision(g, ffi.PRECISION_F16) == 0
    bounds = W.f16_mel_bounds()
    ran, _ = W.check_glow_lengths(eng, g, sd, hp, cases[3:], _oracle, key, bounds, label=key + "-f16", solo_tol=0.1 * bounds["max"])
    assert "wn_f16_kernel" in ran and "gate16_kernel" not in ran
