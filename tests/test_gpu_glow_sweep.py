"""A launch-rule and tile-edge sweep of the acoustic model on the device at the released shape (HP.LJSPEECH: H = 192, 2 heads,
dk = 96), against the CPU oracle at test time (tests/workload_check.py; tests/test_emu_glow_sweep.py is the emulator twin).

Which kernels a GlowTTS call gets moves with the id count, the frame count, the batch and the precision: the attention by P
(256-id MFMA layout, ATTM_MAXP layout, the VALU kernel past 768 ids: glow_forward.h launch_attention), the decoder's 16-row
tiles by pass size (`.wide` from 512 tiles: host_launch.h run_gate16 / run_lin16), 1 x 1 convs of big padded batches back on the
generic tile.  Every call forces its durations, so the compared lengths are exact, and injects seeded noise, so neighbouring
columns differ and a column-indexing error at a tile seam shows."""
import time

import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from tests import workload_check as W
from tests.test_gpu_parity import models

pytestmark = pytest.mark.gpu

ATTENTION = ("attention_mfma_kernel", "attention_mfma_kernel.p768", "attention_kernel")
_oracle = W.GlowOracle()
KEY = "ljspeech-1234"

SWEEP = {
    # axis, scanned range, precision, lengths always compared, cap on the compared lengths, kernels that must run among them
    "encoder-f32": ("P", 800, "f32", (1, 2, 3, 8, 9, 10, 256, 257, 768, 769), 16,
                    ATTENTION + ("oproj_ln_kernel", "lin16_kernel", "lin16_kernel.ln")),
    "decoder-f32": ("F2", 1500, "f32", (1, 2, 3, 4, 5, 1500), 20,
                    ("gate16_kernel", "gate16_kernel.wide", "lin16_kernel", "lin16_kernel.wide", "glow_tail_kernel")),
    # (673, 1500: the fp16 launch has no length rule of its own; the f32 launches around it have, and F = 3000 is 3x the goldens')
    "decoder-f16": ("F2", 1500, "f16", (1, 2, 3, 4, 5, 673, 1500), 20, ("wn_f16_kernel", "glow_tail_kernel")),
}


def _setup(eng):
    hp = HP.LJSPEECH
    (gsd, g), _ = models(eng, hp, HP.HIFIGAN_HIGH)  # synthetic state dict, seed 1234
    return hp, gsd, g


def _transitions(sigs):
    ns = sorted(sigs)
    return [(a, b) for a, b in zip(ns, ns[1:]) if sigs[a] != sigs[b]]


@pytest.mark.parametrize("case", list(SWEEP) + ["batch-rules"])
def test_glow_tile_edge_sweep(gpu_engine, case):
    """encoder-f32 / decoder-f32 / decoder-f16 (batch-rules: see batch_rules): a lone call at every length of the scanned axis
    gives the kernel signature per length; the first length of each signature, the transitions (n and n + 1), the lengths below
    every tile and the tile-edge lengths (workload_check.edge_frames) against the oracle as lone calls and as one ragged padded
    batch; every kernel of the launch rules must have run among them."""
    if case == "batch-rules":
        return batch_rules(gpu_engine)
    axis, hi, prec, must, cap, need = SWEEP[case]
    eng = gpu_engine
    hp, gsd, g = _setup(eng)
    nb = hp.n_blocks_dec
    t = time.perf_counter()
    if prec == "f16":
        assert eng.set_precision(g, ffi.PRECISION_F16) == 0
    try:
        sigs = W.scan_glow_signatures(eng, g, hp, axis, 1, hi, label=case)
        t_scan = time.perf_counter() - t
        trans = _transitions(sigs)
        print(f"{case}: transitions {trans}")
        if axis == "P":
            assert (256, 257) in trans and (768, 769) in trans, trans
            for P, s in sigs.items():
                want = ATTENTION[0] if P <= 256 else ATTENTION[1] if P <= 768 else ATTENTION[2]
                assert s & set(ATTENTION) == {want}, (P, sorted(s))
        elif prec == "f32":  # gate16 / lin16 `.wide` from 512 16-row tiles: ceil(F2 / 32) * 24 >= 512 at F2 = 673
            assert (672, 673) in trans and "gate16_kernel.wide" in sigs[673] and "gate16_kernel.wide" not in sigs[672], trans
        tiles = W.glow_tiles(hp, prec)
        if prec == "f16":  # the edges of this case come from the fp16 launch's tile
            tiles = [t_ for t_ in tiles if t_[0].startswith("wn_f16")]
            assert [(w, h) for _, _, w, h in tiles] == [(48, 8)]
        # edges from 33 on: a tile edge next to a full tile (the lengths below every tile are in `must`)
        edges = W.edge_frames(hp, tiles, 33, hi, W.glow_axis(hp, axis))
        ns = W.choose_glow_lengths(sigs, must, edges, cap=cap, label=case)
        cases = [W.GlowCase(hp, axis, n) for n in ns]
        if axis == "F2":
            cases.append(W.GlowCase(hp, axis, 77, odd_sum=True))  # an odd duration sum: F truncated to even
        t = time.perf_counter()
        o0 = _oracle.seconds
        if prec == "f32":
            ran, ran_b = W.check_glow_lengths(eng, g, gsd, hp, cases, _oracle, KEY, label=case)
        else:
            bounds = W.f16_mel_bounds("ljspeech")

            def launches(counts, tag):
                assert counts.get("wn_f16_kernel", 0) == nb, (tag, counts)
                assert counts.get("gate16_kernel", 0) == 0 and counts.get("gate16_kernel.wide", 0) == 0, (tag, counts)

            ran, ran_b = W.check_glow_lengths(eng, g, gsd, hp, cases, _oracle, KEY, bounds, label=case, solo_tol=0.1 * bounds["max"],
                                              on_counts=launches)
        if axis == "P":  # the duration predictor and duration_kernel's ceil path: the forced calls never read them
            for n in ns:
                W.check_plain_durations(eng, g, gsd, hp, n, label=case)
        else:  # the exact seam check (the fp16 bound is ~25x what the launch costs: one missing halo column would pass it)
            for n in (300, 1500):
                print(f"{case}: F2 {n}: {W.check_interior_columns_equal(eng, g, hp, n, label=case)} interior columns bit-equal")
    finally:
        eng.set_precision(g, ffi.PRECISION_F32)
    print(f"{case}: scan {t_scan:.1f} s, compare {time.perf_counter() - t:.1f} s (oracle {_oracle.seconds - o0:.1f} s)")
    for k in need:
        assert k in ran | ran_b, (case, k, sorted(ran | ran_b))
    if axis == "F2":
        assert any(k.startswith("conv_mfma_kernel") for k in ran), sorted(ran)  # the generic tile (the first block's start conv)


def batch_rules(gpu_engine):
    """Padded batches chosen so that each batch-size rule of the launch code happens once (by `kernel_counts`), every row against
    the oracle and against its lone call:
    (a) `gate16_kernel.wide` / `lin16_kernel.wide` through the batch, not the length: 8 rows of F2 <= 100 are 4 * 24 * 8 = 768
        16-row tiles, a lone row 96;
    (b) the `K == 1 && B > 1 && tiles > 512` rule of run_lin16: proj_m (80 rows: gy = 5, no `.wide` form) at 8 rows of <= 450 ids is
        15 * 5 * 8 = 600 tiles and goes back to the generic tile: one more conv_mfma launch than the longest row's lone call;
    (c) 1 id next to 769 ids: the VALU attention in a batch (its rows padded to ATT_ROWS, the score scratch's row stride)."""
    eng = gpu_engine
    hp, gsd, g = _setup(eng)
    t = time.perf_counter()

    def generic(counts):
        return sum(n for k, n in counts.items() if k.startswith("conv_mfma_kernel"))

    seen = {}

    def keep(counts, tag):
        seen[tag] = dict(counts)

    # (a)
    cases = [W.GlowCase(hp, "F2", n) for n in (100, 97, 65, 99, 33, 98, 81, 96)]
    ran, ran_b = W.check_glow_lengths(eng, g, gsd, hp, cases, _oracle, KEY, label="batch-rules (a)", rows=cases)
    assert not {"gate16_kernel.wide", "lin16_kernel.wide"} & ran, sorted(ran)
    assert {"gate16_kernel.wide", "lin16_kernel.wide"} <= ran_b, sorted(ran_b)
    # (b)
    cases = [W.GlowCase(hp, "P", n) for n in (433, 450, 420, 447, 449, 425, 448, 431)]
    seen.clear()
    W.check_glow_lengths(eng, g, gsd, hp, cases, _oracle, KEY, label="batch-rules (b)", rows=cases, on_counts=keep)
    lone = next(c for tag, c in seen.items() if tag.endswith("[P=450]"))
    batch = next(c for tag, c in seen.items() if "," in tag)
    print(f"batch-rules (b): generic conv launches: lone P=450 {generic(lone)}, batch of 8 {generic(batch)}")
    assert generic(batch) == generic(lone) + 1, (lone, batch)
    # (c)
    cases = [W.GlowCase(hp, "P", 1), W.GlowCase(hp, "P", 769)]
    ran, ran_b = W.check_glow_lengths(eng, g, gsd, hp, cases, _oracle, KEY, label="batch-rules (c)", rows=cases)
    assert "attention_kernel" in ran_b and not set(ATTENTION[:2]) & ran_b, sorted(ran_b)
    print(f"batch-rules: {time.perf_counter() - t:.1f} s (oracle {_oracle.seconds:.1f} s over the module)")
