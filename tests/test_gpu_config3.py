"""BASELINE config 3 (bench.py's 256-utterance work list, ljspeech GlowTTS + 'high') and a tile-edge sweep of the vocoders on
the device, against the CPU oracle at test time (tests/workload_check.py).

The golden cases cover a handful of lengths; which kernels a vocoder call gets moves with the frame count, the batch and the
load (csrc/host_launch.h).  Config 3 at the bench's length_scale 0.65 spans F = 390 ... 936, across the pair-kernel switches
of the 64- / 32-channel stages (F = 472 / 492), the 128-row tile of the 128-channel stage (F = 511) and, under load, its
128-column tiles (F = 511).  The sweep scans F = 1 ... 1100 per vocoder for the lengths where the launch rules change."""
import time

import pytest

from bench import config3_ids
from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.audio import ljspeech_audio_settings
from tests import workload_check as W

pytestmark = pytest.mark.gpu

LENGTH_SCALE = 0.65  # bench.py's default
SEED = 1234          # bench.py's config3 leg: seed = 1234 + utterance index
NEAR = (472, 492, 511)

_c = {}


def _setup(eng):
    if not _c:
        t = time.perf_counter()
        ghp, vhp = HP.LJSPEECH, HP.HIFIGAN_HIGH
        gsd = synthetic.make_glow_state_dict(ghp, seed=1234)
        vsd = synthetic.make_hifigan_state_dict(vhp, seed=1234)
        rows = config3_ids(ghp.num_symbols)
        _c.update(ghp=ghp, vhp=vhp, gsd=gsd, vsd=vsd, g=eng.load_glow(ghp, gsd), v=eng.load_hifigan(vhp, vsd), rows=rows,
                  s=ljspeech_audio_settings(), ref=[W.oracle_frames(gsd, ghp, r, LENGTH_SCALE) for r in rows])
        print(f"config 3 setup (models, 256 oracle frame counts): {time.perf_counter() - t:.1f} s")
    return _c


def test_config3_bench_form_under_load_and_alone(gpu_engine):
    """Every utterance through the bench's call, 8 in flight and one at a time: bit-equal float and int16 results (the
    128-column tiles of the 128-channel stage run only under load, from F = 511), frame counts against the oracle; then the
    same with both models in fp16 (what `half=True` selects)."""
    c = _setup(gpu_engine)
    eng, g, v = gpu_engine, c["g"], c["v"]
    t = time.perf_counter()
    lone = W.check_load_independence(eng, g, v, c["rows"], LENGTH_SCALE, SEED, c["s"], threads=8, need=("rb_group_kernel.nb4",),
                                      label="f32")
    c["lone"] = lone
    frames = [lone[i][0] for i in range(len(c["rows"]))]
    c["exempt"] = W.check_frames(frames, c["ref"], c["ghp"].n_sqz, "config 3")
    print(f"config 3 frames {min(frames)} ... {max(frames)}; f32 bench form: {time.perf_counter() - t:.1f} s")
    t = time.perf_counter()
    assert eng.set_precision(v, ffi.PRECISION_F16) == 0
    assert eng.set_precision(g, ffi.PRECISION_F16) == 0
    try:
        lone16 = W.check_load_independence(eng, g, v, c["rows"], LENGTH_SCALE, SEED, c["s"], threads=8, need=("pair_f16_group_kernel",),
                                           label="f16")
    finally:
        eng.set_precision(v, ffi.PRECISION_F32)
        eng.set_precision(g, ffi.PRECISION_F32)
    assert [lone16[i][0] for i in range(len(c["rows"]))] == frames  # durations stay f32
    print(f"f16 bench form: {time.perf_counter() - t:.1f} s")


def test_config3_micro_batches_and_oracle(gpu_engine):
    """The shard at batch 1 and batch 8 (within 1 LSB), the seeded mels of every 4th utterance plus the shortest and longest
    against the oracle, and ~12 utterances end to end against the oracle in both forms: the first micro-batch, the longest,
    and the ones whose F sits nearest the launch-rule switches 472 / 492 / 511."""
    c = _setup(gpu_engine)
    eng, g, v, rows = gpu_engine, c["g"], c["v"], c["rows"]
    if "lone" not in c:
        c["lone"] = W.bench_form(eng, g, v, rows, LENGTH_SCALE, SEED, c["s"])
        c["exempt"] = W.check_frames([c["lone"][i][0] for i in range(len(rows))], c["ref"], c["ghp"].n_sqz, "config 3")
    lone, exempt = c["lone"], c["exempt"]
    t = time.perf_counter()
    W.check_micro_batches(eng, g, v, rows, LENGTH_SCALE, SEED, c["s"], batch=8)
    print(f"micro-batches: {time.perf_counter() - t:.1f} s")
    frames = {i: lone[i][0] for i in range(len(rows))}
    ok = [i for i in range(len(rows)) if i not in exempt]
    shortest, longest = min(ok, key=lambda i: frames[i]), max(ok, key=lambda i: frames[i])
    t = time.perf_counter()
    pick_mel = sorted(set(ok[::4]) | {shortest, longest})
    ref_mels = W.check_mels(eng, g, c["gsd"], c["ghp"], rows, LENGTH_SCALE, SEED, pick_mel, exempt, label="config 3")
    print(f"mels ({len(pick_mel)}): {time.perf_counter() - t:.1f} s")
    from larynx_amd import sharding

    first = sharding.micro_batches(list(range(len(rows))), [len(r) for r in rows], 8)[0]
    pick = set(first) | {longest} | {min(ok, key=lambda i: (abs(frames[i] - f), i)) for f in NEAR}
    pick = sorted(i for i in pick if i not in exempt)
    print("end to end:", [(i, frames[i]) for i in pick])
    t = time.perf_counter()
    W.check_waves_end_to_end(eng, g, v, c["gsd"], c["vsd"], c["ghp"], c["vhp"], rows, LENGTH_SCALE, SEED, c["s"], pick, lone, ref_mels,
                             label="config 3")
    print(f"waveforms ({len(pick)}): {time.perf_counter() - t:.1f} s")


_oracle = W.OracleWaves()
_models = {}

SWEEP = {
    # quality, precision, kernels that must run across the compared lengths
    "high": ("high", "f32", ("rb_group_kernel.snake", "rb_group_kernel", "conv_group_kernel", "rb_pair_group_kernel", "pair_group_kernel")),
    "high_f16": ("high", "f16", ("conv_f16_group_kernel", "pair_f16_group_kernel")),
    "medium": ("medium", "f32", ("mrf_small_kernel", "mrf8_kernel")),
    "low": ("low", "f32", ("conv_group_kernel",)),
}


@pytest.mark.parametrize("case", list(SWEEP))
def test_vocoder_tile_edge_sweep(gpu_engine, case):
    """A lone batch-1 call at every F = 1 ... 1100: the kernel signature per F; the first F of each signature, the transitions
    (F and F + 1) and the tile-edge lengths (workload_check.edge_frames) against the oracle at batch 1 and as one ragged batch;
    every kernel of the model's launch rules must have run among them."""
    quality, prec, need = SWEEP[case]
    vhp = HP.VOCODER_QUALITY[quality]
    if quality not in _models:
        vsd = synthetic.make_hifigan_state_dict(vhp, seed=1234)
        _models[quality] = (vsd, gpu_engine.load_hifigan(vhp, vsd))
    vsd, v = _models[quality]
    eng = gpu_engine
    t = time.perf_counter()
    if prec == "f16":
        assert eng.set_precision(v, ffi.PRECISION_F16) == 0
    try:
        sigs = W.scan_signatures(eng, v, vhp.num_mels, 1, 1100, label=case)
        t_scan = time.perf_counter() - t
        edges = W.cover_edges(W.edge_frames(vhp, W.vocoder_tiles(vhp, prec), 1, 1100))
        Fs = W.choose_lengths(sigs, edges, cap=12)
        print(f"{case}: lengths {Fs} (edge cover {edges})")
        t = time.perf_counter()
        o0 = _oracle.seconds
        if prec == "f32":
            ran = W.check_lengths(eng, v, vsd, vhp, Fs, _oracle, quality, W.F32_SWEEP, label=case)
        else:  # a row of a padded batch: the same tiles as its lone call (pair_f16 / conv_f16 deal a row its own tiles)
            bounds = W.f16_wave_bounds(vhp)
            ran = W.check_lengths(eng, v, vsd, vhp, Fs, _oracle, quality, bounds, label=case, solo_rms=0.1 * bounds["rms"])
    finally:
        eng.set_precision(v, ffi.PRECISION_F32)
    print(f"{case}: scan {t_scan:.1f} s, compare {time.perf_counter() - t:.1f} s (oracle {_oracle.seconds - o0:.1f} s)")
    for k in need:
        assert k in ran, (case, k, sorted(ran))
