#!/usr/bin/env python3
"""Time `mi355tts_shift` on the device next to the vocoder call whose output it reads and next to the `mi355tts_pitch` and
`mi355tts_resample` calls on the same row; record its launches one by one and what the tests' checks measure on this device.

    python tools/shift_probe.py [--out profiles/shift.md] [--reps 30] [--warmup 5]

One process, one engine, one session.  The standard utterance: a 617-frame mel through HiFi-GAN (157 952 samples at 22 050 Hz).
Timed, as host wall clock around complete synchronised calls, alternating: `mi355tts_hifigan_infer` on that mel (float row to the
host); `mi355tts_pitch` and `mi355tts_resample` (by 5 / 6) of its float row with device pointers; `mi355tts_shift` by 6 / 5 in the
PITCH mode (float row; normalised int16) and the TEMPO mode with device pointers, and in the PITCH mode with host pointers (the
copies are inside).  The library's own event-timed launch durations follow, per kernel.  The utterance of synthetic weights reads
as unvoiced, so the designed signal, tiled to the same length, is timed as well: its frames move.  For information only: no test
gates on a time."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

# (not measurements of this tool: how the host code was checked on the CPU)
STATIC_NOTES = """## Host sanitizers (CPU only)

The host side (`csrc/shift_forward.h`: argument checks, workspace carving, staging, delivery) and the kernels' index arithmetic run
under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program: the library's CPU-emulator flavour and
`tests/c_abi/shift_ragged.c` (both modes; a ragged batch of five rows, one empty and one shorter than a pitch hop; every output;
float and int16 input; a batch without a sample; each row again as its own batch-1 call and with its own positions fed back), all
compiled with the sanitizers and linked into one executable, no Python in the process:

    SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -g -O0"
    clang++ -x c++ -std=c++17 $SAN -Itests/hipemu/include -c larynx_amd/csrc/mi355tts.hip -o mi355tts.o
    clang++ -x c++ -std=c++17 $SAN -Itests/hipemu/include -c tests/hipemu/hipemu_runtime.cpp -o runtime.o
    clang -std=c99 $SAN -Iinclude -c tests/c_abi/shift_ragged.c -o main.o
    clang++ $SAN main.o mi355tts.o runtime.o -o shift_ragged_san -lpthread -lm -ldl && ./shift_ragged_san

Result, with the sanitizers' default options: the ten rows and "ok", exit status 0, no report from either sanitizer.
""".splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "shift.md"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first (INTEGRATION.md "Sharing a process with PyTorch")
    from larynx_amd import ffi
    from larynx_amd import hparams as HP
    from larynx_amd import synthetic
    from larynx_amd.engine import Engine
    from larynx_amd.resample import Resampler
    from larynx_amd.shift import PitchShifter
    from tests import pitch_np as P
    from tests import test_emu_shift as T

    eng = Engine(0)
    vhp = HP.HIFIGAN_HIGH
    voc = eng.load_hifigan(vhp, synthetic.make_hifigan_state_dict(vhp, seed=1234))
    frames = 617
    mel = eng.mel_from_numpy(np.random.default_rng(1).standard_normal((1, vhp.num_mels, frames)).astype(np.float32))
    row, _ = eng.hifigan_infer(voc, mel, want_float=True, want_int16=False)
    N = row.shape[1]
    up, down = 6, 5
    sh = PitchShifter(eng, 22050, ratio=(up, down))
    tempo = PitchShifter(eng, 22050, ratio=(up, down), tempo=True)
    rs = Resampler(eng, up, down)  # by down / up, on its own
    L = tempo.length(N)
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE
    designed = np.resize(P.designed_signal(), N).astype(np.float32)[None]
    dev_in = {"utterance": torch.from_numpy(row).cuda().contiguous(), "designed": torch.from_numpy(designed).cuda().contiguous()}
    out_f = torch.zeros((1, L), dtype=torch.float32, device="cuda")
    out_i = torch.zeros((1, L), dtype=torch.int16, device="cuda")
    F = sh.tracker.frames(N)
    planes = [torch.zeros((1, F), dtype=torch.float32, device="cuda") for _ in range(3)]

    def shift_dev(model, src, f32=True, normalize=False):
        return eng.shift_raw(model.model_id, dev_in[src].data_ptr(), None, [N], N, out_f.data_ptr() if f32 else None,
                             out_i.data_ptr() if normalize else None, L, ffi.PCM_NORMALIZE if normalize else ffi.PCM_SATURATE, flags=flags)

    calls = {
        "`mi355tts_hifigan_infer`, 617 frames, float row to the host": lambda: eng.hifigan_infer(voc, mel, want_float=True, want_int16=False),
        "pitch, three planes, device pointers": lambda: eng.pitch_raw(sh.tracker.model_id, dev_in["utterance"].data_ptr(), None, [N], N,
                                                                      *(p.data_ptr() for p in planes), None, F, flags),
        "resample by 5 / 6, float, device pointers": lambda: eng.resample_raw(rs.model_id, dev_in["utterance"].data_ptr(), None, [N], N, out_f.data_ptr(),
                                                                              None, L, 0, flags),
        "shift 6 / 5, PITCH mode, float, device pointers": lambda: shift_dev(sh, "utterance"),
        "shift 6 / 5, PITCH mode, normalised int16, device pointers": lambda: shift_dev(sh, "utterance", f32=False, normalize=True),
        "shift 6 / 5, TEMPO mode, float, device pointers": lambda: shift_dev(tempo, "utterance"),
        "shift 6 / 5, PITCH mode, float, device pointers, the designed signal": lambda: shift_dev(sh, "designed"),
        "shift 6 / 5, PITCH mode, float, host pointers": lambda: eng.shift(sh.model_id, row),
    }
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for i in range(args.warmup + args.reps):
        for k, fn in calls.items():  # alternating: every side sees the same machine state
            t0 = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t0
            del r
            if i >= args.warmup:
                times[k].append(dt)
    med = {k: statistics.median(v) for k, v in times.items()}
    voc_key = next(iter(calls))
    rows = [f"| {k} | {1e3 * med[k]:.3f} | {1e3 * min(v):.3f} | {1e3 * max(v):.3f} | {med[k] / med[voc_key]:.3f} |" for k, v in times.items()]

    # the library's own launch times (HIP events around every launch), per kernel
    eng.set_profiling(True)
    overhead_us = eng.profile_event_overhead_us()
    per_kernel, totals = {}, {}
    for k in list(calls)[:7]:
        calls[k]()
        eng.profile_reset()
        for _ in range(args.reps):
            calls[k]()
        totals[k] = sum(v["ms"] for v in eng.profile().values()) / args.reps
        per_kernel[k] = {name: (v["launches"] // args.reps, 1e3 * v["ms"] / args.reps) for cls in eng.profile_kernels().values() for name, v in cls.items()}
    eng.profile_reset()
    eng.set_profiling(False)
    kernel_rows = []
    for k in list(calls)[1:7]:
        cells = ", ".join(f"`{name.split('/')[0]}` {us:.1f}" + (f" ({n} launches)" if n > 1 else "") for name, (n, us) in per_kernel[k].items())
        kernel_rows.append(f"| {k} | {1e3 * totals[k]:.1f} | {cells} |")
    r = eng.shift(sh.model_id, designed[0], want_positions=T.S.lengths(N, up, down, 1024)[1], want_f0=F)
    moved = int((r["positions"] != T.S.anchors(len(r["positions"]), up, down, 1024)[1]).sum())

    # what the tests' checks measure on this device
    chain_rows = []
    for ratio in T.PITCH_RATIOS:
        proto, dev = T.check_chain(eng, ratio)
        chain_rows.append(f"| {ratio[0]} / {ratio[1]} | {100 * proto[0]:.1f} % / {100 * proto[1]:.1f} % / {100 * proto[2]:.2f} % | "
                          f"{100 * dev[0]:.1f} % / {100 * dev[1]:.1f} % / {100 * dev[2]:.2f} % |")
    T.check_exact_periods(eng)
    T.check_positions(eng)

    pk, sk = "pitch, three planes, device pointers", "shift 6 / 5, PITCH mode, float, device pointers"
    rk = "resample by 5 / 6, float, device pointers"
    lines = [
        "# Pitch shift and tempo on the device",
        "",
        f"`tools/shift_probe.py`, one process, one session; median of {args.reps} alternating repetitions after {args.warmup} warm-up rounds; host",
        f"wall clock around complete, synchronised calls.  The row is the HiFi-GAN output of a {frames}-frame mel ({N} samples, {F} pitch frames;",
        f"synthetic weights: it reads as unvoiced, so every s_k = a_k); the shifter is `PitchShifter(engine, 22050, ratio=(6, 5))`: N = 1024,",
        f"{len(r['positions'])} overlap-add frames, {L} stretched samples, resampled by 5 / 6 back to {N}.  \"The designed signal\" is tests/pitch_np.py's,",
        f"tiled to the same length: {moved} of its {len(r['positions'])} frames move by whole periods.  The last column is the call's median over the",
        "vocoder call's.  For information only: no test gates on a time.",
        "",
        "| call | median ms | min ms | max ms | / vocoder |",
        "|---|---|---|---|---|",
        *rows,
        "",
        f"The shift call against the two calls it contains: {1e3 * med[sk]:.3f} ms against {1e3 * med[pk]:.3f} + {1e3 * med[rk]:.3f} = "
        f"{1e3 * (med[pk] + med[rk]):.3f} ms for `mi355tts_pitch` + `mi355tts_resample` on the same row (two calls, two synchronisations;",
        "the resample call there reads the row itself, not its stretch).",
        "",
        f"Event-timed launches (HIP events around every launch, mean of {args.reps} calls, microseconds; an empty event pair costs {overhead_us:.1f} us here",
        f"and is included in every launch's figure; launches without a counted name are filed under `-`: the resampler's).  The vocoder call's",
        f"launches sum to {totals[voc_key]:.3f} ms.",
        "",
        "| call | all launches, us | per kernel, us |",
        "|---|---|---|",
        *kernel_rows,
        "",
        "Not measured: the kernels under rocprofv3, counters, other batch sizes, other ratios.",
        "",
        "## The tests' checks on the device",
        "",
        "tests/test_gpu_shift.py, PITCH mode on the designed signal (2.4 s): of the frames voiced in the input, the share still voiced in the",
        "delivered row / of those, the share whose f0 ratio lies within 2 % of up / down / the median relative error — read with the float64",
        "YIN oracle, for the float64 prototype on the host and for the device's row.  Positions and the overlap-add equal numpy bit for bit",
        "on every frame and sample; the exact-period rows (P = 100, 120, 97, 240 at 6/5, 4/5, 9/8, 55/49) are in phase on every frame",
        "and within 1 ulp of the input's own values on every interior sample.",
        "",
        "| ratio | float64 prototype | device |",
        "|---|---|---|",
        *chain_rows,
        "",
        *STATIC_NOTES,
    ]
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    eng.close()


if __name__ == "__main__":
    main()
