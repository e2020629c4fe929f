#!/usr/bin/env python3
"""Time `mi355tts_pitch` on the device next to the vocoder call whose output it reads and next to the float64 oracle on the host;
record how far the device's track lies from the oracle on the tests' signals, with the anchors and the decided shares.

    python tools/pitch_probe.py [--out profiles/pitch.md] [--reps 30] [--warmup 5]

One process, one engine, one session.  The standard utterance: a 617-frame mel through HiFi-GAN (157 952 samples at 22 050 Hz).
Timed, as host wall clock around complete synchronised calls, alternating: `mi355tts_hifigan_infer` on that mel (float row to
the host); `mi355tts_pitch` of its float row with the default tracker of `larynx_amd.pitch`, with host pointers (the copies are
inside) and with device pointers (torch tensors), the three planes alone and with the d' rows; the float64 oracle of
tests/pitch_np.py on the host.  The library's own event-timed launch duration follows.  For information only: no test gates on a
time."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

# (not measurements of this tool: what the CPU emulator gave for the same checks, and how the host code was checked on the CPU)
STATIC_NOTES = """## The same checks on the CPU emulator

`pytest tests/test_emu_pitch.py -s`: the emulator runs the kernel's own arithmetic with the host's `fmaf` and `log10f`.  Its d'
planes, f0 and periodicity equal the float32 restatement of tests/pitch_np.py bit for bit on all four signals (so the measured
value equals the anchor); only level_db differs (another `log10f`).

| signal | decided | voiced | f0 (relative) | periodicity | level_db | cmnd |
|---|---|---|---|---|---|---|
| designed, 22 050 Hz | 100.0 % | 71.4 % | 9.148e-08 | 2.005e-07 | 6.823e-06 (anchor 1.225e-05) | 1.754e-05 |
| designed, 16 000 Hz | 100.0 % | 71.8 % | 8.398e-08 | 4.561e-07 | 7.346e-06 (anchor 9.770e-06) | 1.523e-05 |
| ljspeech_high_short5 | 100.0 % | 0.0 % | - | 1.229e-07 | 9.232e-07 (anchor 2.098e-06) | 7.938e-07 |
| ljspeech_high_echo | 100.0 % | 0.0 % | - | 1.260e-07 | 1.343e-06 (anchor 1.790e-06) | 8.149e-07 |

## Host sanitizers (CPU only)

The host side (`csrc/pitch_forward.h`: argument checks, workspace carving, staging, delivery) and the kernel's index arithmetic
run under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program: the library's CPU-emulator flavour and
`tests/c_abi/pitch_ragged.c` (a ragged batch of five rows, one empty and one shorter than a hop, every output, float and int16
input, a batch without a frame, each row again as its own batch-1 call), all compiled with the sanitizers and linked into one
executable, no Python in the process:

    SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -g -O0"
    clang++ -x c++ -std=c++17 $SAN -Itests/hipemu/include -c larynx_amd/csrc/mi355tts.hip -o mi355tts.o
    clang++ -x c++ -std=c++17 $SAN -Itests/hipemu/include -c tests/hipemu/hipemu_runtime.cpp -o runtime.o
    clang -std=c99 $SAN -Iinclude -c tests/c_abi/pitch_ragged.c -o main.o
    clang++ $SAN main.o mi355tts.o runtime.o -o pitch_ragged_san -lpthread -lm -ldl && ./pitch_ragged_san

Result, with the sanitizers' default options: the five rows and "ok", exit status 0, no report from either sanitizer.
""".splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "pitch.md"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first (INTEGRATION.md "Sharing a process with PyTorch")
    from larynx_amd import ffi
    from larynx_amd import hparams as HP
    from larynx_amd import synthetic
    from larynx_amd.engine import Engine
    from larynx_amd.pitch import PitchTracker
    from tests import pitch_np as P
    from tests import test_emu_pitch as T

    eng = Engine(0)
    vhp = HP.HIFIGAN_HIGH
    voc = eng.load_hifigan(vhp, synthetic.make_hifigan_state_dict(vhp, seed=1234))
    frames = 617
    mel = eng.mel_from_numpy(np.random.default_rng(1).standard_normal((1, vhp.num_mels, frames)).astype(np.float32))
    row, _ = eng.hifigan_infer(voc, mel, want_float=True, want_int16=False)
    N = row.shape[1]
    tr = PitchTracker(eng, 22050)
    m, T1 = tr.model_id, tr.tau_max + 1
    F = tr.frames(N)
    dev_in = torch.from_numpy(row).cuda().contiguous()
    planes = [torch.zeros((1, F), dtype=torch.float32, device="cuda") for _ in range(3)]
    cm = torch.zeros((1, F, T1), dtype=torch.float32, device="cuda")
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE
    geom = dict(sample_rate=22050, hop=tr.hop, W=tr.window, tau_min=tr.tau_min, tau_max=tr.tau_max)
    calls = {
        "`mi355tts_hifigan_infer`, 617 frames, float row to the host": lambda: eng.hifigan_infer(voc, mel, want_float=True, want_int16=False),
        "pitch, three planes, host pointers": lambda: eng.pitch(m, row),
        "pitch, three planes and d', host pointers": lambda: eng.pitch(m, row, want_cmnd=T1),
        "pitch, three planes, device pointers": lambda: eng.pitch_raw(m, dev_in.data_ptr(), None, [N], N, *(p.data_ptr() for p in planes), None, F, flags),
        "pitch, three planes and d', device pointers": lambda: eng.pitch_raw(m, dev_in.data_ptr(), None, [N], N, *(p.data_ptr() for p in planes),
                                                                              cm.data_ptr(), F, flags),
        "the float64 oracle on the host (numpy)": lambda: P.track(row[0], theta=tr.threshold, interpolate=True, dtype=np.float64, **geom),
    }
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for i in range(args.warmup + args.reps):
        for k, fn in calls.items():  # alternating: every side sees the same machine state
            if k.startswith("the float64") and not args.warmup <= i < args.warmup + 3:
                continue  # (seconds per run: three repetitions are enough)
            t0 = time.perf_counter()
            r = fn()
            dt = time.perf_counter() - t0
            del r
            if i >= args.warmup:
                times[k].append(dt)
    med = {k: statistics.median(v) for k, v in times.items()}
    voc_key = next(iter(calls))
    rows = [f"| {k} | {1e3 * med[k]:.3f} | {1e3 * min(v):.3f} | {1e3 * max(v):.3f} | {med[k] / med[voc_key]:.3f} |" for k, v in times.items()]

    # the library's own launch times (HIP events around every launch)
    eng.set_profiling(True)
    overhead_us = eng.profile_event_overhead_us()
    totals = {}
    for k in ("pitch, three planes, device pointers", "pitch, three planes and d', device pointers", voc_key):
        calls[k]()
        eng.profile_reset()
        for _ in range(args.reps):
            calls[k]()
        totals[k] = sum(v["ms"] for v in eng.profile().values()) / args.reps
    eng.profile_reset()
    eng.set_profiling(False)
    pk, ck = list(totals)[:2]
    terms = F * tr.window * tr.tau_max
    voiced = int((eng.pitch(m, row)["f0"] > 0).sum())

    # the deviations of the tests' checks, on this device
    dev_rows = []
    cases = [("designed, 22 050 Hz", lambda: T.check_designed(eng)), ("designed, 16 000 Hz", lambda: T.check_designed(eng, T.GEOM16)),
             ("ljspeech_high_short5", lambda: T.check_golden(eng, "ljspeech_high_short5")), ("ljspeech_high_echo", lambda: T.check_golden(eng, "ljspeech_high_echo"))]
    for name, fn in cases:
        o, ok, fig = fn()
        cells = " | ".join("-" if fig[k] is None else f"{fig[k][0]:.3e} / {fig[k][1]:.3e} / {fig[k][2]:.3e}" for k in ("f0 (relative)", "periodicity", "level_db", "cmnd"))
        dev_rows.append(f"| {name} | {len(ok)} | {100 * ok.mean():.1f} % | {100 * o['voiced'].mean():.1f} % | {cells} |")
    T.check_exact_periods(eng)

    lines = [
        "# YIN pitch tracker on the device",
        "",
        f"`tools/pitch_probe.py`, one process, one session; median of {args.reps} alternating repetitions after {args.warmup} warm-up rounds; host",
        f"wall clock around complete, synchronised calls.  The row is the HiFi-GAN output of a {frames}-frame mel ({N} samples: {F} pitch frames, of",
        f"which {voiced} read as voiced — synthetic weights); the tracker is `PitchTracker(engine, 22050)`: lags {tr.tau_min} .. {tr.tau_max}, window",
        f"{tr.window}, hop {tr.hop}, i.e. {terms / 1e6:.0f} M difference terms a call.  The last column is the call's median over the vocoder call's.",
        "For information only: no test gates on a time.",
        "",
        "| call | median ms | min ms | max ms | / vocoder |",
        "|---|---|---|---|---|",
        *rows,
        "",
        f"Event-timed launch (HIP events around the launch, mean of {args.reps} calls; an empty event pair costs {overhead_us:.1f} us here, included):",
        f"`pitch_kernel` takes {1e3 * totals[pk]:.1f} us for the three planes and {1e3 * totals[ck]:.1f} us with the d' rows, against {totals[voc_key]:.3f} ms",
        f"for the vocoder call's launches ({100 * totals[pk] / totals[voc_key]:.2f} % of it).  With the event pair taken off, {terms / 1e6:.0f} M terms in",
        f"{1e3 * totals[pk] - overhead_us:.1f} us are {terms / max(1e3 * totals[pk] - overhead_us, 1e-9) / 1e6:.2f} T terms/s (a term: one subtraction, one fma, one 4-byte",
        "LDS read).  Not measured: the kernel under rocprofv3, counters, other batch sizes.",
        "",
        "## Deviations from the float64 oracle on the device",
        "",
        "The tests' checks (tests/test_gpu_pitch.py), on the decided frames: measured / anchor (the float32 restatement's own deviation) /",
        "the smallest bound applied (16 x the anchor, never below 4 float32 ulps of the value).  The exact-period rows (P = 45, 64, 127,",
        "128, 129, 320, 441) gave periodicity 1.0, f0 = 22050 / P and d'(P) = 0 bit for bit on all 18 interior frames each.",
        "",
        "| signal | frames | decided | voiced | f0 (relative) | periodicity | level_db | cmnd |",
        "|---|---|---|---|---|---|---|---|",
        *dev_rows,
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
