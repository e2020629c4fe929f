#!/usr/bin/env python3
"""Time `mi355tts_loudness` on the device next to the vocoder call that feeds it, next to `mi355tts_resample` and next to the
float64 oracle on the host, and record its deviations.

    python tools/loudness_probe.py [--out profiles/loudness.md] [--reps 30] [--warmup 5]

One process, one engine, one session.  The standard utterance: a 617-frame mel through HiFi-GAN (157 952 samples at 22 050 Hz).
Timed, as host wall clock around complete synchronised calls, alternating: `mi355tts_hifigan_infer` on that mel (float row to
the host); `mi355tts_loudness` of its float row, measuring only and delivering int16 at -16 LUFS, with host pointers (the copies
are inside) and with device pointers (torch tensors); `mi355tts_resample` of the row to 16 000 Hz with device pointers; the
oracle of tests/loudness_np.py (scipy.signal.lfilter twice, blocks, gates) on the host.  The library's own event-timed launch
durations per kernel follow, then the deviations of the tests' cases.  For information only: no test gates on a time."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

# (not a measurement of this tool: how the host code was checked on the CPU, kept with the figures)
SANITIZER_NOTE = """## Host sanitizers (CPU only)

The host side (`csrc/loudness_forward.h`: argument checks, workspace carving, staging, delivery) and the kernels' index arithmetic
run under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program: the library's CPU-emulator flavour and
`tests/c_abi/loudness_ragged.c` (the ragged batch of eight rows, every output, float and int16 input, each row again as its own
batch-1 call), all compiled with the sanitizers and linked into one executable, no Python in the process:

    SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -g -O1"
    clang++ -x c++ -std=c++17 $SAN -Itests/hipemu/include -c larynx_amd/csrc/mi355tts.hip -o mi355tts.o
    clang++ -x c++ -std=c++17 $SAN -Itests/hipemu/include -c tests/hipemu/hipemu_runtime.cpp -o runtime.o
    clang -std=c99 $SAN -Iinclude -c tests/c_abi/loudness_ragged.c -o main.o
    clang++ $SAN main.o mi355tts.o runtime.o -o loudness_ragged_san -lpthread -lm -ldl && ./loudness_ragged_san

(The whole translation unit is instrumented: at -O1 that compile takes tens of minutes, at -O0 about one.)  Result,
with the sanitizers' default options: the eight rows and "ok", exit status 0, no report from either sanitizer.
""".splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "loudness.md"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first (INTEGRATION.md "Sharing a process with PyTorch")
    from larynx_amd import ffi
    from larynx_amd import hparams as HP
    from larynx_amd import synthetic
    from larynx_amd.engine import Engine
    from larynx_amd.loudness import Loudness
    from larynx_amd.resample import Resampler
    from tests import loudness_np as L
    from tests import test_emu_loudness as T

    eng = Engine(0)
    vhp = HP.HIFIGAN_HIGH
    voc = eng.load_hifigan(vhp, synthetic.make_hifigan_state_dict(vhp, seed=1234))
    frames = 617
    mel = eng.mel_from_numpy(np.random.default_rng(1).standard_normal((1, vhp.num_mels, frames)).astype(np.float32))
    row, _ = eng.hifigan_infer(voc, mel, want_float=True, want_int16=False)
    N = row.shape[1]
    dev_in = torch.from_numpy(row).cuda().contiguous()
    oi = torch.zeros((1, N), dtype=torch.int16, device="cuda")
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE
    m = Loudness(eng, 22050).model_id
    rs = Resampler(eng, 22050, 16000)
    of16 = torch.zeros((1, rs.length(N)), dtype=torch.float32, device="cuda")
    nan = float("nan")
    calls = {
        "`mi355tts_hifigan_infer`, 617 frames, float row to the host": lambda: eng.hifigan_infer(voc, mel, want_float=True, want_int16=False),
        "loudness, measure, host pointers": lambda: eng.loudness(m, row),
        "loudness, -16 LUFS int16, host pointers": lambda: eng.loudness(m, row, target=-16.0, ceiling=T.CEILING, want_int16=True),
        "loudness, measure, device pointers": lambda: eng.loudness_raw(m, dev_in.data_ptr(), None, [N], N, nan, 1.0, 30.0, flags=flags),
        "loudness, -16 LUFS int16, device pointers": lambda: eng.loudness_raw(m, dev_in.data_ptr(), None, [N], N, -16.0, T.CEILING, 30.0, None,
                                                                               oi.data_ptr(), N, None, flags),
        "`mi355tts_resample` -> 16 000, float, device pointers": lambda: eng.resample_raw(rs.model_id, dev_in.data_ptr(), None, [N], N,
                                                                                          of16.data_ptr(), None, of16.shape[1], ffi.PCM_SATURATE, flags),
        "the float64 oracle on the host (scipy.signal.lfilter twice, blocks, gates)": lambda: L.oracle(row[0], 22050),
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
    kernel_rows = []
    totals = {}
    for k in ("loudness, -16 LUFS int16, device pointers", "`mi355tts_resample` -> 16 000, float, device pointers", voc_key):
        calls[k]()
        eng.profile_reset()
        for _ in range(args.reps):
            calls[k]()
        totals[k] = sum(v["ms"] for v in eng.profile().values()) / args.reps
        if k.startswith("loudness"):
            for name, acc in sorted(eng.profile_kernels()["elementwise"].items()):
                kernel_rows.append(f"| {name.rsplit('/', 1)[0]} | {acc['launches'] // args.reps} | {1e3 * acc['ms'] / args.reps:.1f} |")
    eng.profile_reset()
    eng.set_profiling(False)
    lk, rk = list(totals)[:2]

    dev_rows = []  # the tests' cases against the float64 oracle
    cases = [(f"voiced, N = {n}", T.row(n), 22050) for n in (8820, 11025, 30000, 60000)]
    cases += [("997 Hz tone, 2 s", L.tone(96000, 48000), 48000), ("997 Hz tone, 2 s", L.tone(44100, 22050), 22050),
              ("1 s at 0.5, 2 s at 1e-4", T.gated_signal(1e-4), 22050), ("1 s at 0.5, 2 s at 0.05", T.gated_signal(0.05), 22050)]
    for what, x, fs in cases:
        w64, _, l64 = L.oracle(x, fs)
        w32, _, l32 = L.restate_f32(x, fs)
        r = eng.loudness(T.meter(eng, fs).model_id, x, want_weighted=True)
        dev_rows.append(f"| {what} | {fs} | {np.abs(r['weighted'] - w64).max():.2e} | {np.abs(w32 - w64).max():.2e} | {l64:.4f} | "
                        f"{abs(float(r['lufs'][0]) - l64):.2e} | {abs(float(l32) - l64):.2e} |")

    lines = [
        "# Loudness on the device: BS.1770 integrated loudness and gain-to-target delivery",
        "",
        f"`tools/loudness_probe.py`, one process, one session; median of {args.reps} alternating repetitions after {args.warmup} warm-up rounds; host",
        f"wall clock around complete, synchronised calls.  The row is the HiFi-GAN output of a {frames}-frame mel ({N} samples); the last",
        "column is the call's median over the vocoder call's.  For information only: no test gates on a time.",
        "",
        "| call | median ms | min ms | max ms | / vocoder |",
        "|---|---|---|---|---|",
        *rows,
        "",
        f"Event-timed launches (HIP events around every launch, mean of {args.reps} calls; an empty event pair costs {overhead_us:.1f} us here, included",
        f"per launch): the delivering loudness call's six launches sum to {1e3 * totals[lk]:.1f} us, the resample call's one to {1e3 * totals[rk]:.1f} us, the vocoder",
        f"call's to {totals[voc_key]:.3f} ms ({100 * totals[lk] / totals[voc_key]:.1f} % and {100 * totals[rk] / totals[voc_key]:.1f} % of it).",
        "",
        "| kernel | launches | us per call |",
        "|---|---|---|",
        *kernel_rows,
        "",
        "## Deviations from the float64 oracle",
        "",
        "Cases and rule of the tests (tests/test_emu_loudness.py): every K-weighted sample and the integrated value may lie 16 x as far from the",
        "float64 oracle as the float32 restatement of the recurrence does on the same input (L: never tighter than 4 ulp, never looser than 0.1 LU).",
        "",
        "| signal | rate | device, samples | float32 restatement, samples | L (oracle) | device, LU | restatement, LU |",
        "|---|---|---|---|---|---|---|",
        *dev_rows,
        "",
        *SANITIZER_NOTE,
    ]
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines))
    print("\n".join(lines))
    eng.close()


if __name__ == "__main__":
    main()
