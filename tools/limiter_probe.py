#!/usr/bin/env python3
"""Time `mi355tts_limit` on the device next to the vocoder call that feeds it, next to `mi355tts_loudness` and next to the float64
oracle on the host; record how far a limited row's true peak sits above the ceiling, and how often the single gain's cap binds on
the golden utterances.

    python tools/limiter_probe.py [--out profiles/limiter.md] [--reps 30] [--warmup 5]

One process, one engine, one session.  The standard utterance: a 617-frame mel through HiFi-GAN (157 952 samples at 22 050 Hz).
Timed, as host wall clock around complete synchronised calls, alternating: `mi355tts_hifigan_infer` on that mel (float row to
the host); `mi355tts_loudness` of its float row delivering int16 at -16 LUFS; `mi355tts_limit` of the row as a meter call and
limiting to int16, with host pointers (the copies are inside) and with device pointers (torch tensors); the whole
`Loudness.normalize_limited`; the float64 oracle of tests/limiter_np.py on the host.  The library's own event-timed launch
durations per kernel follow.  For information only: no test gates on a time."""
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

The host side (`csrc/limiter_forward.h`: argument checks, workspace carving, staging, delivery) and the kernels' index arithmetic
run under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program: the library's CPU-emulator flavour and
`tests/c_abi/limit_ragged.c` (a ragged batch of eight rows, two of them empty, a gain per row, every output, float and int16
input, a meter call, a batch of empty rows, each row again as its own batch-1 call), all compiled with the sanitizers and linked
into one executable, no Python in the process:

    SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -g -O0"
    clang++ -x c++ -std=c++17 $SAN -Itests/hipemu/include -c larynx_amd/csrc/mi355tts.hip -o mi355tts.o
    clang++ -x c++ -std=c++17 $SAN -Itests/hipemu/include -c tests/hipemu/hipemu_runtime.cpp -o runtime.o
    clang -std=c99 $SAN -Iinclude -c tests/c_abi/limit_ragged.c -o main.o
    clang++ $SAN main.o mi355tts.o runtime.o -o limit_ragged_san -lpthread -lm -ldl && ./limit_ragged_san

Result, with the sanitizers' default options: the eight rows and "ok", exit status 0, no report from either sanitizer.
""".splitlines()


def cap_binding_rows(target=-16.0, ceiling=10 ** (-1 / 20)):
    """The golden utterances (the reference's own float rows): does ceiling / max|x| cap the gain the target asks for?"""
    from tests import loudness_np as L
    from tests.golden_util import CASES, load_batch8, load_case

    rows = [(n, np.asarray(load_case(n)["wav"], np.float32)) for n in CASES]
    rows += [(f"batch8[{i}]", np.asarray(w, np.float32)) for i, w in enumerate(load_batch8()["wav"])]
    out, binds = [], 0
    for name, w in rows:
        l, pk = L.oracle(w, 22050)[2], float(np.abs(w).max())
        g = 10 ** ((target - l) / 20)
        b = g * pk > ceiling
        binds += int(b)
        out.append(f"| {name} | {len(w)} | {l:.2f} | {pk:.3f} | {20 * np.log10(pk) - l:.1f} | {20 * np.log10(g):+.1f} | {'yes' if b else 'no'} |")
    return out, binds, len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "limiter.md"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first (INTEGRATION.md "Sharing a process with PyTorch")
    from larynx_amd import ffi
    from larynx_amd import hparams as HP
    from larynx_amd import synthetic
    from larynx_amd.engine import Engine
    from larynx_amd.limiter import Limiter
    from larynx_amd.loudness import Loudness
    from tests import limiter_np as M
    from tests import loudness_np as L
    from tests import test_emu_limiter as T

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
    meter = Loudness(eng, 22050)
    lim = Limiter(eng, 22050)
    m, lm = meter.model_id, lim.model_id
    l0 = float(meter.measure(row)[0])
    g = np.array([10 ** ((-16.0 - l0) / 20)], np.float32)
    tp0 = float(lim.true_peak(row)[0])
    calls = {
        "`mi355tts_hifigan_infer`, 617 frames, float row to the host": lambda: eng.hifigan_infer(voc, mel, want_float=True, want_int16=False),
        "`mi355tts_loudness`, -16 LUFS int16, host pointers": lambda: eng.loudness(m, row, target=-16.0, ceiling=T.CEILING, want_int16=True),
        "limit, meter call, host pointers": lambda: eng.limit(lm, row),
        "limit, int16, host pointers": lambda: eng.limit(lm, row, gain=g, ceiling=T.CEILING, want_int16=True),
        "limit, meter call, device pointers": lambda: eng.limit_raw(lm, dev_in.data_ptr(), None, [N], N, None, 1.0, flags=flags),
        "limit, int16, device pointers": lambda: eng.limit_raw(lm, dev_in.data_ptr(), None, [N], N, g, T.CEILING, None, oi.data_ptr(), N, None, flags),
        "`Loudness.normalize_limited`, -16 LUFS int16, host pointers (measure, limit, measure[, limit])":
            lambda: meter.normalize_limited(row, target=-16.0, limiter=lim),
        "the float64 oracle of one limiter pass on the host (numpy)": lambda: M.oracle(row[0], g[0], T.CEILING, lim.oversample, lim.taps, lim.lookahead,
                                                                                         lim.release, lim.window),
    }
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for i in range(args.warmup + args.reps):
        for k, fn in calls.items():  # alternating: every side sees the same machine state
            if k.startswith("the float64") and i >= args.warmup + 3:
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

    # the library's own launch times (HIP events around every launch), per kernel
    eng.set_profiling(True)
    overhead_us = eng.profile_event_overhead_us()
    kernel_rows = []
    totals = {}
    for k in ("limit, int16, device pointers", "limit, meter call, device pointers", "`mi355tts_loudness`, -16 LUFS int16, host pointers", voc_key):
        calls[k]()
        eng.profile_reset()
        for _ in range(args.reps):
            calls[k]()
        totals[k] = sum(v["ms"] for v in eng.profile().values()) / args.reps
        if k == "limit, int16, device pointers":
            for name, acc in sorted(eng.profile_kernels()["elementwise"].items()):
                kernel_rows.append(f"| {name.rsplit('/', 1)[0]} | {acc['launches'] // args.reps} | {1e3 * acc['ms'] / args.reps:.1f} |")
    eng.profile_reset()
    eng.set_profiling(False)
    lk, mk, ldk = list(totals)[:3]

    # how far a limited row's true peak sits above the ceiling (a measurement, not a guarantee of the design)
    over_rows = []
    cfg = T.config(eng)
    signals = [("0.9 sin(2 pi n / 4 + pi / 4), 4000 samples", M.intersample(4000), 1.0, 0.5),
               ("tone plus clicks, 4 s", M.tone_with_clicks(4 * 22050), 12.0, T.CEILING),
               ("voiced with clicks at the seams, 9000 samples", T.seam_row(), T.GAIN, T.CEILING),
               ("voiced, 60 000 samples", T.row(T.LONG), T.GAIN, T.CEILING),
               ("the standard utterance at the gain -16 LUFS asks for", row[0], float(g[0]), T.CEILING)]
    for what, x, gain, ceiling in signals:
        r = eng.limit(cfg.model_id, x, gain=gain, ceiling=ceiling, want_float=True)
        tp_in = float(r["true_peak"][0]) * gain
        tp_out = float(eng.limit(cfg.model_id, r["f32"])["true_peak"][0])
        c32 = float(np.float32(ceiling))
        over_rows.append(f"| {what} | {gain:.3f} | {tp_in:.4f} | {c32:.6f} | {np.abs(r['f32']).max():.6f} | {tp_out:.6f} | "
                         f"{20 * np.log10(tp_out / c32):+.4f} | {r['min_gain'][0]:.4f} |")

    cap_rows, binds, total = cap_binding_rows()
    after = float(meter.measure(meter.normalize_limited(row, target=-16.0, limiter=lim))[0])
    lines = [
        "# True-peak meter and look-ahead limiter on the device",
        "",
        f"`tools/limiter_probe.py`, one process, one session; median of {args.reps} alternating repetitions after {args.warmup} warm-up rounds; host",
        f"wall clock around complete, synchronised calls.  The row is the HiFi-GAN output of a {frames}-frame mel ({N} samples, {l0:.2f} LUFS, true",
        f"peak {tp0:.4f}; `normalize_limited` delivers it at {after:.3f} LUFS); the last column is the call's median over the vocoder call's.  For",
        "information only: no test gates on a time.",
        "",
        "| call | median ms | min ms | max ms | / vocoder |",
        "|---|---|---|---|---|",
        *rows,
        "",
        f"Event-timed launches (HIP events around every launch, mean of {args.reps} calls; an empty event pair costs {overhead_us:.1f} us here, included",
        f"per launch): the limiting call's six launches sum to {1e3 * totals[lk]:.1f} us, the meter call's two to {1e3 * totals[mk]:.1f} us, the delivering",
        f"loudness call's six to {1e3 * totals[ldk]:.1f} us, the vocoder call's to {totals[voc_key]:.3f} ms ({100 * totals[lk] / totals[voc_key]:.1f} %, "
        f"{100 * totals[mk] / totals[voc_key]:.1f} % and {100 * totals[ldk] / totals[voc_key]:.1f} % of it).",
        "",
        "| kernel | launches | us per call |",
        "|---|---|---|",
        *kernel_rows,
        "",
        "## The true peak of limited rows",
        "",
        "A limited row's SAMPLE peak never passes the ceiling (the clamp).  Its TRUE peak is read here by a meter call on the delivered float",
        "row: the curve is smooth, not constant, so the interpolated output is not the interpolated input times the curve, and the true",
        "peak may sit a little above the ceiling.  A measurement on these signals (os 4, la 33, 50 ms release), not a guarantee of the design.",
        "",
        "| signal | gain | true peak asked for | ceiling | sample peak out | true peak out | dB over the ceiling | smallest gain |",
        "|---|---|---|---|---|---|---|---|",
        *over_rows,
        "",
        "## How often the single gain's cap binds on the golden utterances",
        "",
        "The reference's own float rows of tests/golden (synthetic weights: these are not voices anybody recorded), float64 oracle, target",
        f"-16 LUFS under -1 dBFS: the cap `ceiling / max|x|` binds on {binds} of {total}.  Their peak-to-loudness ratio is 7 - 11 dB, under the 13 - 20 dB of",
        "recorded speech, so on these rows `normalize_limited` equals `normalize`; the limiter earns its place on rows like the tests'",
        "tone-plus-clicks row (-28.5 LUFS delivered by one gain, -16.0 through the limiter) and on real voices, which this repository has none of.",
        "",
        "| utterance | samples | LUFS | peak | peak - LUFS, dB | gain asked for, dB | cap binds |",
        "|---|---|---|---|---|---|---|",
        *cap_rows,
        "",
        *SANITIZER_NOTE,
    ]
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))
    eng.close()


if __name__ == "__main__":
    main()
