#!/usr/bin/env python3
"""Time `mi355tts_resample` on the device next to the vocoder call that feeds it and next to a host polyphase resampler, and
record its deviations.

    python tools/resample_probe.py [--out profiles/resample.md] [--reps 30] [--warmup 5]

One process, one engine, one session.  The standard utterance: a 617-frame mel through HiFi-GAN (157 952 samples at 22 050 Hz).
Timed, as host wall clock around complete synchronised calls, alternating: `mi355tts_hifigan_infer` on that mel (float row to
the host); `mi355tts_resample` of its float row to 8 000, 16 000 and 48 000 Hz, float-only and MI355TTS_PCM_NORMALIZE (int16
only), with host pointers (the copies are inside) and with device pointers (torch tensors); `scipy.signal.resample_poly` of the
same row with the same prototype on the host (float64, its own arithmetic).  The library's own event-timed launch durations of
the device-pointer calls follow, then the deviations of the tests' parity cases.  For information only: no test gates on a time."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "resample.md"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first (INTEGRATION.md "Sharing a process with PyTorch")
    from scipy import signal

    from larynx_amd import ffi
    from larynx_amd import hparams as HP
    from larynx_amd import synthetic
    from larynx_amd.engine import Engine
    from larynx_amd.resample import Resampler
    from tests import resample_np as R

    eng = Engine(0)
    vhp = HP.HIFIGAN_HIGH
    voc = eng.load_hifigan(vhp, synthetic.make_hifigan_state_dict(vhp, seed=1234))
    frames = 617
    mel = eng.mel_from_numpy(np.random.default_rng(1).standard_normal((1, vhp.num_mels, frames)).astype(np.float32))
    row, _ = eng.hifigan_infer(voc, mel, want_float=True, want_int16=False)
    N = row.shape[1]
    dev_in = torch.from_numpy(row).cuda().contiguous()
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE
    calls = {"`mi355tts_hifigan_infer`, 617 frames, float row to the host": lambda: eng.hifigan_infer(voc, mel, want_float=True, want_int16=False)}
    keep = []
    for rate in (8000, 16000, 48000):
        rs = Resampler(eng, 22050, rate)
        n_out = rs.length(N)
        of = torch.zeros((1, n_out), dtype=torch.float32, device="cuda")
        oi = torch.zeros((1, n_out), dtype=torch.int16, device="cuda")
        keep += [of, oi]
        m = rs.model_id
        calls[f"-> {rate}, float, host pointers"] = lambda m=m: eng.resample(m, row)
        calls[f"-> {rate}, NORMALIZE, host pointers"] = lambda m=m: eng.resample(m, row, want_float=False, want_int16=True, normalize=True)
        calls[f"-> {rate}, float, device pointers"] = lambda m=m, of=of, n_out=n_out: eng.resample_raw(
            m, dev_in.data_ptr(), None, [N], N, of.data_ptr(), None, n_out, ffi.PCM_SATURATE, flags)
        calls[f"-> {rate}, NORMALIZE, device pointers"] = lambda m=m, oi=oi, n_out=n_out: eng.resample_raw(
            m, dev_in.data_ptr(), None, [N], N, None, oi.data_ptr(), n_out, ffi.PCM_NORMALIZE, flags)
        win = rs.taps.astype(np.float64) / rs.up
        calls[f"-> {rate}, `scipy.signal.resample_poly` on the host (float64)"] = lambda rs=rs, win=win: signal.resample_poly(
            row[0].astype(np.float64), rs.up, rs.down, window=win)
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

    def share(what):
        v = [100.0 * med[k] / med[voc_key] for k in med if what in k]
        return f"{min(v):.1f} - {max(v):.1f} %"

    # the library's own launch times: the device-pointer calls only, per rate and mode
    launch_rows = []
    eng.set_profiling(True)
    for k, fn in calls.items():
        if "device pointers" not in k:
            continue
        fn()
        eng.profile_reset()
        for _ in range(args.reps):
            fn()
        p = eng.profile()["elementwise"]
        launch_rows.append(f"| {k} | {p['launches'] // args.reps} | {1e3 * p['ms'] / args.reps:.1f} |")
    eng.profile_reset()
    eng.hifigan_infer(voc, mel, want_float=True, want_int16=False)
    voc_ms = sum(v["ms"] for v in eng.profile().values())
    overhead_us = eng.profile_event_overhead_us()
    eng.set_profiling(False)

    dev_rows = []  # the parity cases of the tests: tone plus seeded noise against the float64 oracle
    for rate, (up, down) in R.RATIOS.items():
        taps, _ = R.design(up, down)
        m = eng.load_resampler(taps, up, down)
        for n in (257, 700, 1500):
            x = R.tone_noise(n)
            y = R.oracle(x, taps, up, down)
            err = float(np.abs(eng.resample(m, x)[0] - y).max())
            e32 = float(np.abs(R.restate_f32(x, taps, up, down) - y).max())
            bound = R.a_priori_bound(taps, up, float(np.abs(x).max()))
            dev_rows.append(f"| {rate} | {up} / {down} | {n} | {err:.2e} | {e32:.2e} | {err / e32:.2f} | {bound:.2e} |")

    lines = [
        "# Resampling on the device: 22 050 Hz rows to 8 / 16 / 48 kHz",
        "",
        f"`tools/resample_probe.py`, one process, one session; median of {args.reps} alternating repetitions after {args.warmup} warm-up rounds; host",
        f"wall clock around complete, synchronised calls.  The row is the HiFi-GAN output of a {frames}-frame mel ({N} samples); the last",
        "column is the call's median over the vocoder call's.  For information only: no test gates on a time.",
        "",
        "| call | median ms | min ms | max ms | / vocoder |",
        "|---|---|---|---|---|",
        *rows,
        "",
        f"Of the vocoder call: {share('device pointers')} with device pointers, {share('host pointers')} with host pointers, {share('scipy')} for the host resampler.",
        "",
        f"Event-timed launches of the device-pointer calls (mean of {args.reps} calls; an empty event pair costs {overhead_us:.1f} us here, included",
        f"per launch); the vocoder call's launches sum to {voc_ms:.3f} ms under the same clock:",
        "",
        "| call | launches | us per call |",
        "|---|---|---|",
        *launch_rows,
        "",
        "## Deviations from the float64 oracle",
        "",
        "Cases and rule of the parity tests (tests/test_emu_resample.py): tone plus seeded noise, |x| <= 1; the device may lie 16 x the float32",
        "restatement's own error from the oracle, never above T * 2^-24 * (worst-phase sum of abs taps) * max|x|.",
        "",
        "| rate out | up / down | N | device | float32 restatement | ratio | a-priori bound |",
        "|---|---|---|---|---|---|---|",
        *dev_rows,
        "",
    ]
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines))
    print("\n".join(lines))
    eng.close()


if __name__ == "__main__":
    main()
