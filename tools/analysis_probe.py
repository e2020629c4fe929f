#!/usr/bin/env python3
"""Time the mel analysis call on the device next to restatements of the same arithmetic, and record its deviations.

    python tools/analysis_probe.py [--out profiles/analysis.md] [--reps 30] [--warmup 5]

One process, one engine.  Timed: `Engine.mel_from_audio` (host float32 waveform in, the mel left on the device: the copy of the
waveform to the device is inside, the call returns after its stream has drained) at B = 1 for 620 frames and at B = 8 ragged;
`mel_from_audio_raw` on a torch tensor already on the device; a torch restatement on the device (index gather, rfft, matmul,
log: eager kernels, synchronised) and the float32 numpy restatement (tests/analysis_np.py) on the host CPU.  The repetitions
alternate, every figure comes with its minimum and maximum.  For information only: no test gates on a time.

The second table holds the deviations of the device from the float64 oracle on the tests' cases, under the tests' metrics, next
to the float32 restatement's (the anchors)."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def speechlike(n, seed):
    """A deterministic signal with a moving harmonic structure and a noise floor, peak 0.9."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 22050.0
    f0 = 120.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t + seed)
    phase = 2 * np.pi * np.cumsum(f0) / 22050.0
    x = sum(np.sin(k * phase) / k for k in range(1, 24)) * (0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t)) + 0.01 * rng.randn(n)
    return (0.9 * x / np.abs(x).max()).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "analysis.md"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first (INTEGRATION.md "Sharing a process with PyTorch")
    from larynx_amd import ffi
    from larynx_amd.audio import ljspeech_audio_settings, mel_basis
    from larynx_amd.engine import Engine
    from tests import analysis_np as A
    from tests import test_emu_analysis as T

    eng = Engine(0)
    s = ljspeech_audio_settings()
    basis = mel_basis(22050, 1024, 80, 0.0, 8000)
    model = eng.load_analysis(basis, "hifigan")
    one = speechlike(620 * 256, 1)[None]
    lens = (620 * 256, 97 * 256 + 13, 411 * 256, 385, 256 * 256 + 255, 530 * 256, 33 * 256, 600 * 256 + 100)
    ragged = np.zeros((8, max(lens)), np.float32)
    for b, n in enumerate(lens):
        ragged[b, :n] = speechlike(n, 10 + b)
    t_basis = torch.from_numpy(basis).cuda()
    t_win = torch.from_numpy(A.window("hifigan", np.float32)).cuda()

    def torch_restatement(dev, samples):
        out = []
        for b, n in enumerate(samples):
            F = A.frame_count("hifigan", n)
            idx = 256 * torch.arange(F, device="cuda")[:, None] + torch.arange(1024, device="cuda")[None, :] - 384
            idx = torch.where(idx < 0, -idx, torch.where(idx >= n, 2 * (n - 1) - idx, idx))
            spec = torch.fft.rfft(dev[b][idx] * t_win, dim=1)
            mag = torch.sqrt(spec.real * spec.real + spec.imag * spec.imag + 1e-9)
            amp = t_basis @ mag.T
            voc = torch.log(torch.clamp(amp, min=1e-5))
            raw = torch.log10(torch.clamp(amp, min=1e-5))
            raw = torch.clamp((2.0 * s.max_norm) * (((raw - s.ref_level_db) - s.min_level_db) / (-s.min_level_db)) - s.max_norm, -s.max_norm, s.max_norm)
            out.append((raw, voc))
        torch.cuda.synchronize()
        return out

    rows = []
    for tag, wav, samples in (("B = 1, 620 frames", one, (one.shape[1],)), ("B = 8 ragged, " + "/".join(str(n // 256) for n in lens) + " frames", ragged, lens)):
        dev = torch.from_numpy(wav).cuda().contiguous()
        torch.cuda.synchronize()
        calls = {
            "`mi355tts_mel_from_audio`, host waveform in (one launch + the copy)": lambda: eng.mel_from_audio(model, wav, samples=samples, audio_settings=s),
            "`mi355tts_mel_from_audio`, waveform already on the device": lambda: eng.mel_from_audio_raw(model, dev.data_ptr(), None, samples, wav.shape[1], s, flags=ffi.IN_DEVICE),
            "torch restatement on the device (eager, synchronised)": lambda: torch_restatement(dev, samples),
            "float32 numpy restatement on the host CPU": lambda: [A.analyze(wav[b, :n], basis, "hifigan", s, np.float32) for b, n in enumerate(samples)],
        }
        times = {k: [] for k in calls}
        for i in range(args.warmup + args.reps):
            for k, fn in calls.items():  # alternating: every side sees the same machine state
                t0 = time.perf_counter()
                r = fn()
                dt = time.perf_counter() - t0
                del r
                if i >= args.warmup:
                    times[k].append(dt)
        for k, v in times.items():
            rows.append(f"| {tag} | {k} | {1e3 * statistics.median(v):.3f} | {1e3 * min(v):.3f} | {1e3 * max(v):.3f} |")
        # the torch restatement agrees with the call (so the two rows time the same arithmetic)
        mel = eng.mel_from_audio(model, wav, samples=samples, audio_settings=s).numpy("voc")
        ref = torch_restatement(dev, samples)
        for b, n in enumerate(samples):
            F = A.frame_count("hifigan", n)
            assert A.metric_a(mel[b, :, :F], ref[b][1].cpu().numpy()) < 1e-5

    eng.set_profiling(True)
    eng.profile_reset()
    eng.mel_from_audio(model, one, audio_settings=s)
    eng.mel_from_audio(model, ragged, samples=lens, audio_settings=s)
    prof = eng.profile_kernels()
    overhead_us = eng.profile_event_overhead_us()
    eng.set_profiling(False)

    dev_rows = []
    for framing in T.FRAMINGS:
        for case in T.CASES:
            mel = eng.mel_from_audio(T.analysis_models(eng)[framing], T.wave(case), audio_settings=s)
            amp, raw, voc, anchors = T.oracle(case, framing)
            sel = A.selection(amp)
            got = (A.metric_a(mel.numpy("voc")[0], voc), A.metric_b(mel.numpy("voc")[0], voc, sel), A.metric_b(mel.numpy("raw")[0], raw, sel))
            dev_rows.append(f"| {case} | {framing} | {100 * sel.mean():.1f} % | " + " | ".join(f"{g:.2e} ({a:.2e})" for g, a in zip(got, anchors)) + " |")

    lines = [
        "# Mel analysis on the device: waveform -> mel in one launch",
        "",
        f"`tools/analysis_probe.py`, one process; median of {args.reps} alternating repetitions after {args.warmup} warm-up rounds; host wall clock",
        "around complete, synchronised calls.  HIFIGAN framing, ljspeech audio settings, 80 channels.  For information only: no test",
        "gates on a time.",
        "",
        "| input | what | median ms | min ms | max ms |",
        "|---|---|---|---|---|",
        *rows,
        "",
        f"Event-timed launches of the two host calls above (an empty event pair costs {overhead_us:.1f} us here, included):",
        "",
        "| kernel | launches | total ms | us per launch |",
        "|---|---|---|---|",
    ]
    for cls, kernels in prof.items():
        for name, v in kernels.items():
            if v["launches"]:
                lines.append(f"| `{name.split('/')[0]}` ({cls}) | {v['launches']} | {v['ms']:.3f} | {1e3 * v['ms'] / v['launches']:.1f} |")
    lines += [
        "",
        "## Deviations from the float64 oracle: device (float32 restatement)",
        "",
        "Metrics and oracles as in tests/test_emu_analysis.py; the bound is 16 x the figure in brackets, capped at 1e-5 (A) and 1e-3 (B, raw).",
        "",
        "| case | framing | selected | A | B | raw |",
        "|---|---|---|---|---|---|",
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
