#!/usr/bin/env python3
"""Time the Griffin-Lim vocoder on the device against the code that existed before it: 61 chained calls of the
denoiser's STFT round trip (`mi355tts_op_denoise`: one forward + one inverse STFT of the same conventions per call).

    python tools/griffin_lim_probe.py [--out profiles/griffin_lim.md] [--reps 20] [--warmup 3]

One process, one engine.  Every timed region is a complete, stream-synchronised library call (both entry points
return after their stream has drained).  Writes a markdown report: the median 60-iteration call on the 596-frame
`S120` mel, the median of 61 x `op_denoise` on a signal of the same length, their ratio, and the per-kernel times of
one profiled call (`mi355tts_profile_kernels_json`)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "griffin_lim.md"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    from larynx_amd.audio import mel_basis
    from larynx_amd.engine import Engine

    eng = Engine(0)
    mel = np.load(REPO / "tests" / "golden" / "ljspeech_high_S120.npz")["mel_voc"].astype(np.float32)
    mel = mel if mel.ndim == 3 else mel[None]
    T = mel.shape[2] - 1
    N = T * 256 + 1024
    model = eng.load_griffin_lim(mel_basis(22050, 1024, 80, 0.0, 8000), 1000.0, 60)
    batch = eng.mel_from_numpy(mel)

    def gl_call():
        t0 = time.perf_counter()
        f32, _, _ = eng.griffin_lim_infer(model, batch, seed=1, iterations=60)
        return time.perf_counter() - t0, f32

    for _ in range(args.warmup):
        _, wav = gl_call()
    assert np.isfinite(wav).all() and wav.shape == (1, N)

    # the denoiser round trip on a signal of the same length (a multiple of 256 by construction); strength 0 keeps the
    # magnitudes, so the chain stays finite: what is timed is 61 forward + 61 inverse STFTs and 61 overlap-adds
    sig = (wav[0] / max(float(np.abs(wav).max()), 1e-30)).astype(np.float32)
    bias = np.zeros(513, np.float32)

    def dn_chain():
        x = sig[None]
        t0 = time.perf_counter()
        for _ in range(61):
            x = eng.denoise(x, bias, 0.0)
        return time.perf_counter() - t0

    for _ in range(args.warmup):
        dn_chain()
    gl, dn = [], []
    for _ in range(args.reps):  # alternating: both sides see the same machine state
        gl.append(gl_call()[0])
        dn.append(dn_chain())

    eng.set_profiling(True)
    eng.profile_reset()
    gl_call()
    prof = eng.profile_kernels()
    counts = {k: v for k, v in eng.kernel_counts().items() if v}
    overhead_us = eng.profile_event_overhead_us()
    eng.set_profiling(False)

    gl_ms, dn_ms = 1e3 * statistics.median(gl), 1e3 * statistics.median(dn)
    lines = [
        "# Griffin-Lim vocoder on the device: 60 iterations against 61 denoiser round trips",
        "",
        f"`tools/griffin_lim_probe.py`, one process; median of {args.reps} alternating repetitions after {args.warmup} warm-up calls of each; every timed region is a",
        "complete library call that returns after its stream has drained (host wall clock around the call).",
        f"Input: the `ljspeech_high_S120` golden's vocoder mel, {mel.shape[2]} frames -> {T} STFT frames, {N} samples.",
        "",
        "| what | median ms | min ms | max ms |",
        "|---|---|---|---|",
        f"| `mi355tts_griffin_lim_infer`, 60 iterations (mel on the device, float signal to the host) | {gl_ms:.3f} | {1e3 * min(gl):.3f} | {1e3 * max(gl):.3f} |",
        f"| 61 x `mi355tts_op_denoise` on {N} samples (host buffers, as the operator is exposed) | {dn_ms:.3f} | {1e3 * min(dn):.3f} | {1e3 * max(dn):.3f} |",
        f"| ratio Griffin-Lim / denoiser chain | {gl_ms / dn_ms:.4f} | | |",
        f"| the reference's Python loop on the same mel (CPU, measured on a DIFFERENT host) | 2800 | | |",
        "",
        "The denoiser operator copies its signal to the device and back on every call and synchronises 61 times; the Griffin-Lim",
        "call keeps the signal on the device as overlapping synthesis frames and synchronises once.  That is part of what the",
        "comparison is about: it is the code a caller had before this vocoder existed.",
        "",
        f"## Per kernel, one profiled 60-iteration call (event-timed; an empty event pair costs {overhead_us:.1f} us here, included in every launch's figure)",
        "",
        "| kernel | launches | total ms | us per launch |",
        "|---|---|---|---|",
    ]
    for cls, kernels in prof.items():
        for name, v in kernels.items():
            if v["launches"]:
                lines.append(f"| `{name.split('/')[0]}` ({cls}) | {v['launches']} | {v['ms']:.3f} | {1e3 * v['ms'] / v['launches']:.1f} |")
    lines += ["", "Launch counts of that call: `" + json.dumps(counts) + "`", ""]
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines))
    print("\n".join(lines))
    eng.unload(model)
    eng.close()


if __name__ == "__main__":
    main()
