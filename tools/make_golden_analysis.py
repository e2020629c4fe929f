#!/usr/bin/env python3
"""Make the mel-analysis fixtures tests/golden/analysis/<case>.npz from the reference's own functions.

    python tools/make_golden_analysis.py [reference checkout; default $LARYNX_REFERENCE or /root/reference]

`larynx/audio.py` needs nothing but numpy and is loaded by file path (`import larynx` needs gruut).  The reference never
analyses a recording on its inference path, but it carries every piece of the REFERENCE framing: `transform` (its `stft`:
1024-point frames at range(0, len - 1024, 256), np.hanning), `mel_basis`, and on `AudioSettings` `amp_to_db`, `normalize`
and `dynamic_range_compression`.  Chained in float64 on a float32 waveform they give, per case:

    ref_amp [80, T]   mel_basis @ magnitude
    ref_voc [80, T]   dynamic_range_compression(ref_amp)
    ref_raw [80, T]   normalize(amp_to_db(ref_amp)) under the ljspeech voice's audio settings

The HIFIGAN framing is not in the reference: its oracle is the float64 restatement tests/analysis_np.py, which the emulator
test pins to the arrays above through the REFERENCE framing.  The anchors `f32_<framing>_{a,b,raw}` record how far the
all-float32 restatement lies from the float64 one under the tests' metrics (analysis_np.metric_a / metric_b): the yardstick
every device bound is a multiple of.  Cases: the two golden waveforms and the designed signal (analysis_np.designed_signal),
the only one that reaches the 1e-5 clamp."""
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

GOLDEN_CASES = ("ljspeech_high_short5", "ljspeech_high_echo")


def main():
    root = Path(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LARYNX_REFERENCE", "/root/reference"))
    spec = importlib.util.spec_from_file_location("_ref_larynx_audio", root / "larynx" / "audio.py")
    audio = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = audio  # dataclasses looks the module up while the class is being made
    spec.loader.exec_module(audio)
    from larynx_amd.audio import ljspeech_audio_settings
    from tests import analysis_np as A

    ours = ljspeech_audio_settings()
    settings = audio.AudioSettings(**{k: getattr(ours, k) for k in audio.AudioSettings.__dataclass_fields__})
    basis = audio.mel_basis(settings.sample_rate, 1024, settings.mel_channels, settings.mel_fmin, settings.mel_fmax)
    out_dir = REPO / "tests" / "golden" / "analysis"
    out_dir.mkdir(parents=True, exist_ok=True)
    waves = {c: np.load(REPO / "tests" / "golden" / f"{c}.npz")["wav"].astype(np.float32) for c in GOLDEN_CASES}
    waves["designed"] = A.designed_signal()
    for case, wav in waves.items():
        mag, _ = audio.transform(wav[None])
        amp = basis @ mag[0]
        fx = dict(case=np.array(case), samples=np.int64(len(wav)), ref_amp=amp,
                  ref_voc=settings.dynamic_range_compression(amp), ref_raw=settings.normalize(settings.amp_to_db(amp)))
        assert amp.dtype == np.float64 and amp.shape == (80, A.frame_count("reference", len(wav)))
        report = {}
        for framing in ("reference", "hifigan"):
            amp64, raw64, voc64 = A.analyze(wav, basis, framing, ours, np.float64)
            _, raw32, voc32 = A.analyze(wav, basis, framing, ours, np.float32)
            sel = A.selection(amp64)
            fx[f"f32_{framing}_a"] = np.float64(A.metric_a(voc32, voc64))
            fx[f"f32_{framing}_b"] = np.float64(A.metric_b(voc32, voc64, sel))
            fx[f"f32_{framing}_raw"] = np.float64(A.metric_b(raw32, raw64, sel))
            fx[f"share_{framing}"] = np.float64(sel.mean())
            report[framing] = {k: float(fx[f"f32_{framing}_{k}"]) for k in ("a", "b", "raw")}
            report[framing]["share"] = float(sel.mean())
            report[framing]["at_clamp"] = float((amp64 <= 1e-5).mean())
            if framing == "reference":  # the restatement against the reference's chain, float64 both
                sel_ref = A.selection(amp)
                report["restatement_vs_reference"] = (A.metric_a(voc64, fx["ref_voc"]), A.metric_b(voc64, fx["ref_voc"], sel_ref),
                                                      A.metric_b(raw64, fx["ref_raw"], sel_ref))
        np.savez_compressed(out_dir / f"{case}.npz", **fx)
        print(case, "samples", len(wav), report, "bytes", (out_dir / f"{case}.npz").stat().st_size)


if __name__ == "__main__":
    main()
