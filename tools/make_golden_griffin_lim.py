#!/usr/bin/env python3
"""Make the Griffin-Lim fixtures tests/golden/griffin_lim/<case>.npz from the reference's own functions.

    python tools/make_golden_griffin_lim.py [reference checkout; default $LARYNX_REFERENCE or /root/reference]

`import larynx` needs gruut; the two modules the vocoder consists of do not, so they are loaded by file path:
`larynx/audio.py` as `larynx.audio`, `larynx/constants.py` as `larynx.constants`, then `larynx/griffin_lim.py`, whose
`GriffinLimVocoder.mels_to_audio` runs unchanged.  Its only random input is `np.random.rand` inside `griffin_lim_iter`:
`np.random.seed(seed)` right before the call makes the draw `RandomState(seed).rand(513, T)`, which the tests repeat.

Each fixture holds: the golden case's name, the phase seed, the reference's signal (cast to float32) after 1 and after 60
iterations, `audio_float_to_int16` of the latter, the reference's `mel_basis` (and 16 sampled entries of it), and
`ref_f32_rel_rms_1` / `ref_f32_rel_rms_60`: how far the all-float32 numpy restatement (tests/griffin_lim_np.py) lies from
the reference — the yardstick of the device tests."""
import importlib.util
import os
import sys
import types
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

CASES = ("ljspeech_high_short5", "ljspeech_high_echo")
SEED = 0


def load_reference(root: Path):
    pkg = types.ModuleType("larynx")
    pkg.__path__ = []  # a package without an __init__ of its own
    sys.modules["larynx"] = pkg
    mods = {}
    for name in ("audio", "constants", "griffin_lim"):
        spec = importlib.util.spec_from_file_location(f"larynx.{name}", root / "larynx" / f"{name}.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"larynx.{name}"] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["audio"], mods["constants"], mods["griffin_lim"]


def main():
    root = Path(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LARYNX_REFERENCE", "/root/reference"))
    audio, constants, gl = load_reference(root)
    from tests import griffin_lim_np as G

    out_dir = REPO / "tests" / "golden" / "griffin_lim"
    out_dir.mkdir(parents=True, exist_ok=True)
    config = constants.VocoderModelConfig(model_path=Path("."), session_options=None)
    for case in CASES:
        mel = np.load(REPO / "tests" / "golden" / f"{case}.npz")["mel_voc"].astype(np.float32)
        if mel.ndim == 2:
            mel = mel[None]
        signals = {}
        for iters in (1, 60):
            voc = gl.GriffinLimVocoder(config, iterations=iters)
            np.random.seed(SEED)
            signals[iters] = voc.mels_to_audio(mel)
        basis = voc.mel_basis
        T = mel.shape[2] - 1
        assert signals[60].shape == (T * 256 + 1024,), signals[60].shape
        phase0 = G.initial_phase(SEED, T)
        mag32 = G.magnitudes(mel[0], basis, 1000.0, np.float32)
        _, kept = G.griffin_lim(mag32, phase0, 60, np.float32, keep=(1, 60))
        rms = {i: G.rel_rms(kept[i], signals[i]) for i in (1, 60)}
        sample = np.linspace(0, basis.size - 1, 16).astype(np.int64)
        np.savez_compressed(
            out_dir / f"{case}.npz",
            case=np.array(case), phase_seed=np.int64(SEED),
            signal_1=signals[1].astype(np.float32), signal_60=signals[60].astype(np.float32),
            int16_60=audio.audio_float_to_int16(signals[60]),
            mel_basis=basis.astype(np.float32), mel_basis_sample_index=sample, mel_basis_sample=basis.reshape(-1)[sample].astype(np.float32),
            ref_f32_rel_rms_1=np.float64(rms[1]), ref_f32_rel_rms_60=np.float64(rms[60]),
        )
        print(case, "frames", T, "peak", float(np.abs(signals[60]).max()), "f32 restatement rel rms", rms,
              "bytes", (out_dir / f"{case}.npz").stat().st_size)


if __name__ == "__main__":
    main()
