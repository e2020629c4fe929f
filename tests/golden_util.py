import json
import os
from pathlib import Path

import numpy as np

from larynx_amd import hparams as HP

GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = sorted(p.stem for p in GOLDEN.glob("*.npz"))


def reference_has(path) -> bool:
    """True when `path` (a file of the reference checkout) exists and this user can read it: a tree that exists but is not
    readable counts as absent (Path.is_file raises PermissionError there instead of returning False)."""
    try:
        return Path(path).is_file() and os.access(path, os.R_OK)
    except OSError:
        return False


def load_case(name):
    z = np.load(GOLDEN / f"{name}.npz")
    d = {k: z[k] for k in z.files}
    d["glow_hp"] = HP.GlowHParams.from_config(json.loads(str(d["glow"])))
    d["voc_hp"] = HP.HifiGanHParams.from_config(json.loads(str(d["vocoder"])))
    d["noise"] = np.random.default_rng(1234).standard_normal((d["glow_hp"].mel_channels, 16 * len(d["ids"]) + 64)).astype(np.float32)
    return d


def load_batch8():
    """BASELINE config 4: rows of the thorsten + 'medium' B = 8 batch, each produced by the
    reference at B = 1 (oracle/make_golden.py)."""
    z = np.load(GOLDEN / "batch8" / "thorsten_medium_batch8.npz")
    ghp = HP.GlowHParams.from_config(json.loads(str(z["glow"])))
    return dict(
        glow_hp=ghp,
        voc_hp=HP.HifiGanHParams.from_config(json.loads(str(z["vocoder"]))),
        noise_scale=float(z["noise_scale"]),
        length_scale=float(z["length_scale"]),
        noise=np.random.default_rng(int(z["noise_seed"])).standard_normal((8, ghp.mel_channels, 2200)).astype(np.float32),
        ids=[z[f"ids{b}"] for b in range(8)],
        mel=[z[f"mel{b}"] for b in range(8)],
        wav=[z[f"wav{b}"] for b in range(8)],
        ref_half_rms=[float(z[f"ref_half_rms{b}"]) for b in range(8)],  # the reference's generator under .half() vs its own f32 waveform
    )


def load_glow_half_reference():
    """Per golden case: what the reference's own decoder under .half() (and both models under .half()) costs against its f32
    outputs (oracle/make_golden_glow_half.py) — the bar of the HIP library's fp16 acoustic mode."""
    return json.loads((GOLDEN / "glow_half_reference.json").read_text())
