"""TEST INFRASTRUCTURE — the fixtures of forced alignment, tests/golden/align/<case>.npz.

Runs ONLY where the reference exists (like oracle/make_golden.py, whose import stub and model builder it uses).  Per case:
the reference's own FlowGenerator gives x_m (its encoder) and z = decoder(mel, reverse=False) in float32 and, with the same
model under .double(), in float64; tests/align_np.py gives the scores; the reference's own `maximum_path`
(glow_tts/utils.py:59-96) gives the path.  Written: ids, the golden file that holds the mel (by name, not duplicated),
z_ref (float32), z_err64 (max |z_ref - z64|), durations_ref, score_ref (and the speaker of the multi-speaker row).

Asserted per case, because exact integer equality is only a fair test where the decisions are not near ties: F >= P; the
durations are unchanged under three uniform +-1e-3 perturbations of the scores and with the float64 z; the restated
recurrence of tests/align_np.py returns the reference's durations.

Usage:  python -m tools.make_golden_align     (from the repository root)
"""
from __future__ import annotations

import dataclasses
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from larynx_amd import hparams as HP  # noqa: E402
from larynx_amd import synthetic  # noqa: E402
from oracle.make_golden import GOLDEN, build_ref_glow, import_reference  # noqa: E402
from tests import align_np  # noqa: E402

MULTI = dataclasses.replace(HP.LJSPEECH, n_speakers=4, gin_channels=48)
MULTI_FILE = "multispeaker/ljspeech_4speakers.npz"
# name -> (voice, golden file, key prefix inside it, speaker)
CASES = {
    "ljspeech_high_short5": (HP.LJSPEECH, "ljspeech_high_short5.npz", "", None),
    "ljspeech_high_echo": (HP.LJSPEECH, "ljspeech_high_echo.npz", "", None),
    "thorsten_medium_veg": (HP.THORSTEN, "thorsten_medium_veg.npz", "", None),
    "ljspeech_high_S120": (HP.LJSPEECH, "ljspeech_high_S120.npz", "", None),
    "multispeaker_dave_s3": (MULTI, MULTI_FILE, "dave_s3.", 3),
}


def latent(model, ids, mel, speaker, dtype):
    """-> (x_m [M, P], z [M, F]) of the reference model in `dtype`; F is the mel's length cut down to a multiple of n_sqz"""
    import torch

    with torch.no_grad():
        text = torch.LongTensor(np.asarray(ids)).unsqueeze(0)
        lengths = torch.LongTensor([text.shape[1]])
        g = None
        if speaker is not None:
            g = torch.nn.functional.normalize(model.emb_g(torch.LongTensor([int(speaker)]))).unsqueeze(-1)
        x_m, _x_logs, _logw, _x_mask = model.encoder(text, lengths, g=g)
        y = torch.from_numpy(np.ascontiguousarray(mel[None])).to(dtype)
        y, y_lengths, _ = model.preprocess(y, torch.LongTensor([y.shape[2]]), y.shape[2])
        z_mask = torch.ones(1, 1, y.shape[2], dtype=dtype)
        z, _logdet = model.decoder(y, z_mask, g=g, reverse=False)
    return x_m[0].numpy(), z[0].numpy()


def main():
    gm, _hm, _hc, _ra = import_reference()
    import glow_tts.utils as gu
    import torch

    np.bool = bool  # the reference's maximum_path still spells it np.bool (utils.py:69)
    out_dir = GOLDEN / "align"
    out_dir.mkdir(parents=True, exist_ok=True)
    models = {}
    for name, (hp, file, prefix, speaker) in CASES.items():
        if hp not in models:
            sd = synthetic.make_glow_state_dict(hp, seed=1234)
            models[hp] = (build_ref_glow(gm, hp, sd), build_ref_glow(gm, hp, sd, prepare=lambda m: m.double()))
        m32, m64 = models[hp]
        gold = np.load(GOLDEN / file)
        ids, mel = gold[prefix + "ids"], gold[prefix + "mel"]
        x32, z32 = latent(m32, ids, mel, speaker, torch.float32)
        x64, z64 = latent(m64, ids, mel, speaker, torch.float64)
        P, F = len(ids), z32.shape[1]
        assert F >= P, (name, P, F)
        z_err64 = float(np.abs(z32.astype(np.float64) - z64).max())
        logp = align_np.scores(x32, z32, np.float32)

        def ref_durations(value):
            v = torch.from_numpy(np.ascontiguousarray(value, np.float32))[None]
            return gu.maximum_path(v, torch.ones_like(v)).numpy()[0].sum(-1).astype(np.int32)

        d_ref = ref_durations(logp)
        d_np, score, _ = align_np.maximum_path(logp)
        assert np.array_equal(d_ref, d_np), name
        rng = np.random.default_rng(5)
        for _ in range(3):
            assert np.array_equal(ref_durations(logp + rng.uniform(-1e-3, 1e-3, logp.shape).astype(np.float32)), d_ref), name
        assert np.array_equal(ref_durations(align_np.scores(x64, z64, np.float64)), d_ref), name
        assert d_ref.min() >= 1 and int(d_ref.sum()) == F
        extra = {} if speaker is None else {"speaker": np.int32(speaker)}
        np.savez_compressed(out_dir / f"{name}.npz", ids=ids, mel_file=file, mel_key=prefix + "mel", z_ref=z32.astype(np.float32),
                            z_err64=np.float64(z_err64), durations_ref=d_ref, score_ref=np.float32(score), **extra)
        print(f"{name}: P={P} F={F} max|z|={np.abs(z32).max():.3f} z_err64={z_err64:.3e} score={float(score):.3f}")


if __name__ == "__main__":
    main()
