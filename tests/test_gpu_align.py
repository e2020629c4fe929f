"""Forced alignment on the device: the path operator against tests/align_np.py (exact), z / durations / score against the
reference's fixtures (tests/golden/align, made by tools/make_golden_align.py), the round trip with synthesis, batch rows,
truncation, the refusals, the schedule and the Python surface.  Measured z errors: profiles/align.md."""
import dataclasses
import json
from pathlib import Path

import numpy as np
import pytest

from larynx_amd import hparams as HP
from larynx_amd import synthetic
from tests.golden_util import GOLDEN
from tests.test_emu_align import (PATH_SHAPES, PATH_SPILL, check_batch_rows, check_dropin, check_path, check_path_ragged,
                                  check_path_ties, check_refusals, check_round_trip, check_schedule, check_truncation)
from tests.test_gpu_parity import models

pytestmark = pytest.mark.gpu

F32 = np.float32
FIXTURES = sorted(p.stem for p in (GOLDEN / "align").glob("*.npz"))
MULTI = dataclasses.replace(HP.LJSPEECH, n_speakers=4, gin_channels=48)
# the recovery table of the issue: (P, synthetic_phoneme_ids seed, length_scale)
ROUND_TRIPS = [(9, 3, 1.0), (57, 21, 1.0), (120, 1234, 0.65)]
_multi = {}


def fixture(name):
    z = np.load(GOLDEN / "align" / f"{name}.npz")
    d = {k: z[k] for k in z.files}
    gold = np.load(GOLDEN / str(d["mel_file"]))
    d["mel"] = gold[str(d["mel_key"])]
    d["hp"] = HP.GlowHParams.from_config(json.loads(str(gold["glow"])))
    d["speaker"] = int(d["speaker"]) if "speaker" in d else None
    return d


def glow_model(eng, hp):
    if hp.n_speakers > 1:  # not in test_gpu_parity's cache (its key is a pair of presets)
        if "g" not in _multi:
            _multi["g"] = eng.load_glow(hp, synthetic.make_glow_state_dict(hp, seed=1234))
        return _multi["g"]
    return models(eng, hp, HP.HIFIGAN_MEDIUM)[0][1]


def ids_of(P, seed):
    return synthetic.synthetic_phoneme_ids(np.random.default_rng(seed), P, HP.LJSPEECH.num_symbols)


# the 257 x 700 case has 8 ids per lane; 1024 x 2048 has 16 and 65536 words of direction bits: past the 24576 the kernel
# keeps in LDS, like PATH_SPILL at one id per lane
@pytest.mark.parametrize("P,F", PATH_SHAPES + [(257, 700), (1024, 2048), PATH_SPILL, (2048, 2048)])
def test_path_operator_exact(gpu_engine, P, F):
    check_path(gpu_engine, np.random.default_rng(P * 1000 + F).standard_normal((P, F)).astype(F32) * 3)


def test_path_operator_ties_and_ragged_batch(gpu_engine):
    check_path_ties(gpu_engine, 9, 30, 1)
    check_path_ties(gpu_engine, 70, 75, 2)
    check_path_ties(gpu_engine, 300, 640, 3)
    check_path_ragged(gpu_engine, 3)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_latent_durations_and_score(gpu_engine, name):
    """max|z - z_ref| <= 4 z_err64 (z_err64: the reference's own float32 pass against its float64 pass), the durations
    exactly the reference's, the score within 1e-4 relative (a sequential f32 sum of F <= 1100 same-sign terms is off by at
    most F 2^-24 = 6.6e-5 relative)."""
    c = fixture(name)
    g = glow_model(gpu_engine, c["hp"])
    dur, score, z = gpu_engine.glow_align(g, c["ids"], c["mel"], speaker_ids=c["speaker"], want_latent=True)
    F = c["z_ref"].shape[1]
    err = float(np.abs(z[0, :, :F] - c["z_ref"]).max())
    rel = abs(float(score[0]) - float(c["score_ref"])) / abs(float(c["score_ref"]))
    print(f"{name}: P={len(c['ids'])} F={F} max|z - z_ref|={err:.3e} z_err64={float(c['z_err64']):.3e} ratio={err / float(c['z_err64']):.2f} "
          f"duration mismatches={int(np.sum(dur[0] != c['durations_ref']))} score={float(score[0]):.3f} rel={rel:.2e}")
    assert err <= 4.0 * float(c["z_err64"])
    assert np.array_equal(dur[0], c["durations_ref"])
    assert rel <= 1e-4


@pytest.mark.parametrize("P,seed,length_scale", ROUND_TRIPS)
def test_round_trip_with_synthesis(gpu_engine, P, seed, length_scale):
    check_round_trip(gpu_engine, glow_model(gpu_engine, HP.LJSPEECH), ids_of(P, seed), length_scale)


def test_multispeaker_round_trip(gpu_engine):
    check_round_trip(gpu_engine, glow_model(gpu_engine, MULTI), ids_of(31, 5), speaker=1)


def test_batch_rows(gpu_engine):
    """z of a batch row against its solo call: other tiles, another f32 summation order — the size of the reference's own
    float32 error on these shapes (z_err64 <= 6.7e-6), allowed four times like the fixture bound: 2.7e-5"""
    g = glow_model(gpu_engine, HP.LJSPEECH)
    a, b = fixture("ljspeech_high_short5"), fixture("ljspeech_high_echo")
    ids57 = ids_of(57, 21)
    mel57 = gpu_engine.glow_infer(g, ids57, 0.0, 1.0).numpy("raw")[0]
    check_batch_rows(gpu_engine, g, [a["ids"], b["ids"], ids57], [a["mel"], b["mel"], mel57], z_tol=2.7e-5)


def test_truncation(gpu_engine):
    c = fixture("ljspeech_high_echo")
    check_truncation(gpu_engine, glow_model(gpu_engine, HP.LJSPEECH), c["ids"], c["mel"])
    odd, _ = gpu_engine.glow_align(glow_model(gpu_engine, HP.LJSPEECH), c["ids"], np.concatenate([c["mel"], c["mel"][:, :1]], axis=1))
    assert np.array_equal(odd[0], c["durations_ref"])


def test_refusals(gpu_engine):
    check_refusals(gpu_engine, glow_model(gpu_engine, HP.LJSPEECH), glow_model(gpu_engine, MULTI), HP.LJSPEECH)


def test_schedule(gpu_engine):
    check_schedule(gpu_engine, glow_model(gpu_engine, HP.LJSPEECH), HP.LJSPEECH, ids_of(57, 21))


def test_dropin(gpu_engine):
    from larynx_amd.constants import TextToSpeechModelConfig
    from larynx_amd.glow_tts import HipGlowTextToSpeech

    tts = HipGlowTextToSpeech(TextToSpeechModelConfig(model_path=Path("unused")), state_dict=synthetic.make_glow_state_dict(HP.LJSPEECH, seed=1234),
                              model_config=HP.LJSPEECH.to_config())
    check_dropin(tts, 256, ids_of(57, 21))
    multi = HipGlowTextToSpeech(TextToSpeechModelConfig(model_path=Path("unused")), state_dict=synthetic.make_glow_state_dict(MULTI, seed=1234),
                                model_config=MULTI.to_config())
    check_dropin(multi, 256, ids_of(20, 6), {"speaker_id": 2})
