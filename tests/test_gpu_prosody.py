"""Phoneme timings and per-phoneme duration control (`mi355tts_prosody`) on the device: the durations against the
reference's own `logw` (every golden case, exact), forced durations against the reference's mel, scaled durations against
the oracle, the fused call, the round trip, ragged batches and the launch counts."""

import numpy as np
import pytest

from larynx_amd import hparams as HP
from larynx_amd import synthetic
from tests.golden_util import CASES, load_case
from tests.test_emu_prosody import (MARGIN, attn_durations, check_fused_call, check_ragged_batch, check_round_trip,
                                    check_scaled_against_oracle, clears_margin, oracle_logw, scaled_w)
from tests.test_gpu_parity import models
from tests.test_multispeaker import golden as speakers_golden

pytestmark = pytest.mark.gpu

F32 = np.float32


def expected_from_logw(logw, length_scale, n_sqz, F):
    """The expected value: d = ceil(exp(logw) * length_scale) in float32 from the REFERENCE's logw, cum = cumsum(d),
    expected = diff(minimum(cum, F), prepend=0) with F the reference mel's frame count."""
    w = scaled_w(np.asarray(logw, F32).reshape(-1), length_scale)
    assert clears_margin(w, MARGIN), "fixture precondition: an id within 1e-5 (relative) of a duration step"
    d = np.ceil(w).astype(np.int64)
    exp_d, F_own = attn_durations(d, n_sqz)
    assert F_own == F  # the reference's frame count follows from its own logw
    return d, exp_d


@pytest.mark.parametrize("name", CASES)
def test_durations_equal_the_references(gpu_engine, name):
    """Exact integer equality for every id, sum == F, frames unchanged; then the expected durations forced in
    with the golden's injected noise meet test_golden_reference_parity's bar (raw mel <= 5e-5 max-abs, same F)."""
    c = load_case(name)
    (gsd, g), _ = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    ns, ls = float(c["noise_scale"]), float(c["length_scale"])
    F = c["mel"].shape[1]
    d, exp_d = expected_from_logw(c["logw"], ls, c["glow_hp"].n_sqz, F)
    if name in ("ljspeech_high_S120", "ljspeech_high_echo"):
        assert int(d.sum()) == F + 1  # the odd sums: the last id with frames loses one
    plain = gpu_engine.glow_infer(g, c["ids"], ns, ls, noise=c["noise"])
    mel = gpu_engine.glow_infer(g, c["ids"], ns, ls, noise=c["noise"], want_durations=True)
    got = mel.durations
    print(name, "durations mismatches:", int(np.sum(got[0] != exp_d)), "sum", int(got.sum()), "F", F)
    assert got.shape == (1, len(c["ids"])) and got.dtype == np.int32
    assert np.array_equal(got[0], exp_d)
    assert int(got.sum()) == F and int(mel.frames[0]) == F and np.array_equal(mel.frames, plain.frames)
    assert np.array_equal(mel.numpy("raw"), plain.numpy("raw"))
    # forced durations against the reference
    forced = gpu_engine.glow_infer(g, c["ids"], ns, ls, noise=c["noise"], durations=exp_d)
    err = float(np.abs(forced.numpy("raw")[0] - c["mel"]).max())
    print(name, "forced-durations mel max-abs vs the reference:", err)
    assert int(forced.frames[0]) == F and np.array_equal(forced.durations[0], exp_d)
    assert err <= 5e-5


def test_multispeaker_durations_equal_the_references(gpu_engine):
    z, hp, names, noise = speakers_golden()
    sd = synthetic.make_glow_state_dict(hp, seed=1234)
    g = gpu_engine.load_glow(hp, sd)
    try:
        for name in names:
            ids, ls, ns = z[f"{name}.ids"], float(z[f"{name}.length_scale"]), float(z[f"{name}.noise_scale"])
            spk = int(z[f"{name}.speaker"])
            ref = z[f"{name}.mel"]
            F = ref.shape[1]
            _, exp_d = expected_from_logw(z[f"{name}.logw"], ls, hp.n_sqz, F)
            mel = gpu_engine.glow_infer(g, ids, ns, ls, noise=noise(ids), speaker_ids=spk, want_durations=True)
            print(name, "durations mismatches:", int(np.sum(mel.durations[0] != exp_d)))
            assert np.array_equal(mel.durations[0], exp_d) and int(mel.durations.sum()) == F == int(mel.frames[0])
            # speaker_id combines with both inputs
            forced = gpu_engine.glow_infer(g, ids, ns, ls, noise=noise(ids), speaker_ids=spk, durations=exp_d)
            err = float(np.abs(forced.numpy("raw")[0] - ref).max())
            print(name, "forced-durations mel max-abs vs the reference:", err)
            assert int(forced.frames[0]) == F and err <= 5e-5
            ones = gpu_engine.glow_infer(g, ids, ns, ls, noise=noise(ids), speaker_ids=spk, id_scales=np.ones(len(ids), F32))
            assert np.array_equal(ones.numpy("raw"), mel.numpy("raw"))
    finally:
        gpu_engine.unload(g)


def test_fused_call(gpu_engine):
    (gsd, g), (vsd, v) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_MEDIUM)
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(21), 57, HP.LJSPEECH.num_symbols)
    check_fused_call(gpu_engine, g, v, ids, HP.HIFIGAN_MEDIUM.hop)


def test_round_trip(gpu_engine):
    (gsd, g), _ = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_HIGH)
    for n, seed, ls in ((120, 11, 0.65), (28, 12, 1.0), (200, 13, 1.0), (1, 14, 1.0)):
        ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(seed), n, HP.LJSPEECH.num_symbols)
        check_round_trip(gpu_engine, g, ids, ls, seed)
    from tests.test_emu_prosody import draw_scales

    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(15), 90, HP.LJSPEECH.num_symbols)
    check_round_trip(gpu_engine, g, ids, 0.9, 15, scales=draw_scales(90, 15))


def test_scaled_durations_against_the_oracle_tiny(gpu_engine):
    """TINY_GLOW on the device, the emulator test's cases and bar (test_glow_single_utterance: atol 2e-5, rtol 1e-4)."""
    hp = HP.TINY_GLOW
    sd = synthetic.make_glow_state_dict(hp, seed=7)
    g = gpu_engine.load_glow(hp, sd)
    try:
        for n, ls, seed in ((23, 1.0, 3), (40, 0.8, 4), (5, 1.3, 6)):
            ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(seed), n, hp.num_symbols)
            check_scaled_against_oracle(gpu_engine, g, sd, hp, ids, oracle_logw(sd, hp, ids), ls, 0.667, seed, atol=2e-5, rtol=1e-4)
    finally:
        gpu_engine.unload(g)


def test_scaled_durations_against_the_oracle_echo(gpu_engine):
    """The full-size 28-id `echo` case: logw from the golden (the reference's), mel against the oracle run with the expected
    durations, at the bar the full-size device tests hold against the oracle (5e-5 max-abs:
    test_shortest_utterances_full_size_models)."""
    c = load_case("ljspeech_high_echo")
    (gsd, g), _ = models(gpu_engine, c["glow_hp"], c["voc_hp"])
    check_scaled_against_oracle(gpu_engine, g, gsd, c["glow_hp"], c["ids"], np.asarray(c["logw"], F32).reshape(-1),
                                float(c["length_scale"]), float(c["noise_scale"]), 8, atol=5e-5, rtol=0.0)


def test_ragged_batch_equals_rows_alone(gpu_engine):
    hp = HP.TINY_GLOW
    g = gpu_engine.load_glow(hp, synthetic.make_glow_state_dict(hp, seed=7))
    try:
        check_ragged_batch(gpu_engine, g, hp.num_symbols)
    finally:
        gpu_engine.unload(g)
    (gsd, g), _ = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_HIGH)
    check_ragged_batch(gpu_engine, g, HP.LJSPEECH.num_symbols, lens=(47, 120, 90), seed=6)


def test_launch_counts_do_not_change(gpu_engine):
    """The same launches per kernel name with and without prosody, no new kernel name, and a prosody call never joins
    a coalesced pass while `call_coalesce` is on."""
    (gsd, g), (vsd, v) = models(gpu_engine, HP.LJSPEECH, HP.HIFIGAN_HIGH)
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(3), 120, HP.LJSPEECH.num_symbols)
    sc = np.where(np.arange(120) % 3 == 0, 1.5, 1.0).astype(F32)

    def counts(**kw):
        gpu_engine.profile_reset()
        gpu_engine.glow_infer(g, ids, 0.667, 0.65, seed=1, **kw).free()
        return gpu_engine.kernel_counts()

    counts()
    plain = counts()
    assert sum(plain.values()) > 0
    assert counts(want_durations=True) == plain
    own = gpu_engine.glow_infer(g, ids, 0.667, 0.65, seed=1, want_durations=True).durations[0]
    assert counts(durations=own) == plain
    assert counts(id_scales=np.ones(120, F32)) == plain
    timed = counts(id_scales=sc)  # another frame count may move a tile choice, never the number of launches or add a name
    assert set(timed) == set(plain) and sum(timed.values()) == sum(plain.values())
    assert not any("duration" in k or "prosody" in k for k in timed)
    try:
        gpu_engine.set_option("call_coalesce", 0)
        fused = []
        for kw in ({}, {"return_durations": True}, {"id_scales": np.ones(120, F32)}):
            gpu_engine.profile_reset()
            gpu_engine.synthesize(g, v, ids, 0.667, 0.65, seed=1, **kw)
            fused.append(gpu_engine.kernel_counts())
        assert fused[1] == fused[0] and fused[2] == fused[0]
        lanes = max(gpu_engine.get_call_coalesce_default(), 2)
        gpu_engine.set_option("call_coalesce", lanes)
        p0, r0 = gpu_engine.coalesce_stats()
        gpu_engine.synthesize(g, v, ids, 0.667, 0.65, seed=1)
        p1, r1 = gpu_engine.coalesce_stats()
        assert (p1 - p0, r1 - r0) == (1, 1)  # a plain batch-1 call rides the coalescer ...
        gpu_engine.synthesize(g, v, ids, 0.667, 0.65, seed=1, return_durations=True)
        gpu_engine.synthesize(g, v, ids, 0.667, 0.65, seed=1, id_scales=sc)
        gpu_engine.synthesize(g, v, ids, 0.667, 0.65, seed=1, durations=own)
        assert gpu_engine.coalesce_stats() == (p1, r1)  # ... a prosody call never does
    finally:
        gpu_engine.set_option("call_coalesce", gpu_engine.get_call_coalesce_default())
