"""The Python engine's marshalling in front of the GlowTTS entry points, on the CPU emulator build with the tiny synthetic models:
which C entry point a call's arguments select, what counts as phoneme ids, and what counts as explicit noise."""
import dataclasses

import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic

MULTI_GLOW = dataclasses.replace(HP.TINY_GLOW, n_speakers=3, gin_channels=20)


@pytest.fixture(scope="module")
def tiny(emu_engine):
    """g: a single-speaker voice (it refuses speaker ids), gm: a multi-speaker one (it demands them), v: a vocoder."""
    gsd = synthetic.make_glow_state_dict(HP.TINY_GLOW, seed=7)
    msd = synthetic.make_glow_state_dict(MULTI_GLOW, seed=8)
    vsd = synthetic.make_hifigan_state_dict(HP.TINY_HIFIGAN, seed=7)
    return dict(g=emu_engine.load_glow(HP.TINY_GLOW, gsd), gm=emu_engine.load_glow(MULTI_GLOW, msd),
                v=emu_engine.load_hifigan(HP.TINY_HIFIGAN, vsd))


def _ids(n, seed):
    return synthetic.synthetic_phoneme_ids(np.random.default_rng(seed), n, HP.TINY_GLOW.num_symbols)


# ---------------------------------------------------------------- entry-point selection
class RecordingLib:
    """Stands in for `Engine.lib`: every attribute is the real library's; a call of a `mi355tts_glow_infer*` /
    `mi355tts_synthesize*` entry point is noted by name."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("mi355tts_glow_infer", "mi355tts_synthesize")):
            return fn

        def noted(*args):
            self.calls.append(name)
            return fn(*args)

        return noted


# the arguments of a call -> the suffix of the entry point it must reach; "multi": the call needs the multi-speaker voice
SELECTION = [
    (dict(id_scales=np.ones(6, np.float32)), False, "_prosody"),
    (dict(durations=np.full(6, 2, np.int32)), False, "_prosody"),
    (dict(want_durations=True), False, "_prosody"),
    (dict(want_durations=True, speaker_ids=[1, 2], row_seeds=[5, 6]), True, "_prosody"),
    (dict(want_durations=True, speaker_ids=[1, 2]), True, "_prosody"),
    (dict(speaker_ids=[1, 2]), True, "_speakers"),
    (dict(speaker_ids=2, row_seeds=[5, 6]), True, "_speakers"),
    (dict(row_seeds=[5, 6]), False, "_rows"),
    (dict(), False, ""),
]


def _call_args(kw, multi):
    """The ids (two rows with speakers or row seeds, else one of 6 ids: the prosody vectors above are [6]) and the keywords."""
    two = multi or "row_seeds" in kw
    return ([_ids(6, 1), _ids(4, 2)] if two else _ids(6, 1)), dict(kw)


@pytest.mark.parametrize("kw,multi,suffix", SELECTION)
def test_glow_infer_reaches_the_narrowest_entry_point(emu_engine, tiny, monkeypatch, kw, multi, suffix):
    ids, kw = _call_args(kw, multi)
    rec = RecordingLib(emu_engine.lib)
    monkeypatch.setattr(emu_engine, "lib", rec)
    mel = emu_engine.glow_infer(tiny["gm" if multi else "g"], ids, seed=3, **kw)
    assert rec.calls == ["mi355tts_glow_infer" + suffix], (kw, rec.calls)
    assert mel.batch == (2 if isinstance(ids, list) else 1)
    mel.free()


@pytest.mark.parametrize("kw,multi,suffix", [c for c in SELECTION if "row_seeds" not in c[0]])
def test_synthesize_reaches_the_narrowest_entry_point(emu_engine, tiny, monkeypatch, kw, multi, suffix):
    ids, kw = _call_args(kw, multi)
    if "want_durations" in kw:
        kw["return_durations"] = kw.pop("want_durations")
    rec = RecordingLib(emu_engine.lib)
    monkeypatch.setattr(emu_engine, "lib", rec)
    res = emu_engine.synthesize(tiny["gm" if multi else "g"], tiny["v"], ids, seed=3, **kw)
    # (the call is repeated once when the guessed buffer was too small: the same entry point then)
    assert set(rec.calls) == {"mi355tts_synthesize" + suffix} and len(rec.calls) <= 2, (kw, rec.calls)
    assert len(res) == (4 if kw.get("return_durations") else 3)


def test_row_seeds_need_one_seed_per_row_and_no_noise(emu_engine, tiny):
    M = HP.TINY_GLOW.mel_channels
    with pytest.raises(ValueError, match="row_seeds: one seed per row, and no explicit noise"):
        emu_engine.glow_infer(tiny["g"], [_ids(6, 1), _ids(4, 2)], row_seeds=[5])
    with pytest.raises(ValueError, match="row_seeds: one seed per row, and no explicit noise"):
        emu_engine.glow_infer(tiny["g"], _ids(6, 1), row_seeds=[5], noise=np.zeros((M, 400), np.float32))


# ---------------------------------------------------------------- ids intake
def _same_mels(eng, g, forms, seed):
    mels = [eng.glow_infer(g, ids, 0.667, 1.0, seed=seed) for ids in forms]
    first = mels[0].numpy("raw")
    for m in mels[1:]:
        assert np.array_equal(m.frames, mels[0].frames) and m.numpy("raw").tobytes() == first.tobytes()
    for m in mels:
        m.free()
    return mels[0].frames


def test_every_form_of_ids_gives_the_same_call(emu_engine, tiny):
    """A vector, a list of rows (arrays, lists or tuples, ragged or not) and a 2-D array are one and the same batch: with the
    device's seeded noise the mels agree bit for bit, and the fused call's frame counts agree."""
    a, b, c = _ids(5, 11), _ids(3, 12), _ids(5, 13)
    g, v = tiny["g"], tiny["v"]
    forms_1 = [a, [a], a[None]]
    forms_2 = [[a, c], np.stack([a, c])]
    forms_r = [[a, b], (list(map(int, a)), tuple(b))]
    assert _same_mels(emu_engine, g, forms_1, 21).shape == (1,)
    assert _same_mels(emu_engine, g, forms_2, 22).shape == (2,)
    ragged = _same_mels(emu_engine, g, forms_r, 23)
    assert ragged.shape == (2,) and ragged[0] > ragged[1] > 0
    for forms, B, seed in ((forms_1, 1, 21), (forms_2, 2, 22), (forms_r, 2, 23)):
        frames = [emu_engine.synthesize(g, v, ids, 0.667, 1.0, seed=seed)[0] for ids in forms]
        assert all(np.array_equal(f, frames[0]) for f in frames[1:]) and frames[0].shape == (B,) and np.all(frames[0] > 0)


def test_no_rows_and_empty_rows_are_the_librarys_refusals(emu_engine, tiny):
    g, v = tiny["g"], tiny["v"]
    none = np.zeros(0, np.int64)
    with pytest.raises(ffi.Mi355ttsError, match="empty batch") as e:
        emu_engine.synthesize(g, v, [])
    assert e.value.code == -1
    with pytest.raises(ffi.Mi355ttsError, match="empty batch"):
        emu_engine.glow_infer(g, [])
    for ids in (none, [none], [none, none]):
        with pytest.raises(ffi.Mi355ttsError) as e:
            emu_engine.glow_infer(g, ids)
        assert e.value.code == -1
        with pytest.raises(ffi.Mi355ttsError) as e:
            emu_engine.synthesize(g, v, ids)
        assert e.value.code == -1
    # the process goes on
    assert int(emu_engine.synthesize(g, v, _ids(6, 1), seed=1)[0][0]) > 0


# ---------------------------------------------------------------- noise intake
def test_noise_of_another_batch_size_is_refused(emu_engine, tiny):
    """[1, M, F] noise with two rows of ids would be read past its end as the second row's."""
    g, v = tiny["g"], tiny["v"]
    M = HP.TINY_GLOW.mel_channels
    ids = _ids(6, 1)
    for noise in (np.zeros((1, M, 400)), np.zeros((M, 400)), np.zeros((3, M, 400))):
        with pytest.raises(ValueError, match="noise batch mismatch"):
            emu_engine.synthesize(g, v, [ids, ids], noise=noise)
        with pytest.raises(ValueError, match="noise batch mismatch"):
            emu_engine.glow_infer(g, [ids, ids], noise=noise)
        with pytest.raises(ValueError, match="noise batch mismatch"):
            emu_engine.glow_infer_taps(g, [ids, ids], noise=noise)


def test_two_dimensional_noise_is_the_batch_of_one(emu_engine, tiny):
    g, v = tiny["g"], tiny["v"]
    M = HP.TINY_GLOW.mel_channels
    ids = _ids(8, 3)
    noise = np.random.default_rng(4).standard_normal((M, 400)).astype(np.float32)
    m2, m3 = emu_engine.glow_infer(g, ids, noise=noise), emu_engine.glow_infer(g, ids, noise=noise[None])
    assert int(m2.frames[0]) > 0 and np.array_equal(m2.frames, m3.frames) and m2.numpy("raw").tobytes() == m3.numpy("raw").tobytes()
    # float64 noise is converted, not reinterpreted
    m64 = emu_engine.glow_infer(g, ids, noise=noise.astype(np.float64))
    assert m64.numpy("raw").tobytes() == m2.numpy("raw").tobytes()
    f2, _, w2 = emu_engine.synthesize(g, v, ids, noise=noise)
    f3, _, w3 = emu_engine.synthesize(g, v, ids, noise=noise[None])
    assert np.array_equal(f2, m2.frames) and np.array_equal(f2, f3) and np.array_equal(w2, w3) and np.any(w2 != 0)
    for m in (m2, m3, m64):
        m.free()
