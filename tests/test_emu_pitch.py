"""The YIN pitch tracker (csrc/pitch.h: one launch per call) on the CPU emulator.

Oracle: tests/pitch_np.py — the definition of include/mi355tts.h in float64 (`dtype=np.float64`) and its float32 restatement in
the kernel's documented summation orders.  The reference has no pitch code, so the float64 statement is the standard.

Bounds.  Rows with an exact integer period have no tolerance: periodicity 1.0, f0 = float32(fs) / float32(P) and d'(P) = 0 bit
for bit (the difference form).  Everything else is compared on the DECIDED frames — those on which the oracle at theta (1 - 1e-3),
theta and theta (1 + 1e-3) picks the same lag and the same voicing — where the device's voicing must equal the oracle's, and f0
(relative, voiced frames), periodicity, level_db and the whole d' plane (absolute) must lie within the project's yardstick: 16 x
the restatement's own largest deviation from the oracle on the same frames, never below 4 float32 ulps of the compared value.
Batch rows, int16 input and device pointers have no tolerance.  The check functions are shared with tests/test_gpu_pitch.py."""
import ctypes as C

import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.pitch import PitchTrack, PitchTracker, get_pitch_tracker, pitch_per_span
from tests import pitch_np as P
from tests import resample_np as R
from tests.golden_util import load_case
from tests.test_emu_resample import numpy_alloc

FS = 22050
THETA = 0.15
GEOM = dict(sample_rate=FS, hop=256, W=1024, tau_min=45, tau_max=441)          # the issue's test parameters
GEOM16 = dict(sample_rate=16000, hop=186, W=640, tau_min=32, tau_max=320)      # PitchTracker(engine, 16000)'s defaults
PERIODS = (45, 64, 127, 128, 129, 320, 441)  # both ends of the lag range, both sides of the 64-lane and 256-thread seams
EDGE_ROWS = (0, 255, 256, 257, 300, 4608)
RAGGED = (4608, 0, 300, 2000)
MIN_DECIDED = 0.95
GOLDEN_SAMPLES = 40000
_cache = {}


def model(eng, geom=GEOM, theta=THETA, interpolate=True):
    key = ("model", id(eng), tuple(sorted(geom.items())), theta, interpolate)
    if key not in _cache:
        _cache[key] = eng.load_pitch(geom["sample_rate"], geom["hop"], geom["W"], geom["tau_min"], geom["tau_max"], theta, interpolate)
    return _cache[key]


def designed(fs=FS):
    """The designed signal at 22 050 Hz, or resampled on the host (the float64 oracle of tests/resample_np.py) to 16 000 Hz."""
    if ("sig", fs) not in _cache:
        x = P.designed_signal()
        if fs != FS:
            g = np.gcd(fs, FS)
            x = R.oracle(x.astype(np.float64), R.design(fs // g, FS // g)[0], fs // g, FS // g).astype(np.float32)
        _cache["sig", fs] = x
    return _cache["sig", fs]


def voiced_row(n):
    """`n` samples from the start of the designed signal's glide."""
    return designed()[6615:6615 + n].copy()


def reference(x, key, geom=GEOM, theta=THETA, interpolate=True):
    """(the float64 oracle, the decided frames, the float32 restatement) of one row: computed once, never changed."""
    key = ("ref", key, tuple(sorted(geom.items())), theta, interpolate)
    if key not in _cache:
        o, ok = P.decided(x, theta, interpolate=interpolate, **geom)
        _cache[key] = (o, ok, P.track(x, theta=theta, interpolate=interpolate, dtype=np.float32, **geom))
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(eng, x, geom=GEOM, theta=THETA, interpolate=True, samples=None):
    return eng.pitch(model(eng, geom, theta, interpolate), x, samples, want_cmnd=geom["tau_max"] + 1)


def within(tag, got, ref, r32, relative=False):
    """max |got - ref| against max(16 x the restatement's own, 4 ulp of the value), element by element; prints and returns what it
    measured: (the largest deviation, the restatement's, the smallest bound applied)."""
    if ref.size == 0:
        return None
    ref = ref.astype(np.float64)
    scale = np.abs(ref) if relative else 1.0
    err = np.abs(got.astype(np.float64) - ref) / scale
    anchor = float((np.abs(r32.astype(np.float64) - ref) / scale).max())
    floor = 4.0 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) / scale
    bound = np.maximum(16.0 * anchor, floor)
    print(f"  {tag}: {float(err.max()):.3e} from the oracle (restatement {anchor:.3e}, bound {float(bound.min()):.3e})")
    assert (err <= bound).all(), tag
    return float(err.max()), anchor, float(bound.min())


def compare(tag, got, x, key, geom=GEOM, theta=THETA, interpolate=True, min_decided=MIN_DECIDED):
    """One row against the oracle on its decided frames -> (oracle, decided frames, {quantity: what `within` measured})."""
    o, ok, r32 = reference(x, key, geom, theta, interpolate)
    F = len(ok)
    assert got["f0"].shape == got["periodicity"].shape == got["level_db"].shape == (F,) and got["cmnd"].shape == (F, geom["tau_max"] + 1)
    if F == 0:
        return o, ok, {}
    share, voiced = float(ok.mean()), float(o["voiced"].mean())
    print(f"{tag}: {F} frames, {100 * share:.1f} % decided, {100 * voiced:.1f} % voiced")
    assert share >= min_decided, tag
    assert np.array_equal(got["f0"][ok] > 0, o["voiced"][ok]), tag
    assert (got["cmnd"][:, 0] == 1.0).all()
    v = ok & o["voiced"]
    figures = {"f0 (relative)": within("f0 (relative)", got["f0"][v], o["f0"][v], r32["f0"][v], relative=True)}
    for k in ("periodicity", "level_db", "cmnd"):
        figures[k] = within(k, got[k][ok], o[k][ok], r32[k][ok])
    return o, ok, figures


def check_exact_periods(eng):
    """Check 1: tiled rows.  Every frame whose span lies wholly inside the row: no tolerance."""
    hop, W, tmax = GEOM["hop"], GEOM["W"], GEOM["tau_max"]
    for period in PERIODS:
        x = P.periodic_row(period)
        r = run(eng, x, interpolate=False)
        inside = [t for t in range(len(x) // hop) if t * hop - W // 2 >= 0 and t * hop - W // 2 + W + tmax <= len(x)]
        assert len(inside) == 18
        want = np.float32(FS) / np.float32(period)
        print(f"P = {period}: f0 {r['f0'][inside[0]]!r} (expected {want!r}), periodicity {r['periodicity'][inside[0]]!r}")
        assert (bits(r["periodicity"][inside]) == bits(np.float32(1.0))).all(), period
        assert (bits(r["f0"][inside]) == bits(want)).all(), period
        assert (r["cmnd"][inside, period] == 0.0).all(), period


def check_designed(eng, geom=GEOM):
    """Checks 2 and 3: the designed signal."""
    fs = geom["sample_rate"]
    x = designed(fs)
    o, ok, figures = compare(f"designed signal at {fs} Hz", run(eng, x, geom), x, "designed", geom)
    assert len(ok) == 206 and 0.6 < o["voiced"].mean() < 0.85
    return o, ok, figures


def check_golden(eng, case):
    """Check 5: vocoder output of synthetic weights — unvoiced on every frame, the argmin path."""
    x = np.ascontiguousarray(load_case(case)["wav"].reshape(-1)[:GOLDEN_SAMPLES], np.float32)
    o, ok, figures = compare(case, run(eng, x), x, case)
    assert not o["voiced"].any() and len(ok) > 20
    return o, ok, figures


def check_edges(eng):
    """Check 4, the rows alone: frame counts (none for 0 and 255 samples), rows shorter than the window, silence."""
    mid = model(eng)
    for n in EDGE_ROWS:
        x = voiced_row(n)
        r = run(eng, x)
        assert r["frames"][0] == n // 256 == eng.pitch_frames(mid, n) and r["f0"].shape == (n // 256,)
        compare(f"N = {n}", r, x, ("edge", n), min_decided=0.0)
    r = run(eng, np.zeros(3000, np.float32))
    assert r["f0"].shape == (11,) and not r["f0"].any() and not r["periodicity"].any()
    assert (r["level_db"] == -100.0).all() and (r["cmnd"] == 1.0).all()


def ragged_batch():
    batch = np.full((len(RAGGED), 4700), 0.25, np.float32)  # what lies past a row's samples must not be read
    for b, n in enumerate(RAGGED):
        batch[b, :n] = voiced_row(n)
    return batch


def check_ragged_batch(eng):
    """A ragged batch of 4, unsorted, one row empty: every row the bits of its own batch-1 call, zeros behind its frames."""
    batch = ragged_batch()
    r = run(eng, batch, samples=RAGGED)
    assert r["f0"].shape == (4, 18) and r["cmnd"].shape == (4, 18, 442) and list(r["frames"]) == [n // 256 for n in RAGGED]
    for b, n in enumerate(RAGGED):
        one, F = run(eng, batch[b, :n]), n // 256
        for k in ("f0", "periodicity", "level_db", "cmnd"):
            assert np.array_equal(bits(r[k][b, :F]), bits(one[k])) and not r[k][b, F:].any(), (k, n)
    print(f"rows of {RAGGED} samples in one batch: each bit-identical to its batch-1 call")


def check_int16_input(eng):
    i16 = np.round(voiced_row(4608) * 32767 / 0.6).astype(np.int16)
    i16[:2] = (-32768, 32767)
    a, b = run(eng, i16), run(eng, i16.astype(np.float32) * np.float32(2.0 ** -15))
    assert (a["f0"] > 0).sum() > 10
    for k in ("f0", "periodicity", "level_db", "cmnd"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def check_device_pointers(eng, alloc):
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE (`alloc`: tests/test_emu_resample.py): float32 and int16 device rows in, all four
    outputs to pre-filled device buffers with a stride past the longest row's frames: the host call's bits, zeros up to the
    stride.  Then a batch whose rows hold no frame, to host and to device destinations: zeros."""
    mid, T1 = model(eng), GEOM["tau_max"] + 1
    batch = ragged_batch()
    B, in_ld, out_ld = len(RAGGED), batch.shape[1], 18 + 5
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE

    def outputs(buffer):
        return [buffer(np.full((B, out_ld), 7.0, np.float32)) for _ in range(3)] + [buffer(np.full((B, out_ld, T1), 7.0, np.float32))]

    for src in (batch, np.round(batch * 32767).astype(np.int16)):
        host = eng.pitch(mid, src, RAGGED, want_cmnd=T1)
        dev, keep = alloc(src)
        ptrs = (None, dev) if src.dtype == np.int16 else (dev, None)
        outs = outputs(alloc)
        eng.pitch_raw(mid, ptrs[0], ptrs[1], RAGGED, in_ld, *(p for p, _ in outs), out_ld, flags)
        for k, (_, get) in zip(("f0", "periodicity", "level_db", "cmnd"), outs):
            got = get()
            assert np.array_equal(bits(got[:, :18]), bits(host[k])) and not got[:, 18:].any(), k
        h_ptrs = (None, src.ctypes.data) if src.dtype == np.int16 else (src.ctypes.data, None)
        for in_ptrs, buffer, fl in ((h_ptrs, numpy_alloc, 0), (ptrs, alloc, flags)):
            outs = outputs(buffer)
            eng.pitch_raw(mid, in_ptrs[0], in_ptrs[1], (0, 255, 100, 0), in_ld, *(p for p, _ in outs), out_ld, fl)
            assert not any(get().any() for _, get in outs)
        del keep


def check_schedule(eng):
    """Exactly one launch, under the kernel's name, for a batch of 1 and a ragged batch of 4; none for a batch without frames."""
    mid = model(eng)
    eng.set_profiling(True)
    try:
        for x, samples, launches in ((voiced_row(4608), None, 1), (ragged_batch(), RAGGED, 1), (ragged_batch(), (0, 255, 100, 0), 0)):
            eng.profile_reset()
            eng.pitch(mid, x, samples, want_cmnd=442)
            prof = eng.profile()
            ran = {k: v for k, v in eng.kernel_counts().items() if v}
            print(f"batch of {1 if samples is None else len(samples)}: {ran}, {prof['elementwise']['ms']:.4f} ms")
            assert ran == ({"pitch_kernel": 1} if launches else {})
            assert prof["elementwise"]["launches"] == launches and all(v["launches"] == 0 for k, v in prof.items() if k != "elementwise")
    finally:
        eng.set_profiling(False)
        eng.profile_reset()
    counts = eng.kernel_counts()
    assert not any(counts.values()) and len(counts) == 44 and list(counts)[-1] == "attention_kernel"  # the pinned keys, unchanged


def _refused(fn, what, code=-1):
    with pytest.raises(ffi.Mi355ttsError) as e:
        fn()
    msg = str(e.value).split(": ", 1)[1]
    assert e.value.code == code and msg and what in msg, str(e.value)


def check_refusals(eng):
    """Every limit of the header: MI355TTS_ERR_INVALID with its reason, and the context still works."""
    lib, mid = eng.lib, C.c_int()

    def load(sr=FS, hop=256, window=1024, tmin=45, tmax=441, theta=THETA, params=True, out=True):
        p = ffi.PitchParamsC(sr, hop, window, tmin, tmax, theta, 1)
        return lambda: ffi.check(lib, lib.mi355tts_load_pitch(eng._ctx, C.byref(p) if params else None, C.byref(mid) if out else None))

    _refused(load(params=False), "null")
    _refused(load(out=False), "null")
    _refused(load(sr=0), "sample_rate")
    for bad in (0, -1, 4097):
        _refused(load(hop=bad), "hop")
    for bad in (60, 0, 1022, 2052, 4096):
        _refused(load(window=bad), "window")
    for tmin, tmax in ((0, 441), (442, 441), (45, 1025), (-3, -1)):
        _refused(load(tmin=tmin, tmax=tmax), "tau_min")
    # (window <= 2048 and tau_max <= 1024 already keep window + tau_max within 3072: the largest of both is accepted)
    for ok in (dict(window=2048, tmin=1, tmax=1024, hop=4096), dict(window=64, tmin=1, tmax=1, hop=1, theta=1.0)):
        load(**ok)()
        eng.unload(mid.value)
    for bad in (0.0, -0.1, 1.0001, np.nan, np.inf):
        _refused(load(theta=bad), "threshold")
    m = model(eng)
    x = np.ascontiguousarray(voiced_row(700))
    i16 = np.zeros(700, np.int16)
    outs = [np.full(4, 7.0, np.float32) for _ in range(3)]
    cm = np.zeros((4, 442), np.float32)
    n = np.array([700], np.int64)

    def call(f32=x.ctypes.data, s16=None, samples=n, in_ld=700, f0=outs[0].ctypes.data, per=outs[1].ctypes.data, lvl=outs[2].ctypes.data,
             cmnd=cm.ctypes.data, out_ld=4, mdl=m, B=1):
        s_p = None if samples is None else samples.ctypes.data_as(C.POINTER(C.c_int64))
        return lambda: ffi.check(lib, lib.mi355tts_pitch(eng._ctx, mdl, f32, s16, s_p, B, in_ld, f0, per, lvl, cmnd, out_ld, 0))

    _refused(call(samples=None), "null")
    _refused(call(s16=i16.ctypes.data), "exactly one")
    _refused(call(f32=None), "exactly one")
    _refused(call(B=0), "batch")
    _refused(call(in_ld=-1), "in_ld")
    for bad in (-1, 701):
        _refused(call(samples=np.array([bad], np.int64)), "samples[0]")
    _refused(call(f0=None, per=None, lvl=None), "no output")
    _refused(call(out_ld=1), "out_ld")
    _refused(call(out_ld=-1), "out_ld")
    _refused(call(mdl=10 ** 6), "no pitch tracker", code=-5)
    with pytest.raises(ffi.Mi355ttsError):
        eng.pitch_frames(m, -1)
    call()()  # the context still works: two frames, then the zeros up to out_ld
    one = run(eng, x)
    assert np.array_equal(bits(outs[0][:2]), bits(one["f0"])) and not outs[0][2:].any() and np.array_equal(bits(cm[:2]), bits(one["cmnd"]))
    call(f0=None, lvl=None, cmnd=None)()  # one plane alone
    assert np.array_equal(bits(outs[1][:2]), bits(one["periodicity"]))
    gone = eng.load_pitch(FS, 256, 1024, 45, 441)
    assert np.array_equal(bits(eng.pitch(gone, x)["f0"]), bits(one["f0"]))
    eng.unload(gone)
    _refused(lambda: eng.pitch(gone, x), "no pitch tracker", code=-5)


def check_sentence_path(tts, voc, n_ids=(11, 4, 26)):
    """Check 6: `phonemes_to_speech(pitch=True)` on the TINY models."""
    import larynx_amd

    rng = np.random.default_rng(41)
    sents = [(f"s{i}", synthetic.synthetic_phoneme_ids(rng, n, HP.TINY_GLOW.num_symbols)) for i, n in enumerate(n_ids)]
    settings = {"seed": 77}
    run_ = lambda **kw: list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, **kw))  # noqa: E731
    for base, rate in ((dict(), FS), (dict(alignment=True), FS), (dict(alignment=True, sample_rate=16000, loudness=-16.0), 16000)):
        today, withp = run_(**base), run_(pitch=True, **base)
        tracker = get_pitch_tracker(voc.engine, rate)
        assert tracker is get_pitch_tracker(voc.engine, rate) and tracker.sample_rate == rate
        for a, b in zip(today, withp):
            assert a.pitch is None and a.phoneme_pitch is None
            assert b.audio.dtype == np.int16 and a.audio.tobytes() == b.audio.tobytes() and a.sample_rate == b.sample_rate == rate
            assert isinstance(b.pitch, PitchTrack) and (b.pitch.hop, b.pitch.sample_rate) == (tracker.hop, rate)
            F = b.audio.size // tracker.hop
            assert b.pitch.f0.shape == b.pitch.periodicity.shape == b.pitch.level_db.shape == (F,)
            exp = tracker.track(b.audio)
            assert np.array_equal(bits(exp.f0), bits(b.pitch.f0)) and np.array_equal(bits(exp.level_db), bits(b.pitch.level_db))
            if base.get("alignment"):
                assert np.array_equal(a.phoneme_spans, b.phoneme_spans)
                assert b.phoneme_pitch.shape == (len(b.phoneme_spans), 2) and b.phoneme_pitch.dtype == np.float32
                assert np.array_equal(b.phoneme_pitch, pitch_per_span(b.pitch, b.phoneme_spans))
            else:
                assert b.phoneme_spans is None and b.phoneme_pitch is None
            print(f"{b.text} at {rate} Hz: {b.audio.size} samples, {F} frames, {int((b.pitch.f0 > 0).sum())} voiced")


# ---------------------------------------------------------------- CPU only: the oracle and the host-side pieces
@pytest.mark.parametrize("geom", (GEOM, GEOM16), ids=("22050", "16000"))
def test_oracle_decides_the_designed_signal(geom):
    """The condition of checks 2 and 3, with the oracle alone: at least 95 % of the frames are decided, and the float32
    restatement picks the oracle's lag on them."""
    x = designed(geom["sample_rate"])
    o, ok, r32 = reference(x, "designed", geom)
    print(f"{geom['sample_rate']} Hz: {len(ok)} frames, {100 * ok.mean():.1f} % decided, {100 * o['voiced'].mean():.1f} % voiced")
    assert len(ok) == 206 and ok.mean() >= MIN_DECIDED and 0.6 < o["voiced"].mean() < 0.85
    assert np.array_equal(r32["lag"][ok], o["lag"][ok]) and np.array_equal(r32["voiced"][ok], o["voiced"][ok])
    # the segments read as designed: the glide rises from 90 to 180 Hz, the vibrato stays within 3 % of 220 Hz, 440 over a weak 220
    # reads 440, the 1e-4 tone is tracked at -84 dB, and silence and noise are unvoiced
    fs, hop = geom["sample_rate"], geom["hop"]
    at = lambda sec: int(round(sec * fs / hop))  # noqa: E731
    f0 = o["f0"]
    glide = f0[at(0.35):at(0.75)]
    assert (glide > 0).all() and (np.diff(glide) > 0).all() and 90 < glide[0] < 110 and 150 < glide[-1] < 180
    assert (np.abs(f0[at(1.15):at(1.55)] / 220.0 - 1.0) < 0.035).all()
    assert (np.abs(f0[at(1.65):at(1.85)] / 440.0 - 1.0) < 0.01).all()
    quiet = slice(at(1.95), at(2.05))
    assert (np.abs(f0[quiet] / 130.0 - 1.0) < 0.01).all() and (o["level_db"][quiet] < -80).all()
    assert not f0[:at(0.25)].any() and not f0[at(0.85):at(1.05)].any()


def test_pitch_per_span():
    track = PitchTrack(np.array([0, 100, 110, 0, 200, 0, 0, 300], np.float32), np.zeros(8, np.float32), np.zeros(8, np.float32), 10, 1000)
    spans = np.array([[0, 30], [30, 31], [31, 40], [40, 80], [75, 75], [50, 70], [70, 200]], np.int64)
    got = pitch_per_span(track, spans)
    assert got.dtype == np.float32 and got.shape == (7, 2)
    assert np.array_equal(got, np.array([[105, 2 / 3], [0, 0], [0, 0], [250, 0.5], [0, 0], [0, 0], [300, 1]], np.float32))
    with pytest.raises(ValueError):
        pitch_per_span(PitchTrack(np.zeros((2, 3), np.float32), None, None, 10, 1000), spans)


# ---------------------------------------------------------------- the emulator's runs
@pytest.fixture(autouse=True)
def leave_no_counts(request):
    """The session's engine is shared: its launch counters go back to zero behind every test here."""
    yield
    if "emu_engine" in request.fixturenames:
        request.getfixturevalue("emu_engine").profile_reset()


def test_exact_periods(emu_engine):
    check_exact_periods(emu_engine)


def test_designed_signal(emu_engine):
    check_designed(emu_engine)


def test_second_geometry(emu_engine):
    check_designed(emu_engine, GEOM16)


@pytest.mark.parametrize("case", ("ljspeech_high_short5", "ljspeech_high_echo"))
def test_golden_utterances(emu_engine, case):
    check_golden(emu_engine, case)


def test_edges_and_silence(emu_engine):
    check_edges(emu_engine)


def test_ragged_batch(emu_engine):
    check_ragged_batch(emu_engine)


def test_int16_input(emu_engine):
    check_int16_input(emu_engine)


def test_device_pointers(emu_engine):
    check_device_pointers(emu_engine, numpy_alloc)


def test_schedule(emu_engine):
    check_schedule(emu_engine)


def test_refusals_and_unload(emu_engine):
    check_refusals(emu_engine)


def test_tracker_object(emu_engine):
    t = PitchTracker(emu_engine, 16000)
    assert (t.tau_min, t.tau_max, t.window, t.hop) == (32, 320, 640, 186) and (t.threshold, t.interpolate) == (0.15, True)
    t22 = get_pitch_tracker(emu_engine, FS)
    assert t22 is get_pitch_tracker(emu_engine, FS) and (t22.tau_min, t22.tau_max, t22.window, t22.hop) == (45, 441, 896, 256)
    wide = PitchTracker(emu_engine, 48000, fmin=47.0)
    assert (wide.tau_max, wide.window) == (1021, 2048)
    x = voiced_row(4608)
    one = t22.track(x)
    assert isinstance(one, PitchTrack) and one.f0.shape == one.periodicity.shape == one.level_db.shape == (18,) and one.f0.dtype == np.float32
    assert (one.hop, one.sample_rate) == (256, FS) and t22.frames(4608) == 18 and (one.f0 > 0).sum() > 10
    two = t22.track(np.stack([x, x]), samples=(4608, 300))
    assert two.f0.shape == (2, 18) and np.array_equal(bits(two.f0[0]), bits(one.f0)) and not two.f0[1, 1:].any()
    assert t22.track(np.round(x * 32767).astype(np.int16)).f0.shape == (18,)
    with pytest.raises(ValueError):
        PitchTracker(emu_engine, FS, fmin=600.0)
    with pytest.raises(ffi.Mi355ttsError):
        PitchTracker(emu_engine, 48000, fmin=40.0)  # 1200 lags


def run_c_program(lib_path, tmp_path):
    """tests/c_abi/pitch_ragged.c against `lib_path`: a ragged batch with an empty row through the plain C ABI, every output, both
    input forms, each row compared with its batch-1 call inside the program.  (The same program is what the host sanitizers
    run: profiles/pitch.md.)"""
    import shutil
    import subprocess
    from pathlib import Path

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    repo = Path(__file__).resolve().parent.parent
    lib_path = Path(lib_path).resolve()
    exe = tmp_path / "pitch_ragged"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-O1", f"-I{repo / 'include'}",
                    str(repo / "tests" / "c_abi" / "pitch_ragged.c"), "-o", str(exe), str(lib_path), f"-Wl,-rpath,{lib_path.parent}", "-lm"], check=True)
    out = subprocess.run([str(exe), "0"], check=True, capture_output=True, text=True, timeout=600).stdout.splitlines()
    print("\n".join(out))
    assert out[-1] == "ok" and len(out) >= 5, out


def test_c_caller(emu_library, tmp_path):
    run_c_program(emu_library, tmp_path)


def test_sentence_path(emu_library):
    from tests.test_emu_analysis import tiny_voice
    from tests.test_emu_resample import vocoder

    check_sentence_path(tiny_voice(emu_library), vocoder(emu_library))
