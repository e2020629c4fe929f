"""Loudness (csrc/loudness.h: BS.1770-4 integrated loudness of delivered rows and gain-to-target delivery, five launches to
measure, a sixth to deliver) on the CPU emulator.

Oracle: tests/loudness_np.py — the definition of include/mi355tts.h in float64 (`oracle`: scipy.signal.lfilter twice, blocks,
gates) and its float32 restatement (`restate_f32`).

Bound: the K-weighted samples may lie 16 x as far from the float64 oracle as the float32 restatement does on the same input (the
project's rule), and never less than half an ulp of the row's largest weighted sample is allowed (the outputs ARE float32
values: an impulse's first samples are exact in both).  The integrated value is bounded the same way, never tighter than 4 ulp of
the float32 result (the final log and rounding), never looser than 0.1 LU (the meter tolerance of EBU Tech 3341).  The seam,
linearity, delivery and batch tests have no tolerance.  The check functions are shared with tests/test_gpu_loudness.py."""
import ctypes as C
import io
import math

import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.loudness import Loudness, get_loudness, k_weighting
from tests import loudness_np as L

FS = 22050
BLOCK, HOP = 8820, 2205
CHUNK, GROUP = 64, 64 * 256  # LD_CHUNK, LD_GROUP of csrc/loudness.h: a thread's samples, a workgroup's
LONG = 60000                 # three workgroups and a part of a fourth
LENGTHS = (0, 1, BLOCK - 1, BLOCK, BLOCK + HOP - 1, BLOCK + HOP, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, LONG)
RAGGED = (BLOCK, 0, LONG, CHUNK + 1, 1, BLOCK + HOP - 1, 2 * CHUNK + 1, BLOCK - 1)
CEILING = 10 ** (-1 / 20)
LAUNCHES_MEASURE, LAUNCHES_DELIVER = 5, 6
KERNELS = ("loudness_chunk_kernel", "loudness_carry_kernel", "loudness_weight_kernel", "loudness_segment_kernel", "loudness_gate_kernel")
_cache = {}


def meter(eng, fs=FS):
    key = (id(eng), fs)
    if key not in _cache:
        _cache[key] = Loudness(eng, fs)
    return _cache[key]


def reference(x, fs, key):
    """(float64 weighted, float64 L, the restatement's sample error, its L error): computed once per case, never changed."""
    key = ("ref", fs, key)
    if key not in _cache:
        w64, _, l64 = L.oracle(x, fs)
        w32, _, l32 = L.restate_f32(x, fs)
        e32 = float(np.abs(w32 - w64).max()) if len(x) else 0.0
        el = abs(float(l32) - l64) if np.isfinite(l64) else 0.0
        _cache[key] = (w64, l64, e32, el)
    return _cache[key]


def row(n):
    return L.voiced(n, FS, seed=n % 7)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def sample_bound(w64, e32):
    return max(16.0 * e32, 2.0 ** -24 * float(np.abs(w64).max())) if len(w64) else 0.0


def lufs_bound(l64, el):
    return min(max(16.0 * el, 4.0 * ulp32(l64)), 0.1)


def check_against_oracle(eng, x, fs, key, what):
    """One batch-1 call: every weighted sample and the integrated value against the float64 oracle, by the bound."""
    w64, l64, e32, el = reference(x, fs, key)
    r = eng.loudness(meter(eng, fs).model_id, x, want_weighted=True)
    w, lufs = r["weighted"], float(r["lufs"][0])
    assert w.shape == x.shape and w.dtype == np.float32 and r["gain"][0] == 1.0
    assert r["peak"][0] == (np.abs(x).max() if len(x) else 0.0)
    err = float(np.abs(w - w64).max()) if len(x) else 0.0
    if not np.isfinite(l64):
        print(f"{what}: sample error {err:.2e} (restatement {e32:.2e}), L = {lufs} (oracle {l64})")
        assert lufs == l64 and err <= sample_bound(w64, e32)
        return r
    dl = abs(lufs - l64)
    print(f"{what}: sample error {err:.2e} (restatement {e32:.2e}, bound {sample_bound(w64, e32):.2e}), L = {lufs:.6f} "
          f"(oracle {l64:.6f}): off by {dl:.2e} LU (restatement {el:.2e}, bound {lufs_bound(l64, el):.2e})")
    assert err <= sample_bound(w64, e32) and dl <= lufs_bound(l64, el)
    return r


def check_calibration(eng):
    """A 2 s, 997 Hz full-scale sine reads -3.01 LUFS at 48 000 Hz (no oracle: the standard's own figure) and what the oracle
    reads, -2.981, at 22 050 Hz."""
    x = L.tone(96000, 48000)
    r = check_against_oracle(eng, x, 48000, "tone48", "997 Hz at 48 000 Hz")
    assert abs(float(r["lufs"][0]) + 3.01) <= 0.1 and abs(L.oracle(x, 48000)[2] + 3.0103) <= 2e-4
    x = L.tone(44100, FS)
    check_against_oracle(eng, x, FS, "tone22", "997 Hz at 22 050 Hz")
    assert abs(L.oracle(x, FS)[2] + 2.981) <= 1e-3


def check_row_lengths(eng):
    """Rows at the edges of a block, a hop, a chunk and a workgroup, each alone against the oracle; then eight of them, unsorted,
    in one batch: every row the bits of its own batch-1 call."""
    m = meter(eng)
    assert (m.block, m.hop) == (BLOCK, HOP)
    alone = {}
    for n in LENGTHS:
        alone[n] = check_against_oracle(eng, row(n), FS, n, f"N = {n}")
    assert np.isneginf(alone[0]["lufs"][0]) and np.isfinite(alone[1]["lufs"][0]) and np.isfinite(alone[BLOCK - 1]["lufs"][0])
    batch = np.full((len(RAGGED), LONG + 40), 0.25, np.float32)  # what lies past a row's samples must not be read
    for b, n in enumerate(RAGGED):
        batch[b, :n] = row(n)
    r = eng.loudness(m.model_id, batch, RAGGED, target=-20.0, ceiling=CEILING, want_float=True, want_int16=True, want_weighted=True)
    for b, n in enumerate(RAGGED):
        one = eng.loudness(m.model_id, batch[b, :n], target=-20.0, ceiling=CEILING, want_float=True, want_int16=True, want_weighted=True)
        assert np.array_equal(bits(one["weighted"]), bits(alone[n]["weighted"])) and bits(one["lufs"])[0] == bits(alone[n]["lufs"])[0]
        for k in ("lufs", "gain", "peak"):
            assert bits(r[k])[b] == bits(one[k])[0], (k, n)
        for k in ("weighted", "f32"):
            assert np.array_equal(bits(r[k][b, :n]), bits(one[k])) and not r[k][b, n:].any(), (k, n)
        assert np.array_equal(r["i16"][b, :n], one["i16"]) and not r["i16"][b, n:].any()
    print(f"rows of {RAGGED} samples in one batch: each bit-identical to its batch-1 call")


def check_seams(eng):
    """A unit impulse on either side of a chunk seam and of a workgroup seam: the cascade's impulse response runs across the seam
    within the sample bound, and nothing sounds before the impulse."""
    m = meter(eng)
    for k, n in ((CHUNK - 1, 700), (CHUNK, 700), (GROUP - 1, GROUP + 700), (GROUP, GROUP + 700)):
        x = np.zeros(n, np.float32)
        x[k] = 1.0
        w64, _, e32, _ = reference(x, FS, ("impulse", k, n))
        w = eng.loudness(m.model_id, x, want_weighted=True)["weighted"]
        err = float(np.abs(w - w64).max())
        print(f"impulse at {k} of {n}: error {err:.2e} (restatement {e32:.2e}, bound {sample_bound(w64, e32):.2e}), "
              f"response after the seam up to {np.abs(w[k + 2:]).max():.3f}")
        assert not w[:k].any() and w[k] == np.float32(L.coefficients(FS)[0]["shelf_b"][0])
        assert err <= sample_bound(w64, e32) and np.abs(w[k + CHUNK:]).max() > 1e-3  # (it is still sounding a chunk later)


def gated_signal(quiet):
    return np.concatenate([L.tone(FS, FS, amp=0.5), L.tone(2 * FS, FS, amp=quiet)])


def check_linearity(eng):
    """weighted(2 x) == 2 weighted(x) bit for bit; the same blocks pass the gates, L moves by 20 log10 2 within 2 ulp."""
    m = meter(eng)
    for name, x in (("voiced", row(30000)), ("gated", gated_signal(0.05) * np.float32(0.4))):
        a = eng.loudness(m.model_id, x, want_weighted=True)
        b = eng.loudness(m.model_id, x * np.float32(2), want_weighted=True)
        d = float(b["lufs"][0]) - float(a["lufs"][0]) - 20 * math.log10(2)
        print(f"{name}: L({a['lufs'][0]:.6f}) -> L(2 x) = {b['lufs'][0]:.6f}: {d:.2e} from 20 log10 2")
        assert np.array_equal(bits(b["weighted"]), bits(a["weighted"] * np.float32(2))) and np.abs(a["weighted"]).max() > 0.01
        assert abs(d) <= 2 * ulp32(b["lufs"][0])


def check_gating(eng):
    """1 s of tone, then 2 s far below it: under -70 LUFS the absolute gate drops the tail, 20 dB down the relative gate does.
    Either way the meter reads what the oracle reads, more than 1 LU above the ungated mean."""
    for quiet, gate in ((1e-4, "absolute"), (0.05, "relative")):
        x = gated_signal(quiet)
        _, z, l64 = L.oracle(x, FS)
        plain = L.ungated(z)
        passed = L.gated(z)[1]
        assert l64 - plain > 1.0 and 0 < passed.sum() < len(z)  # the oracle alone, first
        under = L.OFFSET + 10 * np.log10(z) < L.ABS_GATE
        if gate == "absolute":  # (the first wholly quiet block still carries the filter's tail: the relative gate drops that one)
            assert under.sum() >= 10 and not passed[under].any() and (~passed & ~under).sum() <= 1
        else:
            assert not under.any()
        r = check_against_oracle(eng, x, FS, ("gate", quiet), f"{gate} gate ({int(passed.sum())} of {len(z)} blocks pass)")
        print(f"  gated {l64:.4f}, ungated {plain:.4f}")
        assert float(r["lufs"][0]) - plain > 1.0


def expected_i16(f32):
    return np.clip(np.rint(f32.astype(np.float64) * 32768), -32768, 32767).astype(np.int16)


def crest_heavy(n=30000):
    x = (0.004 * np.random.default_rng(3).standard_normal(n)).astype(np.float32)
    x[::997] = 0.9
    x[500::1994] = -0.95
    return x


def check_gain(eng):
    m = meter(eng)
    x = row(30000)
    r = eng.loudness(m.model_id, x, target=-16.0, ceiling=CEILING, want_float=True, want_int16=True)
    g = r["gain"][0]
    exp = L.gain(r["lufs"][0], r["peak"][0], -16.0, CEILING, 30.0)
    print(f"voiced row: L = {r['lufs'][0]:.4f}, gain {g:.6f} (definition {exp:.6f}), delivered peak {np.abs(r['f32']).max():.4f}")
    assert g.dtype == np.float32 and abs(float(g) - exp) <= ulp32(exp) and 1.5 < g < 3.0
    assert np.array_equal(bits(r["f32"]), bits(x * g)) and np.array_equal(r["i16"], expected_i16(r["f32"]))
    after = eng.loudness(m.model_id, r["f32"])["lufs"][0]
    assert abs(float(after) + 16.0) <= 4 * ulp32(16.0)  # (two roundings of L and one of g: 1.3 ulp of 16 at most)
    # a crest-heavy row whose target would clip: the ceiling decides
    x = crest_heavy()
    r = eng.loudness(m.model_id, x, target=-6.0, ceiling=CEILING, want_float=True, want_int16=True)
    g, peak = r["gain"][0], r["peak"][0]
    want = 10 ** ((-6.0 - float(r["lufs"][0])) / 20)
    top = np.abs(r["i16"].astype(np.int32)).max()
    print(f"crest-heavy row: L = {r['lufs'][0]:.3f}, the target asks for gain {want:.3f}, delivered {g:.6f} = ceiling / {peak:.3f}; "
          f"peak {np.abs(r['f32']).max():.6f}, int16 {top}")
    cap = float(np.float32(CEILING)) / float(peak)  # (the ceiling travels as a float)
    assert want > cap and abs(float(g) - cap) <= ulp32(g) and peak == np.float32(0.95)
    assert np.abs(r["f32"]).max() <= np.float32(CEILING) and top <= round(CEILING * 32768) < 32767
    assert np.array_equal(bits(r["f32"]), bits(x * g)) and np.array_equal(r["i16"], expected_i16(r["f32"]))
    # near silence: the largest gain decides
    x = (1e-3 * np.random.default_rng(4).standard_normal(30000)).astype(np.float32)
    r = eng.loudness(m.model_id, x, target=-16.0, ceiling=CEILING, max_gain_db=30.0, want_float=True)
    print(f"near-silent noise: L = {r['lufs'][0]:.3f}, gain {r['gain'][0]:.5f}")
    assert -70 < r["lufs"][0] < -50 and abs(float(r["gain"][0]) - 10 ** 1.5) <= ulp32(10 ** 1.5)
    assert np.array_equal(bits(r["f32"]), bits(x * r["gain"][0]))
    # silence: nothing to measure
    r = eng.loudness(m.model_id, np.zeros(30000, np.float32), target=-16.0, ceiling=CEILING, want_float=True, want_int16=True)
    assert np.isneginf(r["lufs"][0]) and r["gain"][0] == 1.0 and r["peak"][0] == 0 and not r["f32"].any() and not r["i16"].any()
    # measure only
    x = row(30000)
    r = eng.loudness(m.model_id, x, target=float("nan"), ceiling=0.01, want_float=True, want_int16=True)
    assert r["gain"][0] == 1.0 and np.array_equal(bits(r["f32"]), bits(x)) and np.array_equal(r["i16"], expected_i16(x))


def check_int16_input(eng):
    m = meter(eng)
    i16 = np.round(row(30000) * 32767).astype(np.int16)
    i16[:2] = (-32768, 32767)
    kw = dict(target=-20.0, ceiling=CEILING, want_float=True, want_int16=True, want_weighted=True)
    a = eng.loudness(m.model_id, i16, **kw)
    b = eng.loudness(m.model_id, i16.astype(np.float32) * np.float32(2.0 ** -15), **kw)
    assert a["peak"][0] == 1.0 and a["gain"][0] < 1.0
    for k in ("lufs", "gain", "peak", "weighted", "f32"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(a["i16"], b["i16"])


def check_schedule(eng):
    """Five launches measure and a sixth delivers, for a row of one block and for the long row alike, under their names."""
    m = meter(eng)
    eng.set_profiling(True)
    try:
        for n in (BLOCK, LONG):
            for kw, launches in ((dict(), LAUNCHES_MEASURE), (dict(want_weighted=True), LAUNCHES_MEASURE),
                                 (dict(target=-16.0, want_int16=True), LAUNCHES_DELIVER)):
                eng.profile_reset()
                eng.loudness(m.model_id, row(n), **kw)
                prof, counts = eng.profile(), eng.kernel_counts()
                ran = {k: v for k, v in counts.items() if v}
                print(f"N = {n} {kw}: {prof['elementwise']['launches']} launches, {prof['elementwise']['ms']:.4f} ms: {sorted(ran)}")
                assert prof["elementwise"]["launches"] == launches
                assert all(v["launches"] == 0 for k, v in prof.items() if k != "elementwise"), prof
                names = KERNELS + (("loudness_apply_kernel",) if launches == LAUNCHES_DELIVER else ())
                assert ran == {k: 1 for k in names}
                assert set(eng.profile_kernels()["elementwise"]) == {f"{k}/0" for k in names}
    finally:
        eng.set_profiling(False)
        eng.profile_reset()
    assert not any(eng.kernel_counts().values())


def _refused(fn, what, code=-1):
    with pytest.raises(ffi.Mi355ttsError) as e:
        fn()
    msg = str(e.value).split(": ", 1)[1]
    assert e.value.code == code and msg and what in msg, str(e.value)


def check_refusals(eng):
    lib, mid = eng.lib, C.c_int()
    c, block, hop = L.coefficients(FS)

    def load(block=block, hop=hop, params=True, out=True, **bad):
        p = ffi.LoudnessParamsC()
        for k, v in c.items():
            v = v.copy()
            if k in bad:
                v[bad[k][0]] = bad[k][1]
            setattr(p, k, (C.c_float * len(v))(*v.tolist()))
        p.block, p.hop = block, hop
        return lambda: ffi.check(lib, lib.mi355tts_load_loudness(eng._ctx, C.byref(p) if params else None, C.byref(mid) if out else None))

    _refused(load(params=False), "null")
    _refused(load(out=False), "null")
    for k, n in (("shelf_b", 3), ("shelf_a", 2), ("hp_b", 3), ("hp_a", 2)):
        for i in range(n):
            for v in (np.nan, np.inf, -np.inf):
                _refused(load(**{k: (i, v)}), "not finite")
    for b in (0, -5):
        _refused(load(block=b, hop=1), "block")
    for h in (0, -1, block + 1):
        _refused(load(hop=h), "hop")
    load(block=7, hop=7)()  # hop = block: accepted
    eng.unload(mid.value)
    m = meter(eng).model_id
    x = np.ascontiguousarray(row(700))
    i16 = np.zeros(700, np.int16)
    of, oi = np.zeros(710, np.float32), np.zeros(710, np.int16)
    res = np.zeros(3, np.float32)
    n = np.array([700], np.int64)

    def call(f32=x.ctypes.data, s16=None, samples=n, in_ld=700, target=-16.0, ceiling=1.0, max_db=30.0, o32=of.ctypes.data, o16=oi.ctypes.data,
             out_ld=710, mdl=m, B=1):
        s_p = None if samples is None else samples.ctypes.data_as(C.POINTER(C.c_int64))
        return lambda: ffi.check(lib, lib.mi355tts_loudness(eng._ctx, mdl, f32, s16, s_p, B, in_ld, target, ceiling, max_db, o32, o16, out_ld,
                                                            res[0:].ctypes.data, res[1:].ctypes.data, res[2:].ctypes.data, None, 0))

    _refused(call(samples=None), "null")
    _refused(call(s16=i16.ctypes.data), "exactly one")
    _refused(call(f32=None), "exactly one")
    _refused(call(B=0), "empty batch")
    _refused(call(in_ld=-1), "in_ld")
    for bad in (-1, 701):
        _refused(call(samples=np.array([bad], np.int64)), "samples[0]")
    big = (1 << 24) + 1  # (refused before anything is read)
    _refused(call(samples=np.array([big], np.int64), in_ld=big, out_ld=big), "2^24")
    _refused(call(out_ld=699), "out_ld")
    _refused(call(out_ld=-1), "out_ld")
    for bad in (0.0, -0.5, 1.0001, np.nan, np.inf):
        _refused(call(ceiling=bad), "peak_ceiling")
    for bad in (np.nan, np.inf, -np.inf):
        _refused(call(max_db=bad), "max_gain_db")
    _refused(call(mdl=10 ** 6), "no loudness meter", code=-5)
    call(o32=None, o16=None, out_ld=0)()  # no output pointer at all: valid, measures only
    assert -40 < res[0] < -10 and res[1] > 1.0 and res[2] == np.abs(x).max()
    call()()  # the context still works
    assert np.abs(of[:700]).max() > 0.1 and not of[700:].any()
    gone = eng.load_loudness(block=block, hop=hop, **c)
    assert np.isfinite(eng.loudness(gone, x)["lufs"][0])
    eng.unload(gone)
    _refused(lambda: eng.loudness(gone, x), "no loudness meter", code=-5)
    with pytest.raises(ValueError):
        eng.load_loudness(c["shelf_b"][:2], c["shelf_a"], c["hp_b"], c["hp_a"], block, hop)


def check_device_pointers(eng, alloc):
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE: device buffers (`alloc`: tests/test_emu_resample.py; float32 and int16 in, both
    delivered forms and the weighted rows out, row strides past the rows' samples, outputs pre-filled) give the host call's bits
    and zero tails up to the strides.  Then a batch whose rows are all empty, to host and to device destinations: zero outputs,
    zero weighted rows, -inf LUFS, gain 1, peak 0."""
    from tests.test_emu_resample import numpy_alloc

    m = meter(eng).model_id
    B = len(RAGGED)
    batch = np.full((B, LONG + 40), 0.25, np.float32)
    for b, n in enumerate(RAGGED):
        batch[b, :n] = row(n)
    i16 = np.round(batch * 32767).astype(np.int16)
    in_ld, out_ld = batch.shape[1], LONG + 61
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE

    def outputs(buffer):
        return buffer(np.full((B, out_ld), 7.0, np.float32)), buffer(np.full((B, out_ld), 7, np.int16)), buffer(np.full((B, in_ld), 7.0, np.float32))

    for src in (batch, i16):
        host = eng.loudness(m, src, RAGGED, target=-20.0, ceiling=CEILING, want_float=True, want_int16=True, want_weighted=True)
        dev, keep = alloc(src)
        ptrs = (None, dev) if src.dtype == np.int16 else (dev, None)
        (pf, get_f), (pi, get_i), (pw, get_w) = outputs(alloc)
        lufs, gain, peak = eng.loudness_raw(m, ptrs[0], ptrs[1], RAGGED, in_ld, -20.0, CEILING, 30.0, pf, pi, out_ld, pw, flags)
        f, i, w = get_f(), get_i(), get_w()
        for got, k in ((lufs, "lufs"), (gain, "gain"), (peak, "peak")):
            assert np.array_equal(bits(got), bits(host[k])), k
        assert np.array_equal(bits(f[:, :in_ld]), bits(host["f32"])) and not f[:, in_ld:].any()
        assert np.array_equal(i[:, :in_ld], host["i16"]) and not i[:, in_ld:].any()
        assert np.array_equal(bits(w), bits(host["weighted"]))
        for b, n in enumerate(RAGGED):
            assert not f[b, n:].any() and not i[b, n:].any() and not w[b, n:].any()
        # measuring only, from device memory
        lufs2, gain2, _ = eng.loudness_raw(m, ptrs[0], ptrs[1], RAGGED, in_ld, float("nan"), 1.0, 30.0, flags=ffi.IN_DEVICE)
        assert np.array_equal(bits(lufs2), bits(lufs)) and np.all(gain2 == 1.0)
        # no sample in any row
        h_ptrs = (None, src.ctypes.data) if src.dtype == np.int16 else (src.ctypes.data, None)
        for in_ptrs, buffer, fl in ((h_ptrs, numpy_alloc, 0), (ptrs, alloc, flags)):
            (pf, get_f), (pi, get_i), (pw, get_w) = outputs(buffer)
            lufs, gain, peak = eng.loudness_raw(m, in_ptrs[0], in_ptrs[1], (0, 0, 0), in_ld, -20.0, CEILING, 30.0, pf, pi, out_ld, pw, fl)
            assert np.all(lufs == -np.inf) and np.all(gain == 1.0) and not peak.any()
            assert not get_f()[:3].any() and not get_i()[:3].any() and not get_w()[:3].any()
        del keep


def check_sentence_path(tts, voc):
    import larynx_amd
    from larynx_amd.resample import get_resampler
    from larynx_amd.streaming import stream_raw_pcm

    def float_row(ids, before=0, after=0):
        return voc.mels_to_float_padded(tts.phonemes_to_mels(ids, settings=settings), None, before, after)

    rng = np.random.default_rng(41)
    sents = [(f"s{i}", synthetic.synthetic_phoneme_ids(rng, n, HP.TINY_GLOW.num_symbols)) for i, n in enumerate((11, 4, 26))]
    settings = {"seed": 77}
    s = tts.audio_settings
    assert s.sample_rate == FS
    today = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, alignment=True))
    same = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, alignment=True, loudness=None))
    for a, b in zip(today, same):
        assert b.audio.dtype == np.int16 and np.array_equal(a.audio, b.audio) and np.array_equal(a.phoneme_spans, b.phoneme_spans)
    m22 = get_loudness(voc.engine, FS)
    assert get_loudness(voc.engine, FS) is m22 and (m22.block, m22.hop) == (BLOCK, HOP)
    top = round(CEILING * 32768)

    def at_level(audio, meter_, what):
        """the delivered row reads -16 (int16 rounding and the project's bound both lie far inside the 0.1 LU meter tolerance),
        or sits at the ceiling, or took the largest gain"""
        lufs = float(meter_.measure(audio)[0])
        peak = int(np.abs(audio.astype(np.int32)).max())
        print(f"{what}: {audio.size} samples, {lufs:.3f} LUFS, int16 peak {peak}")
        assert abs(lufs + 16.0) <= 0.1 or top - 1 <= peak <= top
        return lufs

    leveled = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, alignment=True, loudness=-16))
    plain = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, loudness=-16.0))
    read = []
    for (text, ids), a, b, p in zip(sents, today, leveled, plain):
        exp = m22.normalize(float_row(ids), target=-16.0)
        assert b.sample_rate == FS and b.audio.dtype == np.int16 and b.audio.shape == a.audio.shape
        assert np.array_equal(b.audio, exp) and np.array_equal(p.audio, exp) and p.phoneme_spans is None
        assert np.array_equal(a.phoneme_spans, b.phoneme_spans)
        read.append(at_level(b.audio, m22, text))
    assert any(abs(v + 16.0) <= 0.1 for v in read)  # (not every row may sit at its ceiling)
    # pauses travel inside the float row and are part of what is measured
    text, ids = sents[0]
    audio = larynx_amd.sentence_task_leveled(text, ids, s, tts, settings, voc, None, 10, 20, None, -16.0)
    assert np.array_equal(audio, m22.normalize(float_row(ids, 220, 441), target=-16.0)) and audio.size == today[0].audio.size + 661
    assert not audio[:220].any() and not audio[-441:].any()
    assert np.array_equal(larynx_amd.sentence_task_leveled(text, ids, s, tts, settings, voc, None, 10, 20), today_padded(larynx_amd, sents[0], s, tts, settings, voc))
    sink = io.BytesIO()
    stats = stream_raw_pcm(iter(sents), tts, voc, sink, tts_settings=settings, loudness=-16)
    assert sink.getvalue() == b"".join(r.audio.tobytes() for r in plain)
    assert stats.sentences == 3 and stats.samples == sum(r.audio.size for r in plain)
    sink = io.BytesIO()
    stream_raw_pcm(iter(sents), tts, voc, sink, tts_settings=settings, loudness=None)
    assert sink.getvalue() == b"".join(r.audio.tobytes() for r in today)
    # another rate: resampled first, then measured with the 16 kHz coefficients
    rs, m16 = get_resampler(voc.engine, FS, 16000), get_loudness(voc.engine, 16000)
    assert (m16.block, m16.hop) == (6400, 1600) and not np.array_equal(m16.coefficients["hp_a"], m22.coefficients["hp_a"])
    at16 = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, sample_rate=16000, loudness=-16))
    for (text, ids), r in zip(sents, at16):
        exp = m16.normalize(rs.resample(float_row(ids)), target=-16.0)
        assert r.sample_rate == 16000 and np.array_equal(r.audio, exp)
        at_level(r.audio, m16, f"{text} at 16 kHz")
    sink = io.BytesIO()
    stream_raw_pcm(iter(sents), tts, voc, sink, tts_settings=settings, sample_rate=16000, loudness=-16)
    assert sink.getvalue() == b"".join(r.audio.tobytes() for r in at16)


def today_padded(larynx_amd, sent, s, tts, settings, voc):
    return larynx_amd.sentence_task(sent[0], sent[1], s, tts, settings, voc, None, 10, 20)


# ---------------------------------------------------------------- CPU only: the design and the oracle
def test_design_reproduces_the_standards_table():
    c = k_weighting(48000)
    table = {"shelf_b": (1.53512485958697, -2.69169618940638, 1.19839281085285), "shelf_a": (-1.69065929318241, 0.73248077421585),
             "hp_b": (1.0, -2.0, 1.0), "hp_a": (-1.99004745483398, 0.99007225036621)}
    for k, v in table.items():
        err = float(np.abs(c[k] - np.array(v)).max())
        print(f"{k}: {err:.1e} from the table")
        assert c[k].dtype == np.float64 and err <= 1e-12
    for fs in (8000, 16000, 22050, 24000, 44100):  # no published table: the filters stay stable and keep their shape
        c = k_weighting(fs)
        for a in (c["shelf_a"], c["hp_a"]):
            assert np.abs(np.roots(np.r_[1.0, a])).max() < 1.0
    r = np.abs(np.roots(np.r_[1.0, k_weighting(FS)["hp_a"]])).max()
    print(f"high-pass pole radius at 22 050 Hz: {r:.5f}")
    assert abs(r - 0.989) < 1e-3


def test_restatement_error_is_what_the_bound_is_built_on():
    w64, l64, e32, el = reference(row(30000), FS, 30000)
    print(f"float32 restatement on 30 000 voiced samples: sample error {e32:.2e} of a {np.abs(w64).max():.2f} peak, L off by {el:.2e} LU")
    assert 1e-6 < e32 < 1e-4 and el < 1e-3


# ---------------------------------------------------------------- the emulator's runs
@pytest.fixture(autouse=True)
def leave_no_counts(request):
    """The session's engine is shared: its launch counters go back to zero behind every test here."""
    yield
    if "emu_engine" in request.fixturenames:
        request.getfixturevalue("emu_engine").profile_reset()


def test_calibration_tone(emu_engine):
    check_calibration(emu_engine)


def test_row_lengths_and_ragged_batch(emu_engine):
    check_row_lengths(emu_engine)


def test_seams(emu_engine):
    check_seams(emu_engine)


def test_linearity_is_bit_exact(emu_engine):
    check_linearity(emu_engine)


def test_gating(emu_engine):
    check_gating(emu_engine)


def test_gain_and_delivery(emu_engine):
    check_gain(emu_engine)


def test_int16_input(emu_engine):
    check_int16_input(emu_engine)


def test_schedule(emu_engine):
    check_schedule(emu_engine)


def test_device_pointers(emu_engine):
    from tests.test_emu_resample import numpy_alloc

    check_device_pointers(emu_engine, numpy_alloc)


def test_refusals_and_unload(emu_engine):
    check_refusals(emu_engine)


def run_c_program(lib_path, tmp_path):
    """tests/c_abi/loudness_ragged.c against `lib_path`: the ragged batch through the plain C ABI, each row compared with its
    batch-1 call inside the program.  (The same program is what the host sanitizers run: profiles/loudness.md.)"""
    import re
    import shutil
    import struct
    import subprocess
    from pathlib import Path

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    repo = Path(__file__).resolve().parent.parent
    lib_path = Path(lib_path).resolve()
    exe = tmp_path / "loudness_ragged"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-O1", f"-I{repo / 'include'}",
                    str(repo / "tests" / "c_abi" / "loudness_ragged.c"), "-o", str(exe), str(lib_path), f"-Wl,-rpath,{lib_path.parent}", "-lm"], check=True)
    out = subprocess.run([str(exe), "0"], check=True, capture_output=True, text=True, timeout=600).stdout.splitlines()
    assert out[-1] == "ok" and len(out) == len(RAGGED) + 1, out
    for line, n in zip(out, RAGGED):
        m = re.match(r"row \d+ n (\d+) lufs ([0-9a-f]{8}) gain ([0-9a-f]{8}) peak ([0-9a-f]{8})", line)
        assert m and int(m.group(1)) == n, line
        lufs, gain, peak = (struct.unpack("<f", struct.pack("<I", int(m.group(k), 16)))[0] for k in (2, 3, 4))
        print(f"C caller, N = {n}: {lufs:.4f} LUFS, gain {gain:.5f}, peak {peak:.4f}")
        assert (lufs == -np.inf and gain == 1.0 and peak == 0.0) if n == 0 else (-40 < lufs < 0 and 0 < np.float32(gain) * np.float32(peak) <= np.float32(CEILING))


def test_c_caller(emu_library, tmp_path):
    run_c_program(emu_library, tmp_path)


def test_sentence_path(emu_library):
    from tests.test_emu_analysis import tiny_voice
    from tests.test_emu_resample import vocoder

    check_sentence_path(tiny_voice(emu_library), vocoder(emu_library))
