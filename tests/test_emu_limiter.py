"""The true-peak meter and look-ahead limiter (csrc/limiter.h: two launches meter, six limit) on the CPU emulator.

Oracle: tests/limiter_np.py — the definition of include/mi355tts.h in float64 (`oracle`) and its float32 restatement
(`restate_f32`), both sequential.

Bounds.  With release a = 0 nothing is carried and every step is pinned: the curve, both delivered forms, the true peak and
the smallest gain equal the restatement bit for bit, and the true peak equals max|mi355tts_resample(x, os, 1)| (maxed with
max|x|) bit for bit.  With a > 0 the device carries a^len * d in one product where the restatement multiplies len times, so the
curve is compared with the float64 oracle under the project's rule: 16 x the restatement's own error on the same
input, never tighter than 4 ulp of 1.0.  The limiter property s[n] <= min(c[n], c[n - 1]) holds in real arithmetic up to the
window's permitted distance from sum 1 (1e-6, the load-time check) and is asserted with that plus the case's bound.  Batch rows,
int16 input and device pointers have no tolerance.  The check functions are shared with tests/test_gpu_limiter.py."""
import ctypes as C
import io

import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.limiter import design_interpolator, get_limiter, release_coefficient, smoothing_window
from larynx_amd.loudness import get_loudness
from tests import limiter_np as M
from tests import loudness_np as L
from tests.test_emu_resample import numpy_alloc

FS = 22050
TILE, CHUNK, GROUP = 256, 16, 4096  # LM_TILE, LM_CHUNK, LM_GROUP of csrc/limiter.h
LA = 33                              # 1.5 ms at 22 050 Hz
A50 = float(np.float32(release_coefficient(FS, 50.0)))
LONG = 60000
CEILING = 10 ** (-1 / 20)
GAIN = 4.0  # the voiced rows peak at 0.27: their own crests pass the ceiling, not the clicks alone
ULP1 = 2.0 ** -23
WINDOW_TOL = 1e-6
LAUNCHES_METER, LAUNCHES_LIMIT = 2, 6
METER_KERNELS = {"limiter_peak_kernel": 1, "limiter_reduce_kernel": 1}
LIMIT_KERNELS = {"limiter_peak_kernel": 1, "limiter_reduce_kernel": 2, "limiter_hold_kernel": 1, "limiter_carry_kernel": 1,
                 "limiter_apply_kernel": 1}
# rows at the edges of a tile, a chunk and a workgroup, the last two also where the row's POSITIONS (samples + la) meet them
LENGTHS = (0, 1, 2, LA, LA + 1, CHUNK - 1, CHUNK, CHUNK + 1, TILE - 1, TILE, TILE + 1, GROUP - LA - 1, GROUP - LA, GROUP - LA + 1,
           GROUP - 1, GROUP, GROUP + 1, LONG)
RAGGED = (TILE + 1, 0, 9000, 1, GROUP - LA, 2, LA, GROUP + 1)
# peaks on both sides of a chunk seam and of a workgroup seam, in samples and in positions (sample + la)
SEAM_ROW = 9000
SEAM_PEAKS = (CHUNK - 1, CHUNK, 3 * CHUNK - LA - 1, 3 * CHUNK - LA, GROUP - LA - 1, GROUP - LA, GROUP - 1, GROUP, 2 * GROUP - LA - 1,
              2 * GROUP - LA)
_cache = {}


class Config:
    """One loaded limiter: its tables as the device holds them."""

    def __init__(self, eng, os, la, a):
        self.os, self.la, self.a = os, la, float(np.float32(a))
        self.taps = design_interpolator(os)[0] if os > 1 else None
        self.w = smoothing_window(la)
        self.model_id = eng.load_limiter(self.taps, self.w, os, self.a)

    @property
    def key(self):
        return (self.os, self.la, self.a)

    def args(self):
        return (self.os, self.taps, self.la, self.a, self.w)


def config(eng, os=4, la=LA, a=A50):
    key = ("cfg", id(eng), os, la, float(np.float32(a)))
    if key not in _cache:
        _cache[key] = Config(eng, os, la, a)
    return _cache[key]


def reference(x, gain, ceiling, cfg, key):
    """(float64 oracle, float32 restatement) of one case: computed once, never changed."""
    key = ("ref", cfg.key, float(gain), float(ceiling), key)
    if key not in _cache:
        _cache[key] = (M.oracle(x, gain, ceiling, *cfg.args()), M.restate_f32(x, gain, ceiling, *cfg.args()))
    return _cache[key]


def row(n, peaks=None):
    """A voiced row whose own crests pass the ceiling at GAIN here and there, with clicks at `peaks` (default: its two ends)."""
    x = L.voiced(n, FS, seed=n % 7)
    for i, p in enumerate((0, n - 1) if peaks is None else peaks):
        if 0 <= p < n:
            x[p] = 0.9 if i % 2 == 0 else -0.9
    return x


def seam_row():
    return row(SEAM_ROW, SEAM_PEAKS)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def expected_i16(f32):
    return np.clip(np.rint(f32.astype(np.float64) * 32768), -32768, 32767).astype(np.int16)


def limit(eng, cfg, x, gain=GAIN, ceiling=CEILING, samples=None):
    return eng.limit(cfg.model_id, x, samples, gain=gain, ceiling=ceiling, want_float=True, want_int16=True, want_curve=True)


def bound(err32):
    return max(16.0 * err32, 4.0 * ULP1)


def check_property(r, x, gain, ceiling, o64, slack, what):
    """The limiter property on one delivered row."""
    n = len(x)
    top = round(ceiling * 32768)
    assert r["f32"].shape == (n,) and r["curve"].shape == (n,) and r["i16"].dtype == np.int16
    if n == 0:
        return
    assert np.abs(r["f32"]).max() <= np.float32(ceiling), what
    assert np.abs(r["i16"].astype(np.int32)).max() <= top, what
    assert r["curve"].max() <= 1.0 and r["curve"].min() >= 0.0, what
    c = o64["c"]
    both = np.minimum(c, np.concatenate([[1.0], c[:-1]]))
    excess = float((r["curve"].astype(np.float64) - both).max())
    print(f"  {what}: curve - min(c[n], c[n-1]) at most {excess:.2e} (allowed {WINDOW_TOL + slack:.2e}), smallest gain {r['min_gain'][0]:.4f}")
    assert excess <= WINDOW_TOL + slack, what
    assert r["min_gain"][0] == r["curve"].min()


def check_exact_case(eng, cfg, x, key, what, resampler=None):
    """a = 0: everything equals the float32 restatement bit for bit."""
    assert cfg.a == 0.0
    o64, r32 = reference(x, GAIN, CEILING, cfg, key)
    r = limit(eng, cfg, x)
    n = len(x)
    lim = int((r32["c"] < 1).sum())
    print(f"{what}: N = {n}, os {cfg.os}, la {cfg.la}: true peak {r['true_peak'][0]:.6f}, {lim} samples ask for less than 1")
    assert np.array_equal(bits(r["curve"]), bits(r32["s"])), what
    assert np.array_equal(bits(r["f32"]), bits(r32["y"])), what
    assert np.array_equal(r["i16"], r32["i16"]) and np.array_equal(r["i16"], expected_i16(r["f32"])), what
    assert bits(r["true_peak"])[0] == bits(r32["TP"])[0] and bits(r["min_gain"])[0] == bits(r32["min_gain"])[0], what
    meter = eng.limit(cfg.model_id, x)
    assert bits(meter["true_peak"])[0] == bits(r["true_peak"])[0] and meter["min_gain"][0] == 1.0 and meter["f32"] is None
    if resampler is not None and n:
        u = eng.resample(resampler, x)[0]
        assert u.shape == (n * cfg.os,)
        assert bits(r["true_peak"])[0] == bits(max(np.abs(u).max(), np.abs(x).max()))[0], what
    check_property(r, x, GAIN, CEILING, o64, bound(float(np.abs(r32["s"] - o64["s"]).max()) if n else 0.0), what)
    return r


def check_exact(eng):
    """Item 1 and the shapes of item 4 with a = 0: every length alone; then the other oversampling factors and look-aheads."""
    cfg = config(eng, 4, LA, 0.0)
    rs = eng.load_resampler(cfg.taps, 4, 1)
    try:
        some = 0
        for n in LENGTHS:
            r = check_exact_case(eng, cfg, row(n), n, f"N = {n}", rs)
            some += int(n > 0 and r["min_gain"][0] < 1.0)
        assert some >= len(LENGTHS) - 4  # (the clicks at the rows' ends are limited: the test is not vacuous)
        check_exact_case(eng, cfg, seam_row(), "seams", "peaks at the seams", rs)
    finally:
        eng.unload(rs)
    for os, la in ((1, LA), (4, 0), (2, 1024), (8, 5)):
        c2 = config(eng, os, la, 0.0)
        rs = eng.load_resampler(c2.taps, os, 1) if os > 1 else None
        try:
            for n in sorted({1, 2, la, la + 1, TILE + 1, GROUP - la, GROUP + 1}):
                if n > 0:
                    check_exact_case(eng, c2, row(n), n, f"os {os}, la {la}, N = {n}", rs)
            check_exact_case(eng, c2, seam_row(), "seams", f"os {os}, la {la}, peaks at the seams", rs)
        finally:
            if rs is not None:
                eng.unload(rs)


def check_release_case(eng, cfg, x, key, what):
    o64, r32 = reference(x, GAIN, CEILING, cfg, key)
    r = limit(eng, cfg, x)
    e32 = float(np.abs(r32["s"].astype(np.float64) - o64["s"]).max())
    err = float(np.abs(r["curve"].astype(np.float64) - o64["s"]).max())
    ey = float(np.abs(r["f32"].astype(np.float64) - o64["y"]).max())
    etp = abs(float(r["true_peak"][0]) - float(o64["TP"]))
    etp32 = abs(float(r32["TP"]) - float(o64["TP"]))
    print(f"{what}: N = {len(x)}, os {cfg.os}, la {cfg.la}, a {cfg.a:.6f}: curve {err:.2e} from the oracle (restatement {e32:.2e}, "
          f"bound {bound(e32):.2e}); delivered row {ey:.2e}; true peak {etp:.2e} (restatement {etp32:.2e}); smallest gain {r['min_gain'][0]:.4f}")
    assert err <= bound(e32) and etp <= bound(etp32)
    assert r["min_gain"][0] < 0.9 and np.array_equal(r["i16"], expected_i16(r["f32"]))
    check_property(r, x, GAIN, CEILING, o64, bound(e32), what)
    return r


def check_release(eng):
    """Item 2: a > 0, the curve against the float64 oracle; the seams of chunks and workgroups carry the release."""
    for os, la, a in ((4, LA, A50), (1, 0, 0.9), (2, 1024, 0.9995)):
        cfg = config(eng, os, la, a)
        check_release_case(eng, cfg, seam_row(), "seams", "peaks at the seams")
        check_release_case(eng, cfg, row(GROUP - la), GROUP - la, "one workgroup of positions")
    cfg = config(eng)
    r = check_release_case(eng, cfg, row(LONG, (0, LONG - 1, 20000, 3 * GROUP - LA - 1)), LONG, "the long row")
    # the release is still holding the curve down a chunk and a workgroup behind a click, and nothing moves before its look-ahead
    p = 100
    x = np.zeros(2 * GROUP, np.float32)
    x[p] = 0.9
    s = check_release_case(eng, cfg, x, "click", "one click")["curve"]
    print(f"click at {p}: curve {s[p]:.4f} there, {s[p + 2 * CHUNK]:.4f} two chunks later, {s[p + GROUP]:.6f} a workgroup later")
    assert s[p] < 0.5 and s[p] < s[p + 2 * CHUNK] < s[p + GROUP] < 1.0
    assert (s[:p - LA - 17] == 1.0).all()  # (the interpolator reaches 16 samples back, the hold la more)
    return r


def check_passthrough(eng):
    """A row under the ceiling everywhere (TP G <= ceiling) comes back as x G exactly, with curve 1.0."""
    for cfg in (config(eng), config(eng, 1, 0, 0.9), config(eng, 2, 1024, 0.9995)):
        x = L.voiced(5000, FS, seed=2)
        tp = float(eng.limit(cfg.model_id, x)["true_peak"][0])
        g = np.float32(0.98 * np.float32(CEILING) / tp)
        assert np.float32(tp) * g <= np.float32(CEILING) and g > 1.0
        r = limit(eng, cfg, x, gain=g)
        print(f"os {cfg.os}, la {cfg.la}: true peak {tp:.4f}, gain {g:.4f}: delivered peak {np.abs(r['f32']).max():.4f}, curve in [{r['curve'].min()}, {r['curve'].max()}]")
        assert np.array_equal(bits(r["f32"]), bits(x * g)) and (r["curve"] == 1.0).all() and r["min_gain"][0] == 1.0
        assert np.array_equal(r["i16"], expected_i16(x * g))
    r = limit(eng, config(eng), np.zeros(700, np.float32))
    assert r["true_peak"][0] == 0.0 and not r["f32"].any() and (r["curve"] == 1.0).all()


def ragged_batch():
    batch = np.full((len(RAGGED), 9000 + 40), 0.25, np.float32)  # what lies past a row's samples must not be read
    for b, n in enumerate(RAGGED):
        batch[b, :n] = seam_row() if n == SEAM_ROW else row(n)
    gains = np.array([GAIN, 1.0, 2.5, 3.0, GAIN, 0.5, GAIN, 1.7], np.float32)
    return batch, gains


def check_ragged_batch(eng):
    """Eight rows, unsorted, each with its own gain, in one batch: every row the bits of its own batch-1 call."""
    cfg = config(eng)
    batch, gains = ragged_batch()
    r = limit(eng, cfg, batch, gain=gains, samples=RAGGED)
    m = eng.limit(cfg.model_id, batch, RAGGED)
    for b, n in enumerate(RAGGED):
        one = limit(eng, cfg, batch[b, :n], gain=gains[b])
        for k in ("true_peak", "min_gain"):
            assert bits(r[k])[b] == bits(one[k])[0], (k, n)
        assert bits(m["true_peak"])[b] == bits(one["true_peak"])[0]
        for k in ("f32", "curve"):
            assert np.array_equal(bits(r[k][b, :n]), bits(one[k])) and not r[k][b, n:].any(), (k, n)
        assert np.array_equal(r["i16"][b, :n], one["i16"]) and not r["i16"][b, n:].any()
    assert r["true_peak"][1] == 0.0 and r["min_gain"][1] == 1.0
    print(f"rows of {RAGGED} samples in one batch: each bit-identical to its batch-1 call")


def check_int16_input(eng):
    cfg = config(eng)
    i16 = np.round(seam_row() * 32767).astype(np.int16)
    i16[:2] = (-32768, 32767)
    a = limit(eng, cfg, i16)
    b = limit(eng, cfg, i16.astype(np.float32) * np.float32(2.0 ** -15))
    assert a["true_peak"][0] >= 1.0 and a["min_gain"][0] < 0.5
    for k in ("true_peak", "min_gain", "f32", "curve"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(a["i16"], b["i16"])


def check_intersample(eng):
    """Item 5: 0.9 sin(2 pi n / 4 + pi / 4) has sample peak 0.636 and true peak 0.9; limited to 0.5, the output's true peak, read by
    a meter call on it, against the oracle's."""
    cfg = config(eng)
    x = M.intersample(4000)
    o64, r32 = reference(x, 1.0, 0.5, cfg, "intersample")
    r = limit(eng, cfg, x, gain=1.0, ceiling=0.5)
    etp, etp32 = abs(float(r["true_peak"][0]) - float(o64["TP"])), abs(float(r32["TP"]) - float(o64["TP"]))
    print(f"sample peak {np.abs(x).max():.4f}, true peak {r['true_peak'][0]:.6f} (oracle {o64['TP']:.6f}: off by {etp:.2e}, restatement {etp32:.2e})")
    assert abs(np.abs(x).max() - 0.9 / np.sqrt(2)) < 1e-6 and abs(float(o64["tp"][200:-200].max()) - 0.9) < 1e-3 and etp <= bound(etp32)  # (the row's abrupt ends ring higher)
    out_tp = float(eng.limit(cfg.model_id, r["f32"])["true_peak"][0])
    otp64 = float(M.true_peaks(o64["y"], cfg.taps, cfg.os, False).max())           # (the float64 row, its float64 true peak)
    otp32 = float(M.true_peaks(r32["y"], cfg.taps, cfg.os, True).max())
    mid = float(M.true_peaks(o64["y"], cfg.taps, cfg.os, False)[200:-200].max())
    print(f"limited to 0.5: the output's true peak {out_tp:.8f} (oracle {otp64:.8f}, away from the row ends {mid:.8f}; restatement "
          f"{abs(otp32 - otp64):.2e} off), sample peak {np.abs(r['f32']).max():.6f}")
    assert abs(out_tp - otp64) <= bound(abs(otp32 - otp64)) and abs(mid - 0.5) < 1e-3
    return out_tp - 0.5


def check_schedule(eng):
    """Item 6: two launches meter, six limit, for a short row and the long row alike, under their names."""
    cfg = config(eng)
    eng.set_profiling(True)
    try:
        for n in (TILE + 1, LONG):
            for kw, names in ((dict(), METER_KERNELS), (dict(want_curve=True), LIMIT_KERNELS), (dict(want_int16=True, gain=GAIN, ceiling=CEILING), LIMIT_KERNELS)):
                eng.profile_reset()
                eng.limit(cfg.model_id, row(n), **kw)
                prof, counts = eng.profile(), eng.kernel_counts()
                ran = {k: v for k, v in counts.items() if v}
                print(f"N = {n} {sorted(kw)}: {prof['elementwise']['launches']} launches, {prof['elementwise']['ms']:.4f} ms: {ran}")
                assert prof["elementwise"]["launches"] == sum(names.values()) == (LAUNCHES_METER if names is METER_KERNELS else LAUNCHES_LIMIT)
                assert all(v["launches"] == 0 for k, v in prof.items() if k != "elementwise"), prof
                assert ran == names
                assert set(eng.profile_kernels()["elementwise"]) == {f"{k}/0" for k in names}
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
    """Item 7: every invalid argument, each with its reason."""
    lib, mid = eng.lib, C.c_int()
    taps0, H = design_interpolator(4)
    w0 = smoothing_window(LA)

    def load(os=4, half_len=H, la=LA, a=0.5, taps=taps0, w=w0, params=True, out=True):
        p = ffi.LimiterParamsC(os, half_len, la, a)
        taps = None if taps is None else np.ascontiguousarray(taps, np.float32)
        w = None if w is None else np.ascontiguousarray(w, np.float32)
        return lambda: ffi.check(lib, lib.mi355tts_load_limiter(eng._ctx, C.byref(p) if params else None, ffi.ptr(taps), ffi.ptr(w),
                                                                C.byref(mid) if out else None))

    _refused(load(params=False), "null")
    _refused(load(out=False), "null")
    _refused(load(w=None), "null")
    _refused(load(taps=None), "null")
    for bad in (0, -1, 9):
        _refused(load(os=bad), "oversample")
    _refused(load(half_len=-1), "half_len")
    _refused(load(half_len=4 * 64, taps=np.zeros(2 * 4 * 64 + 1)), "taps per phase")  # 513 taps over 4 phases: 129 each
    for bad in (np.nan, np.inf, -np.inf):
        t = taps0.copy()
        t[5] = bad
        _refused(load(taps=t), "not finite")
    for bad in (-1, 1025):
        _refused(load(la=bad, w=np.full(1030, 1 / 1030)), "lookahead")
    for bad in (-0.1, 1.0, 1.5, np.nan, np.inf):
        _refused(load(a=bad), "release")
    for bad in (np.nan, np.inf):
        w = w0.copy()
        w[3] = bad
        _refused(load(w=w), "not finite")
    w = w0.copy()
    w[3] = -w[3]
    _refused(load(w=w), "negative")
    _refused(load(w=w0 * np.float32(1.00001)), "sums to")
    _refused(load(w=w0 * np.float32(0.9999)), "sums to")
    load(os=1, taps=None, la=0, w=np.ones(1), a=0.0)()  # oversample 1 reads no taps; the one-entry window; no memory: accepted
    eng.unload(mid.value)
    cfg = config(eng)
    m = cfg.model_id
    x = np.ascontiguousarray(row(700))
    i16 = np.zeros(700, np.int16)
    of, oi, oc = np.zeros(710, np.float32), np.zeros(710, np.int16), np.zeros(700, np.float32)
    res = np.zeros(2, np.float32)
    n = np.array([700], np.int64)
    g1 = np.array([GAIN], np.float32)

    def call(f32=x.ctypes.data, s16=None, samples=n, in_ld=700, gain=g1, ceiling=CEILING, o32=of.ctypes.data, o16=oi.ctypes.data, out_ld=710,
             crv=oc.ctypes.data, mdl=m, B=1):
        s_p = None if samples is None else samples.ctypes.data_as(C.POINTER(C.c_int64))
        return lambda: ffi.check(lib, lib.mi355tts_limit(eng._ctx, mdl, f32, s16, s_p, B, in_ld, ffi.ptr(gain), ceiling, o32, o16, out_ld,
                                                         res[0:].ctypes.data, res[1:].ctypes.data, crv, 0))

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
        _refused(call(ceiling=bad), "ceiling")
    for bad in (np.nan, np.inf, -np.inf, -1.0):
        _refused(call(gain=np.array([bad], np.float32)), "gain[0]")
    _refused(call(mdl=10 ** 6), "no limiter", code=-5)
    _refused(call(mdl=get_loudness(eng, FS).model_id), "no limiter", code=-5)  # (another kind of model)
    call(o32=None, o16=None, out_ld=0, crv=None)()  # no output at all: valid, a meter call
    assert res[0] == np.float32(0.9) or res[0] > 0.9
    call(gain=None)()  # NULL gains: 1
    assert np.array_equal(bits(of[:700]), bits(limit(eng, cfg, x, gain=1.0)["f32"])) and not of[700:].any()
    call()()  # the context still works
    assert 0.8 < np.abs(of[:700]).max() <= np.float32(CEILING) and not of[700:].any() and 0 < res[1] < 1 and res[1] == oc.min()
    gone = eng.load_limiter(cfg.taps, cfg.w, 4, A50)
    assert eng.limit(gone, x)["true_peak"][0] == res[0]
    eng.unload(gone)
    _refused(lambda: eng.limit(gone, x), "no limiter", code=-5)
    with pytest.raises(ValueError):
        eng.load_limiter(cfg.taps[:-1], cfg.w, 4, A50)


def check_the_point(eng):
    """Item 8: the tone-plus-clicks row.  `normalize` stops at the click's cap, far under the target; `normalize_limited` arrives."""
    m, lim = get_loudness(eng, FS), get_limiter(eng, FS)
    assert get_limiter(eng, FS) is lim and (lim.oversample, lim.lookahead) == (4, LA) and abs(lim.release - A50) < 1e-7
    x = M.tone_with_clicks(4 * FS)
    l0 = L.oracle(x, FS)[2]
    # today's delivery: the oracle's capped gain
    g_cap = L.gain(l0, np.abs(x).max(), -16.0, np.float32(CEILING), 30.0)
    want = L.oracle(x.astype(np.float64) * g_cap, FS)[2]
    got = float(m.measure(m.normalize(x, target=-16.0, int16=False))[0])
    print(f"the row reads {l0:.2f} LUFS; normalize: gain {g_cap:.3f} (the target asks for {10 ** ((-16 - l0) / 20):.3f}), delivered {got:.2f} LUFS (oracle {want:.2f})")
    assert abs(got - want) <= 0.1 and want < -16.0 - 6.0
    # the limiter: the oracle with the same one correction pass
    y64, l64, g64, passes = M.normalize_limited(x, FS, -16.0, np.float32(CEILING), 30.0, lim.oversample, lim.taps, lim.lookahead, lim.release, lim.window)
    y = m.normalize_limited(x, target=-16.0, limiter=lim, int16=False)
    got = float(m.measure(y)[0])
    tp = float(lim.true_peak(y)[0])
    print(f"normalize_limited: delivered {got:.3f} LUFS (oracle {l64:.3f} after {passes} passes, gain {g64:.3f}), sample peak {np.abs(y).max():.6f}, "
          f"true peak {tp:.8f} (ceiling {CEILING:.8f})")
    assert passes == 2 and abs(l64 + 16.0) <= 0.1 and abs(got - l64) <= 0.1
    assert np.abs(y).max() <= np.float32(CEILING)
    i16 = m.normalize_limited(x, target=-16.0, limiter=lim)
    assert i16.dtype == np.int16 and np.array_equal(i16, expected_i16(y))
    # a row that needs no limiting: normalize's own output
    x = L.voiced(30000, FS, seed=1, amp=0.2)
    a, b = m.normalize(x, target=-23.0, int16=False), m.normalize_limited(x, target=-23.0, limiter=lim, int16=False)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(m.normalize(x, target=-23.0), m.normalize_limited(x, target=-23.0, limiter=lim))
    assert float(lim.true_peak(a)[0]) < CEILING and np.abs(a).max() > 0.05
    # silence and the empty row: gain 1
    assert not m.normalize_limited(np.zeros(3000, np.float32), limiter=lim).any() and m.normalize_limited(np.zeros(0, np.float32), limiter=lim).shape == (0,)
    with pytest.raises(ValueError):
        m.normalize_limited(x)
    return tp - CEILING


def check_device_pointers(eng, alloc):
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE: device buffers (`alloc`: tests/test_emu_resample.py; float32 and int16 in, both
    delivered forms and the curve out, row strides past the rows' samples, outputs pre-filled) give the host call's bits and zero
    tails up to the strides.  Then a batch whose rows are all empty, to host and to device destinations: zero outputs, a zero
    curve, true peak 0, gain 1."""
    cfg = config(eng)
    batch, gains = ragged_batch()
    B = len(RAGGED)
    i16 = np.round(batch * 32767).astype(np.int16)
    in_ld, out_ld = batch.shape[1], batch.shape[1] + 21
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE

    def outputs(buffer):
        return buffer(np.full((B, out_ld), 7.0, np.float32)), buffer(np.full((B, out_ld), 7, np.int16)), buffer(np.full((B, in_ld), 7.0, np.float32))

    for src in (batch, i16):
        host = eng.limit(cfg.model_id, src, RAGGED, gain=gains, ceiling=CEILING, want_float=True, want_int16=True, want_curve=True)
        dev, keep = alloc(src)
        ptrs = (None, dev) if src.dtype == np.int16 else (dev, None)
        (pf, get_f), (pi, get_i), (pc, get_c) = outputs(alloc)
        tp, mg = eng.limit_raw(cfg.model_id, ptrs[0], ptrs[1], RAGGED, in_ld, gains, CEILING, pf, pi, out_ld, pc, flags)
        f, i, c = get_f(), get_i(), get_c()
        assert np.array_equal(bits(tp), bits(host["true_peak"])) and np.array_equal(bits(mg), bits(host["min_gain"]))
        assert np.array_equal(bits(f[:, :in_ld]), bits(host["f32"])) and not f[:, in_ld:].any()
        assert np.array_equal(i[:, :in_ld], host["i16"]) and not i[:, in_ld:].any()
        assert np.array_equal(bits(c), bits(host["curve"]))
        for b, n in enumerate(RAGGED):
            assert not f[b, n:].any() and not i[b, n:].any() and not c[b, n:].any()
        # a meter call from device memory
        tp2, mg2 = eng.limit_raw(cfg.model_id, ptrs[0], ptrs[1], RAGGED, in_ld, None, 1.0, flags=ffi.IN_DEVICE)
        assert np.array_equal(bits(tp2), bits(tp)) and np.all(mg2 == 1.0)
        # no sample in any row
        h_ptrs = (None, src.ctypes.data) if src.dtype == np.int16 else (src.ctypes.data, None)
        for in_ptrs, buffer, fl in ((h_ptrs, numpy_alloc, 0), (ptrs, alloc, flags)):
            (pf, get_f), (pi, get_i), (pc, get_c) = outputs(buffer)
            tp, mg = eng.limit_raw(cfg.model_id, in_ptrs[0], in_ptrs[1], (0, 0, 0), in_ld, gains[:3], CEILING, pf, pi, out_ld, pc, fl)
            assert not tp.any() and np.all(mg == 1.0)
            assert not get_f()[:3].any() and not get_i()[:3].any() and not get_c()[:3].any()
        del keep


def check_sentence_path(tts, voc, n_ids=(11, 4, 26)):
    """Item 9, on the TINY models."""
    import larynx_amd
    from larynx_amd.resample import get_resampler
    from larynx_amd.streaming import stream_raw_pcm

    def float_row(ids, before=0, after=0):
        return voc.mels_to_float_padded(tts.phonemes_to_mels(ids, settings=settings), None, before, after)

    rng = np.random.default_rng(41)
    sents = [(f"s{i}", synthetic.synthetic_phoneme_ids(rng, n, HP.TINY_GLOW.num_symbols)) for i, n in enumerate(n_ids)]
    settings = {"seed": 77}
    s = tts.audio_settings
    assert s.sample_rate == FS
    run = lambda **kw: list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, **kw))  # noqa: E731
    for base in (dict(alignment=True), dict(alignment=True, loudness=-16.0), dict(loudness=-16.0, sample_rate=16000)):
        today = run(**base)
        for off in (None, False):
            for a, b in zip(today, run(limiter=off, **base)):
                assert b.audio.dtype == np.int16 and np.array_equal(a.audio, b.audio)
                assert (a.phoneme_spans is None and b.phoneme_spans is None) or np.array_equal(a.phoneme_spans, b.phoneme_spans)
    today = run(alignment=True)
    m22, l22 = get_loudness(voc.engine, FS), get_limiter(voc.engine, FS)
    limited = run(alignment=True, loudness=-16, limiter=True)
    plain = run(loudness=-16.0, limiter=True)
    cap = 10 ** (30.0 / 20)
    for (text, ids), a, b, p in zip(sents, today, limited, plain):
        fr = float_row(ids)
        exp = m22.normalize_limited(fr, target=-16.0, limiter=l22)
        assert b.sample_rate == FS and b.audio.dtype == np.int16 and b.audio.shape == a.audio.shape
        assert np.array_equal(b.audio, exp) and np.array_equal(p.audio, exp) and p.phoneme_spans is None
        assert np.array_equal(a.phoneme_spans, b.phoneme_spans)
        lufs, before = float(m22.measure(b.audio)[0]), float(m22.measure(fr)[0])
        largest = 10 ** ((-16.0 - before) / 20) >= cap
        print(f"{text}: {b.audio.size} samples, float row {before:.2f} LUFS -> {lufs:.3f} LUFS, int16 peak {np.abs(b.audio.astype(np.int32)).max()}"
              f"{' (the largest gain)' if largest else ''}")
        assert abs(lufs + 16.0) <= 0.1 or largest
    # pauses travel inside the float row
    text, ids = sents[0]
    audio = larynx_amd.sentence_task_limited(text, ids, s, tts, settings, voc, None, 10, 20, None, -16.0)
    assert np.array_equal(audio, m22.normalize_limited(float_row(ids, 220, 441), target=-16.0, limiter=l22)) and audio.size == today[0].audio.size + 661
    assert not audio[:220].any() and not audio[-441:].any()
    sink = io.BytesIO()
    stats = stream_raw_pcm(iter(sents), tts, voc, sink, tts_settings=settings, loudness=-16, limiter=True)
    assert sink.getvalue() == b"".join(r.audio.tobytes() for r in plain) and stats.sentences == len(sents)
    sink = io.BytesIO()
    stream_raw_pcm(iter(sents), tts, voc, sink, tts_settings=settings, loudness=-16, limiter=False)
    assert sink.getvalue() == b"".join(r.audio.tobytes() for r in run(loudness=-16.0))
    # another rate: resampled first, then measured and limited with the 16 kHz designs
    rs, m16, l16 = get_resampler(voc.engine, FS, 16000), get_loudness(voc.engine, 16000), get_limiter(voc.engine, 16000)
    assert l16.lookahead == 24 and l16.release != l22.release
    for (text, ids), r in zip(sents, run(sample_rate=16000, loudness=-16, limiter=True)):
        exp = m16.normalize_limited(rs.resample(float_row(ids)), target=-16.0, limiter=l16)
        assert r.sample_rate == 16000 and np.array_equal(r.audio, exp)
    # only together with a level
    for fn in (lambda: run(limiter=True), lambda: run(limiter=True, alignment=True),
               lambda: stream_raw_pcm(iter(sents), tts, voc, io.BytesIO(), tts_settings=settings, limiter=True),
               lambda: larynx_amd.sentence_task_limited(text, ids, s, tts, settings, voc, None),
               lambda: larynx_amd.sentence_task_aligned(text, ids, s, tts, settings, voc, None, limiter=True)):
        with pytest.raises(ValueError, match="loudness"):
            fn()


# ---------------------------------------------------------------- CPU only: the designs and the oracle
def test_designs():
    taps, H = design_interpolator(4)
    assert (len(taps), H) == (129, 64) and taps.dtype == np.float32 and np.array_equal(taps, taps[::-1]) and taps[H] == 1.0
    for la in (0, 1, LA, 1024):
        w = smoothing_window(la)
        assert w.shape == (la + 1,) and w.dtype == np.float32 and (w > 0).all() and abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
        assert np.array_equal(w, w[::-1])
    assert abs(release_coefficient(FS, 50.0) - np.exp(-1 / 1102.5)) < 1e-15 and release_coefficient(FS, 0) == 0.0


def test_oracle_on_the_issues_row():
    """The float64 oracle alone on the tone-plus-clicks row: a single gain stops 12 LU short, one limiter pass about 1 LU, the
    correction pass arrives; the limited row's sample peak sits on the ceiling."""
    x = M.tone_with_clicks(4 * FS)
    taps, w, a = design_interpolator(4)[0], smoothing_window(LA), A50
    l0 = L.oracle(x, FS)[2]
    capped = L.oracle(x.astype(np.float64) * L.gain(l0, 0.9, -16.0, CEILING, 30.0), FS)[2]
    one = M.oracle(x, 10 ** ((-16 - l0) / 20), CEILING, 4, taps, LA, a, w)
    l1 = L.oracle(one["y"], FS)[2]
    y, l2, g, passes = M.normalize_limited(x, FS, -16.0, CEILING, 30.0, 4, taps, LA, a, w)
    print(f"row {l0:.2f} LUFS; capped gain {capped:.2f}; one pass {l1:.2f}; {passes} passes {l2:.2f}; sample peak {np.abs(y).max():.8f}")
    assert capped < -27 and -18 < l1 < -16.1 and abs(l2 + 16) <= 0.1 and passes == 2
    assert abs(np.abs(y).max() - np.float32(CEILING)) < 1e-6
    r32 = M.restate_f32(x[:FS], 10 ** ((-16 - l0) / 20), CEILING, 4, taps, LA, a, w)
    e = float(np.abs(r32["s"] - M.oracle(x[:FS], 10 ** ((-16 - l0) / 20), CEILING, 4, taps, LA, a, w)["s"]).max())
    print(f"float32 restatement of the curve: {e:.2e} from the oracle")
    assert e < 1e-4


# ---------------------------------------------------------------- the emulator's runs
@pytest.fixture(autouse=True)
def leave_no_counts(request):
    """The session's engine is shared: its launch counters go back to zero behind every test here."""
    yield
    if "emu_engine" in request.fixturenames:
        request.getfixturevalue("emu_engine").profile_reset()


def test_exact_without_release(emu_engine):
    check_exact(emu_engine)


def test_release_against_the_oracle(emu_engine):
    check_release(emu_engine)


def test_rows_under_the_ceiling_pass_unchanged(emu_engine):
    check_passthrough(emu_engine)


def test_ragged_batch(emu_engine):
    check_ragged_batch(emu_engine)


def test_int16_input(emu_engine):
    check_int16_input(emu_engine)


def test_intersample_peak(emu_engine):
    check_intersample(emu_engine)


def test_schedule(emu_engine):
    check_schedule(emu_engine)


def test_device_pointers(emu_engine):
    check_device_pointers(emu_engine, numpy_alloc)


def test_refusals_and_unload(emu_engine):
    check_refusals(emu_engine)


def test_the_target_is_reached(emu_engine):
    check_the_point(emu_engine)


def run_c_program(lib_path, tmp_path):
    """tests/c_abi/limit_ragged.c against `lib_path`: the ragged batch, zero-length rows included, through the plain C ABI, each
    row compared with its batch-1 call inside the program.  (The same program is what the host sanitizers run:
    profiles/limiter.md.)"""
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
    exe = tmp_path / "limit_ragged"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-O1", f"-I{repo / 'include'}",
                    str(repo / "tests" / "c_abi" / "limit_ragged.c"), "-o", str(exe), str(lib_path), f"-Wl,-rpath,{lib_path.parent}", "-lm"], check=True)
    out = subprocess.run([str(exe), "0"], check=True, capture_output=True, text=True, timeout=600).stdout.splitlines()
    assert out[-1] == "ok" and len(out) > 2, out
    rows = 0
    for line in out[:-1]:
        m = re.match(r"row \d+ n (\d+) tp ([0-9a-f]{8}) min ([0-9a-f]{8}) peak ([0-9a-f]{8})", line)
        assert m, line
        n = int(m.group(1))
        tp, mn, peak = (struct.unpack("<f", struct.pack("<I", int(m.group(k), 16)))[0] for k in (2, 3, 4))
        print(f"C caller, N = {n}: true peak {tp:.4f}, smallest gain {mn:.4f}, delivered peak {peak:.4f}")
        assert (tp == 0.0 and mn == 1.0 and peak == 0.0) if n == 0 else (tp > 0 and 0 < mn <= 1.0 and 0 < peak <= np.float32(CEILING))
        rows += 1
    assert rows >= 6


def test_c_caller(emu_library, tmp_path):
    run_c_program(emu_library, tmp_path)


def test_sentence_path(emu_library):
    from tests.test_emu_analysis import tiny_voice
    from tests.test_emu_resample import vocoder

    check_sentence_path(tiny_voice(emu_library), vocoder(emu_library))
