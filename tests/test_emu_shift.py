"""The pitch shifter (csrc/shift.h: shift_mark_kernel, shift_ola_kernel between pitch_kernel and the resampler) on the CPU emulator.

Oracle: tests/shift_np.py — the definition of include/mi355tts.h in numpy.  The positions (float32 recurrence) and the overlap-add
(two float32 products and one add) are stated BIT FOR BIT; the PITCH mode's resampled row is compared with the float64 chain on
the call's own positions within the project's yardstick (`within` of tests/test_emu_pitch.py: 16 x the float32 restatement's own
distance from float64, never below 4 ulp).  The claim itself — the pitch moves by up / down — is measured with the float64 YIN
oracle of tests/pitch_np.py on the delivered row, first on the float64 prototype's own output, then on the device's.

Check 1's invariant.  Frame k reads x[s_k + i], frame k - 1 reads x[s_(k-1) + Hs + i] under the same output sample, so the two are
in phase on a row of period P exactly when (s_(k-1) + Hs) - s_k — the m of the definition — is a multiple of P.  Written with the
anchors: ((s_k - a_k) - (s_(k-1) - a_(k-1))) - Hs + (a_k - a_(k-1)) = s_k - s_(k-1) - Hs = -m.

The check functions are shared with tests/test_gpu_shift.py."""
import ctypes as C

import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.pitch import PitchTracker
from larynx_amd.shift import PitchShifter, get_pitch_shifter, ola_window, semitone_ratio
from tests import pitch_np as P
from tests import resample_np as R
from tests import shift_np as S
from tests.test_emu_pitch import _refused, bits, designed, voiced_row, within
from tests.test_emu_resample import numpy_alloc

FS = 22050
THETA = 0.15
# PitchTracker(engine, 22050)'s defaults with N = 1024, and a small geometry that puts the frame edges at small rows
GEOM = dict(sample_rate=FS, hop=256, W=896, tau_min=45, tau_max=441, N=1024)
SMALL = dict(sample_rate=FS, hop=16, W=64, tau_min=4, tau_max=24, N=64)
ODD = dict(sample_rate=FS, hop=16, W=64, tau_min=4, tau_max=24, N=68)  # Hs = 34: four outputs of a thread straddle two frames
PERIODS = (100, 120, 97, 240)
RATIOS = ((6, 5), (4, 5), (9, 8), (55, 49))
PITCH_RATIOS = ((6, 5), (4, 5), (55, 49))
EDGE_ROWS = (0, 1, 63, 255, 256, 300, 1025)
RAGGED = (4608, 0, 300, 2000)
_cache = {}


class Model:
    def __init__(self, eng, ratio, tempo, geom):
        self.up, self.down = ratio
        self.geom, self.N, self.tempo = geom, geom["N"], tempo
        self.track = {k: v for k, v in geom.items() if k != "N"}
        self.pitch = eng.load_pitch(FS, geom["hop"], geom["W"], geom["tau_min"], geom["tau_max"], THETA, True)
        self.window = S.window(self.N)
        self.taps = self.resampler = None
        if not tempo:
            self.taps = R.design(self.down, self.up)[0]
            self.resampler = eng.load_resampler(self.taps, self.down, self.up)
        self.id = eng.load_shift(self.up, self.down, self.window, self.pitch, self.resampler or 0)

    def frames(self, n):
        """(L, K, Fp) of a row of n samples."""
        L, K = S.lengths(n, self.up, self.down, self.N)
        return L, K, n // self.geom["hop"]


def model(eng, ratio, tempo=True, geom=GEOM):
    key = ("model", id(eng), ratio, tempo, tuple(sorted(geom.items())))
    if key not in _cache:
        _cache[key] = Model(eng, ratio, tempo, geom)
    return _cache[key]


def run(eng, m, x, samples=None, **kw):
    """One call with every side output: positions [.., Kmax] and f0 [.., Fmax] of the longest row."""
    ns = [np.asarray(x).shape[-1]] if samples is None else list(samples)
    Kmax = max(m.frames(n)[1] for n in ns)
    Fmax = max(m.frames(n)[2] for n in ns)
    if kw.get("positions_in") is not None:
        return eng.shift(m.id, x, samples, **kw)
    return eng.shift(m.id, x, samples, want_positions=Kmax, want_f0=Fmax, **kw)


def small_row(n, seed=0):
    """A two-harmonic tone with a period of 11.3 samples (inside the small geometry's lags 4 .. 24) and a little noise."""
    t = np.arange(n)
    rng = np.random.default_rng(300 + seed)
    return (0.4 * np.sin(2 * np.pi * t / 11.3) + 0.2 * np.sin(4 * np.pi * t / 11.3 + 0.5) + rng.normal(0, 1e-3, n)).astype(np.float32)


def row_for(geom, n):
    return voiced_row(n) if geom is GEOM else small_row(n)


def against_numpy(tag, eng, m, x):
    """One row through the call with all side outputs: f0 = Engine.pitch's bits, the positions = the float32 recurrence on that f0,
    the stretch (TEMPO) = the float32 overlap-add bit for bit, the resampled row (PITCH) within the yardstick.  -> the call's result."""
    n = len(x)
    L, K, Fp = m.frames(n)
    r = run(eng, m, x)
    assert r["positions"].shape == (K,) and r["f0"].shape == (Fp,) and list(r["samples"]) == [n if not m.tempo else L]
    assert r["f32"].shape == (eng.shift_length(m.id, n),) == (int(r["samples"][0]),)
    if n:
        f0 = eng.pitch(m.pitch, x)["f0"] if Fp else np.zeros(0, np.float32)
        assert np.array_equal(bits(r["f0"]), bits(f0)), tag
    pos = S.positions(n, r["f0"], FS, m.geom["hop"], m.up, m.down, m.N)
    assert np.array_equal(pos, r["positions"]), tag
    if m.tempo:
        assert np.array_equal(bits(r["f32"]), bits(S.ola(x, m.window, pos, m.up, m.down))), tag
    elif n:
        z64 = S.chain(x, m.window, pos, m.up, m.down, m.taps, np.float64)
        within(tag, r["f32"], z64, S.chain(x, m.window, pos, m.up, m.down, m.taps, np.float32))
    return r


def check_exact_periods(eng):
    """Check 1: rows with an exact integer period, TEMPO mode.  No tolerance on the positions, 1 ulp on the samples."""
    hop, W, tmax, N = GEOM["hop"], GEOM["W"], GEOM["tau_max"], GEOM["N"]
    Hs = N // 2
    for period in PERIODS:
        x = P.periodic_row(period)
        n = len(x)
        for ratio in RATIOS:
            m = model(eng, ratio)
            up, down = ratio
            r = run(eng, m, x)
            L, K, Fp = m.frames(n)
            s = r["positions"].astype(np.int64)
            c, a = S.anchors(K, up, down, N)
            j = np.minimum(Fp - 1, (c + hop // 2) // hop)
            inside = (j * hop - W // 2 >= 0) & (j * hop - W // 2 + W + tmax <= n)  # the tracker's span of the frame's period
            inside[0] = False
            k = np.nonzero(inside)[0]
            assert len(k) > 5
            # (the default tracker interpolates: its period is P up to the parabola's last digits, and m = rint(q T) is q P exactly)
            assert (np.abs(FS / r["f0"][j[k]].astype(np.float64) - period) < 0.02).all()
            m_k = ((s[k] - a[k]) - (s[k - 1] - a[k - 1])) - Hs + (a[k] - a[k - 1])
            assert np.array_equal(m_k, s[k] - s[k - 1] - Hs) and (m_k % period == 0).all(), (period, ratio)
            # interior samples: the later of the two frames over them is in phase with the earlier, both read inside the row
            t = np.arange(L, dtype=np.int64)
            k1 = t // Hs
            i1 = t - k1 * Hs + Hs
            r1, r2 = s[k1] + i1, s[k1 + 1] + i1 - Hs
            ok = inside[k1 + 1] & (r1 >= 0) & (r1 < n) & (r2 >= 0) & (r2 < n)
            assert ok.sum() > 1000
            u = S.ulps(r["f32"][ok], x[r1[ok] % period])
            print(f"P = {period}, {up}/{down}: {len(k)} frames in phase, {int(ok.sum())} interior samples within {u.max():.2f} ulp")
            assert np.array_equal(x[r1[ok] % period], x[r1[ok]]) and u.max() <= 1.0, (period, ratio)


def check_positions(eng):
    """Check 2: the designed signal: f0_out = Engine.pitch's bits, positions_out = the float32 recurrence on the call's own f0_out;
    check 3's first part on the way: the stretch = the float32 overlap-add on the call's positions."""
    x = designed()
    for ratio in RATIOS:
        m = model(eng, ratio)
        r = against_numpy(f"designed {ratio}", eng, m, x)
        moved = int((r["positions"] != S.anchors(len(r["positions"]), *ratio, m.N)[1]).sum())
        print(f"{ratio[0]}/{ratio[1]}: {len(r['positions'])} frames, {moved} moved by whole periods, {int((r['f0'] > 0).sum())} voiced pitch frames")
        assert moved > 20


def check_injected_positions(eng):
    """Check 3: positions_in — the call's own give the call's bits; a hand-made set with negative positions and positions past
    the row's end gives the numpy bits (zeros where the reads leave the row), in all three geometries."""
    x = designed()
    m = model(eng, (6, 5))
    own = run(eng, m, x)
    again = run(eng, m, x, positions_in=own["positions"])
    assert np.array_equal(bits(again["f32"]), bits(own["f32"])) and again["positions"] is None
    mp = model(eng, (6, 5), tempo=False)
    own = run(eng, mp, x, want_int16=True, normalize=True)
    again = run(eng, mp, x, positions_in=own["positions"], want_int16=True, normalize=True)
    assert np.array_equal(bits(again["f32"]), bits(own["f32"])) and np.array_equal(again["i16"], own["i16"])
    rng = np.random.default_rng(5)
    for geom, n in ((GEOM, 3000), (SMALL, 301), (ODD, 301)):
        for ratio in ((6, 5), (4, 5)):
            m = model(eng, ratio, geom=geom)
            xr = rng.uniform(-0.9, 0.9, n).astype(np.float32)
            L, K, _ = m.frames(n)
            pos = rng.integers(-2 * m.N, n + m.N, K).astype(np.int32)
            pos[:3] = (-5 * m.N, n - 7, n + 10)
            got = run(eng, m, xr, positions_in=pos)
            ref = S.ola(xr, m.window, pos, *ratio)
            assert np.array_equal(bits(got["f32"]), bits(ref)) and (ref == 0).sum() > 10 and (ref != 0).sum() > 10, (geom["N"], ratio)
    print("own positions fed back: the call's bits; hand-made positions (N = 1024, 64, 68): numpy's bits")


def oracle_track(x):
    """f0 of the float64 YIN oracle with the default geometry."""
    return P.track(x, theta=THETA, interpolate=True, dtype=np.float64, **{k: v for k, v in GEOM.items() if k != "N"})["f0"]


def pitch_shares(fx, fz, rho):
    """(share of x's voiced frames still voiced in z, share of those whose f0 ratio is within 2 % of rho, median relative error)."""
    F = min(len(fx), len(fz))
    fx, fz = fx[:F], fz[:F]
    vx = fx > 0
    both = vx & (fz > 0)
    err = np.abs(fz[both] / fx[both] / rho - 1.0)
    return both.sum() / vx.sum(), float((err <= 0.02).mean()), float(np.median(err))


def prototype(ratio):
    """The float64 prototype on the designed signal (computed once): (its delivered row, the shares of its own output)."""
    if ("proto", ratio) not in _cache:
        x = designed()
        up, down = ratio
        z = S.shift(x, S.window(GEOM["N"]), up, down, R.design(down, up)[0], THETA, np.float64, **{k: v for k, v in GEOM.items() if k != "N"})[0]
        if "fx" not in _cache:
            _cache["fx"] = oracle_track(x)
        _cache["proto", ratio] = (z, pitch_shares(_cache["fx"], oracle_track(z), up / down))
    return _cache["proto", ratio]


def check_chain(eng, ratio):
    """Check 4, PITCH mode on the designed signal: (a) the delivered row against the float64 chain on the call's positions; (b) the
    claim: the float64 YIN oracle reads f0 x up / down from it — asserted on the prototype's own output first."""
    x = designed()
    up, down = ratio
    _, (p_voiced, p_near, p_med) = prototype(ratio)
    print(f"{up}/{down} prototype: {100 * p_voiced:.1f} % still voiced, {100 * p_near:.1f} % within 2 %, median error {100 * p_med:.2f} %")
    assert p_voiced >= 0.95 and p_near >= 0.95, "the algorithm itself"
    m = model(eng, ratio, tempo=False)
    r = against_numpy(f"designed {ratio} PITCH", eng, m, x)
    assert r["f32"].shape == x.shape
    voiced, near, med = pitch_shares(_cache["fx"], oracle_track(r["f32"]), up / down)
    print(f"{up}/{down} device:    {100 * voiced:.1f} % still voiced, {100 * near:.1f} % within 2 %, median error {100 * med:.2f} %")
    assert voiced >= 0.95 and near >= 0.95
    return (p_voiced, p_near, p_med), (voiced, near, med)


def check_identity_and_edges(eng):
    """Check 5."""
    x = designed()
    one = model(eng, (1, 1))
    r = run(eng, one, x)
    nz = x != 0
    assert r["f32"].shape == x.shape and not r["f32"][~nz].any()
    u = S.ulps(r["f32"][nz], x[nz])
    print(f"1/1: the input within {u.max():.2f} ulp")
    assert u.max() <= 1.0
    for geom in (GEOM, SMALL):
        for tempo, ratio in ((True, (6, 5)), (True, (4, 5)), (False, (6, 5)), (False, (4, 5))):
            m = model(eng, ratio, tempo, geom)
            for n in EDGE_ROWS:
                r = against_numpy(f"N = {geom['N']}, {ratio}, tempo {tempo}, n = {n}", eng, m, row_for(geom, n))
                assert eng.shift_length(m.id, n) == (m.frames(n)[0] if tempo else n) == len(r["f32"])
            r = run(eng, m, np.zeros(700, np.float32), want_int16=True, normalize=True)
            assert not r["f32"].any() and not r["i16"].any() and not r["f0"].any()
            assert np.array_equal(r["positions"], S.anchors(len(r["positions"]), *ratio, m.N)[1])
    small = model(eng, (6, 5), True, SMALL)
    r = run(eng, small, small_row(1025))
    assert (r["f0"] > 0).sum() > 40 and (r["positions"] != S.anchors(len(r["positions"]), 6, 5, 64)[1]).sum() > 10  # the small rows are voiced


def ragged_batch():
    batch = np.full((len(RAGGED), 4700), 0.25, np.float32)  # what lies past a row's samples must not be read
    for b, n in enumerate(RAGGED):
        batch[b, :n] = voiced_row(n)
    return batch


def check_batch_forms(eng, alloc):
    """Check 6: a ragged batch of 4, unsorted, one row empty: every row the bits of its batch-1 call, zeros behind it; int16 input =
    the equal float input; device pointers (pre-filled destinations, strides past the longest row) = the host call."""
    batch = ragged_batch()
    i16 = np.round(batch * 32767).astype(np.int16)
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE
    for tempo in (False, True):
        m = model(eng, (6, 5), tempo)
        dims = [m.frames(n) for n in RAGGED]
        outs = [n if not tempo else L for n, (L, _, _) in zip(RAGGED, dims)]
        Omax, Kmax, Fmax = max(outs), max(d[1] for d in dims), max(d[2] for d in dims)
        r = run(eng, m, batch, RAGGED, want_int16=True)
        rn = run(eng, m, batch, RAGGED, want_float=False, want_int16=True, normalize=True)
        assert r["f32"].shape == (4, Omax) and r["positions"].shape == (4, Kmax) and r["f0"].shape == (4, Fmax) and list(r["samples"]) == outs
        for b, n in enumerate(RAGGED):
            one = run(eng, m, batch[b, :n], want_int16=True)
            one_n = run(eng, m, batch[b, :n], want_float=False, want_int16=True, normalize=True)
            o, (_, K, F) = outs[b], dims[b]
            assert np.array_equal(bits(r["f32"][b, :o]), bits(one["f32"])) and not r["f32"][b, o:].any(), n
            assert np.array_equal(r["i16"][b, :o], one["i16"]) and not r["i16"][b, o:].any(), n
            assert np.array_equal(rn["i16"][b, :o], one_n["i16"]) and not rn["i16"][b, o:].any(), n
            assert np.array_equal(r["positions"][b, :K], one["positions"]) and not r["positions"][b, K:].any(), n
            assert np.array_equal(bits(r["f0"][b, :F]), bits(one["f0"])) and not r["f0"][b, F:].any(), n
            if n:
                # the reference's audio_float_to_int16 on the delivered row (it truncates: the peak lands on 32767 or 32766)
                assert np.array_equal(one_n["i16"], R.float_to_int16(one["f32"])) and np.abs(one_n["i16"].astype(np.int32)).max() >= 32766
        # int16 input: the bits of the equal float32 input
        a = run(eng, m, i16, RAGGED, want_int16=True)
        f = run(eng, m, i16.astype(np.float32) * np.float32(2.0 ** -15), RAGGED, want_int16=True)
        for k in ("f32", "f0"):
            assert np.array_equal(bits(a[k]), bits(f[k])), k
        assert np.array_equal(a["i16"], f["i16"]) and np.array_equal(a["positions"], f["positions"])
        # device pointers
        ld, pos_ld, f0_ld, in_ld = Omax + 21, Kmax + 3, Fmax + 2, batch.shape[1]
        for src, host, host_n in ((batch, r, rn), (i16, a, run(eng, m, i16, RAGGED, want_float=False, want_int16=True, normalize=True))):
            dev, keep = alloc(src)
            ptrs = (None, dev) if src.dtype == np.int16 else (dev, None)
            for mode, want in ((ffi.PCM_SATURATE, host["i16"]), (ffi.PCM_NORMALIZE, host_n["i16"])):
                (pf, get_f), (pi, get_i) = alloc(np.full((4, ld), 7.0, np.float32)), alloc(np.full((4, ld), 7, np.int16))
                (pp, get_p), (p0, get_0) = alloc(np.full((4, pos_ld), 7, np.int32)), alloc(np.full((4, f0_ld), 7.0, np.float32))
                got = eng.shift_raw(m.id, ptrs[0], ptrs[1], RAGGED, in_ld, pf, pi, ld, mode, positions_ptr=pp, pos_ld=pos_ld, f0_ptr=p0,
                                    f0_ld=f0_ld, flags=flags)
                assert list(got) == outs
                fo, io, po, f0o = get_f(), get_i(), get_p(), get_0()
                assert np.array_equal(bits(fo[:, :Omax]), bits(host["f32"])) and not fo[:, Omax:].any()
                assert np.array_equal(io[:, :Omax], want) and not io[:, Omax:].any()
                assert np.array_equal(po[:, :Kmax], host["positions"]) and not po[:, Kmax:].any()
                assert np.array_equal(bits(f0o[:, :Fmax]), bits(host["f0"])) and not f0o[:, Fmax:].any()
            # positions_in from device memory, at its own stride
            (pq, _), (pf, get_f) = alloc(np.pad(host["positions"], ((0, 0), (0, 3)))), alloc(np.full((4, ld), 7.0, np.float32))
            eng.shift_raw(m.id, ptrs[0], ptrs[1], RAGGED, in_ld, pf, None, ld, positions_in_ptr=pq, pos_ld=pos_ld, flags=flags)
            assert np.array_equal(bits(get_f()[:, :Omax]), bits(host["f32"])) and not get_f()[:, Omax:].any()
            # no sample in any row: zeros, to host and to device destinations
            host_src = np.ascontiguousarray(src)
            h_ptrs = (None, host_src.ctypes.data) if src.dtype == np.int16 else (host_src.ctypes.data, None)
            for in_ptrs, buffer, fl in ((h_ptrs, numpy_alloc, 0), (ptrs, alloc, flags)):
                (pf, get_f), (pi, get_i) = buffer(np.full((4, ld), 7.0, np.float32)), buffer(np.full((4, ld), 7, np.int16))
                (pp, get_p), (p0, get_0) = buffer(np.full((4, pos_ld), 7, np.int32)), buffer(np.full((4, f0_ld), 7.0, np.float32))
                got = eng.shift_raw(m.id, in_ptrs[0], in_ptrs[1], (0, 0, 0, 0), in_ld, pf, pi, ld, positions_ptr=pp, pos_ld=pos_ld, f0_ptr=p0,
                                    f0_ld=f0_ld, flags=fl)
                assert not got.any() and not get_f().any() and not get_i().any() and not get_p().any() and not get_0().any()
            del keep
        print(f"tempo {tempo}: rows of {RAGGED} samples = their batch-1 calls; int16 = float input; device = host pointers")


def check_schedule(eng):
    """Check 7: the launches by kernel name and in all."""
    x, batch = voiced_row(4608), ragged_batch()
    names = {"pitch_kernel": 1, "shift_mark_kernel": 1, "shift_ola_kernel": 1}
    eng.set_profiling(True)
    try:
        for tempo in (False, True):
            m = model(eng, (6, 5), tempo)
            pos = run(eng, m, x)["positions"]
            extra = 0 if tempo else 1  # the resampler's launch
            cases = [
                (dict(), names, 3 + extra), (dict(want_float=False, want_int16=True), names, 3 + extra),
                (dict(want_int16=True, normalize=True), names, 4 + extra),
                (dict(want_float=False, want_int16=True, normalize=True), names, 4 + extra),
                (dict(positions_in=pos), {"shift_ola_kernel": 1}, 1 + extra),
            ]
            for kw, want, launches in cases:
                for audio, samples in ((x, None), (batch, RAGGED)):
                    if "positions_in" in kw and samples is not None:
                        continue
                    eng.profile_reset()
                    run(eng, m, audio, samples, **kw)
                    prof = eng.profile()
                    ran = {k: v for k, v in eng.kernel_counts().items() if v}
                    assert ran == want and prof["elementwise"]["launches"] == launches, (tempo, kw, ran, prof["elementwise"])
                    assert all(v["launches"] == 0 for k, v in prof.items() if k != "elementwise")
            eng.profile_reset()
            run(eng, m, batch, (0, 0, 0, 0))
            assert not any(eng.kernel_counts().values()) and eng.profile()["elementwise"]["launches"] == 0
            eng.profile_reset()
            run(eng, m, batch, (0, 255, 100, 0))  # rows without a pitch frame: no pitch_kernel, every position its anchor
            assert {k: v for k, v in eng.kernel_counts().items() if v} == {"shift_mark_kernel": 1, "shift_ola_kernel": 1}
            print(f"tempo {tempo}: {3 + extra} launches for float / saturating int16, {4 + extra} normalised, none for an empty batch")
    finally:
        eng.set_profiling(False)
        eng.profile_reset()
    counts = eng.kernel_counts()
    assert not any(counts.values()) and len(counts) == 44 and list(counts)[-1] == "attention_kernel"  # the pinned keys, unchanged


def check_refusals(eng):
    """Check 8: every limit of the header with its reason; the context still works; the pinned models outlive their ids."""
    lib, mid = eng.lib, C.c_int()
    pitch = eng.load_pitch(FS, 256, 896, 45, 441)
    rs = eng.load_resampler(R.design(5, 6)[0], 5, 6)
    win = S.window(1024)

    def load(up=6, down=5, N=1024, pt=pitch, res=0, w=win, params=True, out=True, window=True):
        p = ffi.ShiftParamsC(up, down, N, pt, res)
        w = np.ascontiguousarray(w, np.float32)
        return lambda: ffi.check(lib, lib.mi355tts_load_shift(eng._ctx, C.byref(p) if params else None, w.ctypes.data if window else None,
                                                              C.byref(mid) if out else None))

    _refused(load(params=False), "null")
    _refused(load(out=False), "null")
    _refused(load(window=False), "null")
    for up, down in ((0, 5), (65, 1), (6, -1), (1, 65)):
        _refused(load(up=up, down=down), "outside [1, 64]")
    for up, down in ((6, 4), (64, 2), (5, 5)):
        _refused(load(up=up, down=down), "coprime")
    for bad in (60, 0, 1022, 2052, 4096, -4):
        _refused(load(N=bad, w=np.ones(4096, np.float32)), "window")
    for bad in (np.nan, np.inf, -np.inf):
        w = win.copy()
        w[1023] = bad
        _refused(load(w=w), "not finite")
    _refused(load(pt=10 ** 6), "no pitch tracker", code=-5)
    _refused(load(pt=rs), "no pitch tracker", code=-5)
    _refused(load(res=10 ** 6), "no resampler", code=-5)
    _refused(load(res=pitch), "no resampler", code=-5)
    _refused(load(res=rs, up=4, down=5), "ratio")
    _refused(load(res=rs, up=5, down=6), "ratio")
    one = eng.load_resampler(R.HAND_TAPS, 1, 1)
    _refused(load(res=one, up=1, down=1), "up == down")
    for ok in (dict(N=64, w=np.ones(64, np.float32), up=64, down=1), dict(N=2048, w=np.ones(2048, np.float32), up=1, down=64), dict(up=1, down=1)):
        load(**ok)()
        eng.unload(mid.value)
    load(res=rs)()
    m = mid.value
    tempo = eng.load_shift(6, 5, win, pitch)
    x = np.ascontiguousarray(voiced_row(700))
    i16 = np.zeros(700, np.int16)
    of, oi = np.full(900, 7.0, np.float32), np.full(900, 7, np.int16)
    po, f0 = np.full(8, 7, np.int32), np.full(4, 7.0, np.float32)
    n = np.array([700], np.int64)

    def call(f32=x.ctypes.data, s16=None, samples=n, in_ld=700, pin=None, o32=of.ctypes.data, o16=oi.ctypes.data, out_ld=900, mode=0,
             pout=po.ctypes.data, pos_ld=8, f0p=f0.ctypes.data, f0_ld=4, mdl=m, B=1, ctx=True):
        s_p = None if samples is None else samples.ctypes.data_as(C.POINTER(C.c_int64))
        return lambda: ffi.check(lib, lib.mi355tts_shift(eng._ctx if ctx else None, mdl, f32, s16, s_p, B, in_ld, pin, o32, o16, out_ld, mode, pout,
                                                         pos_ld, f0p, f0_ld, None, 0))

    _refused(call(samples=None), "null")
    _refused(call(ctx=False), "null")
    _refused(call(s16=i16.ctypes.data), "exactly one")
    _refused(call(f32=None), "exactly one")
    _refused(call(B=0), "batch")
    _refused(call(in_ld=-1), "in_ld")
    _refused(call(o32=None, o16=None), "no output")
    _refused(call(mode=2), "pcm_mode")
    for bad in (-1, 701):
        _refused(call(samples=np.array([bad], np.int64)), "samples[0]")
    _refused(call(samples=np.array([2 ** 24 + 1], np.int64), in_ld=2 ** 25), "2^24")
    _refused(call(out_ld=699), "out_ld")
    _refused(call(out_ld=839, mdl=tempo), "out_ld")  # 840 = ceil(700 * 6 / 5)
    _refused(call(pos_ld=2), "pos_ld")               # K = 839 / 512 + 2 = 3
    _refused(call(pos_ld=2, pout=None, f0p=None, pin=po.ctypes.data), "pos_ld")
    _refused(call(f0_ld=1), "f0_ld")                 # Fp = 2
    _refused(call(pin=po.ctypes.data), "positions_in")
    _refused(call(pin=po.ctypes.data, pout=None), "positions_in")
    _refused(call(mdl=10 ** 6), "no pitch shifter", code=-5)
    _refused(call(mdl=pitch), "no pitch shifter", code=-5)
    with pytest.raises(ffi.Mi355ttsError):
        eng.shift_length(m, -1)
    with pytest.raises(ffi.Mi355ttsError):
        eng.shift_length(m, 2 ** 24 + 1)
    call()()  # the context still works
    want = eng.shift(m, x, want_int16=True, want_positions=3, want_f0=2)
    assert np.array_equal(bits(of[:700]), bits(want["f32"])) and not of[700:].any() and np.array_equal(oi[:700], want["i16"]) and not oi[700:].any()
    assert np.array_equal(po[:3], want["positions"]) and not po[3:].any() and np.array_equal(bits(f0[:2]), bits(want["f0"])) and not f0[2:].any()
    call(o16=None, pout=None, f0p=None, pos_ld=0, f0_ld=0)()  # the float row alone
    assert np.array_equal(bits(of[:700]), bits(want["f32"]))
    # the shift model pins its two models: their ids may go first
    eng.unload(pitch)
    eng.unload(rs)
    _refused(lambda: eng.pitch(pitch, x), "no pitch tracker", code=-5)
    after = eng.shift(m, x, want_int16=True, want_positions=3, want_f0=2)
    for k in ("f32", "f0"):
        assert np.array_equal(bits(after[k]), bits(want[k]))
    assert np.array_equal(after["i16"], want["i16"]) and np.array_equal(after["positions"], want["positions"])
    eng.unload(m)
    eng.unload(tempo)
    eng.unload(one)
    _refused(lambda: eng.shift(m, x), "no pitch shifter", code=-5)


def check_shifter_object(eng):
    """Check 9: the PitchShifter object."""
    sh = PitchShifter(eng, FS, semitones=2)
    assert (sh.up, sh.down, sh.N, sh.tempo) == (55, 49, 1024, False) and isinstance(sh.tracker, PitchTracker)
    assert (sh.tracker.hop, sh.tracker.window, sh.tracker.tau_min, sh.tracker.tau_max) == (256, 896, 45, 441)
    assert (sh.resampler.up, sh.resampler.down) == (49, 55) and np.array_equal(sh.window, S.window(1024))
    x = voiced_row(4608)
    y = sh.shift(x)
    assert y.shape == x.shape and y.dtype == np.float32 and sh.length(4608) == 4608
    ref = run(eng, model(eng, (55, 49), tempo=False), x)
    assert np.array_equal(bits(y), bits(ref["f32"]))
    pcm = sh.shift(x, normalize=True)
    assert pcm.dtype == np.int16 and np.array_equal(pcm, R.float_to_int16(y))
    two = sh.shift(np.stack([x, x]), samples=(4608, 300))
    assert two.shape == (2, 4608) and np.array_equal(bits(two[0]), bits(y)) and not two[1, 300:].any()
    assert sh.shift(np.round(x * 32767).astype(np.int16)).shape == (4608,)
    slow = PitchShifter(eng, FS, ratio=(12, 10), tempo=True)
    assert (slow.up, slow.down, slow.resampler) == (6, 5, None) and slow.length(1000) == 1200 and slow.shift(x[:1000]).shape == (1200,)
    assert np.array_equal(bits(slow.shift(x)), bits(run(eng, model(eng, (6, 5)), x)["f32"]))
    same = PitchShifter(eng, FS, semitones=0)
    assert (same.up, same.down, same.resampler) == (1, 1, None) and S.ulps(same.shift(x), x).max() <= 1.0
    kept = get_pitch_shifter(eng, FS, -3)
    assert kept is get_pitch_shifter(eng, FS, -3.0) and (kept.up, kept.down) == semitone_ratio(-3) and kept is not get_pitch_shifter(eng, FS, 3)
    for bad in (dict(), dict(semitones=1, ratio=(6, 5)), dict(ratio=(0, 5))):
        with pytest.raises(ValueError):
            PitchShifter(eng, FS, **bad)
    with pytest.raises(ValueError):
        get_pitch_shifter(eng, FS, 12.5)


def check_sentence_path(tts, voc, n_ids=(11, 4, 26)):
    """Check 9: `phonemes_to_speech(pitch_shift=)` and `stream_raw_pcm(pitch_shift=)` on the TINY models."""
    import io

    import larynx_amd
    from larynx_amd.limiter import get_limiter
    from larynx_amd.loudness import get_loudness
    from larynx_amd.pitch import PitchTrack, get_pitch_tracker
    from larynx_amd.resample import get_resampler
    from larynx_amd.streaming import stream_raw_pcm

    rng = np.random.default_rng(41)
    sents = [(f"s{i}", synthetic.synthetic_phoneme_ids(rng, n, HP.TINY_GLOW.num_symbols)) for i, n in enumerate(n_ids)]
    settings = {"seed": 77}
    eng = voc.engine
    run_ = lambda **kw: list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, **kw))  # noqa: E731

    def float_row(ids, before=0, after=0):
        return voc.mels_to_float_padded(tts.phonemes_to_mels(ids, settings=settings), None, before, after)

    today = run_(alignment=True)
    eng.profile_reset()
    for nothing in (None, 0):
        same = run_(alignment=True, pitch_shift=nothing)
        for a, b in zip(today, same):
            assert a.audio.tobytes() == b.audio.tobytes() and np.array_equal(a.phoneme_spans, b.phoneme_spans) and b.sample_rate == FS
    assert not any(v for k, v in eng.kernel_counts().items() if k.startswith("shift_")) and ("shift", (FS, 2.0)) not in getattr(eng, "_kept", {})
    sh = get_pitch_shifter(eng, FS, 2)
    assert (sh.up, sh.down) == (55, 49)
    up2 = run_(alignment=True, pitch_shift=2)
    plain2 = run_(pitch_shift=2)
    assert sum(v for k, v in eng.kernel_counts().items() if k.startswith("shift_")) == 2 * 2 * len(sents)
    for (text, ids), a, b, p in zip(sents, today, up2, plain2):
        exp = sh.shift(float_row(ids), normalize=True)
        assert b.audio.dtype == np.int16 and b.audio.shape == a.audio.shape and b.sample_rate == FS and b.text == text
        assert np.array_equal(b.audio, exp) and np.array_equal(p.audio, exp) and p.phoneme_spans is None
        assert np.array_equal(a.phoneme_spans, b.phoneme_spans) and not np.array_equal(a.audio, b.audio)
        assert np.abs(b.audio.astype(np.int32)).max() >= 32766
        print(f"{text}: {a.audio.size} samples, +2 semitones differs in {int((a.audio != b.audio).sum())} of them")
    # it composes: another rate, a level with the limiter, the pitch track of what was delivered
    rs, ld, lim = get_resampler(eng, FS, 16000), get_loudness(eng, 16000), get_limiter(eng, 16000)
    at16 = run_(alignment=True, pitch_shift=2, sample_rate=16000)
    lev = run_(pitch_shift=2, sample_rate=16000, loudness=-16.0, limiter=True)
    trk = run_(alignment=True, pitch_shift=2, pitch=True)
    tracker = get_pitch_tracker(eng, FS)
    for (text, ids), a, b, c, d, e in zip(sents, today, at16, lev, trk, up2):
        shifted = sh.shift(float_row(ids))
        assert b.sample_rate == c.sample_rate == 16000 and np.array_equal(b.audio, rs.resample(shifted, normalize=True))
        assert np.array_equal(b.phoneme_spans, larynx_amd.alignment.scale_spans(a.phoneme_spans, 320, 441))
        assert np.array_equal(c.audio, ld.normalize_limited(rs.resample(shifted), target=-16.0, limiter=lim))
        assert np.array_equal(d.audio, e.audio) and isinstance(d.pitch, PitchTrack) and np.array_equal(d.phoneme_spans, a.phoneme_spans)
        assert np.array_equal(bits(d.pitch.f0), bits(tracker.track(d.audio).f0)) and d.phoneme_pitch.shape == (len(ids), 2)
    # pauses travel inside the shifted row; the tasks agree with each other
    text, ids = sents[0]
    s = tts.audio_settings
    audio, sp = larynx_amd.sentence_task_shifted(text, ids, s, tts, settings, voc, None, 10, 20, pitch_shift=2, alignment=True)
    assert np.array_equal(audio, sh.shift(float_row(ids, 220, 441), normalize=True)) and audio.size == today[0].audio.size + 661
    assert sp[0, 0] == 220 and np.array_equal(sp, today[0].phoneme_spans + 220)
    assert np.array_equal(audio, larynx_amd.sentence_task_shifted(text, ids, s, tts, settings, voc, None, 10, 20, pitch_shift=2))
    assert np.array_equal(larynx_amd.sentence_task_shifted(text, ids, s, tts, settings, voc, None, 10, 20),
                          larynx_amd.sentence_task(text, ids, s, tts, settings, voc, None, 10, 20))
    sink = io.BytesIO()
    stats = stream_raw_pcm(iter(sents), tts, voc, sink, tts_settings=settings, pitch_shift=2)
    assert sink.getvalue() == b"".join(r.audio.tobytes() for r in plain2) and stats.sentences == 3
    sink = io.BytesIO()
    stream_raw_pcm(iter(sents), tts, voc, sink, tts_settings=settings, pitch_shift=2, sample_rate=16000, loudness=-16.0, limiter=True)
    assert sink.getvalue() == b"".join(r.audio.tobytes() for r in lev)
    sink = io.BytesIO()
    stream_raw_pcm(iter(sents), tts, voc, sink, tts_settings=settings, pitch_shift=0)
    assert sink.getvalue() == b"".join(r.audio.tobytes() for r in today)
    for bad in (12.01, -13, 100):
        with pytest.raises(ValueError):
            run_(pitch_shift=bad)
        with pytest.raises(ValueError):
            stream_raw_pcm(iter(sents), tts, voc, io.BytesIO(), tts_settings=settings, pitch_shift=bad)


# ---------------------------------------------------------------- CPU only: the oracle and the host-side pieces
def test_semitone_ratio_and_window():
    assert semitone_ratio(0) == (1, 1) and semitone_ratio(12) == (2, 1) and semitone_ratio(2) == (55, 49) and semitone_ratio(-12) == (1, 2)
    assert semitone_ratio(7) == (3, 2) and semitone_ratio(-2) == (49, 55)
    for st in np.arange(-12, 12.25, 0.25):
        up, down = semitone_ratio(st)
        assert 1 <= up <= 64 and 1 <= down <= 64 and np.gcd(up, down) == 1 and abs(up / down / 2.0 ** (st / 12.0) - 1.0) < 4e-3
    for N in (64, 68, 1024, 2048):
        w = ola_window(N)
        assert w.dtype == np.float32 and w.shape == (N,) and np.array_equal(w, S.window(N))
        assert (w[:N // 2] + w[N // 2:] == np.float32(1.0)).all() and w[0] == 0.0 and w[N // 2] == 1.0  # float32 sums: exactly 1
        hann = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)
        assert np.abs(w - hann).max() < 1e-7
    with pytest.raises(ValueError):
        ola_window(63)


def test_recurrence_agrees_in_both_precisions():
    """The condition of check 2: on the designed signal the float32 and the float64 recurrence give the same positions on every
    frame, for every ratio of the tests, so no frame needs to be left out."""
    x = designed()
    track = {k: v for k, v in GEOM.items() if k != "N"}
    f0 = P.track(x, theta=THETA, interpolate=True, dtype=np.float32, **track)["f0"]
    for up, down in RATIOS:
        a = S.positions(len(x), f0, FS, 256, up, down, 1024, np.float32)
        b = S.positions(len(x), f0, FS, 256, up, down, 1024, np.float64)
        assert np.array_equal(a, b) and len(a) == S.lengths(len(x), up, down, 1024)[1]


@pytest.mark.parametrize("ratio", PITCH_RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
def test_prototype_moves_the_pitch(ratio):
    """The algorithm alone, in float64 on the host: the shares of check 4 (b)."""
    _, (voiced, near, med) = prototype(ratio)
    print(f"{ratio[0]}/{ratio[1]}: {100 * voiced:.1f} % still voiced, {100 * near:.1f} % within 2 %, median error {100 * med:.2f} %")
    assert voiced >= 0.95 and near >= 0.95


# ---------------------------------------------------------------- the emulator's runs
@pytest.fixture(autouse=True)
def leave_no_counts(request):
    """The session's engine is shared: its launch counters go back to zero behind every test here."""
    yield
    if "emu_engine" in request.fixturenames:
        request.getfixturevalue("emu_engine").profile_reset()


def test_exact_periods(emu_engine):
    check_exact_periods(emu_engine)


def test_positions_bit_for_bit(emu_engine):
    check_positions(emu_engine)


def test_injected_positions(emu_engine):
    check_injected_positions(emu_engine)


@pytest.mark.parametrize("ratio", PITCH_RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
def test_chain_and_claim(emu_engine, ratio):
    check_chain(emu_engine, ratio)


def test_identity_and_edges(emu_engine):
    check_identity_and_edges(emu_engine)


def test_batch_int16_and_device_pointers(emu_engine):
    check_batch_forms(emu_engine, numpy_alloc)


def test_schedule(emu_engine):
    check_schedule(emu_engine)


def test_refusals_and_unload(emu_engine):
    check_refusals(emu_engine)


def test_shifter_object(emu_engine):
    check_shifter_object(emu_engine)


def run_c_program(lib_path, tmp_path):
    """tests/c_abi/shift_ragged.c against `lib_path`: a ragged batch with an empty row through the plain C ABI in both modes, every
    output, both input forms, each row compared with its batch-1 call and its own positions fed back, inside the program."""
    import shutil
    import subprocess
    from pathlib import Path

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    repo = Path(__file__).resolve().parent.parent
    lib_path = Path(lib_path).resolve()
    exe = tmp_path / "shift_ragged"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-O1", f"-I{repo / 'include'}",
                    str(repo / "tests" / "c_abi" / "shift_ragged.c"), "-o", str(exe), str(lib_path), f"-Wl,-rpath,{lib_path.parent}", "-lm"], check=True)
    out = subprocess.run([str(exe), "0"], check=True, capture_output=True, text=True, timeout=600).stdout.splitlines()
    print("\n".join(out))
    assert out[-1] == "ok" and len(out) >= 5, out


def test_c_caller(emu_library, tmp_path):
    run_c_program(emu_library, tmp_path)


def test_sentence_path(emu_library):
    from tests.test_emu_analysis import tiny_voice
    from tests.test_emu_resample import vocoder

    check_sentence_path(tiny_voice(emu_library), vocoder(emu_library))
