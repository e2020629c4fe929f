"""Resampling (csrc/resample.h: delivered rows at another sample rate, one launch, two with MI355TTS_PCM_NORMALIZE) on the CPU
emulator.

Oracle: tests/resample_np.py — the definition of include/mi355tts.h summed directly in float64 (`oracle`, pinned to
`scipy.signal.resample_poly` here), and its float32 restatement in the device's term order (`restate_f32`).

Bound of the parity tests: the device may lie 16 x as far from the float64 oracle as the float32 restatement does on the same
input (the project's rule for the analysis kernel), and never above T * 2^-24 * (worst-phase sum of abs taps) * max|x|: T
roundings of at most half an ulp of a partial sum that the worst phase's abs taps bound.  The impulse test has no tolerance.
The check functions are shared with tests/test_gpu_resample.py."""
import ctypes as C
import io
from pathlib import Path

import numpy as np
import pytest

from larynx_amd import ffi
from larynx_amd import hparams as HP
from larynx_amd import synthetic
from larynx_amd.alignment import scale_spans
from larynx_amd.resample import Resampler, design_lowpass, get_resampler
from tests import resample_np as R

RATES = (16000, 8000, 48000, 44100, 24000)
HAND = ((3, 2), (1, 2), (2, 1))
_cache = {}


def prototype(up, down, kind=None):
    """(taps, H) of `kind` "design" (Kaiser-windowed sinc) or "hand" (the 9-tap hand-made prototype).  Without a kind: what the
    device models of these tests are loaded with — the design for the five ratios of the table, the hand-made taps elsewhere."""
    kind = kind or ("design" if (up, down) in R.RATIOS.values() else "hand")
    return R.design(up, down) if kind == "design" else (R.HAND_TAPS, 4)


def model(eng, up, down):
    key = (id(eng), up, down)
    if key not in _cache:
        _cache[key] = eng.load_resampler(prototype(up, down)[0], up, down)
    return _cache[key]


def reference(up, down, n, seed=0):
    """(x, float64 oracle, the float32 restatement's error, the a-priori bound): computed once per case, never changed."""
    key = ("ref", up, down, n, seed)
    if key not in _cache:
        taps, _ = prototype(up, down)
        x = R.tone_noise(n, seed)
        y = R.oracle(x, taps, up, down)
        e32 = float(np.abs(R.restate_f32(x, taps, up, down) - y).max())
        _cache[key] = (x, y, e32, R.a_priori_bound(taps, up, float(np.abs(x).max())))
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_impulses(eng, up, down):
    """x = delta_k gives y[n] == taps[n * down - k * up + H] bit for bit, 0 where the index leaves the prototype."""
    taps, H = prototype(up, down)
    m = model(eng, up, down)
    seam = int(round(255.5 * down / up))  # its response is centred between outputs 255 and 256
    cases = [(700, 0), (700, 1), (700, 699)]
    # at 160 / 441 700 samples give 254 outputs, one tile: the seam needs a longer row there
    cases.append((700 if R.out_length(700, up, down) > 300 else 1500, seam))
    for N, k in cases:
        x = np.zeros(N, np.float32)
        x[k] = 1.0
        y, _, n_out = eng.resample(m, x)
        assert n_out[0] == len(y) == R.out_length(N, up, down)
        idx = np.arange(len(y), dtype=np.int64) * down - k * up + H
        inside = (idx >= 0) & (idx <= 2 * H)
        exp = np.where(inside, taps[np.clip(idx, 0, 2 * H)], np.float32(0)) + np.float32(0)  # (the sum starts from +0)
        hit = np.flatnonzero(inside)
        print(f"{up}/{down} N={N} k={k}: outputs {hit[0]}..{hit[-1]} carry the prototype, {int((bits(y) != bits(exp)).sum())} differ")
        if k == seam:
            assert hit[0] <= 255 and hit[-1] >= 256
        assert np.array_equal(bits(y), bits(exp))


def check_lengths(eng):
    """N_out and the zero tail up to out_ld, at the edges of a row and of a tile."""
    for (up, down), sizes in (((160, 441), (0, 1, 2, 5)), ((320, 441), (0, 1, 2, 5, 351, 352, 353)), ((320, 147), (1500,))):
        taps, H = prototype(up, down)
        m = model(eng, up, down)
        for N in sizes:
            n_out = R.out_length(N, up, down)
            assert eng.resample_length(m, N) == n_out
            x = R.tone_noise(max(N, 1), 5)[:N]
            ld = n_out + 37
            f32 = np.full((1, ld), 7.0, np.float32)
            i16 = np.full((1, ld), 7, np.int16)
            xin = np.ascontiguousarray(x) if N else np.zeros(1, np.float32)
            got = eng.resample_raw(m, xin.ctypes.data, None, [N], N, f32.ctypes.data, i16.ctypes.data, ld)
            assert got[0] == n_out
            assert np.all(f32[0, n_out:] == 0) and np.all(i16[0, n_out:] == 0)
            y = R.oracle(x, taps, up, down)
            err = float(np.abs(f32[0, :n_out] - y).max()) if n_out else 0.0
            print(f"{up}/{down} N={N}: {n_out} outputs, tail of 37 zero, max error {err:.2e}")
            assert err <= R.a_priori_bound(taps, up, 1.0)
            if N and n_out:
                assert np.abs(f32[0, :n_out]).max() > 0
    assert {R.out_length(n, 320, 441) for n in (351, 352, 353)} == {255, 256, 257} and R.out_length(1500, 320, 147) == 3266
    assert R.taps_per_phase(prototype(160, 441)[1], 160) == 89  # 5 samples are shorter than one phase


def check_parity(eng, rate, n):
    up, down = R.RATIOS[rate]
    x, y, e32, bound = reference(up, down, n)
    got, _, n_out = eng.resample(model(eng, up, down), x)
    assert got.shape == y.shape and n_out[0] == len(y) and np.isfinite(got).all()
    err = float(np.abs(got - y).max())
    print(f"22050 -> {rate} ({up}/{down}) N={n}: device {err:.2e}, float32 restatement {e32:.2e} (x {err / e32:.2f}), a-priori bound {bound:.2e}")
    assert 0 < e32 and err <= 16.0 * e32 and err <= bound
    return err, e32


def check_ragged(eng, up, down):
    """B = 3, samples (700, 0, 257), in_ld 768: every row equals its batch-1 call bit for bit, in all three output forms."""
    m = model(eng, up, down)
    samples = (700, 0, 257)
    batch = np.full((3, 768), 0.25, np.float32)  # what lies past a row's samples must not be read
    for b, n in enumerate(samples):
        batch[b, :n] = R.tone_noise(n, 10 + b)
    f32, sat, n_out = eng.resample(m, batch, samples, want_int16=True)
    _, nrm, _ = eng.resample(m, batch, samples, want_float=False, want_int16=True, normalize=True)
    exp = [R.out_length(n, up, down) for n in samples]
    assert list(n_out) == exp and f32.shape == sat.shape == nrm.shape == (3, max(exp))
    for b, n in enumerate(samples):
        assert np.all(f32[b, exp[b]:] == 0) and np.all(sat[b, exp[b]:] == 0) and np.all(nrm[b, exp[b]:] == 0)
        if not n:
            continue
        one, one_sat, one_n = eng.resample(m, batch[b, :n], want_int16=True)
        _, one_nrm, _ = eng.resample(m, batch[b, :n], want_float=False, want_int16=True, normalize=True)
        assert one_n[0] == exp[b] and np.array_equal(bits(one), bits(f32[b, : exp[b]]))
        assert np.array_equal(one_sat, sat[b, : exp[b]]) and np.array_equal(one_nrm, nrm[b, : exp[b]])
        assert np.abs(one).max() > 0.1
    print(f"{up}/{down}: rows of {samples} samples -> {exp}, each bit-identical to its batch-1 call")


def check_int16_input(eng, up, down):
    m = model(eng, up, down)
    i16 = np.round(R.tone_noise(700, 3) * 32767).astype(np.int16)
    i16[:2] = (-32768, 32767)
    a, _, _ = eng.resample(m, i16)
    b, _, _ = eng.resample(m, i16.astype(np.float32) * np.float32(2.0 ** -15))
    assert np.abs(a).max() > 0.1 and np.array_equal(bits(a), bits(b))


def burst(n=700):
    """+-1 square-ish burst: the low-pass overshoots full scale at its edges."""
    x = np.zeros(n, np.float32)
    x[100:300] = 1.0
    x[300:500] = -1.0
    return x


def check_int16_output(eng, up, down):
    m = model(eng, up, down)
    f32, sat, _ = eng.resample(m, burst(), want_int16=True)
    exp = np.clip(np.rint(f32.astype(np.float64) * 32768), -32768, 32767).astype(np.int16)
    print(f"{up}/{down} saturate: float peak {f32.max():.4f} / {f32.min():.4f}, int16 {sat.max()} / {sat.min()}")
    assert f32.max() > 1.0 and f32.min() < -1.0
    assert np.array_equal(sat, exp) and sat.max() == 32767 and sat.min() == -32768
    x = R.tone_noise(700, 8) * np.float32(0.3)
    f32, nrm, _ = eng.resample(m, x, want_int16=True, normalize=True)
    exp = R.float_to_int16(f32)
    d = int(np.abs(nrm.astype(np.int32) - exp.astype(np.int32)).max())
    print(f"{up}/{down} normalize: float peak {np.abs(f32).max():.4f}, int16 peak {np.abs(nrm.astype(np.int32)).max()}, {d} LSB from numpy")
    assert d <= 1 and np.abs(nrm.astype(np.int32)).max() == 32767
    _, zero, _ = eng.resample(m, np.zeros(300, np.float32), want_int16=True, normalize=True)
    assert zero.shape == (R.out_length(300, up, down),) and not zero.any()


def check_schedule(eng, up, down):
    """One launch in class `elementwise`, two with NORMALIZE, none anywhere else and no counted kernel name."""
    m = model(eng, up, down)
    x = R.tone_noise(700, 2)
    eng.set_profiling(True)
    try:
        for kw, launches in ((dict(), 1), (dict(want_int16=True), 1), (dict(want_int16=True, normalize=True), 2),
                             (dict(want_float=False, want_int16=True, normalize=True), 2)):
            eng.profile_reset()
            eng.resample(m, x, **kw)
            prof = eng.profile()
            counts = eng.kernel_counts()
            print(f"{up}/{down} {kw}: {prof['elementwise']['launches']} launches, {prof['elementwise']['ms']:.4f} ms")
            assert prof["elementwise"]["launches"] == launches
            assert all(v["launches"] == 0 for k, v in prof.items() if k != "elementwise"), prof
            assert all(v == 0 for v in counts.values()), counts
            assert set(eng.profile_kernels()) == {"elementwise"} and set(eng.profile_kernels()["elementwise"]) == {"-/0"}
    finally:
        eng.set_profiling(False)
        eng.profile_reset()


def _refused(fn, what, code=-1):
    with pytest.raises(ffi.Mi355ttsError) as e:
        fn()
    msg = str(e.value).split(": ", 1)[1]
    assert e.value.code == code and msg and what in msg, str(e.value)


def check_refusals(eng):
    lib, mid = eng.lib, C.c_int()
    taps = R.HAND_TAPS

    def load(up, down, half_len, t=taps, params=True, out=True):
        p = ffi.ResamplerParamsC(up, down, half_len)
        return lambda: ffi.check(lib, lib.mi355tts_load_resampler(eng._ctx, C.byref(p) if params else None, None if t is None else t.ctypes.data,
                                                                  C.byref(mid) if out else None))

    _refused(load(3, 2, 4, t=None), "null")
    _refused(load(3, 2, 4, params=False), "null")
    _refused(load(3, 2, 4, out=False), "null")
    for up, down in ((0, 1), (1025, 1), (1, 0), (1, 1025), (-3, 2)):
        _refused(load(up, down, 4), "outside [1, 1024]")
    _refused(load(2, 4, 4), "coprime")
    _refused(load(320, 320, 4), "coprime")
    _refused(load(3, 2, -1), "half_len")
    _refused(load(1, 2, 64, t=np.zeros(129, np.float32)), "taps per phase")
    for bad in (np.nan, np.inf, -np.inf):
        t = taps.copy()
        t[6] = bad
        _refused(load(3, 2, 4, t=t), "not finite")
    load(2, 1, 64, t=np.zeros(129, np.float32))()  # the same 129 taps over two phases: 65 each, accepted
    eng.unload(mid.value)
    m = model(eng, 3, 2)
    x = np.ascontiguousarray(R.tone_noise(700, 1))
    i16 = np.zeros(700, np.int16)
    of = np.zeros(1050, np.float32)
    oi = np.zeros(1050, np.int16)
    n = np.array([700], np.int64)

    def call(f32=x.ctypes.data, s16=None, samples=n, in_ld=700, o32=of.ctypes.data, o16=oi.ctypes.data, out_ld=1050, mode=0, mdl=m):
        s_p = None if samples is None else samples.ctypes.data_as(C.POINTER(C.c_int64))
        return lambda: ffi.check(lib, lib.mi355tts_resample(eng._ctx, mdl, f32, s16, s_p, 1, in_ld, o32, o16, out_ld, mode, None, 0))

    _refused(call(samples=None), "null")
    _refused(call(s16=i16.ctypes.data), "exactly one")
    _refused(call(f32=None), "exactly one")
    _refused(call(o32=None, o16=None), "no output")
    for bad in (-1, 701):
        _refused(call(samples=np.array([bad], np.int64)), "samples[0]")
    big = (1 << 24) + 1  # (refused before anything is read)
    _refused(call(samples=np.array([big], np.int64), in_ld=big), "2^24")
    _refused(call(out_ld=1049), "out_ld")
    _refused(call(out_ld=-1), "out_ld")
    for mode in (2, -1):
        _refused(call(mode=mode), "pcm_mode")
    _refused(call(mdl=10 ** 6), "no resampler", code=-5)
    _refused(lambda: eng.resample_length(10 ** 6, 5), "no resampler", code=-5)
    _refused(lambda: eng.resample_length(m, -1), "samples")
    _refused(lambda: eng.resample_length(m, big), "samples")
    call()()  # the context still works
    assert np.abs(of).max() > 0.1
    gone = eng.load_resampler(taps, 2, 1)
    assert eng.resample_length(gone, 7) == 14
    eng.unload(gone)
    _refused(lambda: eng.resample(gone, x), "no resampler", code=-5)
    with pytest.raises(ValueError):
        eng.load_resampler(taps[:8], 3, 2)


def check_direct_path(eng):
    """down / up above ~7: the tile's inputs no longer fit the staged span and the kernel reads them in place — same definition,
    same bound, impulses still exact."""
    up, down = 1, 16
    taps, H = prototype(up, down)
    m = model(eng, up, down)
    x = R.tone_noise(5000, 4)  # 313 outputs: two tiles
    y = R.oracle(x, taps, up, down)
    got, _, _ = eng.resample(m, x)
    e32 = float(np.abs(R.restate_f32(x, taps, up, down) - y).max())
    err = float(np.abs(got - y).max())
    print(f"1/16 N=5000 (unstaged): device {err:.2e}, float32 restatement {e32:.2e}")
    assert len(got) == 313 and err <= 16.0 * e32 and err <= R.a_priori_bound(taps, up, 1.0)
    i16 = np.round(x * 32767).astype(np.int16)
    a, _, _ = eng.resample(m, i16)
    b, _, _ = eng.resample(m, i16.astype(np.float32) * np.float32(2.0 ** -15))
    assert np.array_equal(bits(a), bits(b))
    d = np.zeros(5000, np.float32)
    d[4096] = 1.0  # c = 16 n + 4 - 4096: outputs 256 (tap 4) alone
    got, _, _ = eng.resample(m, d)
    exp = np.zeros(313, np.float32)
    exp[256] = taps[4]
    assert np.array_equal(bits(got), bits(exp))


def vocoder(library_path=None):
    from larynx_amd.constants import VocoderModelConfig
    from larynx_amd.hifi_gan import HipHiFiGanVocoder

    return HipHiFiGanVocoder(VocoderModelConfig(model_path=Path("unused")), library_path=library_path,
                             state_dict=synthetic.make_hifigan_state_dict(HP.TINY_HIFIGAN, seed=3), model_config=HP.TINY_HIFIGAN.to_config())


def numpy_alloc(a):
    """`alloc(array)` of the device-pointer checks -> (pointer, fetch) of a device buffer that starts as a copy of `array`;
    `fetch()` gives its contents.  The emulator's device memory is the host's."""
    a = np.array(a)
    return a.ctypes.data, lambda: a


def torch_alloc(a):
    """The same on the GPU (the tensor lives as long as `fetch` does)."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), lambda: t.cpu().numpy()


def check_device_pointers(eng, alloc):
    """MI355TTS_IN_DEVICE | MI355TTS_OUT_DEVICE: device buffers (float32 and int16 in, all three output forms, row strides past the
    rows' samples, outputs pre-filled) give the host call's bits and zero tails up to out_ld.  Then a batch whose rows are all
    empty, to host and to device destinations: every output element zero, every length 0."""
    up, down = 320, 441
    m = model(eng, up, down)
    samples = (700, 0, 257)
    batch = np.full((3, 768), 0.25, np.float32)
    for b, n in enumerate(samples):
        batch[b, :n] = R.tone_noise(n, 10 + b)
    i16 = np.round(batch * 32767).astype(np.int16)
    ld = R.out_length(700, up, down) + 21
    flags = ffi.IN_DEVICE | ffi.OUT_DEVICE
    for src in (batch, i16):
        host_f, host_sat, n_out = eng.resample(m, src, samples, want_int16=True)
        _, host_nrm, _ = eng.resample(m, src, samples, want_float=False, want_int16=True, normalize=True)
        dev, keep = alloc(src)
        ptrs = (None, dev) if src.dtype == np.int16 else (dev, None)
        for mode, host_i, with_float in ((ffi.PCM_SATURATE, host_sat, True), (ffi.PCM_NORMALIZE, host_nrm, True), (ffi.PCM_NORMALIZE, host_nrm, False)):
            (pf, get_f), (pi, get_i) = alloc(np.full((3, ld), 7.0, np.float32)), alloc(np.full((3, ld), 7, np.int16))
            got = eng.resample_raw(m, ptrs[0], ptrs[1], samples, 768, pf if with_float else None, pi, ld, mode, flags)
            assert list(got) == list(n_out)
            f, i = get_f(), get_i()
            w = host_f.shape[1]
            if with_float:
                assert np.array_equal(bits(f[:, :w]), bits(host_f)) and not f[:, w:].any()
            else:
                assert np.all(f == 7.0)
            assert np.array_equal(i[:, :w], host_i) and not i[:, w:].any()
        # no sample in any row
        host_src = np.ascontiguousarray(src)
        h_ptrs = (None, host_src.ctypes.data) if src.dtype == np.int16 else (host_src.ctypes.data, None)
        for in_ptrs, buffer, fl in ((h_ptrs, numpy_alloc, 0), (ptrs, alloc, flags)):
            (pf, get_f), (pi, get_i) = buffer(np.full((3, ld), 7.0, np.float32)), buffer(np.full((3, ld), 7, np.int16))
            got = eng.resample_raw(m, in_ptrs[0], in_ptrs[1], (0, 0, 0), 768, pf, pi, ld, ffi.PCM_SATURATE, fl)
            assert not got.any() and not get_f().any() and not get_i().any()
        del keep


def check_sentence_path(tts, voc):
    import larynx_amd
    from larynx_amd.streaming import stream_raw_pcm

    def float_row(ids, before, after):  # the vocoder's float row as the sentence path makes it (the voice fuses the mel transforms)
        return voc.mels_to_float_padded(tts.phonemes_to_mels(ids, settings=settings), None, before, after)

    rng = np.random.default_rng(41)
    sents = [(f"s{i}", synthetic.synthetic_phoneme_ids(rng, n, HP.TINY_GLOW.num_symbols)) for i, n in enumerate((11, 4, 26))]
    settings = {"seed": 77}
    s = tts.audio_settings
    assert s.sample_rate == 22050
    today = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, alignment=True))
    for rate in (None, 22050):
        same = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, alignment=True, sample_rate=rate))
        for a, b in zip(today, same):
            assert b.sample_rate == 22050 and b.audio.dtype == np.int16 and np.array_equal(a.audio, b.audio)
            assert np.array_equal(a.phoneme_spans, b.phoneme_spans)
    rs = get_resampler(voc.engine, 22050, 16000)
    assert (rs.up, rs.down) == (320, 441) and get_resampler(voc.engine, 22050, 16000) is rs
    at16 = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, alignment=True, sample_rate=16000))
    plain16 = list(larynx_amd.phonemes_to_speech(sents, tts, voc, tts_settings=settings, sample_rate=16000))
    for (text, ids), a, b, p in zip(sents, today, at16, plain16):
        n = a.audio.size
        n16 = -(-n * 320 // 441)
        row = float_row(ids, 0, 0)
        assert row.shape == (n,) and row.dtype == np.float32
        exp = rs.resample(row, normalize=True)
        print(f"{text}: {n} samples at 22050 -> {b.audio.size} at 16000, peak {np.abs(b.audio.astype(np.int32)).max()}")
        assert b.sample_rate == p.sample_rate == 16000 and b.text == text
        assert b.audio.dtype == np.int16 and b.audio.shape == (n16,) == (rs.length(n),)
        assert np.array_equal(b.audio, exp) and np.array_equal(p.audio, exp) and p.phoneme_spans is None
        assert np.abs(b.audio.astype(np.int32)).max() == 32767
        sp = b.phoneme_spans
        assert sp.shape == (len(ids), 2) and sp.dtype == np.int64 and np.array_equal(sp, scale_spans(a.phoneme_spans, 320, 441))
        assert sp[0, 0] == 0 and np.all(sp[1:, 0] == sp[:-1, 1]) and np.all(sp[:, 1] >= sp[:, 0]) and sp[-1, 1] <= b.audio.size
    # pauses travel inside the float row: 10 ms + 20 ms at 22050 Hz, then resampled
    text, ids = sents[0]
    audio, sp = larynx_amd.sentence_task_aligned(text, ids, s, tts, settings, voc, None, 10, 20, 16000)
    row = float_row(ids, 220, 441)
    assert np.array_equal(audio, rs.resample(row, normalize=True)) and audio.size == rs.length(today[0].audio.size + 661)
    assert np.array_equal(audio, larynx_amd.sentence_task_at_rate(text, ids, s, tts, settings, voc, None, 10, 20, 16000))
    assert sp[0, 0] == 220 * 320 // 441 and sp[-1, 1] == (today[0].audio.size + 220) * 320 // 441
    sink = io.BytesIO()
    stats = stream_raw_pcm(iter(sents), tts, voc, sink, tts_settings=settings, sample_rate=16000)
    assert sink.getvalue() == b"".join(r.audio.tobytes() for r in plain16)
    assert stats.sentences == 3 and stats.samples == sum(r.audio.size for r in plain16)
    sink = io.BytesIO()
    stream_raw_pcm(iter(sents), tts, voc, sink, tts_settings=settings, sample_rate=22050)
    assert sink.getvalue() == b"".join(r.audio.tobytes() for r in today)


def check_sentence_path_griffin_lim(tts, library_path=None):
    """A vocoder that delivers the float signal itself (Griffin-Lim): the pauses are padded on the host, then the row is resampled
    and normalised like any other."""
    import larynx_amd
    from larynx_amd.constants import VocoderModelConfig
    from larynx_amd.griffin_lim import HipGriffinLimVocoder

    voc = HipGriffinLimVocoder(VocoderModelConfig(model_path=Path("unused")), num_mels=HP.TINY_GLOW.mel_channels, iterations=4, seed=7,
                               library_path=library_path)
    ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(2), 13, HP.TINY_GLOW.num_symbols)
    settings, s = {"seed": 77}, tts.audio_settings
    today = larynx_amd.sentence_task("gl", ids, s, tts, settings, voc, None, 10, 20)
    assert today.dtype == np.float32 and np.all(today[:220] == 0) and np.all(today[-441:] == 0)
    rs = get_resampler(voc.engine, 22050, 8000)
    got = larynx_amd.sentence_task_at_rate("gl", ids, s, tts, settings, voc, None, 10, 20, 8000)
    print(f"Griffin-Lim: {today.size} float samples at 22050 -> {got.size} int16 at 8000, peak {np.abs(got.astype(np.int32)).max()}")
    assert got.dtype == np.int16 and got.shape == (rs.length(today.size),)
    assert np.array_equal(got, rs.resample(today, normalize=True)) and np.abs(got.astype(np.int32)).max() == 32767
    res = list(larynx_amd.phonemes_to_speech([("gl", ids)], tts, voc, tts_settings=settings, sample_rate=8000))
    assert res[0].sample_rate == 8000 and res[0].audio.shape == (rs.length(today.size - 661),)


# ---------------------------------------------------------------- CPU only: the oracle and the design
@pytest.mark.parametrize("ratio,kind", [(R.RATIOS[r], "design") for r in RATES] + [(r, "hand") for r in HAND])
def test_oracle_is_resample_poly(ratio, kind):
    """The five designed ratios, and (3, 2), (1, 2), (2, 1) with the 9 hand-made taps (2 / 1 is in both lists: once with its
    65-tap design, once with the 9 taps)."""
    signal = pytest.importorskip("scipy.signal")
    up, down = ratio
    taps, H = prototype(up, down, kind)
    assert len(taps) == 2 * H + 1 == (9 if kind == "hand" else 2 * 16 * max(up, down) + 1) and np.array_equal(taps, taps[::-1])
    for n in (1, 5, 700):
        x = R.tone_noise(n, n)
        ref = signal.resample_poly(x.astype(np.float64), up, down, window=taps.astype(np.float64) / up)
        got = R.oracle(x, taps, up, down)
        err = float(np.abs(got - ref).max())
        print(f"{up}/{down} {kind} ({len(taps)} taps) N={n}: {len(got)} outputs, oracle vs resample_poly {err:.1e}")
        assert got.shape == ref.shape and err <= 1e-12


def tone_response(rate, freq):
    """An 8 192-sample, amplitude-0.5 tone through the float64 oracle: (max deviation from the ideal tone at the new rate, level
    in dB re the input), both on the middle half."""
    up, down = R.RATIOS[rate]
    taps, _ = R.design(up, down)
    x = 0.5 * np.sin(2 * np.pi * freq * np.arange(8192) / 22050.0)
    y = R.oracle(x, taps, up, down)
    n = np.arange(len(y))
    mid = slice(len(y) // 4, 3 * len(y) // 4)
    ideal = 0.5 * np.sin(2 * np.pi * freq * n * down / (up * 22050.0))
    return float(np.abs(y - ideal)[mid].max()), 20 * np.log10(max(float(np.abs(y[mid]).max()), 1e-300) / 0.5)


def test_design_properties():
    for rate in RATES:
        up, down = R.RATIOS[rate]
        taps, H = design_lowpass(up, down)
        ref, ref_h = R.design(up, down)
        assert H == ref_h and taps.dtype == np.float32 and np.array_equal(taps, ref)  # the package's design is the oracle's
        dc = R.table(taps.astype(np.float64), up).sum(axis=1)
        print(f"22050 -> {rate}: {len(taps)} taps, T = {R.taps_per_phase(H, up)}, phase DC gains in [{dc.min():.6f}, {dc.max():.6f}], "
              f"worst-phase sum of abs taps {R.worst_phase_abs_sum(taps, up):.3f}")
        assert dc.shape == (up,) and np.abs(dc - 1.0).max() <= 1e-4
    assert [(len(R.design(*R.RATIOS[r])[0]), R.taps_per_phase(R.design(*R.RATIOS[r])[1], R.RATIOS[r][0])) for r in RATES] == [
        (14113, 45), (14113, 89), (10241, 33), (65, 33), (5121, 33)]
    for rate in (8000, 16000, 48000):
        dev, _ = tone_response(rate, 1000.0)
        print(f"1 kHz -> {rate}: {dev:.2e} from the ideal tone")
        assert dev <= 2e-5
    for rate, freq in ((8000, 5000.0), (16000, 10000.0)):
        _, db = tone_response(rate, freq)
        print(f"{freq:.0f} Hz -> {rate}: {db:.1f} dB")
        assert db <= -80.0


def test_resampler_object(emu_engine):
    r = Resampler(emu_engine, 22050, 8000)
    assert (r.up, r.down) == (160, 441) and r.length(700) == 254 == emu_engine.resample_length(r.model_id, 700) and r.length(0) == 0
    x = R.tone_noise(700, 6)
    y = r.resample(x)
    assert y.dtype == np.float32 and y.shape == (254,) and np.abs(y - reference(160, 441, 700, 6)[1]).max() <= 16 * reference(160, 441, 700, 6)[2]
    assert r.resample(x, normalize=True).dtype == np.int16
    same = Resampler(emu_engine, 16000, 16000)
    assert same.model_id is None and same.resample(x) is x and same.length(9) == 9 and (same.up, same.down) == (1, 1)
    for rate_in, rate_out in ((22050, 22051), (22050, 1), (0, 8000)):  # 22051 / 22050 and 1 / 22050: factors above 1024
        with pytest.raises(ValueError):
            Resampler(emu_engine, rate_in, rate_out)
    with pytest.raises(ValueError):
        Resampler(emu_engine, 22050, 16000, zero_crossings=64)  # 129 taps per phase


# ---------------------------------------------------------------- the emulator's runs
@pytest.mark.parametrize("ratio", [(3, 2), (320, 441), (160, 441), (320, 147)])
def test_impulses_are_exact(emu_engine, ratio):
    check_impulses(emu_engine, *ratio)


def test_lengths_and_edges(emu_engine):
    check_lengths(emu_engine)


@pytest.mark.parametrize("n", (257, 700, 1500))
@pytest.mark.parametrize("rate", RATES)
def test_parity(emu_engine, rate, n):
    check_parity(emu_engine, rate, n)


@pytest.mark.parametrize("ratio", [(320, 441), (320, 147)])
def test_ragged_batch_rows_equal_their_batch1_calls(emu_engine, ratio):
    check_ragged(emu_engine, *ratio)


@pytest.mark.parametrize("ratio", [(160, 441), (320, 147)])
def test_int16_input_and_output(emu_engine, ratio):
    check_int16_input(emu_engine, *ratio)
    check_int16_output(emu_engine, *ratio)


def test_schedule(emu_engine):
    check_schedule(emu_engine, 320, 441)


def test_refusals_and_unload(emu_engine):
    check_refusals(emu_engine)


def test_unstaged_path(emu_engine):
    check_direct_path(emu_engine)


def test_device_pointers(emu_engine):
    check_device_pointers(emu_engine, numpy_alloc)


def test_sentence_path(emu_library):
    from tests.test_emu_analysis import tiny_voice

    tts = tiny_voice(emu_library)
    check_sentence_path(tts, vocoder(emu_library))
    check_sentence_path_griffin_lim(tts, emu_library)
