"""TEST ORACLE — the true-peak meter and look-ahead limiter as include/mi355tts.h "limiter" defines them, in numpy.

`oracle` is the definition in float64, sequential.  `restate_f32` is the same steps in float32, sequential and in the term
orders of the header (the interpolation is tests/resample_np.py's restatement at up = os, down = 1; the release multiplies by a
once per sample): with a = 0 the device equals it bit for bit, with a > 0 it is the yardstick of the tests' bound (the device
may lie 16 x as far from the float64 oracle as this restatement does on the same input, never less than 4 ulp of 1.0)."""
import numpy as np

from tests import resample_np as R

F = np.float32


def tone_with_clicks(n, fs=22050, amp=0.05, click=0.9, every=9000):
    """A quiet 997 Hz tone carrying a click every `every` samples: a peak-to-loudness ratio no single gain can level."""
    x = amp * np.sin(2 * np.pi * 997.0 * np.arange(n) / float(fs))
    x[::every] = click
    return x.astype(np.float32)


def intersample(n, amp=0.9):
    """amp sin(2 pi n / 4 + pi / 4): every sample at amp / sqrt 2, the true peak amp between them."""
    return (amp * np.sin(2 * np.pi * np.arange(n) / 4.0 + np.pi / 4.0)).astype(np.float32)


def _fma32(acc, w, v):
    """acc + w * v rounded once to float32 (the product of two float32 values is exact in float64)"""
    return (acc.astype(np.float64) + np.float64(w) * v.astype(np.float64)).astype(np.float32)


def interpolate64(x, taps, os):
    """u[m] = sum_i x[i] taps[m + H - i os] for m in [0, N os), float64"""
    x = np.asarray(x, np.float64)
    if os == 1 or len(x) == 0:
        return x.copy()
    taps = np.asarray(taps, np.float64)
    H = (len(taps) - 1) // 2
    up = np.zeros(len(x) * os)
    up[::os] = x
    return np.convolve(up, taps)[H:H + len(x) * os]


def true_peaks(x, taps, os, f32):
    """tp[n] = max(|x[n]|, max_p |u[n os + p]|)"""
    x = np.asarray(x, F)
    if os == 1 or len(x) == 0:
        return np.abs(x) if f32 else np.abs(x.astype(np.float64))
    u = R.restate_f32(x, taps, os, 1) if f32 else interpolate64(x, taps, os)
    return np.maximum(np.abs(x).astype(u.dtype), np.abs(u).reshape(len(x), os).max(axis=1))


def hold(c, la):
    """m at the row's positions j = k + la, k = -la .. N - 1: min(c[k - 1 .. k + la]), c = 1 outside the row"""
    one = np.ones(1, c.dtype)
    cp = np.concatenate([np.repeat(one, la + 1), c, np.repeat(one, la)])
    return np.lib.stride_tricks.sliding_window_view(cp, la + 2).min(axis=1)


def release(m, a):
    """d[k] = max(1 - m[k], a d[k - 1]) from d = 0, in m's own type, one product per sample"""
    e = (m.dtype.type(1) - m).astype(m.dtype)
    if a == 0 or len(e) == 0:
        return e
    a = m.dtype.type(a)
    d = np.empty_like(e)
    prev = m.dtype.type(0)
    for k in range(len(e)):
        prev = max(e[k], a * prev)
        d[k] = prev
    return d


def smooth(d, w, la, n, f32):
    """s[n] = max(0, 1 - sum_j w[j] d[n - j]), j ascending from +0; d at positions: step n - j is position n - j + la"""
    acc = np.zeros(n, F if f32 else np.float64)
    for j in range(la + 1):
        seg = d[la - j:la - j + n]
        acc = _fma32(acc, w[j], seg) if f32 else acc + np.float64(w[j]) * seg
    one = acc.dtype.type(1)
    return np.maximum(one - acc, acc.dtype.type(0))


def run(x, gain, ceiling, os, taps, la, a, w, f32):
    """Every step of the definition -> {"tp", "TP", "c", "s", "y", "i16", "min_gain"} in float32 (`f32`) or float64.  The
    parameters are taken as the device sees them: float32 values, widened."""
    T = F if f32 else np.float64
    x = np.asarray(x, F)
    n = len(x)
    G, C, a = T(F(gain)), T(F(ceiling)), T(F(a))
    w = np.asarray(w, F)
    tp = true_peaks(x, taps, os, f32).astype(T)
    t = (tp * G).astype(T)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(t <= C, T(1), (C / np.where(t > 0, t, T(1))).astype(T)).astype(T)
    if n == 0:
        z = np.zeros(0, T)
        return {"tp": tp, "TP": T(0), "c": c, "s": z, "y": z, "i16": np.zeros(0, np.int16), "min_gain": T(1)}
    d = release(hold(c, la), a)
    s = smooth(d, w, la, n, f32)
    xg = (x.astype(T) * G).astype(T)
    y = np.clip((xg * s).astype(T), -C, C)
    i16 = np.clip(np.rint(y.astype(np.float64) * 32768), -32768, 32767).astype(np.int16)
    return {"tp": tp, "TP": tp.max(), "c": c, "s": s, "y": y, "i16": i16, "min_gain": s.min()}


def oracle(x, gain, ceiling, os, taps, la, a, w):
    return run(x, gain, ceiling, os, taps, la, a, w, False)


def restate_f32(x, gain, ceiling, os, taps, la, a, w):
    return run(x, gain, ceiling, os, taps, la, a, w, True)


def normalize_limited(x, fs, target, ceiling, max_gain_db, os, taps, la, a, w, tolerance=0.1):
    """`Loudness.normalize_limited` in float64 on the loudness oracle: -> (delivered float64 row, its level, the gain, passes)"""
    from tests import loudness_np as L

    l0 = L.oracle(x, fs)[2]
    if not np.isfinite(l0):
        return np.asarray(x, np.float64), l0, 1.0, 1
    cap = 10.0 ** (max_gain_db / 20.0)
    g = min(10.0 ** ((target - l0) / 20.0), cap)
    y = oracle(x, g, ceiling, os, taps, la, a, w)["y"]
    l1 = L.oracle(y, fs)[2]
    if l1 < target - tolerance and g < cap:
        g = min(g * 10.0 ** ((target - l1) / 20.0), cap)
        y = oracle(x, g, ceiling, os, taps, la, a, w)["y"]
        return y, L.oracle(y, fs)[2], g, 2
    return y, l1, g, 1
