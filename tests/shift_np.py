"""TEST ORACLE — the pitch shifter of include/mi355tts.h ("pitch shift and tempo") in numpy.

  lengths      L = ceil(n up / down), K = (L - 1) / Hs + 2 frames
  positions    the recurrence of step 2, in float32 exactly as the header writes it (`dtype=np.float32`: the BIT reference of
               shift_mark_kernel — one division, two rint, one product, each a single float32 operation, which numpy states
               exactly) or in float64 (what the recurrence means)
  ola          step 3 in float32 (two products and one add, each rounded once: the BIT reference of shift_ola_kernel) or float64
  chain        the whole call for given positions: the overlap-add, then — PITCH mode — the first n samples of
               tests/resample_np.py's resampler by down / up (float64: `oracle`; float32: `restate_f32`, an anchor, not a bit
               reference)
  shift        periods (tests/pitch_np.py) -> positions -> chain: the float64 prototype of the whole algorithm

The reference has no such step; the float64 statement is the standard."""
import numpy as np

from tests import pitch_np as P
from tests import resample_np as R


def lengths(n, up, down, N):
    """(L, K) of a row of n samples."""
    L = -((-int(n) * up) // down)
    return L, ((L - 1) // (N // 2) + 2 if L > 0 else 0)


def anchors(K, up, down, N):
    """(c_k, a_k) int64 [K]."""
    Hs = N // 2
    c = np.arange(K, dtype=np.int64) * Hs * down // up
    return c, c - Hs


def positions(n, f0, sample_rate, hop_p, up, down, N, dtype=np.float32):
    """s_k int64 [K] from the row's f0 plane (float32 [Fp], Fp = n // hop_p)."""
    dtype = np.dtype(dtype).type
    Hs = N // 2
    L, K = lengths(n, up, down, N)
    c, a = anchors(K, up, down, N)
    f0 = np.asarray(f0, np.float32)
    Fp = int(n) // hop_p
    assert len(f0) >= Fp
    s = np.zeros(K, np.int64)
    for k in range(K):
        if k == 0 or Fp == 0:
            s[k] = a[k]
            continue
        j = min(Fp - 1, int(c[k] + hop_p // 2) // hop_p)
        if f0[j] == 0:
            s[k] = a[k]
            continue
        T = dtype(sample_rate) / dtype(f0[j])
        e = int(s[k - 1] + Hs - a[k])
        q = np.rint(dtype(e) / T)
        m = np.rint(dtype(q * T))
        s[k] = a[k] + (e - int(m))
    return s


def as_float(x, dtype):
    return P.as_float(x, dtype)


def ola(x, w, pos, up, down, dtype=np.float32):
    """y [L] of one row: x float32 or int16 [n], w float32 [N], pos int [>= K]."""
    dtype = np.dtype(dtype).type
    x = as_float(x, dtype)
    w = np.asarray(w, np.float32).astype(dtype)
    n, N = len(x), len(w)
    Hs = N // 2
    L, K = lengths(n, up, down, N)
    pos = np.asarray(pos, np.int64)
    assert len(pos) >= K
    t = np.arange(L, dtype=np.int64)
    k1 = t // Hs
    i2 = t - k1 * Hs
    i1 = i2 + Hs
    xp = np.concatenate([x, np.zeros(1, dtype)])  # index n: the zero outside the row

    def take(i):
        return xp[np.where((i >= 0) & (i < n), i, n)]

    if L == 0:
        return np.zeros(0, dtype)
    a = (w[i1] * take(pos[k1] + i1)).astype(dtype)
    b = (w[i2] * take(pos[k1 + 1] + i2)).astype(dtype)
    return (a + b).astype(dtype)


def chain(x, w, pos, up, down, taps=None, dtype=np.float64):
    """The delivered row for given positions: TEMPO (taps None): y; PITCH: the first n samples of y resampled by down / up with the
    prototype `taps`."""
    y = ola(x, w, pos, up, down, dtype)
    if taps is None:
        return y
    n = len(x)
    z = R.oracle(y, taps, down, up) if np.dtype(dtype) == np.float64 else R.restate_f32(y, taps, down, up)
    assert len(z) >= n
    return z[:n]


def shift(x, w, up, down, taps, theta=0.15, dtype=np.float64, **geom):
    """The whole algorithm on the host: (delivered row, positions, f0).  `geom`: sample_rate, hop, W, tau_min, tau_max of the tracker."""
    f0 = P.track(x, theta=theta, interpolate=True, dtype=dtype, **geom)["f0"].astype(np.float32)
    pos = positions(len(x), f0, geom["sample_rate"], geom["hop"], up, down, len(w), dtype)
    return chain(x, w, pos, up, down, taps, dtype), pos, f0


def window(N):
    """The periodic Hann of larynx_amd.shift.ola_window, written out independently."""
    i = np.arange(N, dtype=np.float64)
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * i / N)).astype(np.float32)
    w[N // 2:] = np.float32(1.0) - w[:N // 2]
    return w


def ulps(got, ref):
    """|got - ref| in units of ref's float32 spacing."""
    ref = np.asarray(ref, np.float32)
    return np.abs(np.asarray(got, np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
