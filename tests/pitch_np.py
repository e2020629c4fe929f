"""TEST ORACLE — the YIN tracker of include/mi355tts.h ("pitch") in numpy.

`track(..., dtype=np.float64)` is the oracle: the definition with plain float64 sums.  `track(..., dtype=np.float32)` is the
restatement: every step in float32, the interpolation and the final division included, in the summation orders the header
documents and csrc/pitch.h keeps:

  d(tau)   four accumulators from +0, accumulator m takes the terms j = m (mod 4), j ascending, subtract then one fma per term;
           d = (a0 + a1) + (a2 + a3)
  r0       256 accumulators, accumulator i takes j = i, i + 256, ..; each 64 of them summed by the butterfly v[l] += v[l ^ m],
           m = 32 .. 1; r0 = (p0 + p1) + (p2 + p3)
  c(tau)   the lags 1 .. 1024 in 256 groups of four with running sums l1 .. l4; a Hillis-Steele scan of l4 over each 64 groups; the
           four totals in sequence; c = (offset + the scan value of the group before) + l_m

(numpy has no fma: the restatement forms acc + e * e in float64, where the product is exact, and rounds once more to float32 —
a double rounding that differs from the fused operation in rare last bits.  It is an anchor for a bound, not a bit reference.)
The reference has no pitch code; this float64 statement is the standard.  It also builds the designed signals of the tests."""
import numpy as np


def as_float(x, dtype):
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(dtype) * dtype(2.0 ** -15)
    return x.astype(dtype)


def frame_count(n, hop):
    return n // hop


def frames_of(x, hop, W, tau_max):
    """[F, W + tau_max]: frame t holds x[t hop - W / 2 + i], zeros outside the row."""
    n = len(x)
    F = frame_count(n, hop)
    span = W + tau_max
    xp = np.zeros(W // 2 + n + span, x.dtype)
    xp[W // 2:W // 2 + n] = x
    return xp[(np.arange(F) * hop)[:, None] + np.arange(span)[None, :]]


def _fma_acc(acc, e, dtype):
    if dtype == np.float32:
        return (acc.astype(np.float64) + e.astype(np.float64) ** 2).astype(np.float32)
    return acc + e * e


def difference(fr, W, tau_max, dtype):
    """d [F, tau_max + 1] (d[:, 0] = 0)."""
    F = fr.shape[0]
    acc = np.zeros((F, tau_max, 4), dtype)
    lag = (np.arange(1, tau_max + 1)[:, None] + np.arange(4)[None, :])  # [tau, m]
    for j in range(0, W, 4):
        e = fr[:, None, j:j + 4] - fr[:, lag + j]
        acc = _fma_acc(acc, e, dtype)
    d = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
    return np.concatenate([np.zeros((F, 1), dtype), d], axis=1)


def energy(fr, W, dtype):
    x = fr[:, :W]
    if dtype != np.float32:
        return (x * x).sum(axis=1)
    F = x.shape[0]
    steps = -(-W // 256)
    xp = np.zeros((F, steps * 256), dtype)
    xp[:, :W] = x
    acc = np.zeros((F, 256), dtype)
    for k in range(steps):
        acc = _fma_acc(acc, xp[:, 256 * k:256 * (k + 1)], dtype)
    v = acc.reshape(F, 4, 64)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ m]
    p = v[..., 0]
    return (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])


def prefix(d, tau_max, dtype):
    """c [F, tau_max + 1]: c(tau) = d(1) + .. + d(tau)."""
    if dtype != np.float32:
        return np.cumsum(d, axis=1)
    F = d.shape[0]
    g = np.zeros((F, 1024), dtype)
    g[:, :tau_max] = d[:, 1:]
    g = g.reshape(F, 256, 4)
    run = np.empty_like(g)
    run[..., 0] = g[..., 0]
    for m in (1, 2, 3):
        run[..., m] = run[..., m - 1] + g[..., m]
    v = run[..., 3].reshape(F, 4, 64).copy()
    for st in (1, 2, 4, 8, 16, 32):
        nv = v.copy()
        nv[..., st:] = v[..., st:] + v[..., :-st]
        v = nv
    tot = v[..., 63]
    off = np.zeros((F, 4), dtype)
    off[:, 1] = tot[:, 0]
    off[:, 2] = tot[:, 0] + tot[:, 1]
    off[:, 3] = (tot[:, 0] + tot[:, 1]) + tot[:, 2]
    before = np.concatenate([np.zeros((F, 4, 1), dtype), v[..., :-1]], axis=2)
    base = (off[..., None] + before).reshape(F, 256)
    c = (base[..., None] + run).reshape(F, 1024)[:, :tau_max]
    return np.concatenate([np.zeros((F, 1), dtype), c], axis=1)


def track(x, sample_rate, hop, W, tau_min, tau_max, theta, interpolate, dtype=np.float64):
    """{"f0", "periodicity", "level_db": [F]; "cmnd": [F, tau_max + 1]; "lag": int [F]; "voiced": bool [F]} of one row."""
    dtype = np.dtype(dtype).type
    x = as_float(x, dtype)
    fr = frames_of(x, hop, W, tau_max)
    F = fr.shape[0]
    d = difference(fr, W, tau_max, dtype)
    r0 = energy(fr, W, dtype)
    ms = r0 / dtype(W)
    with np.errstate(divide="ignore", invalid="ignore"):
        level = np.where(ms > dtype(1e-10), dtype(10) * np.log10(np.maximum(ms, dtype(1e-10))), dtype(-100)).astype(dtype)
        c = prefix(d, tau_max, dtype)
        tau = np.arange(tau_max + 1).astype(dtype)
        dp = np.where(c > 0, (d * tau[None, :]) / c, dtype(1)).astype(dtype)
    dp[:, 0] = 1
    th = dtype(theta)
    lag = np.zeros(F, np.int64)
    voiced = np.zeros(F, bool)
    f0 = np.zeros(F, dtype)
    for t in range(F):
        r = dp[t, tau_min:tau_max + 1]
        below = np.nonzero(r < th)[0]
        if len(below):
            tp = tau_min + int(below[0])
            while tp + 1 <= tau_max and dp[t, tp + 1] < dp[t, tp]:
                tp += 1
            voiced[t] = True
            ts = dtype(tp)
            if interpolate and tp - 1 >= 1 and tp + 1 <= tau_max:
                a, b, cc = dp[t, tp - 1], dp[t, tp], dp[t, tp + 1]
                den = (a - dtype(2) * b) + cc
                if den > 0:
                    ts = dtype(tp) + (dtype(0.5) * (a - cc)) / den
            f0[t] = dtype(sample_rate) / ts
        else:
            tp = tau_min + int(np.argmin(r))
        lag[t] = tp
    per = np.maximum(dtype(0), dtype(1) - dp[np.arange(F), lag]).astype(dtype)
    return {"f0": f0, "periodicity": per, "level_db": level, "cmnd": dp, "lag": lag, "voiced": voiced}


def decided(x, theta, **params):
    """(the float64 oracle at theta, bool [F]: the frames on which the oracle at theta (1 - 1e-3), theta and theta (1 + 1e-3)
    picks the same integer lag and the same voicing)."""
    runs = [track(x, theta=th, dtype=np.float64, **params) for th in (theta * (1 - 1e-3), theta, theta * (1 + 1e-3))]
    ok = np.ones(len(runs[1]["lag"]), bool)
    for r in (runs[0], runs[2]):
        ok &= (r["lag"] == runs[1]["lag"]) & (r["voiced"] == runs[1]["voiced"])
    return runs[1], ok


# ---------------------------------------------------------------- designed signals
def periodic_row(P, n=6000, seed=0):
    """P random float32 values, tiled: an exact integer period."""
    rng = np.random.default_rng(1000 + 7 * P + seed)
    return np.tile(rng.uniform(-0.5, 0.5, P).astype(np.float32), n // P + 1)[:n]


def _harmonics(phase, count, amp):
    return amp * sum(np.sin(h * phase) / h for h in range(1, count + 1))


def designed_signal(fs=22050):
    """2.4 s: silence | a 6-harmonic glide 90 -> 180 Hz | white noise | 220 Hz with +-3 % vibrato at 5 Hz | 440 Hz over a weak 220 Hz
    | a 130 Hz tone at 1e-4 | a 70 Hz tone in noise."""
    rng = np.random.default_rng(2002)

    def t(sec):
        return np.arange(int(round(sec * fs))) / fs

    parts = [np.zeros(len(t(0.3)))]
    u = t(0.5)
    parts.append(_harmonics(2 * np.pi * (90.0 * u + 0.5 * (180.0 - 90.0) / 0.5 * u * u), 6, 0.3))
    parts.append(rng.normal(0.0, 0.05, len(t(0.3))))
    parts.append(_harmonics(2 * np.pi * (220.0 * u - 220.0 * 0.03 / (2 * np.pi * 5.0) * (np.cos(2 * np.pi * 5.0 * u) - 1.0)), 4, 0.3))
    u = t(0.3)
    parts.append(0.4 * np.sin(2 * np.pi * 440.0 * u) + 0.04 * np.sin(2 * np.pi * 220.0 * u))
    parts.append(_harmonics(2 * np.pi * 130.0 * t(0.2), 3, 1e-4))
    parts.append(_harmonics(2 * np.pi * 70.0 * u, 8, 0.3) + rng.normal(0.0, 0.01, len(u)))
    return np.concatenate(parts).astype(np.float32)
