"""The resampler of csrc/resample.h in numpy: the float64 oracle (the definition in include/mi355tts.h, summed directly), its
float32 restatement (the device's table layout and term order, one rounding per fma emulated in float64 arithmetic rounded
back), and the filter design — written out here independently of larynx_amd/resample.py, which the tests compare it with."""
import numpy as np

# rate_out -> (up, down) from 22 050 Hz: the five ratios of the design table
RATIOS = {16000: (320, 441), 8000: (160, 441), 48000: (320, 147), 44100: (2, 1), 24000: (160, 147)}
HAND_TAPS = np.array([-0.01, 0.03, 0.12, 0.27, 0.33, 0.27, 0.12, 0.03, -0.01], np.float32)  # 9 taps, half_len 4, symmetric


def design(up, down, zero_crossings=16, beta=9.0):
    """Kaiser-windowed sinc in float64, rounded once: (taps float32 [2 H + 1], H)."""
    W = max(up, down)
    H = zero_crossings * W
    j = np.arange(-H, H + 1, dtype=np.float64)
    taps = (up / W) * np.sinc(j / W) * np.kaiser(2 * H + 1, beta)
    return taps.astype(np.float32), H


def out_length(n, up, down):
    return -((-int(n) * up) // down)


def taps_per_phase(half_len, up):
    return -(-(2 * half_len + 1) // up)


def table(taps, up):
    """The polyphase table [up][Tp]: entry [p][t] = taps[p + t * up], T = ceil((2 H + 1) / up) padded to a multiple of 4 with
    zeros."""
    taps = np.asarray(taps)
    T = -(-len(taps) // up)
    Tp = (T + 3) // 4 * 4
    full = np.zeros((Tp, up), taps.dtype)
    full.reshape(-1)[: len(taps)] = taps  # row t, column p = taps[t * up + p]
    return np.ascontiguousarray(full.T)


def oracle(x, taps, up, down):
    """y[n] = sum_i x[i] * taps[n * down + H - i * up] in float64, every product exact, summed by numpy's dot."""
    x = np.asarray(x, np.float64)
    taps = np.asarray(taps, np.float64)
    H = (len(taps) - 1) // 2
    N = len(x)
    y = np.zeros(out_length(N, up, down), np.float64)
    for n in range(len(y)):
        c = n * down + H
        lo = max(0, -((2 * H - c) // up))  # ceil((c - 2 H) / up)
        hi = min(N - 1, c // up)
        if hi >= lo:
            i = np.arange(lo, hi + 1)
            y[n] = np.dot(x[i], taps[c - i * up])
    return y


def restate_f32(x, taps, up, down):
    """The device's arithmetic: float32 table rows, tap t of phase p = c mod up against x[c div up - t], t ascending, one
    float32 fma per term (a float64 product of two float32 values is exact, and float64(acc) + that product, rounded once to
    float32, is the fma's result up to double rounding, which these magnitudes do not reach in practice)."""
    x = np.asarray(x, np.float32)
    tab = table(np.asarray(taps, np.float32), up).astype(np.float64)
    H = (len(taps) - 1) // 2
    N = len(x)
    n = np.arange(out_length(N, up, down), dtype=np.int64)
    c = n * down + H
    p, q = c % up, c // up
    xp = np.concatenate([x.astype(np.float64), [0.0]])  # index N: the zero outside the row
    acc = np.zeros(len(n), np.float32)
    for t in range(tab.shape[1]):
        i = q - t
        xi = xp[np.where((i >= 0) & (i < N), i, N)]
        acc = (acc.astype(np.float64) + tab[p, t] * xi).astype(np.float32)
    return acc


def worst_phase_abs_sum(taps, up):
    return float(np.abs(table(np.asarray(taps, np.float64), up)).sum(axis=1).max())


def a_priori_bound(taps, up, xmax):
    """T * 2^-24 * (worst-phase sum of abs taps) * max|x|: T roundings of half an ulp of a partial sum that never exceeds the
    worst-phase sum of abs taps times max|x|."""
    H = (len(taps) - 1) // 2
    return taps_per_phase(H, up) * 2.0 ** -24 * worst_phase_abs_sum(taps, up) * float(xmax)


def tone_noise(n, seed=0, freq=440.0, rate=22050.0):
    """Tone plus seeded noise, |x| <= 1, float32."""
    rng = np.random.default_rng(seed)
    x = 0.6 * np.sin(2 * np.pi * freq * np.arange(n) / rate) + 0.4 * rng.uniform(-1.0, 1.0, n)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def float_to_int16(y):
    """The reference's audio_float_to_int16 (larynx/audio.py:118-125) on float32 data, as the device applies it."""
    y = np.asarray(y, np.float32)
    peak = np.float32(max(0.01, float(np.abs(y).max()) if y.size else 0.0))
    g = np.float32(32767.0) / peak
    return np.clip(y * g, -32767, 32767).astype(np.int16)
