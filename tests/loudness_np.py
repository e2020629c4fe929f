"""TEST ORACLE — ITU-R BS.1770-4 integrated loudness (mono) as include/mi355tts.h "loudness" defines it, in numpy.

`oracle` is the definition in float64: `scipy.signal.lfilter` twice (shelf, then high-pass), blocks, both gates.  `restate_f32`
is the same recurrence sample by sample in float32, in the order of the formula, with block sums in float64: what a
straightforward float32 implementation gives, and the yardstick of the tests' bound (the device may lie 16 x as far from the
float64 oracle as this restatement does on the same input)."""
import numpy as np

from larynx_amd.loudness import block_and_hop, k_weighting

OFFSET = -0.691
ABS_GATE = -70.0
REL_GATE = -10.0


def coefficients(fs):
    """The ten float32 coefficients the device models of the tests are loaded with, and block / hop."""
    c = {k: v.astype(np.float32) for k, v in k_weighting(fs).items()}
    block, hop = block_and_hop(fs)
    return c, block, hop


def weight64(x, c):
    from scipy.signal import lfilter

    x = np.asarray(x, np.float64)
    if x.size == 0:
        return x
    y = lfilter(np.asarray(c["shelf_b"], np.float64), np.r_[1.0, np.asarray(c["shelf_a"], np.float64)], x)
    return lfilter(np.asarray(c["hp_b"], np.float64), np.r_[1.0, np.asarray(c["hp_a"], np.float64)], y)


def weight32(x, c):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2], each biquad a whole pass, every operation rounded to
    float32, left to right."""
    f = np.float32
    y = np.asarray(x, np.float32)
    for b, a in ((c["shelf_b"], c["shelf_a"]), (c["hp_b"], c["hp_a"])):
        b0, b1, b2, a1, a2 = (f(v) for v in (*b, *a))
        out = np.zeros(len(y), np.float32)
        x1 = x2 = y1 = y2 = f(0)
        for n in range(len(y)):
            x0 = y[n]
            y0 = f(f(f(f(b0 * x0) + f(b1 * x1)) + f(b2 * x2)) - f(a1 * y1)) - f(a2 * y2)
            out[n] = y0
            x2, x1, y2, y1 = x1, x0, y1, y0
        y = out
    return y


def block_means(w, block, hop):
    """z_j over [j hop, j hop + block) for every j with j hop + block <= N, float64; a row with 0 < N < block has ONE block."""
    w = np.asarray(w, np.float64)
    n = len(w)
    if n == 0:
        return np.zeros(0)
    if n < block:
        return np.array([np.mean(w * w)])
    cs = np.concatenate([[0.0], np.cumsum(w * w)])
    j = np.arange((n - block) // hop + 1)
    return (cs[j * hop + block] - cs[j * hop]) / block


def gated(z):
    """-> (L, mask of the blocks past both gates).  L = -inf when none passes the absolute gate."""
    z = np.asarray(z, np.float64)
    with np.errstate(divide="ignore"):
        l = OFFSET + 10 * np.log10(z)
    a = l > ABS_GATE
    if not a.any():
        return -np.inf, a
    rel = OFFSET + 10 * np.log10(z[a].mean()) + REL_GATE
    m = a & (l > rel)
    return OFFSET + 10 * np.log10(z[m].mean()), m


def ungated(z):
    return OFFSET + 10 * np.log10(np.mean(z)) if len(z) else -np.inf


def oracle(x, fs):
    """-> (weighted float64 [N], block mean squares, L)"""
    c, block, hop = coefficients(fs)
    w = weight64(x, c)
    z = block_means(w, block, hop)
    return w, z, gated(z)[0]


def restate_f32(x, fs):
    """The float32 restatement: -> (weighted float32 [N], float32 block mean squares, L as float32)."""
    c, block, hop = coefficients(fs)
    w = weight32(x, c)
    z = block_means(w, block, hop).astype(np.float32)
    return w, z, np.float32(gated(z)[0])


def voiced(n, fs=22050, seed=0, amp=0.3):
    """A voiced test signal: a 140 Hz pulse-like harmonic stack under a slow envelope, plus a little noise; float32 [n]."""
    t = np.arange(n) / float(fs)
    rng = np.random.default_rng(seed)
    s = sum(np.sin(2 * np.pi * 140.0 * k * t + 0.3 * k) / k for k in range(1, 12))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + seed)
    x = amp * (0.5 * env * s + 0.02 * rng.standard_normal(n))
    return x.astype(np.float32)


def tone(n, fs, freq=997.0, amp=1.0):
    return (amp * np.sin(2 * np.pi * freq * np.arange(n) / float(fs))).astype(np.float32)


def gain(L, peak, target, ceiling, max_gain_db):
    """The definition's gain in float64."""
    if np.isnan(target) or not np.isfinite(L):
        return 1.0
    g = min(10.0 ** ((target - float(L)) / 20.0), 10.0 ** (max_gain_db / 20.0))
    return min(g, float(ceiling) / float(peak)) if peak > 0 else g
