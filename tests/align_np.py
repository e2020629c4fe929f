"""Numpy restatement of forced alignment's two host-checkable steps (`mi355tts_glow_align`, csrc/align.h):

* `scores` — Glow-TTS's likelihood of frame j under id t's Gaussian with x_logs = 0 (mean_only voices).  The formula is
  not a line of the reference (its training code is not shipped); include/mi355tts.h states it:
      logp[t][j] = -0.5 M ln(2 pi) - 0.5 sum_c z[c][j]^2 + sum_c x_m[c][t] z[c][j] - 0.5 sum_c x_m[c][t]^2
  in float64, or in float32 with every sum running over c in ascending order and the terms combined as the kernel
  combines them, ((c0 - 0.5 zz) + xz) - 0.5 xx (the kernel uses one fma per term: equal to float32 round-off, not bits).
* `maximum_path` — glow_tts/utils.py:59-96 for one row: lines 73-85 (v = 0; v0 = v shifted by one id with -inf in front;
  max_mask = v1 >= v0, so a tie stays; v = where(x_range <= j, v_max + value[:, j], -inf)) in float32, then the backtrack
  of lines 89-93 from id P - 1 at frame F - 1, returned as the path's row sums (the reference's `attn.sum(-1)`) and the
  final v[P - 1].  Pinned to the reference's own function by tools/make_golden_align.py.
"""
import numpy as np

F32 = np.float32


def scores(x_m: np.ndarray, z: np.ndarray, dtype=np.float64) -> np.ndarray:
    """x_m [M, P], z [M, F] -> logp [P, F]."""
    M = x_m.shape[0]
    if dtype == np.float64:
        x, y = np.asarray(x_m, np.float64), np.asarray(z, np.float64)
        return (-0.5 * M * np.log(2.0 * np.pi) - 0.5 * np.sum(y * y, 0)[None, :]) + x.T @ y - 0.5 * np.sum(x * x, 0)[:, None]
    x, y = np.asarray(x_m, F32), np.asarray(z, F32)
    xz = np.zeros((x.shape[1], y.shape[1]), F32)
    xx = np.zeros(x.shape[1], F32)
    zz = np.zeros(y.shape[1], F32)
    for c in range(M):  # ascending c, float32 throughout
        xz += x[c][:, None] * y[c][None, :]
        xx += x[c] * x[c]
        zz += y[c] * y[c]
    c0 = F32(-0.5 * M * np.log(2.0 * np.pi))
    return ((c0 - F32(0.5) * zz)[None, :] + xz) - (F32(0.5) * xx)[:, None]


def maximum_path(value: np.ndarray):
    """value [P, F] -> (durations int32 [P], score float32, the last v float32 [P])."""
    value = np.asarray(value, F32)
    P, F = value.shape
    assert F >= P >= 1
    direction = np.zeros((P, F), np.int64)
    v = np.zeros(P, F32)
    x_range = np.arange(P)
    neg = F32(-np.inf)
    for j in range(F):
        v0 = np.concatenate([[neg], v[:-1]]).astype(F32)
        stay = v >= v0
        v_max = np.where(stay, v, v0)
        direction[:, j] = stay
        v = np.where(x_range <= j, v_max + value[:, j], neg).astype(F32)
    durations = np.zeros(P, np.int32)
    index = P - 1
    for j in reversed(range(F)):
        durations[index] += 1
        index = index + direction[index, j] - 1
    return durations, F32(v[P - 1]), v
