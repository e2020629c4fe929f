"""TEST INFRASTRUCTURE — a float64 reference of every LAUNCH KIND of the GlowTTS schedule, each with a derived forward-error bound:
what `tests/workload_check.py: check_glow_layers` compares the planes of one call against (`Engine.glow_infer_taps`), launch by
launch, each launch from the planes it actually read.  The vocoder's twin is tests/voc_layers_np.py, whose number formats, `delta_of`
and `bound_f32` are used here, not copied.

Every function takes ONE row's planes [C, L] (the valid columns only; what lies outside a row is zero to every kernel: they mask
columns >= len on load) and the model's weights as the loader hands them to the kernels (f32, unchanged by the packing; the fp16
WaveNet rounds them to fp16), and returns (ref64, delta) per output plane.  The operand roundings are restated from the kernels'
code (csrc/small_kernels.h, gate16.h, coltile.h, conv_mfma.h, wn_f16.h), never from the f32 oracle.

THE RULE, u = 2^-23 (twice the unit round-off: the matrix pipe may chop; used for every elementary f32 operation so that one
constant serves):
  * a contraction of n terms accumulated in f32 in ANY order:  delta = (n + 3) u (sum |w| |x| + |bias| + |res|)   (V.delta_of);
    f32 operands are exact, fp16 operands are restated as rounded;
  * whatever the same launch computes FROM that value carries delta forward by the magnitude of the float64 derivative, to first
    order, plus the f32 evaluation error of the operation itself (k u |value| for k elementary operations):
      - a second contraction: sum |w| delta_in + its own delta;
      - ReLU, max: 1-Lipschitz, delta passes;
      - tanh(a) sigmoid(b): delta_a + delta_b / 4 + E |value|; E for the libm forms (tanhf, expf, 1 / (1 + e), the product):
        the OpenCL full-profile figures the device library documents — tanh 5 ulp, exp 3 ulp (+ 1 for the add, + 2.5 for the
        divide), 0.5 for the product = 12 ulp = E_LIBM = 6 u;
      - LayerNorm (two-pass in every kernel: mean, then the mean of the squared deviations, rsqrtf(var + eps)) by its Jacobian:
        e_mu = mean(dx) + (C + 1) u mean|x|;  e_d = dx + e_mu + u |d|;  e_v = mean(2 |d| e_d) + (C + 3) u v;
        e_r = r (e_v / (2 (v + eps)) + 3 u);  dy = |gamma| (e_d r + |d| e_r) + 3 u (|d r gamma| + |beta|);
        eps = 1e-4 keeps v + eps >= 1e-4 (sigma >= 1e-2), so e_r stays finite on constant columns;
      - softmax then the value sum (all three attention kernels compute s = scale q.k + scale q.Ek, e = expf(s - max),
        p = e / sum e, o = sum p v + sum p Ev): a_j = delta_s_j + u |s_j - max|;
        dp_j = p_j (a_j + sum_k p_k a_k + (P + 8) u)  (the softmax Jacobian; expf 3 ulp, the sum's P - 1 adds, 1 / den, e * inv);
        do = sum_j dp_j (|v_j| [+ |Ev|]) + (P + nrel + 3) u sum_j p_j (|v_j| [+ |Ev|]);
      - the coupling (x1 - m) exp(-logs): (dm + u |x1 - m|) e^-logs + |x1 - m| e^-logs (dlogs + 4 u) + u |value|;
      - the 4 x 4 mix: sum |w| din + 5 u sum |w| |in|;  ActNorm (o - b) s: (do + u |o - b|) |s| + 3 u |value| (s = exp(-logs) is
        computed on the host in float and may be one ulp off the correctly rounded value used here).
  * the acceptance per element is V.bound_f32: |got - ref64| <= delta + 4 * 2^-24 max(1, |ref64|), on every valid column.

wn_f16_kernel is four layers in one launch, and the rule's bound for it is loose by construction: every element of h and of the
gated activations that the carried delta leaves within reach of an fp16 rounding boundary is taken to flip, each in the worst
direction, in every layer.  So its planes meet a second criterion, calibrated on the reference alone as the vocoder walk's flip
share is: the RMS of |plane - ref64| over the launch's planes of a call is at most 4 times that of the float32 restatement
(wn_f16_chain32) — the factor the vocoder's share uses, fixed before any kernel's figure was looked at.  gate_fast's own error E is
measured where the gate conv's weights are zero (the pre-activations are the biases, nothing is carried) over a grid of biases,
4 x the worst value seen (E_GATE_FAST below), and the tests hold that plane to it.

Nothing here is tuned on a kernel's output: `*_chain32` below restate each launch kind in float32, one product at a time into a
float32 accumulator in ANOTHER order, and must pass the same assertion (a bound under which the restatement fails is a wrong
derivation, not a kernel bug)."""
import numpy as np

from tests import voc_layers_np as V

F32, F64 = np.float32, np.float64
U = V.U23
E_LIBM = 6 * U
LN_EPS = 1e-4  # glow_forward.h passes 1e-4f to every LayerNorm (glow_tts/layers.py:22)


def _abs_conv(w, d, dil=1):
    return V.conv_sum(np.abs(np.asarray(w, F64)), np.asarray(d, F64), dil)


# ---- launch kinds ------------------------------------------------------------------------------------------------------------
def embed(emb, ids, H):
    """embed_kernel: x[c, t] = emb[ids[t], c] * sqrtf(H): one f32 product."""
    ref = np.asarray(emb, F32)[np.asarray(ids)].T.astype(F64) * F64(np.sqrt(F32(H)))
    return ref, U * np.abs(ref)


def linear(w, bias, x, dil=1, res=None, relu=False, dx=None):
    """conv_mfma_kernel (linear epilogue) / lin16_kernel: y = act(conv(x) + bias + res), 'same' padding (K - 1) dil / 2, zeros outside
    the row.  `dx`: a bound on what the kernel's operand may differ from `x` by (a value computed earlier in the same launch)."""
    w = np.asarray(w, F32)
    ref = V.conv_sum(w.astype(F64), np.asarray(x, F64), dil) + np.asarray(bias, F64)[:, None]
    if res is not None:
        ref = ref + np.asarray(res, F64)
    mag = V.conv_sum(np.abs(w).astype(F64), np.abs(np.asarray(x, F64)), dil)
    n = int(np.count_nonzero(w.reshape(w.shape[0], -1), axis=1).max())  # (a zero weight's product adds exactly zero: no rounding)
    delta = V.delta_of(n, mag, bias, res)
    if dx is not None:
        delta = delta + _abs_conv(w, dx, dil)
    return (np.maximum(ref, 0.0) if relu else ref), delta


def layernorm(x, gamma, beta, relu=False, dx=None, eps=LN_EPS):
    """LayerNorm over the channels of every column (biased variance, eps inside the root), then ReLU where the prenet has one."""
    x = np.asarray(x, F64)
    C = x.shape[0]
    g, b = np.asarray(gamma, F64)[:, None], np.asarray(beta, F64)[:, None]
    dx = np.zeros_like(x) if dx is None else np.asarray(dx, F64)
    mu = x.mean(axis=0, keepdims=True)
    d = x - mu
    v = (d * d).mean(axis=0, keepdims=True)
    r = 1.0 / np.sqrt(v + eps)
    ref = d * r * g + b
    e_mu = dx.mean(axis=0, keepdims=True) + (C + 1) * U * np.abs(x).mean(axis=0, keepdims=True)
    e_d = dx + e_mu + U * np.abs(d)
    e_v = (2 * np.abs(d) * e_d).mean(axis=0, keepdims=True) + (C + 3) * U * v
    e_r = r * (e_v / (2 * (v + eps)) + 3 * U)
    delta = np.abs(g) * (e_d * r + np.abs(d) * e_r) + 3 * U * (np.abs(d * r * g) + np.abs(b))
    return (np.maximum(ref, 0.0) if relu else ref), delta


def ln_linear(w, bias, x, gamma, beta, ln_relu, dil=1, res=None, relu=False):
    """lin16_kernel.ln: LayerNorm [-> ReLU] of the staged columns, then the conv on them -> (y, delta_y), (normalised x, delta)."""
    xn, dxn = layernorm(x, gamma, beta, ln_relu)
    y, dy = linear(w, bias, xn, dil, res, relu, dx=dxn)
    return (y, dy), (xn, dxn)


def oproj_ln(w, bias, att, x, gamma, beta):
    """oproj_ln_kernel: LayerNorm(x + conv_o(att))."""
    s, ds = linear(w, bias, att, res=x)
    return layernorm(s, gamma, beta, dx=ds)


def ln_proj(x, gamma, beta, pw, pb):
    """layernorm16_kernel with its projection: the normalised column contracted with pw [C] (+ pb) -> [1, L]."""
    xn, dxn = layernorm(x, gamma, beta)
    pw = np.asarray(pw, F64).reshape(-1, 1)
    ref = (pw * xn).sum(axis=0, keepdims=True) + F64(np.asarray(pb).reshape(-1)[0])
    mag = (np.abs(pw) * np.abs(xn)).sum(axis=0, keepdims=True) + abs(F64(np.asarray(pb).reshape(-1)[0]))
    return ref, (np.abs(pw) * dxn).sum(axis=0, keepdims=True) + (x.shape[0] + 3) * U * mag


def gate_value(a, b, da, db, E=E_LIBM):
    ref = np.tanh(a) / (1.0 + np.exp(-b))
    return ref, da + db / 4 + E * np.abs(ref)


def gate(w, bias, x, dil, cond=None, E=E_LIBM):
    """gate16_kernel / conv_mfma_kernel's gate epilogue: tanh(first half) sigmoid(second half) of conv(x) + bias [+ cond]."""
    H = w.shape[0] // 2
    res = None if cond is None else np.repeat(np.asarray(cond, F64)[:, None], x.shape[1], axis=1)
    pre, d = linear(w, bias, x, dil, res)
    return gate_value(pre[:H], pre[H:], d[:H], d[H:], E)


def res_skip(w, bias, acts, h, skip, last):
    """The res_skip 1 x 1 conv: h += rows [0, H), skip (+)= rows [H, 2H); the last layer is all skip.  `skip`: None at layer 0.
    -> (h', delta) or None, (skip', delta)."""
    H = acts.shape[0]
    L = acts.shape[1]
    zero = np.zeros((H, L), F64)
    sk = zero if skip is None else np.asarray(skip, F64)
    res = sk if last else np.concatenate([np.asarray(h, F64), sk], axis=0)
    y, d = linear(w, bias, acts, res=res)
    if last:
        return None, (y, d)
    return (y[:H], d[:H]), (y[H:], d[H:])


def coupling(z1, ml, dml):
    """z1' = (z1 - m) exp(-logs) from m | logs [2 half, L] known to dml."""
    half = ml.shape[0] // 2
    m, logs, dm, dl = ml[:half], ml[half:], dml[:half], dml[half:]
    z1 = np.asarray(z1, F64)
    e = np.exp(-logs)
    ref = (z1 - m) * e
    return ref, (dm + U * np.abs(z1 - m)) * e + np.abs(ref) * (dl + 4 * U) + U * np.abs(ref)


def mix_actnorm(z, dz, winv, an_bias, an_logs, n_split=4):
    """InvConvNear^-1 (the pre-inverted n_split x n_split weight over the channel groups {2k, 2k + 1, half + 2k, half + 2k + 1}:
    glow_tts/layers.py:238-272) and ActNorm^-1 ((o - bias) exp(-logs): layers.py:192-194)."""
    C, T = z.shape
    ns = n_split
    w = np.asarray(winv, F64).reshape(ns, ns)
    grp = lambda x: np.asarray(x, F64).reshape(2, C // ns, ns // 2, T).transpose(0, 2, 1, 3).reshape(ns, C // ns, T)
    ungrp = lambda x: x.reshape(2, ns // 2, C // ns, T).transpose(0, 2, 1, 3).reshape(C, T)
    xs, dxs = grp(z), grp(dz)
    o = ungrp(np.einsum("on,nkt->okt", w, xs))
    do = ungrp(np.einsum("on,nkt->okt", np.abs(w), dxs) + (ns + 1) * U * np.einsum("on,nkt->okt", np.abs(w), np.abs(xs)))
    b = np.asarray(an_bias, F64).reshape(-1, 1)
    s = np.exp(-np.asarray(an_logs, F64).reshape(-1, 1))
    ref = (o - b) * s
    return ref, (do + U * np.abs(o - b)) * s + 3 * U * np.abs(ref)


def coupling_mix(skip, z, w_end, b_end, winv, an_bias, an_logs, ds=None, mix=True):
    """m | logs = end(skip);  z1 = (z1 - m) exp(-logs);  then the mix and ActNorm where the launch has them -> (z', delta)."""
    half = z.shape[0] // 2
    ml, dml = linear(w_end, b_end, skip, dx=ds)
    z1, dz1 = coupling(z[half:], ml, dml)
    zc = np.concatenate([np.asarray(z[:half], F64), z1], axis=0)
    dzc = np.concatenate([np.zeros_like(z1), dz1], axis=0)
    if not mix:
        return zc, dzc
    return mix_actnorm(zc, dzc, winv, an_bias, an_logs)


def glow_tail(acts, skip, z, rs, end, mixw, start):
    """glow_tail_kernel: s = skip + res_skip_last(acts);  m | logs = end(s);  coupling, mix, ActNorm;  h_next = start_next(z0').
    rs / end / start: (w, bias) (`start` None after the last block);  mixw: (winv, an_bias, an_logs) -> (z', dz), (h, dh) or None."""
    s, ds = linear(rs[0], rs[1], acts, res=skip)
    zn, dzn = coupling_mix(s, z, end[0], end[1], *mixw, ds=ds)
    if start is None:
        return (zn, dzn), None
    half = z.shape[0] // 2
    return (zn, dzn), linear(start[0], start[1], zn[:half], dx=dzn[:half])


def attention(qkv, ek, ev, n_heads, window):
    """attention_mfma_kernel (both LDS layouts) and attention_kernel: relative-position self-attention of one row, qkv [3H, P]."""
    qkv = np.asarray(qkv, F64)
    H, P = qkv.shape[0] // 3, qkv.shape[1]
    dk = H // n_heads
    ek, ev = np.asarray(ek, F64).reshape(-1, dk), np.asarray(ev, F64).reshape(-1, dk)
    nrel = 2 * window + 1
    scale = 1.0 / np.sqrt(dk)
    ref, delta = np.zeros((H, P)), np.zeros((H, P))
    i = np.arange(P)
    for h in range(n_heads):
        q, k, v = (qkv[o * H + h * dk : o * H + (h + 1) * dk] for o in range(3))  # [dk, P]
        s, mag = q.T @ k, np.abs(q).T @ np.abs(k)
        rel, relmag = q.T @ ek.T, np.abs(q).T @ np.abs(ek).T  # [P, nrel]
        band = np.zeros((P, P), bool)
        for r in range(nrel):
            j = i + r - window
            ok = (j >= 0) & (j < P)
            s[i[ok], j[ok]] += rel[ok, r]
            mag[i[ok], j[ok]] += relmag[ok, r]
            band[i[ok], j[ok]] = True
        s *= scale
        ds = scale * (dk + 3) * U * mag + 3 * U * np.abs(s)
        mx = s.max(axis=1, keepdims=True)
        e = np.exp(s - mx)
        p = e / e.sum(axis=1, keepdims=True)
        a = ds + U * np.abs(s - mx)
        dp = p * (a + (p * a).sum(axis=1, keepdims=True) + (P + 8) * U)
        o, do = p @ v.T, dp @ np.abs(v).T
        omag = p @ np.abs(v).T
        for r in range(nrel):
            j = i + r - window
            ok = (j >= 0) & (j < P)
            o[ok] += p[i[ok], j[ok]][:, None] * ev[r][None, :]
            do[ok] += dp[i[ok], j[ok]][:, None] * np.abs(ev[r])[None, :]
            omag[ok] += p[i[ok], j[ok]][:, None] * np.abs(ev[r])[None, :]
        ref[h * dk : (h + 1) * dk] = o.T
        delta[h * dk : (h + 1) * dk] = (do + (P + nrel + 3) * U * omag).T
    return ref, delta


def expand(xm, frame_to_id, noise, noise_scale, n_sqz):
    """expand_noise_squeeze_kernel: z[c', t] of squeeze(xm[:, id of frame] + noise * noise_scale): a product and an add."""
    from oracle.glow_tts_np import squeeze

    F = len(frame_to_id)
    a = np.asarray(xm, F64)[:, frame_to_id]
    n = np.asarray(noise, F64)[:, :F] * F64(F32(noise_scale))
    sq = lambda x: squeeze(x, n_sqz)
    return sq(a + n), sq(2 * U * (np.abs(a) + np.abs(n)))


def finalize(z, n_sqz):
    """mel_finalize_kernel's raw plane: the un-squeezed z, a copy."""
    from oracle.glow_tts_np import unsqueeze

    ref = unsqueeze(np.asarray(z, F64), n_sqz)
    return ref, np.zeros_like(ref)


# ---- the fp16 WaveNet: every layer of a block in one launch (wn_f16.h) -----------------------------------------------------------
# E of wn_f16.h's gate_fast (two v_exp_f32, one v_rcp_f32, the +-15 clamp).  No document at hand states those instructions'
# accuracy, so E is measured as the project's rule for that case says: on a model whose last gate convs have zero weights the
# pre-activations are the biases exactly (W.gate_grid_state_dict: tanh arguments to +-18, sigmoid arguments to +-30), and the worst
# |acts - tanh(a) sigmoid(b)| against the float64 FUNCTION over that grid was 1.344e-07 on the device (H = 192; 8.558e-08 at H = 32)
# and 1.712e-07 on the emulator.  E = 4 x the worst of them, an absolute figure (the value is at most 1 in magnitude).
E_GATE_FAST = 4 * 1.712e-07


def wn_gate(a, b, da, db):
    """gate_fast on f32 pre-activations known to (da, db): float64 tanh(a) sigmoid(b), and da |d/da| + db |d/db| + E_GATE_FAST."""
    with np.errstate(over="ignore"):
        t, s = np.tanh(a), 1 / (1 + np.exp(-np.asarray(b, F64)))
    ref = t * s
    return ref, da * s * (1 - t * t) + db * np.abs(t) * s * (1 - s) + E_GATE_FAST


def wn_f16(h, w_in, b_in, w_rs, b_rs):
    """wn_f16_kernel: n layers in one launch (dilation 1: the geometries the kernel takes).  h [H, L] f32 is rounded to fp16 on load
    and again after every layer's `h + res` (f32 add of the fp16 h and the f32 sum), the gated activations once per layer (the
    last layer's leave in f32); weights fp16, biases f32 (the accumulators start from them); the skip sum stays f32.  Walked as V.pair_layer walks a fused
    pair: an intermediate whose float64 value lies within its carried delta of an fp16 rounding boundary may land one spacing off
    (V.requantize), and that widens delta by sum |w| spacing — such elements are not exempted.
    -> (acts of the last layer, delta), (skip sum of layers 0 .. n - 2, delta) or None."""
    n = len(w_in)
    H, L = h.shape
    hv, dh = np.asarray(h, F64), np.zeros((H, L))  # the f32 value about to be rounded to fp16, and what the kernel's may differ by
    skip, dskip = None, None
    for j in range(n):
        h16, slack = V.requantize("f16", hv, dh)
        pre, d = linear(V.fp16(w_in[j]), b_in[j], h16, 1, dx=slack[0])
        g, dg = wn_gate(pre[:H], pre[H:], d[:H], d[H:])
        if j == n - 1:
            return (g, dg), (None if skip is None else (skip, dskip))
        g16, gslack = V.requantize("f16", g, dg)
        rs, drs = linear(V.fp16(w_rs[j]), b_rs[j], g16, dx=gslack[0])
        # h = fp16(h16 + res): the add in f32, then the layer's one rounding (at the top of the loop); skip (+)= the rest in f32
        hv = h16.astype(F64) + rs[:H]
        dh = slack[0] + drs[:H] + U * np.abs(hv)
        if skip is None:
            skip, dskip = rs[H:], drs[H:]
        else:
            skip, dskip = skip + rs[H:], dskip + drs[H:] + U * np.abs(skip + rs[H:])
    raise AssertionError("no layers")


# ---- the float32 restatements: one product at a time into a float32 accumulator, another order ----------------------------------
def embed_chain32(emb, ids, H):
    return (np.asarray(emb, F32)[np.asarray(ids)].T * np.sqrt(F32(H))).astype(F32)


def expand_chain32(xm, frame_to_id, noise, noise_scale, n_sqz):
    """The add before the product's rounding is not the kernel's fused form: noise * scale rounded, then added."""
    from oracle.glow_tts_np import squeeze

    F = len(frame_to_id)
    n = (np.asarray(noise, F32)[:, :F] * F32(noise_scale)).astype(F32)
    return squeeze((np.asarray(xm, F32)[:, frame_to_id] + n).astype(F32), n_sqz)


def linear_chain32(w, bias, x, dil=1, res=None, relu=False):
    acc = V.conv_chain32(np.asarray(w, F32), np.asarray(x, F32), dil) + np.asarray(bias, F32)[:, None]
    if res is not None:
        acc = acc + np.asarray(res, F32)
    return np.maximum(acc, F32(0)) if relu else acc


def _sum_chain32(x):
    acc = np.zeros(x.shape[1:], F32)
    for c in range(x.shape[0] - 1, -1, -1):
        acc = acc + x[c]
    return acc


def layernorm_chain32(x, gamma, beta, relu=False, eps=LN_EPS):
    x = np.asarray(x, F32)
    C = F32(x.shape[0])
    mu = _sum_chain32(x) / C
    d = x - mu[None]
    v = _sum_chain32(d * d) / C
    r = (F32(1) / np.sqrt(v + F32(eps))).astype(F32)
    y = d * r[None] * np.asarray(gamma, F32)[:, None] + np.asarray(beta, F32)[:, None]
    return np.maximum(y, F32(0)) if relu else y.astype(F32)


def gate_chain32(w, bias, x, dil, cond=None):
    H = w.shape[0] // 2
    res = None if cond is None else np.repeat(np.asarray(cond, F32)[:, None], x.shape[1], axis=1)
    pre = linear_chain32(w, bias, x, dil, res)
    return (np.tanh(pre[:H]) * (F32(1) / (F32(1) + np.exp(-pre[H:])))).astype(F32)


def wn_gate32(a, b):
    """gate_fast restated in float32 (exp2 of the rounded argument products)."""
    LOG2E = F32(1.4426950408889634)
    a = np.clip(np.asarray(a, F32), F32(-15), F32(15))
    ea = np.exp2((F32(-2) * LOG2E * a).astype(F32)).astype(F32)
    with np.errstate(over="ignore"):
        eb = np.exp2((-LOG2E * np.asarray(b, F32)).astype(F32)).astype(F32)
        return ((F32(1) - ea) * (F32(1) / ((F32(1) + ea) * (F32(1) + eb)).astype(F32))).astype(F32)


def wn_f16_chain32(h, w_in, b_in, w_rs, b_rs):
    """wn_f16_kernel restated: the same fp16 roundings, every contraction one product at a time into a float32 accumulator in
    another order.  What its planes differ from float64 by is what a correct kernel's may: fp16 roundings of h and of the gated
    activations that flip with the f32 summation order, carried through the layers."""
    n = len(w_in)
    H = h.shape[0]
    h16, skip = V.fp16(h), None
    for j in range(n):
        pre = linear_chain32(V.fp16(w_in[j]), b_in[j], h16)
        g = wn_gate32(pre[:H], pre[H:])
        if j == n - 1:
            return g, skip
        rs = linear_chain32(V.fp16(w_rs[j]), b_rs[j], V.fp16(g))
        h16 = V.fp16(h16 + rs[:H])
        skip = rs[H:] if skip is None else skip + rs[H:]


def coupling_mix_chain32(skip, z, w_end, b_end, winv, an_bias, an_logs, mix=True, n_split=4):
    half = z.shape[0] // 2
    ml = linear_chain32(w_end, b_end, skip)
    z = np.asarray(z, F32)
    z1 = ((z[half:] - ml[:half]) * np.exp(-ml[half:])).astype(F32)
    zc = np.concatenate([z[:half], z1], axis=0)
    return zc if not mix else mix_actnorm_chain32(zc, winv, an_bias, an_logs, n_split)


def mix_actnorm_chain32(zc, winv, an_bias, an_logs, n_split=4):
    """invconv_actnorm_kernel (and the mix of the fused epilogues) restated: the n_split products of a group summed backwards."""
    zc = np.asarray(zc, F32)
    C, T = zc.shape
    ns = n_split
    w = np.asarray(winv, F32).reshape(ns, ns)
    xs = zc.reshape(2, C // ns, ns // 2, T).transpose(0, 2, 1, 3).reshape(ns, C // ns, T)
    o = np.zeros_like(xs)
    for m in range(ns):
        acc = np.zeros(xs.shape[1:], F32)
        for k in range(ns - 1, -1, -1):
            acc = acc + w[m, k] * xs[k]
        o[m] = acc
    o = o.reshape(2, ns // 2, C // ns, T).transpose(0, 2, 1, 3).reshape(C, T)
    s = np.exp(-np.asarray(an_logs, F32).reshape(-1, 1)).astype(F32)
    return ((o - np.asarray(an_bias, F32).reshape(-1, 1)) * s).astype(F32)


def attention_chain32(qkv, ek, ev, n_heads, window):
    qkv = np.asarray(qkv, F32)
    H, P = qkv.shape[0] // 3, qkv.shape[1]
    dk = H // n_heads
    ek, ev = np.asarray(ek, F32).reshape(-1, dk), np.asarray(ev, F32).reshape(-1, dk)
    nrel = 2 * window + 1
    scale = F32(1.0 / np.sqrt(F32(dk)))
    out = np.zeros((H, P), F32)
    i = np.arange(P)
    for h in range(n_heads):
        q, k, v = (qkv[o * H + h * dk : o * H + (h + 1) * dk] for o in range(3))
        s = np.zeros((P, P), F32)
        for c in range(dk - 1, -1, -1):
            s += q[c][:, None] * k[c][None, :]
        rel = np.zeros((P, nrel), F32)
        for c in range(dk - 1, -1, -1):
            rel += q[c][:, None] * ek[:, c][None, :]
        s *= scale
        for r in range(nrel):
            j = i + r - window
            ok = (j >= 0) & (j < P)
            s[i[ok], j[ok]] += rel[ok, r] * scale
        e = np.exp(s - s.max(axis=1, keepdims=True)).astype(F32)
        den = np.zeros(P, F32)
        for j in range(P - 1, -1, -1):
            den += e[:, j]
        p = (e * (F32(1) / den)[:, None]).astype(F32)
        o = np.zeros((P, dk), F32)
        for r in range(nrel):
            j = i + r - window
            ok = (j >= 0) & (j < P)
            o[ok] += p[i[ok], j[ok]][:, None] * ev[r][None, :]
        for j in range(P - 1, -1, -1):
            o += p[:, j][:, None] * v[:, j][None, :]
        out[h * dk : (h + 1) * dk] = o.T
    return out
