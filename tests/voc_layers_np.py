"""TEST INFRASTRUCTURE — a float64 reference of every LAUNCH of the vocoder's reduced-precision schedules, each with a derived
forward-error bound: what `tests/workload_check.py: check_layers` compares the planes of one call against
(`Engine.hifigan_infer_taps`), layer by layer, each layer from the plane its launch actually read.

Whole-network bounds on the fp16 generator cannot go below ~3e-5 RMS: one-ulp fp16 roundings that flip with the f32 summation
order are amplified through 40 layers.  One layer has no such floor: with the operands rounded where the kernel rounds them, the
only freedom a correct kernel has left is the ORDER of its f32 sum, and that is bounded.

Operand roundings, restated from the kernels' code (csrc/conv_f16.h, pair_f16.h, conv_bf16.h, resblock_pair_bf16.h, voc_out.h,
weights_pack.h), not from the f32 oracle:
  * fp16: weights rounded to fp16 to nearest-even; the input is the stored fp16 plane; leaky ReLU on load as packed halves
    `max(x, fp16(x * fp16(0.1f)))`; the MRF average as `fp16(((f32 x + x2) + x3) * (1.0f / nk))`, then the leaky ReLU; bias,
    residual and conv1's output activation in f32 before the ONE rounding to fp16.
  * plain bf16: weights and staged activations rounded to bf16; split bf16 ("bf16x3"): hi = bf16(v), lo = bf16(v - hi) of both,
    products a_hi b_hi + a_hi b_lo + a_lo b_hi (the dropped a_lo b_lo is dropped here too).  Activations are staged from f32:
    `((x + x2) + x3) / nk` and the leaky ReLU in f32.
  * the layers these modes leave on f32 kernels (conv_pre, narrow stages) take f32 operands; conv_post has f32 weights and f32
    activations in every mode (the fp16 one widens its planes, averages with `* (1.0f / nk)` and activates in f32); tanh in float64.

`delta`: the forward error of an f32 sum of n = Cin * K products (exact in f32 for 16-bit operands) in ANY order,
(n + 3) * 2^-23 * (sum |w| |x| + |bias| + |res|); 2^-23 instead of the unit round-off 2^-24 allows for chopped adds in the matrix
pipe, + 3 for the bias, the residual and the activation.  Nothing here is tuned on a kernel's output."""
import numpy as np

F32, F64 = np.float32, np.float64
U23 = 2.0 ** -23
SLOPE = F32(0.1)        # hifi_gan/models.py:13, as the kernels' float argument
SLOPE_POST = F32(0.01)  # F.leaky_relu's default, models.py:198


# ---- number formats ------------------------------------------------------------------------------------------------------
def fp16(x):
    """Round to fp16 (nearest even, one rounding from the array's own type), returned as float32."""
    return np.asarray(x).astype(np.float16).astype(F32)


def bf16(x):
    """float32 -> bf16 to nearest even (weights_pack.h bf16_rne, the device's cast), returned as float32."""
    u = np.ascontiguousarray(x, F32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(F32)


def split_bf16(x):
    hi = bf16(x)
    return hi, bf16(np.asarray(x, F32) - hi)


def ulp_fp16(v):
    """Spacing of fp16 at |v| (subnormal spacing 2^-24 below 2^-14)."""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(v, F64)), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def ulp_bf16(v):
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(v, F64)), 2.0 ** -126)))
    return 2.0 ** (e - 7)


def lrelu_h(x, slope=SLOPE):
    """conv_f16.h lrelu_h8 on fp16 values held as float32: max(v, fp16(v * fp16(slope)))."""
    h = np.asarray(x).astype(np.float16)
    return np.maximum(h, h * np.float16(F32(slope))).astype(F32)


def lrelu32(x, slope=SLOPE):
    x = np.asarray(x, F32)
    return np.where(x > 0, x, x * F32(slope)).astype(F32)


def lrelu64(x, slope=SLOPE):
    return np.where(x > 0, x, x * F64(F32(slope)))


# ---- staging: the planes a launch reads -> the operand its products take ---------------------------------------------------
def stage_f16(planes, in_slope=1.0):
    """conv_f16_mainloop's lstore: fp16 planes (as float32) -> the staged fp16 operand (as float32)."""
    v = np.asarray(planes[0], F32)
    if len(planes) > 1:
        s = v + np.asarray(planes[1], F32)
        if len(planes) > 2:
            s = s + np.asarray(planes[2], F32)
        v = fp16(s * (F32(1.0) / F32(len(planes))))
    return lrelu_h(v, in_slope) if in_slope != 1.0 else v


def stage_f32(planes, in_slope=1.0, by_reciprocal=False):
    """conv_mfma.h / conv_bf16.h / voc_out.h staging: ((x + x2) + x3) / nk and the leaky ReLU in f32 (post_f16_kernel multiplies by
    1.0f / nk instead: `by_reciprocal`)."""
    v = np.asarray(planes[0], F32)
    if len(planes) > 1:
        v = v + np.asarray(planes[1], F32)
        if len(planes) > 2:
            v = v + np.asarray(planes[2], F32)
        v = v * (F32(1.0) / F32(len(planes))) if by_reciprocal else v / F32(len(planes))
    return lrelu32(v, in_slope) if in_slope != 1.0 else v.astype(F32)


def operand_terms(mode, w, x):
    """[(w term, [x terms])]: the products the kernel sums, each exact in f32.  `w`: the f32 weights as loaded; `x`: the staged
    operand (float32)."""
    w, x = np.asarray(w, F32), np.asarray(x, F32)
    if mode == "f16":
        return [(fp16(w), [x])]
    if mode == "bf16":
        return [(bf16(w), [bf16(x)])]
    if mode == "bf16x3":
        (wh, wl), (xh, xl) = split_bf16(w), split_bf16(x)
        return [(wh, [xh, xl]), (wl, [xh])]
    assert mode == "f32", mode
    return [(w, [x])]


# ---- sums ---------------------------------------------------------------------------------------------------------------
def conv_sum(w, x, dil, dtype=F64):
    """sum_{ci, k} w[co, ci, k] x[ci, t + k dil - (K - 1) dil / 2], zeros outside the row: [Cout, L] in `dtype`."""
    Cout, Cin, K = w.shape
    L = x.shape[1]
    pad = (K - 1) * dil // 2
    xp = np.zeros((Cin, L + (K - 1) * dil), dtype)
    xp[:, pad : pad + L] = x
    # one contiguous GEMM: [Cout, K Cin] x [K Cin, L]
    wk = np.ascontiguousarray(w.transpose(0, 2, 1), dtype).reshape(Cout, K * Cin)
    cols = np.concatenate([xp[:, k * dil : k * dil + L] for k in range(K)], axis=0)
    return wk @ cols


def convT_sum(wt, x, u, dtype=F64):
    """ConvTranspose1d(stride u, padding (Ku - u) / 2): y[co, n] = sum_{ci, i} x[ci, i] wt[ci, co, n + pad - i u]: [Cout, L u]."""
    Cin, Cout, Ku = wt.shape
    L = x.shape[1]
    pad = (Ku - u) // 2
    wt = wt.astype(dtype)
    x = x.astype(dtype)
    out = np.zeros((Cout, L * u + Ku), dtype)
    wk = np.ascontiguousarray(wt.transpose(2, 1, 0))  # [Ku][Cout][Cin]
    for k in range(Ku):
        out[:, k : k + L * u : u] += wk[k] @ x
    return out[:, pad : pad + L * u]


def _sums(mode, w, x, op):
    terms = operand_terms(mode, w, x)
    return sum(op(wt, sum(xt.astype(F64) for xt in xs), F64) for wt, xs in terms)


def _magnitude(mode, w, x, op):
    """sum |w| |x| over the products the kernel sums, in float32 times 1.001 (an upper bound of the float64 figure)."""
    terms = operand_terms(mode, w, x)
    return sum(op(np.abs(wt), sum(np.abs(xt) for xt in xs), F32) for wt, xs in terms).astype(F64) * 1.001


def delta_of(n, mag, bias=None, res=None):
    m = mag.copy()
    if bias is not None:
        m += np.abs(np.asarray(bias, F64))[:, None]
    if res is not None:
        m += np.abs(np.asarray(res, F64))
    return (n + 3) * U23 * m


# ---- one function per launch kind: planes in, (ref64, delta) out; every array is ONE row [C, L] ----------------------------
def conv_layer(mode, w, bias, x, dil=1, res=None, out_slope=1.0):
    """A conv launch: y = act_out(bias + res + conv(x staged)).  `x`: the staged operand (stage_f16 / stage_f32)."""
    op = lambda ww, xx, dt: conv_sum(ww, xx, dil, dt)
    ref = _sums(mode, w, x, op) + np.asarray(bias, F64)[:, None]
    if res is not None:
        ref = ref + np.asarray(res, F64)
    delta = delta_of(w.shape[1] * w.shape[2], _magnitude(mode, w, x, op), bias, res)
    return (lrelu64(ref, out_slope) if out_slope != 1.0 else ref), delta


def upsample_layer(mode, wt, bias, x, u):
    """An upsampler launch (polyphase ConvTranspose1d: Ku / u taps per phase)."""
    op = lambda ww, xx, dt: convT_sum(ww, xx, u, dt)
    ref = _sums(mode, wt, x, op) + np.asarray(bias, F64)[:, None]
    delta = delta_of(wt.shape[0] * (wt.shape[2] // u), _magnitude(mode, wt, x, op), bias)
    return ref, delta


def _boundary_distance(t64, r, fmt):
    """Distance of t64 to the nearest rounding boundary of its rounded value r, and the spacing there."""
    if fmt == "f16":
        h = r.astype(np.float16)
        up = np.nextafter(h, np.float16(np.inf)).astype(F64)
        dn = np.nextafter(h, np.float16(-np.inf)).astype(F64)
        r = r.astype(F64)
        spacing = np.maximum(up - r, r - dn)
    else:
        r = r.astype(F64)
        spacing = ulp_bf16(r)
        up, dn = r + spacing, r - spacing  # (one binade below a power of two the lower neighbour is nearer: conservative)
    dist = np.minimum(np.abs(t64 - 0.5 * (r + up)), np.abs(t64 - 0.5 * (r + dn)))
    return dist, spacing


def requantize(mode, t64, delta1):
    """The fused pair's intermediate as the kernel parks it, from its float64 value and the bound delta1 on what the kernel's f32
    accumulator may differ by -> (staged operand float32, {w term index: bound on |kernel's operand - this one|}).
    fp16 / bf16: an element within delta1 of a rounding boundary is unsure and may land one spacing off (ceil(delta1 / spacing)
    spacings where delta1 is larger).  Split bf16: hi + lo carries t to 2^-17."""
    if mode == "f16":
        t = fp16(t64)
        dist, sp = _boundary_distance(t64, t, "f16")
        return t, {0: np.where(dist <= delta1, sp * np.maximum(1.0, np.ceil(delta1 / sp)), 0.0)}
    t32 = t64.astype(F32)
    d1 = delta1 + np.abs(t64) * 2.0 ** -24  # the accumulator's own rounding to f32
    if mode == "f32":
        return t32, {0: d1}
    hi = bf16(t32)
    dist, sp = _boundary_distance(t64, hi, "bf16")
    flip = np.where(dist <= d1, sp * np.maximum(1.0, np.ceil(d1 / sp)), 0.0)
    if mode == "bf16":
        return t32, {0: flip}
    assert mode == "bf16x3", mode
    return t32, {0: d1 + np.abs(t64) * 2.0 ** -17, 1: flip}


def pair_layer(mode, w1, b1, w2, b2, x, x_res, dil):
    """A fused ResBlock1 step without a stored intermediate: y = x + conv2(t), t = lrelu(conv1(x staged, dil)) requantized as the
    kernel parks it.  `x`: the staged operand; `x_res`: the plane itself (the residual).  delta2 grows by sum |w2| * (what an unsure
    element of t may be off by)."""
    t64, delta1 = conv_layer(mode, w1, b1, x, dil, out_slope=SLOPE)
    t, slack = requantize(mode, t64, delta1)
    ref, delta = conv_layer(mode, w2, b2, t, 1, res=x_res)
    terms = operand_terms(mode, w2, t)
    for i, err in slack.items():
        delta = delta + conv_sum(np.abs(terms[i][0]).astype(F64), err, 1)
    return ref, delta


def post_layer(w, bias, x):
    """conv_post + tanh: f32 weights and activations in every mode; `x`: the staged f32 operand.  tanh' <= 1: delta passes."""
    ref, delta = conv_layer("f32", w, bias, x)
    return np.tanh(ref), delta


# ---- acceptance -----------------------------------------------------------------------------------------------------------
def bound_fp16(ref64, delta):
    """Per element of a stored fp16 plane."""
    return 0.5 * ulp_fp16(ref64) + delta


def bound_f32(ref64, delta):
    """Per element of an f32 plane and of the waveform: four f32 ulps on top (tanhf)."""
    return delta + 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref64))


# ---- the float32 restatement: the same layer summed in float32 in another tap order -------------------------------------------
# One product at a time into a float32 accumulator, taps and channels walked backwards, the bias last: n roundings per element, as
# a kernel's accumulator chain has (a BLAS matmul would not do: its blocked sums are several times more accurate than any
# chain, and the share of elements it leaves off the correctly rounded result several times smaller).
def conv_chain32(w, x, dil):
    Cout, Cin, K = w.shape
    L = x.shape[1]
    pad = (K - 1) * dil // 2
    xp = np.zeros((Cin, L + (K - 1) * dil), F32)
    xp[:, pad : pad + L] = x
    w = np.ascontiguousarray(w.transpose(2, 1, 0), F32)  # [K][Cin][Cout]
    acc, tmp = np.zeros((Cout, L), F32), np.empty((Cout, L), F32)
    for k in range(K - 1, -1, -1):
        for ci in range(Cin - 1, -1, -1):
            np.multiply(w[k, ci][:, None], xp[ci, k * dil : k * dil + L][None, :], out=tmp)
            acc += tmp
    return acc


def convT_chain32(wt, x, u):
    Cin, Cout, Ku = wt.shape
    L = x.shape[1]
    pad = (Ku - u) // 2
    wt, x = np.asarray(wt, F32), np.asarray(x, F32)
    out = np.zeros((Cout, L * u + Ku), F32)
    for k in range(Ku - 1, -1, -1):
        for ci in range(Cin - 1, -1, -1):
            out[:, k : k + L * u : u] += wt[ci, :, k][:, None] * x[ci][None, :]
    return out[:, pad : pad + L * u]


def conv_layer32(mode, w, bias, x, dil=1, res=None, out_slope=1.0, transposed_u=None):
    op = (lambda ww, xx: convT_chain32(ww, xx, transposed_u)) if transposed_u else (lambda ww, xx: conv_chain32(ww, xx, dil))
    terms = operand_terms(mode, w, x)
    acc = None
    for wt, xs in reversed(terms):
        for xt in xs:
            y = op(wt, xt)
            acc = y if acc is None else acc + y
    acc = acc + np.asarray(bias, F32)[:, None]
    if res is not None:
        acc = acc + np.asarray(res, F32)
    return lrelu32(acc, out_slope) if out_slope != 1.0 else acc


def pair_layer32(mode, w1, b1, w2, b2, x, x_res, dil):
    t = conv_layer32(mode, w1, b1, x, dil, out_slope=SLOPE)
    return conv_layer32(mode, w2, b2, fp16(t) if mode == "f16" else t, 1, res=x_res)
