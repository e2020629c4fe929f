"""Whole-workload checks against the CPU oracle, shared by the device tests (tests/test_gpu_config3.py) and their emulator
twin (tests/test_sharding.py): frame counts of a work list, the bench form of BASELINE config 3 under load and alone, the
micro-batched shard, mels and waveforms at the lengths where the vocoder's tile choices and tile seams move.

Which kernels a vocoder call gets depends on the frame count, the batch and the load (csrc/host_launch.h: plan_conv,
promote_group_plans, plan_pair, run_group), so the lengths compared here are chosen from the launch-rule transitions the
library itself shows (`kernel_signature`) and from where a stage's last tile is full, one column or narrower than the halo
(`edge_frames`).  The acoustic model has the same kind of rules along the id count, the frame count, the batch and the precision
(csrc/glow_forward.h: launch_attention; host_launch.h: run_gate16, run_lin16): "the GlowTTS sweep" below, shared by
tests/test_gpu_glow_sweep.py and tests/test_emu_glow_sweep.py."""
import threading
import time
import zlib

import numpy as np

from oracle import audio_np, glow_tts_np, hifi_gan_np

F32 = np.float32

# ---- frame counts ------------------------------------------------------------------------------------------------
# The device computes w = exp(logw) * length_scale in f32 from its own logw: an utterance with a duration this close (relative)
# to an integer may legitimately ceil the other way.  2e-5 is ~20x the logw round-off expected of an f32 encoder.
CEIL_MARGIN = 2e-5
MAX_EXEMPT = 16


def oracle_frames(gsd, hp, ids, length_scale):
    """(F, margin): the oracle's frame count and the relative distance of the closest duration to a ceil boundary,
    min |w - round(w)| / max(w, 1) over the phonemes (w = exp(logw) * length_scale in f32)."""
    _, logw = glow_tts_np.text_encoder(gsd, np.asarray(ids, np.int64), hp)
    _, F, _ = glow_tts_np.durations_to_frames(logw, length_scale, hp.n_sqz)
    w = np.exp(logw.astype(F32)) * F32(length_scale)
    margin = float(np.min(np.abs(w - np.round(w)) / np.maximum(w, F32(1.0))))
    return int(F), margin


def check_frames(frames, ref, n_sqz=2, label=""):
    """`frames[i]` (device) against `ref[i]` = oracle_frames(...): equal wherever the margin is >= CEIL_MARGIN; below it
    |dF| <= n_sqz and the utterance is exempt from value checks (at most MAX_EXEMPT of a list).  Returns the exempt indices."""
    exempt = set()
    matched = []
    for i, (f, (F, margin)) in enumerate(zip(frames, ref)):
        f = int(f)
        if margin < CEIL_MARGIN:
            exempt.add(i)
            print(f"{label} frames: utterance {i} exempt (ceil margin {margin:.2e}): device {f}, oracle {F}")
            assert abs(f - F) <= n_sqz, (i, f, F, margin)
        else:
            assert f == F, (i, f, F, margin)
        if f == F:
            matched.append(margin)
    assert len(exempt) <= MAX_EXEMPT, sorted(exempt)
    print(f"{label} frames: {len(frames)} utterances, {len(exempt)} exempt, smallest margin still matched {min(matched):.2e}")
    return exempt


# ---- waveforms -----------------------------------------------------------------------------------------------------------
# f32: the RMS bar of test_vocoder_alone_on_reference_mel; int16 within 1 LSB of the reference's conversion of the oracle's
# waveform; per sample: RMS hides a one-column seam error, so the largest |error| of any sample is bounded too, at 4x the largest
# measured on the device (MI355X, tests/test_gpu_config3.py).  The error scales with the waveform, so there are two figures:
# config 3 end to end (oracle mel -> oracle vocoder; 24 rows, F = 390 ... 936): 3.7e-6; the vocoder sweep's synthetic mels
# (quiet waveforms; 'high' / 'medium' / 'low', F = 1 ... 1100, batch 1 and ragged batches): 2.1e-7.
MAX_ABS_END_TO_END = 3.7e-6
MAX_ABS_SWEEP = 2.1e-7
F32_WAVE = dict(rms=2e-5, max=4 * MAX_ABS_END_TO_END, lsb=1)
F32_SWEEP = dict(rms=2e-5, max=4 * MAX_ABS_SWEEP, lsb=1)


def f16_wave_bounds(vhp):
    """The bar of test_f16_mode_against_the_reference for every committed golden of this vocoder geometry: the largest error
    the reference's own generator under .half() made against its f32 waveform (RMS; max and int16 x 1.5, as there)."""
    from tests.golden_util import CASES, load_case

    got = [c for c in (load_case(n) for n in CASES) if "ref_half_rms" in c and c["voc_hp"] == vhp]
    assert got, vhp
    return dict(rms=max(float(c["ref_half_rms"]) for c in got), max=1.5 * max(float(c["ref_half_max"]) for c in got),
                lsb=1.5 * max(int(c["ref_half_i16"]) for c in got))


def compare_wave(wav, i16, ref, n, bounds=F32_WAVE, label=""):
    """One row: samples [0, n) against the oracle's float waveform `ref` (RMS, max |error|, int16 against the reference's
    conversion of `ref`), the rest of the row exactly 0.  Prints and returns the measured values."""
    wav, i16 = np.asarray(wav), np.asarray(i16)
    assert ref.shape[0] == n and wav.shape[0] >= n and i16.shape[0] == wav.shape[0], (ref.shape, n, wav.shape, i16.shape)
    d = wav[:n].astype(np.float64) - ref.astype(np.float64)
    rms = float(np.sqrt(np.mean(d ** 2)))
    mx = float(np.abs(d).max())
    where = int(np.abs(d).argmax())
    lsb = int(np.abs(i16[:n].astype(np.int32) - audio_np.audio_float_to_int16(ref).astype(np.int32)).max())
    print(f"{label}: n {n} rms {rms:.2e} max {mx:.2e} (sample {where}) int16 {lsb} LSB")
    assert np.all(wav[n:] == 0) and np.all(i16[n:] == 0), label
    assert rms <= bounds["rms"] and mx <= bounds["max"] and lsb <= bounds["lsb"], (label, rms, mx, where, lsb, bounds)
    return rms, mx, lsb


# ---- which kernels ran ---------------------------------------------------------------------------------------------------
def kernel_signature(eng):
    """The `kernel_counts()` names that launched since the last `profile_reset()`."""
    return frozenset(k for k, c in eng.kernel_counts().items() if c > 0)


# The column widths of the vocoder's tiles, one entry per kernel family: (label, precision, stage rule, width of the last tile
# as a function of (C, K)).  Stage rules (ResBlock1 unless named): "conv" = the grouped / single ResBlock convs (C >= 128 in f32,
# every stage of ResBlock2), "pair" = the fused conv1 + conv2 steps (32 / 64 channels), "mrf" = the one-launch narrow stages
# (<= 16 channels), "post" = conv_post on the waveform, "f16conv" / "f16pair" = the fp16 generator's grouped convs and pairs.
TILE_WIDTHS = (
    # conv_mfma.h T_T = WN * NB * 32 of plan_conv's shapes: TILE_TINY 32, TILE_SMALL and TILE_M128 64, TILE_W128 (and
    # rb_group_kernel<11, 7, 3, 4>) 128, TILE_NB2 256
    ("conv_mfma T_T=32", "f32", "conv", lambda C, K: 32),
    ("conv_mfma T_T=64", "f32", "conv", lambda C, K: 64),
    ("conv_mfma T_T=128", "f32", "conv", lambda C, K: 128),
    ("conv_mfma T_T=256", "f32", "conv", lambda C, K: 256),
    # rb_pair.h / resblock_pair.h T2 = T1 - (K - 1), T1 = 128 * NB (host_launch.h plan_pair: NB = 1 at 64 channels, 2 at 32)
    ("pair T2", "f32", "pair", lambda C, K: 128 * (2 if C == 32 else 1) - (K - 1)),
    # mrf_small.h / mrf8: run_mrf_small's T = 256
    ("mrf_small T", "f32", "mrf", lambda C, K: 256),
    # voc_out.h POST_TW
    ("POST_TW", "f32", "post", lambda C, K: 256),
    # hifigan_f16.h h_tile_dims: HT_WIDE 128 columns (128+ rows or Cin > 64), HT_MID / HT_SLIM 256
    ("f16 h_tile_dims", "f16", "f16conv", lambda C, K: 128 if C > 64 else 256),
    # pair_f16.h TO = 32 * NB * WN - (K - 1) of h_pair_tile's shape: 128 columns at C = 128, 256 at C <= 64
    ("pair_f16 TO", "f16", "f16pair", lambda C, K: (128 if C > 64 else 256) - (K - 1)),
    # conv_f16.h HPOST_TW
    ("HPOST_TW", "f16", "post", lambda C, K: 256),
    # "bf16" = both reduced modes of the f32 schedule (split bf16 and plain bf16: the same tiles, another operand split).
    # host_launch.h plan_conv: BF_A / BF_K / BF_C / BF_D are 128 columns wide (BF_B, 32 columns, only under MI355TTS_BF_K=0)
    ("conv_bf16 128 columns", "bf16", "bf16conv", lambda C, K: 128),
    # resblock_pair_bf16.h T2 = T1 - (K - 1), T1 = 32 * NB16 * WN16 = 256 (host_launch.h PAIR_TILES)
    ("pair_bf16 T2", "bf16", "pair", lambda C, K: 256 - (K - 1)),
    # the narrow stages and conv_post stay on their f32 kernels in these modes
    ("mrf_small T", "bf16", "mrf", lambda C, K: 256),
    ("POST_TW", "bf16", "post", lambda C, K: 256),
)


def vocoder_tiles(hp, precision="f32"):
    """The (label, stage, width, halo) tiles a vocoder's kernels use in `precision`; halo = the widest per-side input halo of
    the conv the tile runs first ((K - 1) * dilation / 2)."""
    out = []
    rb1 = hp.resblock == "1"
    last = len(hp.upsample_rates) - 1
    for i in range(len(hp.upsample_rates)):
        C = hp.stage_channels(i)
        chains = list(zip(hp.resblock_kernel_sizes, hp.resblock_dilation_sizes))
        halo_all = max((k - 1) * max(d) // 2 for k, d in chains)
        for label, prec, rule, width in TILE_WIDTHS:
            if prec != precision:
                continue
            if rule == "post":
                if i == last:
                    out.append((label, i, width(C, 7), 3))
                continue
            if rule in ("pair", "f16pair"):
                ok = rb1 and (C in (32, 64) if rule == "pair" else C <= 128)
                if ok:
                    for k, d in chains:
                        out.append((f"{label} K={k}", i, width(C, k), (k - 1) * max(d) // 2))
                continue
            ok = {"conv": (C >= 128) if rb1 else True, "bf16conv": (C >= 128) if rb1 else True, "mrf": rb1 and C <= 16,
                  "f16conv": (C > 128) if rb1 else True}[rule]
            if ok:
                out.append((label, i, width(C, 3), halo_all))
    return sorted(set(out), key=lambda t: (t[1], t[2], t[0]))


def vocoder_axis(hp):
    """The axis length function of the vocoder's tiles: stage i runs on F * prod(upsample_rates[: i + 1]) columns."""
    return lambda F, stage: F * int(np.prod(hp.upsample_rates[: stage + 1]))


def edge_frames(hp, tiles, lo, hi, length=None):
    """{F: [(label, stage, width, kind)]} for every F in [lo, hi] at which the last tile of some entry of `tiles` (vocoder_tiles,
    glow_tiles) is exactly full ("full"), one column wide ("one") or narrower than that kernel's halo ("halo").
    `length(F, stage)`: the columns the entry's kernel runs on at the scanned length F (default: the vocoder's stage length);
    None = the kernel does not run at this F."""
    length = length or vocoder_axis(hp)
    out = {}
    for F in range(max(1, lo), hi + 1):
        hits = []
        for label, stage, width, halo in tiles:
            L = length(F, stage)
            if L is None:
                continue
            r = L % width
            kind = "full" if r == 0 else "one" if r == 1 else "halo" if r < halo else None
            if kind:
                hits.append((label, stage, width, kind))
        if hits:
            out[F] = hits
    return out


def cover_edges(edges, cap=None, have=()):
    """A small set of frame counts that together hit every (stage, width, kind) edge in `edges` (edge_frames): greedy, the F
    that hits the most edges not yet hit, the shorter F on a tie (the oracle's cost grows with F).  `have`: lengths compared
    anyway: the edges they hit need no other length.  At most `cap` lengths."""
    left = {(s, w, k) for hits in edges.values() for (_, s, w, k) in hits}
    for F in have:
        left -= {(s, w, k) for (_, s, w, k) in edges.get(F, ())}
    chosen = []
    while left and (cap is None or len(chosen) < cap):
        F = max(edges, key=lambda f: (len(left & {(s, w, k) for (_, s, w, k) in edges[f]}), -f))
        gain = left & {(s, w, k) for (_, s, w, k) in edges[F]}
        if not gain:
            break
        chosen.append(F)
        left -= gain
    return sorted(chosen)


# ---- the vocoder sweep ---------------------------------------------------------------------------------------------------
def sweep_mel(num_mels, F):
    """The synthetic vocoder input of frame count F (the launch-count tests' 0.57 + 0.06 randn), seeded by F."""
    return (0.57 + 0.06 * np.random.default_rng(1000 + F).standard_normal((num_mels, F))).astype(F32)


def scan_signatures(eng, v, num_mels, lo, hi, label=""):
    """{F: kernel_signature} of a lone batch-1 call at every F in [lo, hi]; prints each signature's range."""
    sigs = {}
    for F in range(lo, hi + 1):
        mb = eng.mel_from_numpy(sweep_mel(num_mels, F))
        eng.profile_reset()
        eng.hifigan_infer(v, mb, want_float=False)
        sigs[F] = kernel_signature(eng)
        mb.free()
    start = lo
    for F in range(lo, hi + 1):
        if F == hi or sigs[F + 1] != sigs[F]:
            print(f"{label} scan: F {start}..{F}: {sorted(sigs[F])}")
            start = F + 1
    return sigs


def choose_lengths(sigs, edges=(), cap=12):
    """One length per signature (its shortest F), then the transitions (F and F + 1 where the signature changes) by increasing
    F until `cap`; then every F of `edges` (cover_edges: a handful)."""
    Fs = sorted(sigs)
    first = {}
    for F in Fs:
        first.setdefault(sigs[F], F)
    chosen = sorted(first.values())
    trans = [f for F in Fs[:-1] if sigs[F] != sigs[F + 1] for f in (F, F + 1)]
    for f in trans:
        if len(chosen) >= cap:
            break
        if f not in chosen:
            chosen.append(f)
    assert len(first) <= cap, "more kernel signatures than the cap: raise the cap"
    return sorted(set(chosen) | set(edges))


class OracleWaves:
    """The oracle's waveform per (vocoder, frame count) of the sweep's mels — computed once, shared by the f32 and the fp16
    comparison of the same mel."""

    def __init__(self):
        self._c = {}
        self.seconds = 0.0

    def __call__(self, vsd, vhp, key, F):
        if (key, F) not in self._c:
            t = time.perf_counter()
            self._c[(key, F)] = hifi_gan_np.hifigan_infer(vsd, vhp, sweep_mel(vhp.num_mels, F))
            self.seconds += time.perf_counter() - t
        return self._c[(key, F)]


def check_lengths(eng, v, vsd, vhp, Fs, oracle, key, bounds=F32_SWEEP, label="", batch=8, solo_rms=1e-5):
    """Each F in `Fs` as a lone batch-1 call against the oracle, then one ragged padded batch of up to `batch` of them: every
    row against the oracle and within RMS `solo_rms` of its batch-1 result (1e-5 in f32, as config 4).  Returns the kernel
    names that ran."""
    hop = vhp.hop
    ran = set()
    solo = {}
    for F in Fs:
        mb = eng.mel_from_numpy(sweep_mel(vhp.num_mels, F))
        eng.profile_reset()
        wav, i16 = eng.hifigan_infer(v, mb)
        sig = kernel_signature(eng)
        ran |= sig
        mb.free()
        solo[F] = wav[0]
        compare_wave(wav[0], i16[0], oracle(vsd, vhp, key, F), F * hop, bounds, f"{label} F={F} B=1")
    rows = sorted(Fs, key=lambda f: (-f, f))[:batch]  # the batch keeps the longest: the most tiles per row
    rows = rows[::2] + rows[1::2][::-1]  # ragged, not sorted
    Fmax = max(rows)
    mel = np.zeros((len(rows), vhp.num_mels, Fmax), F32)
    for b, F in enumerate(rows):
        mel[b, :, :F] = sweep_mel(vhp.num_mels, F)
    mb = eng.mel_from_numpy(mel, np.array(rows, np.int32))
    eng.profile_reset()
    wav, i16 = eng.hifigan_infer(v, mb)
    ran |= kernel_signature(eng)
    mb.free()
    for b, F in enumerate(rows):
        n = F * hop
        compare_wave(wav[b], i16[b], oracle(vsd, vhp, key, F), n, bounds, f"{label} F={F} row {b} of B={len(rows)}")
        d = float(np.sqrt(np.mean((wav[b, :n].astype(np.float64) - solo[F][:n]) ** 2)))
        assert d <= solo_rms, (label, F, d)
    return ran


# ---- the GlowTTS sweep --------------------------------------------------------------------------------------------------
# Which kernels a GlowTTS call gets depends on the id count P, the frame count, the batch and the precision (csrc/glow_forward.h:
# launch_attention; csrc/host_launch.h: run_gate16, run_lin16, plan_conv).  The column widths of its tiles, one entry per kernel
# family: (label, precision ("any" = both), axis, width, per-side halo as a function of the hparams, (lo, hi) = the axis lengths
# of a lone call at which the kernel runs, None = no bound).  Axes: "P" = phoneme ids (the encoder), "F2" = F / n_sqz (the
# decoder's columns), "F" = mel frames.
GLOW_TILE_WIDTHS = (
    # small_kernels.h attention_mfma_kernel: i0 = blockIdx.x * 32 query rows, nkb = (P + 31) / 32 key blocks; the relative-position
    # band reaches window_size keys across a seam.  glow_forward.h launch_attention: P <= ATTM_MAXP = 768
    ("attention_mfma 32 rows / 32 keys", "any", "P", 32, lambda hp: hp.window_size, (1, 768)),
    # small_kernels.h attention_mfma_kernel v_fetch / v_park: V staged in chunks of 64 keys
    ("attention_mfma V chunk", "any", "P", 64, lambda hp: 0, (1, 768)),
    # small_kernels.h ATT_ROWS = 4 query rows per workgroup, ATT_JCH = 64 keys per staged V chunk (attention_kernel, P > ATTM_MAXP)
    ("attention ATT_ROWS", "any", "P", 4, lambda hp: 0, (769, None)),
    ("attention ATT_JCH", "any", "P", 64, lambda hp: 0, (769, None)),
    # host_launch.h run_lin16: TC = 16 * nblk, nblk = 2 below 16 channel groups (Cin 192 / 256: prenet k = 5, FFN conv_1, duration
    # predictor k = 3, the 1 x 1 convs), 1 from 16 groups (the Cin = 768 FFN conv_2)
    ("lin16 TC=32", "any", "P", 32, lambda hp: max(hp.prenet_kernel_size, hp.kernel_size) // 2, None),
    ("lin16 TC=16", "any", "P", 16, lambda hp: hp.kernel_size // 2, None),
    # coltile.h COL_T = 16 (oproj_ln_kernel)
    ("oproj_ln COL_T", "any", "P", 16, lambda hp: 0, None),
    # glow_forward.h launch_layernorm: layernorm16_kernel's grid (n_max + 15) / 16
    ("layernorm16", "any", "P", 16, lambda hp: 0, None),
    # glow_forward.h glow_encoder: embed_kernel's grid (Pmax + 63) / 64
    ("embed", "any", "P", 64, lambda hp: 0, None),
    # gate16.h gate16_kernel: 32 columns per workgroup (host_launch.h run_gate16: gx = (n_max + 31) / 32), halo of the k = 5 conv
    ("gate16 32 columns", "f32", "F2", 32, lambda hp: (hp.kernel_size_dec - 1) // 2, None),
    # host_launch.h run_lin16 on the res_skip 1 x 1 convs: TC = 32
    ("lin16 TC=32", "any", "F2", 32, lambda hp: 0, None),
    # coltile.h COL_T = 16 (glow_tail_kernel)
    ("glow_tail COL_T", "any", "F2", 16, lambda hp: 0, None),
    # wn_f16.h WN_W = 64 columns computed per workgroup, glow_forward.h run_wn_f16: margin = (kernel_size_dec - 1) / 2 * n_block_layers
    # per side recomputed, WN_W - 2 * margin written (48 columns, halo 8 at the released shape)
    ("wn_f16 WN_W - 2 margin", "f16", "F2", lambda hp: 64 - (hp.kernel_size_dec - 1) * hp.n_block_layers,
     lambda hp: (hp.kernel_size_dec - 1) // 2 * hp.n_block_layers, None),
    # glow_forward.h glow_decoder: expand_noise_squeeze_kernel's grid (Fmax + 255) / 256, mel_finalize_kernel's (Fld + 255) / 256
    ("expand_noise_squeeze / mel_finalize", "any", "F", 256, lambda hp: 0, None),
) + tuple(
    # conv_mfma.h T_T = WN * NB * 32 of plan_conv's shapes (TILE_TINY 32, TILE_SMALL / TILE_M128 64, TILE_W128 128, TILE_NB2 256):
    # the generic tile of whatever the 16-row kernels do not take, on both axes
    (f"conv_mfma T_T={w}", "any", axis, w, (lambda hp: max(hp.prenet_kernel_size, hp.kernel_size) // 2) if axis == "P" else
     (lambda hp: (hp.kernel_size_dec - 1) // 2), None)
    for axis in ("P", "F2") for w in (32, 64, 128, 256)
)


def glow_tiles(hp, precision="f32"):
    """The (label, stage, width, halo) tiles of the GlowTTS kernels in `precision`, for edge_frames / cover_edges.  stage =
    (axis, lo, hi): the axis the tile runs along and the lengths at which its kernel runs (glow_axis reads it)."""
    out = []
    for label, prec, axis, width, halo, span in GLOW_TILE_WIDTHS:
        if prec not in ("any", precision):
            continue
        lo, hi = span or (None, None)
        out.append((label, (axis, lo, hi), width(hp) if callable(width) else width, halo(hp)))
    return sorted(set(out), key=lambda t: (t[1][0], t[2], t[0], str(t[1])))


def glow_axis(hp, scanned):
    """The axis length function of a GlowTTS scan along `scanned`: "P" (P ids of 2 frames each: only the encoder's tiles count;
    the decoder has the F2 scan) or "F2" (F = n_sqz * F2)."""
    def length(n, stage):
        axis, lo, hi = stage
        L = {"P": {"P": n}, "F2": {"F2": n, "F": n * hp.n_sqz}}[scanned].get(axis)
        if L is None or (lo is not None and L < lo) or (hi is not None and L > hi):
            return None
        return L
    return length


def glow_ids(hp, P, gsd=None, length_scale=1.0, tries=3):
    """Ids seeded by P (seed 1000 + P); with `gsd`, the first of at most `tries` seeds whose oracle durations at `length_scale`
    clear CEIL_MARGIN (chosen on the CPU from the oracle, never from the device)."""
    from larynx_amd import synthetic

    for t in range(tries):
        ids = synthetic.synthetic_phoneme_ids(np.random.default_rng(1000 + P + t), P, hp.num_symbols)
        if gsd is None or oracle_frames(gsd, hp, ids, length_scale)[1] >= CEIL_MARGIN:
            return ids
    raise AssertionError(f"no ids of length {P} clear the ceil margin in {tries} seeds")


def glow_noise(hp, F, key):
    """The standard-normal noise a sweep call injects, seeded by the compared length; 5 columns wider than the mel: its row stride
    is not the mel's."""
    return np.random.default_rng(2000 + key).standard_normal((hp.mel_channels, F + 5)).astype(F32)


def forced_durations(hp, F2, P=8, odd_sum=False):
    """P forced durations summing to n_sqz * F2 (+ 1 with `odd_sum`: the frame count is truncated to a multiple of n_sqz), split
    unevenly, at least one of them odd wherever the sum allows it."""
    total = hp.n_sqz * F2
    w = np.array([1, 3, 2, 5, 1, 4, 2, 6][:P] + [1] * max(0, P - 8), np.int64)
    d = total * w // int(w.sum())
    d[3 % P] += total - int(d.sum())
    if not np.any(d % 2) and P >= 2:
        i = int(np.argmax(d))
        d[i] -= 1
        d[(i + 1) % P] += 1
    if odd_sum:
        d[P - 1] += 1
    assert int(d.sum()) == total + int(odd_sum) and np.all(d >= 0)
    return d.astype(np.int32)


class GlowCase:
    """One compared call: `n` = the scanned length (P or F2), its ids and forced durations, the frame count they give."""

    def __init__(self, hp, axis, n, odd_sum=False, frames_for=None):
        """`frames_for` (axis "P"): only the first so many ids get their 2 frames, the rest none — a long encoder pass in front of
        a short decoder pass."""
        from tests.test_emu_prosody import attn_durations

        self.axis, self.n, self.odd = axis, int(n), bool(odd_sum)
        self.key = self.n + (100000 if odd_sum else 0) + (200000 if axis == "F2" else 0) + (400000 if frames_for is not None else 0)
        self.ids = glow_ids(hp, self.n if axis == "P" else 8)
        self.d = np.full(self.n, 2, np.int32) if axis == "P" else forced_durations(hp, self.n, 8, odd_sum)
        if frames_for is not None:
            assert axis == "P" and not odd_sum
            self.d[frames_for:] = 0
        self.exp_d, self.F = attn_durations(self.d, hp.n_sqz)  # what the call reports: the last id truncated with the frame count
        self._hp, self._noise = hp, None

    @property
    def noise(self):
        if self._noise is None:
            self._noise = glow_noise(self._hp, self.F, self.key)
        return self._noise

    def __repr__(self):
        return f"{self.axis}={self.n}{'+1 frame' if self.odd else ''}"


def glow_call_signature(eng, g, case):
    """kernel_signature of the case's lone call (the device's own noise: no value is read)."""
    eng.profile_reset()
    eng.glow_infer(g, case.ids, 0.667, 1.0, seed=case.key, durations=case.d).free()
    return kernel_signature(eng)


def scan_glow_signatures(eng, g, hp, axis, lo, hi, label="", only=None):
    """{n: kernel_signature} of a lone call at every n in [lo, hi] (`only`: at these n) along `axis`: "P" = n ids forced to 2
    frames each, "F2" = 8 ids with forced durations summing to n_sqz * n (forced_durations); prints each signature's range."""
    ns = sorted(only) if only is not None else list(range(lo, hi + 1))
    sigs = {n: glow_call_signature(eng, g, GlowCase(hp, axis, n)) for n in ns}
    start = ns[0]
    for a, b in zip(ns, ns[1:] + [None]):
        if b is None or sigs[b] != sigs[a]:
            print(f"{label} scan: {axis} {start}..{a}: {sorted(sigs[a])}")
            start = b
    return sigs


class GlowOracle:
    """The oracle's raw mel per compared case (text encoder -> expansion by the forced durations -> + noise -> the flows in
    reverse: tests/test_emu_prosody.oracle_with_durations), computed once per (weights, case)."""

    def __init__(self):
        self._c = {}
        self.seconds = 0.0

    def __call__(self, gsd, hp, key, case):
        from tests.test_emu_prosody import oracle_with_durations

        k = (key, case.axis, case.key)
        if k not in self._c:
            t = time.perf_counter()
            self._c[k] = oracle_with_durations(gsd, hp, case.ids, case.d, case.noise, 0.667)
            self.seconds += time.perf_counter() - t
        return self._c[k]


def mel_plane(eng, mel):
    """The whole raw plane [B, M, ld] of a mel, the padding columns max_frames .. ld included (`numpy` stops at max_frames)."""
    ptr, ld = mel.plane("raw")
    full = eng.mel_from_device(ptr, [ld] * mel.batch, mel.channels, ld)
    out = full.numpy("raw")
    full.free()
    return out


F32_MEL = dict(max=5e-5, rms=None)  # the project's bar: test_golden_reference_parity, check_mels


def f16_mel_bounds(voice="ljspeech"):
    """The bar of test_f16_acoustic_mode_against_the_reference over the committed goldens of `voice`: the largest deviation of the
    reference's own decoder under .half() from its f32 mel (tests/golden/glow_half_reference.json)."""
    from tests.golden_util import load_glow_half_reference

    got = [v for k, v in load_glow_half_reference().items() if k.startswith(voice)]
    assert got, voice
    return dict(max=max(float(v["dec_half_max"]) for v in got), rms=max(float(v["dec_half_rms"]) for v in got))


def compare_mel(raw, ref, F, bounds, label=""):
    """One row of a raw plane [M, ld]: columns [0, F) against the oracle's mel (max |error| over every element, and RMS where the
    bound has one), the rest of the row exactly 0.  Prints the worst element's column; returns the max |error|."""
    assert ref.shape[1] == F and raw.shape[0] == ref.shape[0] and raw.shape[1] >= F, (label, ref.shape, raw.shape, F)
    assert np.all(raw[:, F:] == 0), (label, "columns past the row's frames are not 0", np.argwhere(raw[:, F:] != 0)[:4].tolist())
    if F == 0:
        return 0.0
    d = np.abs(raw[:, :F].astype(np.float64) - ref)
    mx, rms = float(d.max()), float(np.sqrt(np.mean(d ** 2)))
    ch, col = np.unravel_index(int(d.argmax()), d.shape)
    print(f"{label}: F {F} max-abs {mx:.2e} (channel {ch}, column {col} of {F}) rms {rms:.2e}")
    assert mx <= bounds["max"], (label, mx, int(ch), int(col), bounds)
    assert bounds["rms"] is None or rms <= bounds["rms"], (label, rms, bounds)
    return mx


def check_glow_rows(eng, g, gsd, hp, cases, oracle, key, bounds=F32_MEL, label="", solo=None, solo_tol=1e-5, on_counts=None):
    """`cases` as ONE call (a lone call, or a padded batch in the order given) against the oracle: frames exact, the durations
    read back equal to the forced ones, every element of the raw mel within `bounds`, the plane's padding and every row's tail
    exactly 0; with `solo` ({case key: the lone call's mel}) every row within `solo_tol` max-abs of its lone call.
    `on_counts(kernel_counts, tag)`: the caller's assertions on the call's launches.  Returns (kernel names that ran, [each row's
    mel [M, F]])."""
    B = len(cases)
    Fmax, Pmax = max(c.F for c in cases), max(len(c.ids) for c in cases)
    noise = np.zeros((B, hp.mel_channels, Fmax + 5), F32)
    for b, c in enumerate(cases):
        noise[b, :, : c.noise.shape[1]] = c.noise
    eng.profile_reset()
    mel = eng.glow_infer(g, [c.ids for c in cases], 0.667, 1.0, noise=noise, durations=[c.d for c in cases])
    counts = eng.kernel_counts()
    ran = {k for k, n in counts.items() if n > 0}
    if on_counts:
        on_counts(counts, f"{label} {cases!r}")
    frames, dur = [int(f) for f in mel.frames], mel.durations
    plane = mel_plane(eng, mel) if Fmax else np.zeros((B, hp.mel_channels, 0), F32)
    mel.free()
    assert plane.shape[2] % 4 == 0 and Fmax <= plane.shape[2] < Fmax + 4, (label, plane.shape, Fmax)
    assert dur.shape == (B, Pmax), (label, dur.shape)
    rows = []
    for b, c in enumerate(cases):
        tag = f"{label} {c!r} " + ("B=1" if B == 1 else f"row {b} of B={B}")
        assert frames[b] == c.F, (tag, frames[b], c.F)
        assert np.array_equal(dur[b, : len(c.ids)], c.exp_d) and np.all(dur[b, len(c.ids):] == 0), (tag, dur[b].tolist(), c.exp_d.tolist())
        compare_mel(plane[b], oracle(gsd, hp, key, c), c.F, bounds, tag)
        rows.append(plane[b][:, : c.F].copy())
        if solo is not None and c.F:
            e = float(np.abs(rows[-1].astype(np.float64) - solo[c.key]).max())
            assert e <= solo_tol, (tag, "against its lone call", e, solo_tol)
    return ran, rows


def check_glow_lengths(eng, g, gsd, hp, cases, oracle, key, bounds=F32_MEL, label="", batch=8, solo_tol=1e-5, on_counts=None,
                       rows=None):
    """Each case as a lone call, then the longest <= `batch` of them as one ragged padded batch in unsorted order (`rows`: this
    batch, in this order, instead): every row against the oracle (check_glow_rows) and within `solo_tol` of its lone call.
    Returns (kernel names that ran in the lone calls, kernel names that ran in the batch)."""
    ran, solo = set(), {}
    for c in cases:
        r, got = check_glow_rows(eng, g, gsd, hp, [c], oracle, key, bounds, label, on_counts=on_counts)
        ran |= r
        solo[c.key] = got[0]
    if rows is None:
        rows = sorted(cases, key=lambda c: (-c.F, -len(c.ids), c.key))[:batch]  # the longest: the most tiles per row
        rows = rows[::2] + rows[1::2][::-1]  # ragged, not sorted
    ran_batch = set()
    if len(rows) > 1:
        ran_batch, _ = check_glow_rows(eng, g, gsd, hp, rows, oracle, key, bounds, label, solo=solo, solo_tol=solo_tol, on_counts=on_counts)
    return ran, ran_batch


def check_plain_durations(eng, g, gsd, hp, P, length_scale=1.0, label=""):
    """One plain call (no forced durations) on glow_ids(P): the duration predictor and duration_kernel's ceil path.  The
    durations equal ceil(exp(logw) * length_scale) of the oracle's logw with the last id truncated as attn_durations does."""
    from tests.test_emu_prosody import attn_durations, oracle_logw, scaled_w

    ids = glow_ids(hp, P, gsd, length_scale)
    w = scaled_w(oracle_logw(gsd, hp, ids), length_scale)
    exp_d, F = attn_durations(np.ceil(w).astype(np.int64), hp.n_sqz)
    mel = eng.glow_infer(g, ids, 0.667, length_scale, seed=P, want_durations=True)
    got, frames = mel.durations, int(mel.frames[0])
    mel.free()
    assert got.shape == (1, P) and frames == F == int(got.sum()), (label, P, frames, F)
    assert np.array_equal(got[0], exp_d), (label, P, np.flatnonzero(got[0] != exp_d)[:8].tolist())


def check_interior_columns_equal(eng, g, hp, F2, label=""):
    """A bound-free seam check of the decoder: 8 ids of which ONE gets every frame, no noise -> every decoder column starts from the
    same vector, and the flows are convolutions along time: away from the two ends (further than the decoder's receptive field,
    n_blocks_dec * n_block_layers * (kernel_size_dec - 1) / 2 columns) every column goes through the same arithmetic in the same
    order, whichever tile it falls in, so frames f and f + n_sqz are equal bit for bit.  A tile that recomputes too narrow a halo, or
    reads a neighbour's column, breaks that at its seams.  Returns the number of interior columns."""
    d = np.zeros(8, np.int32)
    d[3] = hp.n_sqz * F2
    mel = eng.glow_infer(g, glow_ids(hp, 8), 0.0, 1.0, durations=d)
    F = int(mel.frames[0])
    raw = mel.numpy("raw")[0]
    mel.free()
    assert F == hp.n_sqz * F2, (label, F)
    reach = hp.n_blocks_dec * hp.n_block_layers * ((hp.kernel_size_dec - 1) // 2) * hp.n_sqz
    a, b = raw[:, reach : F - reach - hp.n_sqz], raw[:, reach + hp.n_sqz : F - reach]
    assert a.shape[1] > 0, (label, "F2 too short for an interior", F2, reach)
    bad = np.flatnonzero(np.any(a != b, axis=0))
    assert bad.size == 0, (label, "decoder columns differ in the interior: frames", (bad[:8] + reach).tolist(),
                           float(np.abs(a - b).max()))
    return a.shape[1] // hp.n_sqz


# ---- the vocoder's counterpart: a constant mel gives a hop-periodic waveform ----------------------------------------
# Every frame of the mel the same column: everything between mel and waveform is a convolution along time, a polyphase
# transposed convolution or a pointwise function, the phase of a transposed convolution at output sample t depends on t modulo the
# stage's cumulative rate, and every cumulative rate divides `hop`.  So samples t and t + hop, both further than the receptive field
# from the two ends, are the same arithmetic on the same numbers in the same order whichever tile, wave or lane computes them, in
# every precision: equal bit for bit.  A tile that stages too narrow a halo, reads a neighbour's or an uninitialised column,
# masks a column too many at its end or deals a row the wrong tile origin breaks that at its seams.  No tolerance, no oracle.
STFT_HOP, STFT_WIN = 256, 1024  # the denoiser's STFT (oracle/denoise_np.py): its frames repeat every 256 samples


def vocoder_reach(hp, denoise=False):
    """Samples from either end of the waveform past which a sample no longer sees the end: the receptive field of the generator,
    from the hparams alone.  3 frames for conv_pre (k = 7); per upsampler i, with rest = hop / (u_0 ... u_i) samples per column of
    its output, ((k_i - u_i) // 2 + u_i) columns for the transposed conv and h columns for its ResBlocks — h = the longest chain's
    sum over its dilations of (K - 1) d / 2 (conv1) + (K - 1) / 2 (conv2, ResBlock1 only); 3 samples for conv_post (k = 7).  With
    the denoiser, one STFT window and one STFT hop more."""
    hop = hp.hop
    rb1 = hp.resblock == "1"
    reach, rest = 3 * hop, hop
    for u, k in zip(hp.upsample_rates, hp.upsample_kernel_sizes):
        rest //= u
        h = max(sum((K - 1) * d // 2 + ((K - 1) // 2 if rb1 else 0) for d in ds)
                for K, ds in zip(hp.resblock_kernel_sizes, hp.resblock_dilation_sizes))
        reach += ((k - u) // 2 + u) * rest + h * rest
    reach += 3
    return reach + (STFT_WIN + STFT_HOP if denoise else 0)


def blind_tiles(hp, precision="f32"):
    """What check_hop_periodic cannot see: a seam that recurs at the same phase of every period shows the same error at t and
    t + hop.  That is every tile of vocoder_tiles(hp, precision) whose width in samples (width * rest, rest = samples per column of
    its stage) divides hop -> [(label, stage, width)].  ("bf16" = both bf16 modes.)  The list is a fact about the periodic check;
    its fp16 / bf16 last-stage entries (HPOST_TW / POST_TW and the last stage's conv tiles) are bounded by check_layers, which
    compares every launch with float64 from its own input plane."""
    hop = hp.hop
    out = []
    for label, stage, width, _ in vocoder_tiles(hp, precision):
        rest = hop // int(np.prod(hp.upsample_rates[: stage + 1]))
        if hop % (width * rest) == 0:
            out.append((label, stage, width))
    return out


def short_frames(hp, precision="f32"):
    """The smallest frame count check_hop_periodic accepts (8 interior periods) whose interior also holds three whole stage-0
    tiles of the widest stage-0 tile of vocoder_tiles(hp, precision) (the stage with the fewest columns per frame: the first to
    run out of seams as F shrinks)."""
    hop, u0 = hp.hop, hp.upsample_rates[0]
    Rf = -(-vocoder_reach(hp) // hop)  # the reach in whole frames
    w = max(width for _, stage, width, _ in vocoder_tiles(hp, precision) if stage == 0)
    F = 2 * Rf + 8
    while (F - Rf) * u0 // w - -(-Rf * u0 // w) < 3:
        F += 1
    return F


def constant_mel(hp, rows):
    """[B, num_mels, max(rows)]: row b = one column (0.57 + 0.06 randn, seeded by the geometry and b) repeated rows[b] times, 0
    behind it."""
    seed = zlib.crc32(repr(hp).encode())
    mel = np.zeros((len(rows), hp.num_mels, max(rows)), F32)
    for b, F in enumerate(rows):
        col = (0.57 + 0.06 * np.random.default_rng(seed + b).standard_normal(hp.num_mels)).astype(F32)
        mel[b, :, :F] = col[:, None]
    return mel


def check_hop_periodic(eng, v, vhp, F, *, rows=None, denoise=0.0, label=""):
    """One vocoder call on a constant mel of F frames (`rows`: a ragged batch of these frame counts, another column per row).  Per
    row, with n = frames * hop, R = vocoder_reach rounded up to whole hops and the period P = hop (with the denoiser: the least
    common multiple of hop and the STFT's hop): samples [R, n - R - P) equal samples [R + P, n - R) bit for bit, float and int16;
    the interior [R, n - R) holds at least 8 periods (a shorter F is refused); the interior's first period is not flat and
    nowhere at +-1.0 (a saturated waveform would be periodic whatever the kernels do); the tail past n is 0.  Returns the
    kernel signature of the call."""
    hop = vhp.hop
    rows = [int(F)] if rows is None else [int(f) for f in rows]
    P = int(np.lcm(hop, STFT_HOP)) if denoise else hop
    reach = vocoder_reach(vhp, bool(denoise))
    R = -(-reach // hop) * hop
    for f in rows:
        if (f * hop - 2 * R) // P < 8:
            raise ValueError(f"{label}: {f} frames leave fewer than 8 periods of {P} samples between the two reaches of {R}")
    mb = eng.mel_from_numpy(constant_mel(vhp, rows), np.array(rows, np.int32))
    try:
        eng.profile_reset()
        wav, i16 = eng.hifigan_infer(v, mb, denoiser_strength=float(denoise))
        sig = kernel_signature(eng)
    finally:
        mb.free()
    rest0 = hop // vhp.upsample_rates[0]
    for b, f in enumerate(rows):
        n = f * hop
        tag = f"{label} F={f} " + ("B=1" if len(rows) == 1 else f"row {b} of B={len(rows)}")
        assert np.all(wav[b, n:] == 0) and np.all(i16[b, n:] == 0), (tag, "samples past the row's end are not 0")
        one = wav[b, R : R + P]
        sd = float(one.std())
        print(f"{tag}: n {n} reach {reach} interior [{R}, {n - R}) = {(n - 2 * R) // P} periods of {P}, period std {sd:.3e} "
              f"peak {float(np.abs(one).max()):.3e}")
        assert sd > 0.0 and np.all(np.isfinite(one)), (tag, "the period is flat", sd)
        assert float(np.abs(one).max()) < 1.0, (tag, "the period touches +-1.0")
        for name, x in (("float", wav[b]), ("int16", i16[b])):
            lo, hi = x[R : n - R - P], x[R + P : n - R]
            bad = np.flatnonzero(lo != hi)
            if bad.size:
                d = np.abs(lo[bad].astype(np.float64) - hi[bad].astype(np.float64))
                first = (bad[:8] + R).tolist()
                raise AssertionError(
                    f"{tag}: {name} samples t and t + {P} differ at {bad.size} of {lo.size} interior samples; first t = {first} "
                    f"(stage-0 columns {[t // rest0 for t in first]}, frames {[t // hop for t in first]}), last t = {int(bad[-1]) + R}, "
                    f"largest difference {float(d.max()):.3e} at t = {int(bad[int(d.argmax())]) + R}")
    return sig


def choose_glow_lengths(sigs, must=(), edges=None, cap=16, label=""):
    """The lengths a GlowTTS case compares, at most `cap`: the first n of each signature and `must`; then the transitions (n and
    n + 1 where the signature changes) by increasing n; then lengths that cover the tile edges `edges` (edge_frames) not hit yet.
    Prints the choice with the edges each length covers, and whatever the cap left out."""
    ns = sorted(sigs)
    first = {}
    for n in ns:
        first.setdefault(sigs[n], n)
    chosen = set(first.values()) | set(must)
    assert len(chosen) <= cap, (label, "more signatures and fixed lengths than the cap", sorted(chosen))
    trans = [m for a, b in zip(ns, ns[1:]) if sigs[a] != sigs[b] for m in (a, b)]
    for m in trans:
        if len(chosen) < cap:
            chosen.add(m)
    if set(trans) - chosen:
        print(f"{label}: transitions without a length (cap {cap}): {sorted(set(trans) - chosen)}")
    edges = edges or {}
    chosen |= set(cover_edges(edges, cap - len(chosen), have=chosen))
    left = {(s, w, k) for hits in edges.values() for (_, s, w, k) in hits}
    for n in sorted(chosen):
        hits = edges.get(n, ())
        left -= {(s, w, k) for (_, s, w, k) in hits}
        print(f"{label} length {n}: " + (", ".join(sorted({f'{lab} {kind}' for (lab, _, _, kind) in hits})) or "-"))
    if left:
        print(f"{label}: edges without a length (cap {cap}): {sorted((s[0], w, k) for (s, w, k) in left)}")
    return sorted(chosen)


# ---- BASELINE config 3 ---------------------------------------------------------------------------------------------------
def bench_form(eng, g, v, rows, length_scale, seed, audio_settings, threads=1):
    """Every utterance through the call bench.py's config3 leg makes (`synthesize(..., seed=seed + i)`), from `threads`
    threads at once -> {i: (frames, f32 row, i16 row)}."""
    out = {}
    errs = []
    lock = threading.Lock()
    nxt = [0]

    def work():
        try:
            while True:
                with lock:
                    i = nxt[0]
                    nxt[0] += 1
                if i >= len(rows):
                    return
                fr, f32, i16 = eng.synthesize(g, v, rows[i], 0.667, length_scale, seed=seed + i, audio_settings=audio_settings,
                                              want_float=True, frames_per_id_guess=12.0 / max(length_scale, 0.05))
                out[i] = (int(fr[0]), f32[0], i16[0])
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work) for _ in range(threads)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    assert sorted(out) == list(range(len(rows)))
    return out


def check_load_independence(eng, g, v, rows, length_scale, seed, audio_settings, threads=8, need=(), label=""):
    """The bench form with `threads` calls in flight and one call at a time: the same frames, float and int16 bits for every
    utterance (the tile choices that depend on the load must not change a result).  `need`: kernel names the loaded pass must
    have run.  Returns the lone pass."""
    eng.profile_reset()
    busy = bench_form(eng, g, v, rows, length_scale, seed, audio_settings, threads)
    sig = kernel_signature(eng)
    lone = bench_form(eng, g, v, rows, length_scale, seed, audio_settings, 1)
    print(f"{label} {threads} threads in flight: {sorted(sig)}")
    for k in need:
        assert k in sig, (k, sorted(sig))
    for i in range(len(rows)):
        (fa, wa, ia), (fb, wb, ib) = busy[i], lone[i]
        assert fa == fb and np.array_equal(wa, wb) and np.array_equal(ia, ib), (label, i, fa, fb)
    return lone


def check_micro_batches(eng, g, v, rows, length_scale, seed, audio_settings, batch=8):
    """`sharding.synthesize_shard` (rank 0 of 1) at batch 1 and at `batch`: the keys 0 ... n - 1 in both, every utterance the
    same length and within 1 int16 LSB (a padded batch picks other tiles: another summation order)."""
    from larynx_amd import sharding

    kw = dict(noise_scale=0.667, length_scale=length_scale, seed=seed, audio_settings=audio_settings)
    one = sharding.synthesize_shard(eng, g, v, rows, 0, 1, batch=1, **kw)
    many = sharding.synthesize_shard(eng, g, v, rows, 0, 1, batch=batch, **kw)
    assert sorted(one) == sorted(many) == list(range(len(rows)))
    worst = 0
    for i in range(len(rows)):
        assert one[i].shape == many[i].shape, (i, one[i].shape, many[i].shape)
        d = int(np.abs(one[i].astype(np.int32) - many[i].astype(np.int32)).max()) if one[i].size else 0
        assert d <= 1, (i, d)
        worst = max(worst, d)
    print(f"micro-batches of {batch} against batch 1: {len(rows)} utterances, largest difference {worst} LSB")
    return one, many


def check_mels(eng, g, gsd, ghp, rows, length_scale, seed, pick, exempt=(), tol=5e-5, label=""):
    """The seeded device mel (batch 1, the stream seed + i) of every utterance in `pick` against the oracle fed the same noise
    field (`gauss_noise(seed + i, 1, M, F + 7)`: what the seeded call draws).  Returns {i: oracle raw mel}."""
    refs = {}
    worst = 0.0
    for i in pick:
        if i in exempt:
            continue
        mel = eng.glow_infer(g, rows[i], 0.667, length_scale, seed=seed + i)
        F = int(mel.frames[0])
        raw = mel.numpy("raw")[0][:, :F]
        mel.free()
        noise = eng.gauss_noise(seed + i, 1, ghp.mel_channels, F + 7)[0]
        ref = glow_tts_np.glow_tts_infer(gsd, ghp, rows[i], noise, 0.667, length_scale)
        assert ref.shape[1] == F, (i, ref.shape, F)
        e = float(np.abs(raw - ref).max())
        assert e <= tol, (label, i, F, e)
        worst = max(worst, e)
        refs[i] = ref
    print(f"{label} mels: {len(refs)} utterances against the oracle, largest max-abs {worst:.2e}")
    return refs


def check_waves_end_to_end(eng, g, v, gsd, vsd, ghp, vhp, rows, length_scale, seed, audio_settings, pick, lone, ref_mels,
                           batch=8, bounds=F32_WAVE, label=""):
    """The utterances in `pick` end to end against the oracle (oracle mel -> oracle vocoder) in both forms: the bench form's
    float rows (`lone`, batch 1) and the rows of their micro-batch of `batch` (sharding.micro_batches: same grouping),
    re-run through glow_infer(row_seeds=...) + hifigan_infer."""
    from larynx_amd import sharding

    hop = vhp.hop
    groups = sharding.micro_batches(list(range(len(rows))), [len(r) for r in rows], batch)
    refs = {}
    for i in pick:
        ref_mel = ref_mels.get(i)
        if ref_mel is None:
            noise = eng.gauss_noise(seed + i, 1, ghp.mel_channels, lone[i][0] + 7)[0]
            ref_mel = glow_tts_np.glow_tts_infer(gsd, ghp, rows[i], noise, 0.667, length_scale)
        refs[i] = hifi_gan_np.hifigan_infer(vsd, vhp, audio_np.mel_to_vocoder_input(ref_mel, audio_settings))
        F, wav, i16 = lone[i]
        assert F * hop == refs[i].shape[0]
        compare_wave(wav, i16, refs[i], F * hop, bounds, f"{label} utterance {i} (F={F}) B=1")
    for grp in groups:
        mine = [i for i in pick if i in grp]
        if not mine:
            continue
        mel = eng.glow_infer(g, [np.asarray(rows[j], np.int64) for j in grp], 0.667, length_scale,
                             row_seeds=[seed + j for j in grp], audio_settings=audio_settings)
        wb, ib = eng.hifigan_infer(v, mel)
        for i in mine:
            b = grp.index(i)
            F = lone[i][0]
            assert int(mel.frames[b]) == F
            compare_wave(wb[b], ib[b], refs[i], F * hop, bounds, f"{label} utterance {i} (F={F}) row {b} of B={len(grp)}")
        mel.free()
    return refs


# ---- layer by layer: every launch of one vocoder call against float64, from that launch's own input plane --------------------
# The planes of one call (`Engine.hifigan_infer_taps`) against tests/voc_layers_np.py: the reference of a layer is computed from
# the planes its launch READ, so no error is carried from layer to layer and every bound is derived (voc_layers_np's `delta`, half
# an fp16 ulp) or calibrated on the reference alone (the flip share).  This bounds what check_hop_periodic cannot see: the seams
# blind_tiles lists for the fp16 / bf16 last stages, and an error all tiles share.
LAYER_PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16": 2, "f16": 3}  # ffi.PRECISION_*
F16_KERNELS = ("conv_f16_kernel", "conv_f16_group_kernel", "pair_f16_group_kernel")
# Kernels that keep a whole stage's chains on chip and write no plane of a single conv or pair: check_layers' callers switch them
# off ("mrf_small" = 0) and they stay outside the layer check (their own tests: the tile-edge sweep and the periodic check).
LAYER_BLIND_KERNELS = ("mrf_small_kernel", "mrf8_kernel")


def layer_mode(kernel, precision):
    """The operand format of the launch counted under `kernel` in a model switched to `precision`."""
    if kernel in F16_KERNELS:
        return "f16"
    if kernel.startswith("conv_bf16") or kernel.startswith("pair_bf16"):
        assert precision in ("bf16x3", "bf16"), (kernel, precision)
        return precision
    return "f32"


def layer_frames(hp, tile_class):
    """The smallest frame count at which every tile of vocoder_tiles(hp, tile_class) has at least two interior seams inside a row
    (three tiles: that covers the three HPOST_TW / POST_TW tiles too) and a ragged last tile — wherever a frame count can make it
    ragged at all (a tile whose width divides the stage's columns per frame is full at every F)."""
    tiles = vocoder_tiles(hp, tile_class)
    axis = vocoder_axis(hp)
    assert tiles, (hp, tile_class)
    F = 1
    while not all(-(-axis(F, stage) // width) >= 3 and (axis(F, stage) % width or axis(1, stage) % width == 0) for _, stage, width, _ in tiles):
        F += 1
        assert F < 4096, (hp, tile_class)
    return F


def layer_mel(num_mels, rows):
    """[B, num_mels, max(rows)]: 2 * randn seeded by the row's length, 0 behind a row's frames."""
    mel = np.zeros((len(rows), num_mels, max(rows)), F32)
    for b, F in enumerate(rows):
        mel[b, :, :F] = (2 * np.random.default_rng(3000 + F + 7 * b).standard_normal((num_mels, F))).astype(F32)
    return mel


def check_layers(engine, hp, precision, frames, options=None, *, v, sd, label="", only=None):
    """One tapped vocoder call of model `v` (weights `sd`) in `precision` on rows of `frames` frames, under `options`
    ({name: (value, default)}).  Asserts: the tapped call returns the plain call's rows bit for bit and launches the same kernels;
    the `wav` tap is those rows; and for every tap after `mel`, on the valid columns of every row, |plane - ref64| within the
    derived bound (voc_layers_np.bound_fp16 / bound_f32), ref64 built from the taps the launch read.  For fp16 planes also: the
    elements that differ from fp16(ref64) at all are at most 4 times as many as in the layers' float32 restatements in another tap
    order (floor: 8 per plane), counted over all the planes a kernel wrote in this call: one restatement of one plane is one draw
    of the share it estimates, and in a fused pair one flipped element of the intermediate moves K * C sums at once, so single
    planes scatter widely; the pool is fixed here, before any kernel's count is looked at.  A schedule whose stages write no plane
    of a single conv or pair (LAYER_BLIND_KERNELS, the serial form's "stage{i}") is refused: switch that fusion off.
    `only`: the tap names to compare (a long call whose point is the seams of a few launches); every tap still exists and the
    rows are still compared.  Returns (rows of {"name", "kernel", "mode", "ratio", "flips", "restated", "n"}, kernel names)."""
    from larynx_amd import weights
    from tests import voc_layers_np as V

    rows = [int(f) for f in np.atleast_1d(frames)]
    options = dict(options or {})
    nk, nd = len(hp.resblock_kernel_sizes), len(hp.resblock_dilation_sizes[0])
    rb1 = hp.resblock == "1"
    W_ = lambda name: weights.resolve_tensor(sd, name + ".weight")
    B_ = lambda name: weights.resolve_tensor(sd, name + ".bias")
    mel = layer_mel(hp.num_mels, rows)
    mb = engine.mel_from_numpy(mel, np.array(rows, np.int32))
    for k, (val, _) in options.items():
        engine.set_option(k, val)
    try:
        engine.set_precision(v, LAYER_PRECISIONS[precision])
        engine.profile_reset()
        plain, _ = engine.hifigan_infer(v, mb, want_int16=False)
        c_plain = engine.kernel_counts()
        engine.profile_reset()
        wav, taps = engine.hifigan_infer_taps(v, mb)
        c_taps = engine.kernel_counts()
    finally:
        engine.set_precision(v, LAYER_PRECISIONS["f32"])
        for k, (_, default) in options.items():
            engine.set_option(k, default)
        mb.free()
    tag = f"{label} {precision} rows {rows}"
    # (every layer is walked before anything fails: a kernel that leaves a column unwritten shows here first, and the walk below
    # names the layer)
    failures = [] if np.array_equal(wav, plain) else [(tag, "the tapped call's rows differ from the plain call's")]
    assert c_taps == c_plain, (tag, "the seam changed what runs", c_taps, c_plain)
    by = {t["name"]: t for t in taps}
    assert len(by) == len(taps) and taps[0]["name"] == "mel" and taps[-1]["name"] == "wav", (tag, [t["name"] for t in taps])
    for b, F in enumerate(rows):
        n = F * hp.hop
        if not (by["wav"]["len"][b] == n and np.array_equal(by["wav"]["x"][b, 0, :n], wav[b, :n])):
            failures.append((tag, "the wav tap is not the returned row", b))
    kernels = {t["kernel"] for t in taps}
    if precision == "f32":
        assert not failures, failures
        return [], kernels

    def plane(name, b):
        t = by[name]
        return t["x"][b, :, : t["len"][b]]

    report = []
    cur = ["pre"]  # the planes the next upsampler (or conv_post) averages on load
    outs = {}
    for t in taps:
        name, kernel = t["name"], t["kernel"]
        mode = layer_mode(kernel, precision)
        if name == "mel":
            for b, F in enumerate(rows):  # the generator's input as the first conv reads it: exact
                want = V.fp16(mel[b, :, :F]) if t["f16"] else mel[b, :, :F]
                assert np.array_equal(plane("mel", b)[: hp.num_mels], want) and not np.any(plane("mel", b)[hp.num_mels :]), (tag, "mel", b)
            continue
        assert kernel not in LAYER_BLIND_KERNELS and not name.startswith("stage"), (tag, name, kernel, "no plane of a single conv or pair: switch this fusion off")
        if only is not None and name not in only:
            if name.startswith("rb") and name.count(".") == 2 and int(name.split(".")[2]) == nd - 1:
                outs.setdefault(int(name[2:].split(".")[0]), []).append(name)
                if len(outs[int(name[2:].split(".")[0])]) == nk:
                    cur = outs[int(name[2:].split(".")[0])]
            continue
        stage = (lambda planes, slope: V.stage_f16(planes, slope)) if mode == "f16" else (lambda planes, slope: V.stage_f32(planes, slope))
        worst, flips, restated, count = (0.0, None), 0, 0, 0
        for b in range(len(rows)):
            got = plane(name, b).astype(np.float64)
            ref32 = None
            if name == "pre":
                x = stage([plane("mel", b)[: hp.num_mels] if not t["f16"] else plane("mel", b)], 1.0)
                w = W_("conv_pre")
                if t["f16"]:  # the packed plane's zero channels past num_mels meet zero weights
                    w = np.concatenate([w, np.zeros((w.shape[0], x.shape[0] - w.shape[1], w.shape[2]), F32)], axis=1)
                args = (mode, w, B_("conv_pre"), x)
                ref, delta = V.conv_layer(*args)
                if mode == "f16":
                    ref32 = V.conv_layer32(*args)
            elif name.startswith("up"):
                i = int(name[2:])
                x = stage([plane(c, b) for c in cur], V.SLOPE)
                u = hp.upsample_rates[i]
                ref, delta = V.upsample_layer(mode, W_(f"ups.{i}"), B_(f"ups.{i}"), x, u)
                if mode == "f16":
                    ref32 = V.conv_layer32(mode, W_(f"ups.{i}"), B_(f"ups.{i}"), x, transposed_u=u)
            elif name.startswith("rb"):
                parts = name[2:].split(".")
                i, j, d = int(parts[0]), int(parts[1]), int(parts[2])
                is_t = len(parts) == 4
                K, dil = hp.resblock_kernel_sizes[j], hp.resblock_dilation_sizes[j][d]
                rin = f"rb{i}.{j}.{d - 1}" if d else f"up{i}"
                xin = plane(rin, b)
                pre_ = f"resblocks.{i * nk + j}"
                if not rb1:
                    args = (mode, W_(f"{pre_}.convs.{d}"), B_(f"{pre_}.convs.{d}"), stage([xin], V.SLOPE), dil, xin)
                    ref, delta = V.conv_layer(*args)
                    ref32 = V.conv_layer32(*args) if mode == "f16" else None
                elif is_t:  # conv1's stored output: activated before its rounding in fp16, raw in the f32 planes
                    args = (mode, W_(f"{pre_}.convs1.{d}"), B_(f"{pre_}.convs1.{d}"), stage([xin], V.SLOPE), dil, None, V.SLOPE if mode == "f16" else 1.0)
                    ref, delta = V.conv_layer(*args)
                    ref32 = V.conv_layer32(*args) if mode == "f16" else None
                elif name + ".t" in by:
                    tin = stage([plane(name + ".t", b)], 1.0 if by[name + ".t"]["f16"] else V.SLOPE)
                    args = (mode, W_(f"{pre_}.convs2.{d}"), B_(f"{pre_}.convs2.{d}"), tin, 1, xin)
                    ref, delta = V.conv_layer(*args)
                    ref32 = V.conv_layer32(*args) if mode == "f16" else None
                else:
                    args = (mode, W_(f"{pre_}.convs1.{d}"), B_(f"{pre_}.convs1.{d}"), W_(f"{pre_}.convs2.{d}"), B_(f"{pre_}.convs2.{d}"),
                            stage([xin], V.SLOPE), xin, dil)
                    ref, delta = V.pair_layer(*args)
                    ref32 = V.pair_layer32(*args) if mode == "f16" else None
                if d == nd - 1 and not is_t and b == 0:
                    outs.setdefault(i, []).append(name)
                    if len(outs[i]) == nk:
                        cur = outs[i]
            else:
                assert name == "wav", (tag, name)
                x = V.stage_f32([plane(c, b) for c in cur], V.SLOPE_POST, by_reciprocal=kernel == "post_f16_kernel")
                ref, delta = V.post_layer(W_("conv_post"), B_("conv_post"), x)
            assert ref.shape == got.shape, (tag, name, b, ref.shape, got.shape)
            stored16 = bool(t["f16"])
            bound = V.bound_fp16(ref, delta) if stored16 else V.bound_f32(ref, delta)
            ratio = np.where(np.isfinite(got), np.abs(got - ref) / bound, np.inf)  # (an element never written is no number)
            at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            if float(ratio[at]) > worst[0]:
                worst = (float(ratio[at]), (b, int(at[0]), int(at[1])))
            if stored16:
                r16 = V.fp16(ref)
                flips += int(np.count_nonzero(got.astype(F32) != r16))
                restated += int(np.count_nonzero(V.fp16(ref32) != r16))
            count += got.size
        report.append(dict(name=name, kernel=kernel, mode=mode, ratio=worst[0], flips=flips, restated=restated, n=count))
        share = f" differing from fp16(ref64): {flips} ({100.0 * flips / count:.3f} %), float32 restatement {restated} ({100.0 * restated / count:.3f} %)" if t["f16"] else ""
        print(f"{tag} {name} [{kernel}, {mode}]: worst err / bound {worst[0]:.3f} at (row, channel, column) {worst[1]} of {count}{share}")
        if not worst[0] <= 1.0:
            failures.append((tag, name, kernel, "outside the derived bound at (row, channel, column)", worst))
    for kernel in sorted({r["kernel"] for r in report if r["mode"] == "f16"}):
        mine = [r for r in report if r["kernel"] == kernel and r["mode"] == "f16"]
        flips, restated, count = (sum(r[k] for r in mine) for k in ("flips", "restated", "n"))
        most = max(mine, key=lambda r: r["flips"] / r["n"])
        print(f"{tag} {kernel}: {len(mine)} planes, {flips} of {count} elements differ from fp16(ref64) ({100.0 * flips / count:.3f} %), float32 "
              f"restatement {restated} ({100.0 * restated / count:.3f} %); the plane with the largest share: {most['name']} {most['flips']} of {most['n']}")
        if flips > max(4 * restated, 8 * len(mine)):
            failures.append((tag, kernel, "more elements differ from the correctly rounded result than the f32 summation order explains", flips, restated, count,
                             "largest share: " + most["name"]))
    assert not failures, failures
    return report, kernels


# ---- layer by layer: every launch of one GlowTTS call against float64, from the planes that launch read -------------------------
# The planes of one call (`Engine.glow_infer_taps`) against tests/glow_layers_np.py.  The acoustic model's passes rewrite their
# planes in place (x, t1, t2, h, acts, skip, z), so the walk keeps the LATEST tap of each tensor and feeds every launch's reference
# the taps it read; a launch that writes two planes (lin16_kernel.ln with its stored normalised input, res_skip, glow_tail_kernel,
# wn_f16_kernel) is computed once and its second plane compared when its tap comes.  Bounds: glow_layers_np's rule; acceptance:
# voc_layers_np.bound_f32 on every valid column of every row, nothing exempt.
GLOW_NAMED_KERNELS = ("attention_mfma_kernel", "attention_mfma_kernel.p768", "attention_kernel", "oproj_ln_kernel", "lin16_kernel",
                      "lin16_kernel.ln", "lin16_kernel.wide", "gate16_kernel", "gate16_kernel.wide", "glow_tail_kernel", "wn_f16_kernel")


def glow_layer_lengths(hp, precision, axis, kinds, lo=1):
    """The smallest length >= `lo` along `axis` ("P" / "F2") at which every tile of glow_tiles(hp, precision) whose label starts with
    one of `kinds` has at least three tiles inside a row, the last one ragged (two interior seams and a partial tile)."""
    widths = sorted({w for lab, stage, w, _ in glow_tiles(hp, precision) if stage[0] == axis and any(lab.startswith(k) for k in kinds)})
    assert widths, (axis, kinds)
    n = lo
    while not all(n > 2 * w and n % w for w in widths):
        n += 1
        assert n < 8192, (axis, kinds, widths)
    return n


WN_RESTATED_LAUNCHES = 2  # wn_f16_kernel launches per call whose planes are restated in float32 (row 0): the first two blocks
_GLOW_TENSORS = {}  # id(state dict) -> (the state dict itself: held, so that its id is not reused; {tensor name: resolved tensor})


def gate_grid_state_dict(sd, hp):
    """`sd` with every block's LAST gate conv silenced (weight_g = 0: the folded weight is exactly zero) and its biases a grid: that
    layer's pre-activations are the biases exactly, whatever h holds, so its `acts` plane isolates the gate epilogue (gate16.h /
    conv_mfma.h: tanhf, expf; wn_f16.h: gate_fast) against float64 tanh(a) sigmoid(b) with nothing carried into the bound.
    tanh biases span +-18 (block parity: +-6, denser around small arguments), past gate_fast's +-15 clamp; the sigmoid biases
    span +-30, dealt across the tanh grid with a stride coprime to H."""
    out = dict(sd)
    H, j = hp.hidden_channels, hp.n_block_layers - 1
    for blk in range(hp.n_blocks_dec):
        key = f"decoder.flows.{3 * blk + 2}.wn.in_layers.{j}"
        out[key + ".weight_g"] = np.zeros_like(np.asarray(sd[key + ".weight_g"]))
        a = np.linspace(-18.0, 18.0, H) if blk % 2 == 0 else np.linspace(-6.0, 6.0, H)
        b = np.linspace(-30.0, 30.0, H)[(np.arange(H) * (7 if blk % 2 == 0 else 11)) % H]
        out[key + ".bias"] = np.concatenate([a, b]).astype(F32)
    return out


def _frame_to_id(exp_d):
    return np.repeat(np.arange(len(exp_d)), np.asarray(exp_d, np.int64))


def check_glow_layers(engine, hp, precision, case, options=None, *, g, sd, label="", speaker_ids=None, restate=False):
    """One tapped GlowTTS call of model `g` (weights `sd`) in `precision` ("f32" / "f16") on the rows `case` (a GlowCase or a list
    of them: one padded batch), durations forced and noise injected, under `options` ({name: (value, default)}).  Asserts: the
    tapped call returns the plain call's mel plane, frames and durations bit for bit and launches the same kernels; the `mel` tap is
    that plane, zero behind every row's frames; and for every tap, on every valid column of every row, |plane - ref64| within the
    derived bound (glow_layers_np / voc_layers_np.bound_f32), ref64 built from the taps the launch read.  Every layer is walked
    before anything fails; the failure names every failing layer, its kernel, its worst err / bound and (row, channel, column).
    `restate`: also the float32 chain restatement of every launch of row 0 against the same bound (a CPU property: the device tests
    leave it off).  Returns (rows of {"name", "kernel", "ratio", "at", "abs", "restated", "n"}, kernel names of the taps, the
    call's kernel_counts)."""
    from larynx_amd import weights
    from tests import glow_layers_np as G
    from tests import voc_layers_np as V

    cases = list(case) if isinstance(case, (list, tuple)) else [case]
    B = len(cases)
    options = dict(options or {})
    H, nh, win = hp.hidden_channels, hp.n_heads, hp.window_size
    nsq, n, nb = hp.n_sqz, hp.n_block_layers, hp.n_blocks_dec
    C = hp.mel_channels * nsq
    half = C // 2
    held, cache = _GLOW_TENSORS.setdefault(id(sd), (sd, {}))  # (folding a weight norm is as dear as a small launch's reference)
    assert held is sd

    def T_(name):
        if name not in cache:
            cache[name] = weights.resolve_tensor(sd, name)
        return cache[name]

    W_ = lambda name: T_(name + ".weight")
    B_ = lambda name: T_(name + ".bias")
    Fmax = max(c.F for c in cases)
    noise = np.zeros((B, hp.mel_channels, Fmax + 5), F32)
    for b, c in enumerate(cases):
        noise[b, :, : c.noise.shape[1]] = c.noise
    kw = dict(noise=noise, durations=[c.d for c in cases])
    if speaker_ids is not None:
        kw["speaker_ids"] = speaker_ids
    ids = [c.ids for c in cases]
    for k, (val, _) in options.items():
        engine.set_option(k, val)
    try:
        assert engine.set_precision(g, LAYER_PRECISIONS[precision]) == 0, (label, precision)
        engine.profile_reset()
        mel = engine.glow_infer(g, ids, 0.667, 1.0, **kw)
        c_plain = engine.kernel_counts()
        plain = (mel_plane(engine, mel), [int(f) for f in mel.frames], mel.durations.copy())
        mel.free()
        engine.profile_reset()
        mel, taps = engine.glow_infer_taps(g, ids, 0.667, 1.0, **kw)
        c_taps = engine.kernel_counts()
        tapped = (mel_plane(engine, mel), [int(f) for f in mel.frames], mel.durations.copy())
        mel.free()
    finally:
        engine.set_precision(g, LAYER_PRECISIONS["f32"])
        for k, (_, default) in options.items():
            engine.set_option(k, default)
    tag = f"{label} {precision} {cases!r}"
    assert c_taps == c_plain, (tag, "the seam changed what runs", c_taps, c_plain)
    failures = []
    if not (np.array_equal(plain[0], tapped[0]) and plain[1] == tapped[1] and np.array_equal(plain[2], tapped[2])):
        failures.append((tag, "the tapped call's mel, frames or durations differ from the plain call's"))
    assert plain[1] == [c.F for c in cases], (tag, plain[1])
    names = [t["name"] for t in taps]
    assert len(set(names)) == len(names) and names[0] == "emb" and names[-1] == "mel", (tag, names)
    by = {t["name"]: t for t in taps}
    for b, c in enumerate(cases):
        t = by["mel"]
        if not (t["len"][b] == c.F and np.array_equal(t["x"][b], tapped[0][b]) and not np.any(t["x"][b][:, c.F :])):
            failures.append((tag, "the mel tap is not the returned plane, or is not zero behind the row's frames", b))

    def plane(name, b):
        t = by[name]
        return t["x"][b, :, : t["len"][b]].astype(np.float64)

    # speaker conditioning (speaker_cond_kernel writes small tables, not planes): float64 from the embedding, with the error of
    # its f32 evaluation (a gin-term contraction of a normalised vector) carried as a bound
    gvec = None
    if speaker_ids is not None:
        spk = np.full(B, speaker_ids) if np.isscalar(speaker_ids) else np.asarray(speaker_ids)
        e = T_("emb_g.weight").astype(np.float64)[spk]
        gvec = e / np.maximum(np.sqrt((e * e).sum(axis=1, keepdims=True)), 1e-12)
        gin = gvec.shape[1]

    def spk_table(w2d, bias, b):
        """w2d [rows, gin] . g + bias -> (value, bound)."""
        w2d = w2d.astype(np.float64)
        val = w2d @ gvec[b] + (0.0 if bias is None else bias.astype(np.float64))
        mag = np.abs(w2d) @ np.abs(gvec[b]) + (0.0 if bias is None else np.abs(bias))
        return val, (2 * gin + 8) * V.U23 * mag  # (the norm's gin-term sum, its root and reciprocal, then the contraction)

    qkv_w = lambda l: np.concatenate([W_(f"encoder.encoder.attn_layers.{l}.conv_{c}") for c in "qkv"], axis=0)
    qkv_b = lambda l: np.concatenate([B_(f"encoder.encoder.attn_layers.{l}.conv_{c}") for c in "qkv"], axis=0)
    NORM = lambda p: (T_(p + ".gamma"), T_(p + ".beta"))
    flow = lambda blk, j: f"decoder.flows.{3 * blk + j}"
    mixw = lambda blk: (T_(flow(blk, 1) + ".weight_inv"), T_(flow(blk, 0) + ".bias").reshape(-1), T_(flow(blk, 0) + ".logs").reshape(-1))
    npre = hp.prenet_layers if hp.prenet else 0
    report, pending, pending32 = [], {}, {}
    wn_restated, wn_sq = {}, {}  # wn_f16_kernel's planes restated in float32; per plane kind [sum err^2 of the kernel, of the restatement, n]
    latest = {}  # tensor -> the tap that holds it now: "x" (the encoder's residual stream), "z", "h", "skip"

    def reference(name, kernel, b):
        """-> {tap name: (ref64, delta)} of the launch that wrote `name`, for row b; and the float32 restatement of `name` (or None)."""
        c = cases[b]
        P = len(c.ids)
        parts = name.split(".")
        if name == "emb":
            return {name: G.embed(T_("encoder.emb.weight"), c.ids, H)}, G.embed_chain32(T_("encoder.emb.weight"), c.ids, H)
        if parts[0] == "pre":
            if parts[1] == "proj":
                src, wn_, ln = f"pre.{npre - 1}", "encoder.pre.proj", NORM(f"encoder.pre.norm_layers.{npre - 1}")
                res = plane("emb", b)
            else:
                i = int(parts[1])
                src, wn_, res = ("emb" if i == 0 else f"pre.{i - 1}"), f"encoder.pre.conv_layers.{i}", None
                ln = None if i == 0 else NORM(f"encoder.pre.norm_layers.{i - 1}")
            if len(parts) == 3:  # the separate LayerNorm's output
                return {name: G.layernorm(plane(src, b), *ln, relu=True)}, G.layernorm_chain32(plane(src, b), *ln, relu=True)
            if ln is None or name + ".ln" in by:
                x = plane(name + ".ln" if ln is not None else src, b)
                return {name: G.linear(W_(wn_), B_(wn_), x, res=res)}, G.linear_chain32(W_(wn_), B_(wn_), x, res=res)
            (y, dy), _ = G.ln_linear(W_(wn_), B_(wn_), plane(src, b), *ln, True, res=res)
            return {name: (y, dy)}, G.linear_chain32(W_(wn_), B_(wn_), G.layernorm_chain32(plane(src, b), *ln, relu=True), res=res)
        if parts[0].startswith("enc") and parts[0] != "enc":
            l = int(parts[0][3:])
            a_ = f"encoder.encoder.attn_layers.{l}"
            f_ = f"encoder.encoder.ffn_layers.{l}"
            x_in = f"enc{l}.x0" if l else ("pre.proj" if npre else "emb")
            what = parts[1]
            if what == "x0":  # the separate LayerNorm of the previous layer's t1 (the fused form files it with qkv)
                ln = NORM(f"encoder.encoder.norm_layers_2.{l - 1}")
                return {name: G.layernorm(plane(f"enc{l - 1}.t1", b), *ln)}, G.layernorm_chain32(plane(f"enc{l - 1}.t1", b), *ln)
            if what == "qkv":
                if l and kernel == "lin16_kernel.ln":
                    ln = NORM(f"encoder.encoder.norm_layers_2.{l - 1}")
                    t1 = plane(f"enc{l - 1}.t1", b)
                    (y, dy), xn = G.ln_linear(qkv_w(l), qkv_b(l), t1, *ln, False)
                    xn32 = G.layernorm_chain32(t1, *ln)
                    return {name: (y, dy), f"enc{l}.x0": xn}, {name: G.linear_chain32(qkv_w(l), qkv_b(l), xn32), f"enc{l}.x0": xn32}
                return {name: G.linear(qkv_w(l), qkv_b(l), plane(x_in, b))}, G.linear_chain32(qkv_w(l), qkv_b(l), plane(x_in, b))
            if what == "att":
                args = (plane(f"enc{l}.qkv", b), T_(a_ + ".emb_rel_k")[0], T_(a_ + ".emb_rel_v")[0], nh, win)
                return {name: G.attention(*args)}, (G.attention_chain32(*args) if restate and b == 0 else None)
            if what == "o":
                args = (W_(a_ + ".conv_o"), B_(a_ + ".conv_o"), plane(f"enc{l}.att", b))
                return {name: G.linear(*args, res=plane(x_in, b))}, G.linear_chain32(*args, res=plane(x_in, b))
            if what == "x1":
                ln = NORM(f"encoder.encoder.norm_layers_1.{l}")
                if f"enc{l}.o" in by:
                    return {name: G.layernorm(plane(f"enc{l}.o", b), *ln)}, G.layernorm_chain32(plane(f"enc{l}.o", b), *ln)
                args = (W_(a_ + ".conv_o"), B_(a_ + ".conv_o"), plane(f"enc{l}.att", b))
                return {name: G.oproj_ln(*args, plane(x_in, b), *ln)}, G.layernorm_chain32(G.linear_chain32(*args, res=plane(x_in, b)), *ln)
            if what == "ffn":
                args = (W_(f_ + ".conv_1"), B_(f_ + ".conv_1"), plane(f"enc{l}.x1", b))
                return {name: G.linear(*args, relu=True)}, G.linear_chain32(*args, relu=True)
            assert what == "t1", name
            args = (W_(f_ + ".conv_2"), B_(f_ + ".conv_2"), plane(f"enc{l}.ffn", b))
            return {name: G.linear(*args, res=plane(f"enc{l}.x1", b))}, G.linear_chain32(*args, res=plane(f"enc{l}.x1", b))
        last_l = hp.n_layers_enc - 1
        if name == "enc.out":
            ln = NORM(f"encoder.encoder.norm_layers_2.{last_l}")
            return {name: G.layernorm(plane(f"enc{last_l}.t1", b), *ln)}, G.layernorm_chain32(plane(f"enc{last_l}.t1", b), *ln)
        pw = "encoder.proj_w"
        if name == "xm":
            args = (W_("encoder.proj_m"), B_("encoder.proj_m"), plane("enc.out", b))
            return {name: G.linear(*args)}, G.linear_chain32(*args)
        if name == "dp.spk":  # speaker_dp_plane_kernel: the speaker half of conv_1 over a constant vector, cut at the row's ends
            w1 = W_(pw + ".conv_1")
            K = w1.shape[2]
            ref, dl, r32 = np.zeros((w1.shape[0], P)), np.zeros((w1.shape[0], P)), np.zeros((w1.shape[0], P), F32)
            t = np.arange(P)
            e32 = T_("emb_g.weight")[spk[b]].astype(F32)  # the restatement: the vector normalised and contracted in float32, backwards
            g32 = e32 * (F32(1) / np.maximum(np.sqrt(np.sum(e32[::-1] * e32[::-1], dtype=F32)), F32(1e-12)))
            for k in range(K):
                val, bd = spk_table(w1[:, H:, k], None, b)
                ok = ((t + k - K // 2 >= 0) & (t + k - K // 2 < P)).astype(np.float64)
                ref += val[:, None] * ok[None, :]
                dl += (bd + V.U23 * K * np.abs(val))[:, None] * ok[None, :]
            for k in range(K - 1, -1, -1):
                v32 = np.zeros(w1.shape[0], F32)
                for i in range(gin - 1, -1, -1):
                    v32 = v32 + w1[:, H + i, k] * g32[i]
                r32 += v32[:, None] * ((t + k - K // 2 >= 0) & (t + k - K // 2 < P)).astype(F32)[None, :]
            return {name: (ref, dl)}, r32
        if name == "dp.1":
            w1 = W_(pw + ".conv_1")[:, :H]
            res = plane("dp.spk", b) if "dp.spk" in by else None
            args = (w1, B_(pw + ".conv_1"), plane("enc.out", b))
            return {name: G.linear(*args, res=res, relu=True)}, G.linear_chain32(*args, res=res, relu=True)
        if name == "dp.2.ln":
            return {name: G.layernorm(plane("dp.1", b), *NORM(pw + ".norm_1"))}, G.layernorm_chain32(plane("dp.1", b), *NORM(pw + ".norm_1"))
        if name == "dp.2":
            wb = (W_(pw + ".conv_2"), B_(pw + ".conv_2"))
            if "dp.2.ln" in by:
                return {name: G.linear(*wb, plane("dp.2.ln", b), relu=True)}, G.linear_chain32(*wb, plane("dp.2.ln", b), relu=True)
            (y, dy), _ = G.ln_linear(*wb, plane("dp.1", b), *NORM(pw + ".norm_1"), False, relu=True)
            return {name: (y, dy)}, G.linear_chain32(*wb, G.layernorm_chain32(plane("dp.1", b), *NORM(pw + ".norm_1")), relu=True)
        if name == "logw.ln":
            return {name: G.layernorm(plane("dp.2", b), *NORM(pw + ".norm_2"))}, G.layernorm_chain32(plane("dp.2", b), *NORM(pw + ".norm_2"))
        if name == "logw":
            wb = (W_(pw + ".proj"), B_(pw + ".proj"))
            if "logw.ln" in by:
                return {name: G.linear(*wb, plane("logw.ln", b))}, G.linear_chain32(*wb, plane("logw.ln", b))
            return ({name: G.ln_proj(plane("dp.2", b), *NORM(pw + ".norm_2"), *wb)},
                    G.linear_chain32(*wb, G.layernorm_chain32(plane("dp.2", b), *NORM(pw + ".norm_2"))))
        if name == "z0":
            args = (plane("xm", b), _frame_to_id(c.exp_d), c.noise, 0.667, nsq)
            return {name: G.expand(*args)}, G.expand_chain32(*args)
        if name == "mel":
            return {name: G.finalize(plane(latest["z"], b), nsq)}, None
        assert parts[0].startswith("blk") and len(parts) == 2, (tag, name)
        blk, what = int(parts[0][3:]), parts[1]
        cp = flow(blk, 2)
        if what == "h":  # the start conv as a launch of its own (the first block's; every block's without the fused tail)
            args = (W_(cp + ".start"), B_(cp + ".start"), plane(latest["z"], b)[:half])
            return {name: G.linear(*args)}, G.linear_chain32(*args)
        if what.startswith("acts"):
            j = int(what[4:])
            if kernel == "wn_f16_kernel":
                assert j == n - 1, name
                w_in = [W_(f"{cp}.wn.in_layers.{i}") for i in range(n)]
                b_in = [B_(f"{cp}.wn.in_layers.{i}") for i in range(n)]
                w_rs = [W_(f"{cp}.wn.res_skip_layers.{i}") for i in range(n - 1)]
                b_rs = [B_(f"{cp}.wn.res_skip_layers.{i}") for i in range(n - 1)]
                acts, skip = G.wn_f16(plane(latest["h"], b), w_in, b_in, w_rs, b_rs)
                out = {name: acts}
                if skip is not None:
                    out[f"blk{blk}.skip{n - 2}"] = skip
                if b == 0 and len(wn_restated) < 2 * WN_RESTATED_LAUNCHES:  # (the calibrated criterion's pool: row 0 of the first launches)
                    a32, s32 = G.wn_f16_chain32(plane(latest["h"], b), w_in, b_in, w_rs, b_rs)
                    wn_restated[name] = a32
                    if s32 is not None:
                        wn_restated[f"blk{blk}.skip{n - 2}"] = s32
                return out, None
            cond = None
            wg, bg = W_(f"{cp}.wn.in_layers.{j}"), B_(f"{cp}.wn.in_layers.{j}")
            x = plane(latest["h"], b)
            dil = hp.dilation_rate ** j
            if gvec is not None:
                cw = W_(cp + ".wn.cond_layer")[:, :, 0][2 * H * j : 2 * H * (j + 1)]
                cond, dcond = spk_table(cw, B_(cp + ".wn.cond_layer")[2 * H * j : 2 * H * (j + 1)], b)
                pre, d = G.linear(wg, bg, x, dil, res=np.repeat(cond[:, None], x.shape[1], axis=1))
                d = d + dcond[:, None]
                return {name: G.gate_value(pre[:H], pre[H:], d[:H], d[H:])}, G.gate_chain32(wg, bg, x, dil, cond)
            return {name: G.gate(wg, bg, x, dil)}, G.gate_chain32(wg, bg, x, dil)
        if what.startswith("h") or what.startswith("skip"):
            j = int(what[1:] if what.startswith("h") else what[4:])
            lastj = j == n - 1
            hj, sj = f"blk{blk}.h{j}", f"blk{blk}.skip{j}"
            wr, br = W_(f"{cp}.wn.res_skip_layers.{j}"), B_(f"{cp}.wn.res_skip_layers.{j}")
            acts, hin = plane(f"blk{blk}.acts{j}", b), plane(latest["h"], b)
            sk = plane(f"blk{blk}.skip{j - 1}", b) if j else None
            hh, ss = G.res_skip(wr, br, acts, hin, sk, lastj)
            zero = np.zeros_like(acts)
            r32 = G.linear_chain32(wr, br, acts, res=(zero if sk is None else sk) if lastj else np.concatenate([hin, zero if sk is None else sk]))
            out = {sj: ss}
            if hh is not None:
                out[hj] = hh
            return out, ({sj: r32} if lastj else {hj: r32[: acts.shape[0]], sj: r32[acts.shape[0] :]})
        z = plane(latest["z"], b)
        end = (W_(cp + ".end"), B_(cp + ".end"))
        if what == "zc":
            args = (plane(f"blk{blk}.skip{n - 1}", b), z, *end, *mixw(blk))
            return {name: G.coupling_mix(*args, mix=False)}, G.coupling_mix_chain32(*args, mix=False)
        assert what == "z", name
        if kernel == "glow_tail_kernel":
            rs = (W_(f"{cp}.wn.res_skip_layers.{n - 1}"), B_(f"{cp}.wn.res_skip_layers.{n - 1}"))
            st = (W_(flow(blk - 1, 2) + ".start"), B_(flow(blk - 1, 2) + ".start")) if blk else None
            acts = plane(f"blk{blk}.acts{n - 1}", b)
            sk = plane(f"blk{blk}.skip{n - 2}", b) if n > 1 else None
            zz, hn = G.glow_tail(acts, sk, z, rs, end, mixw(blk), st)
            out = {name: zz}
            if hn is not None:
                out[f"blk{blk - 1}.h"] = hn
            z32 = G.coupling_mix_chain32(G.linear_chain32(*rs, acts, res=sk), z, *end, *mixw(blk))
            return out, ({name: z32} if st is None else {name: z32, f"blk{blk - 1}.h": G.linear_chain32(*st, z32[:half])})
        if f"blk{blk}.zc" in by:
            zc = plane(f"blk{blk}.zc", b)
            return {name: G.mix_actnorm(zc, np.zeros_like(zc), *mixw(blk), n_split=hp.n_split)}, G.mix_actnorm_chain32(zc, *mixw(blk), n_split=hp.n_split)
        args = (plane(f"blk{blk}.skip{n - 1}", b), z, *end, *mixw(blk))
        return {name: G.coupling_mix(*args)}, G.coupling_mix_chain32(*args)

    for t in taps:
        name, kernel = t["name"], t["kernel"]
        worst, r_worst, count, abs_worst = (0.0, None), None, 0, 0.0
        for b in range(B):
            got = plane(name, b)
            key = (name, b)
            if key not in pending:
                refs, r32 = reference(name, kernel, b)
                for k2, v2 in refs.items():
                    pending[(k2, b)] = v2
                # the launch's float32 restatement: of `name`, or {tap name: plane} for a launch that writes two
                for k2, v2 in (r32 if isinstance(r32, dict) else {name: r32}).items():
                    pending32[(k2, b)] = v2
            ref, delta = pending.pop(key)
            ref32 = pending32.pop(key, None)
            assert ref.shape == got.shape, (tag, name, b, ref.shape, got.shape)
            bound = V.bound_f32(ref, delta)
            ratio = np.where(np.isfinite(got), np.abs(got - ref) / bound, np.inf)  # (an element never written is no number)
            at = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else (0, 0)
            if ratio.size and float(ratio[at]) > worst[0]:
                worst = (float(ratio[at]), (b, int(at[0]), int(at[1])))
            if ratio.size:
                abs_worst = max(abs_worst, float(np.abs(np.where(np.isfinite(got), got - ref, np.inf)).max()))
            if b == 0 and name in wn_restated:
                acc = wn_sq.setdefault("acts" if ".acts" in name else "skip", [0.0, 0.0, 0])
                acc[0] += float(((got - ref) ** 2).sum())
                acc[1] += float(((wn_restated[name].astype(np.float64) - ref) ** 2).sum())
                acc[2] += got.size
                if restate:
                    r_worst = float((np.abs(wn_restated[name].astype(np.float64) - ref) / bound).max())
            if restate and b == 0 and ref32 is not None and ratio.size:
                r_worst = float((np.abs(ref32.astype(np.float64) - ref) / bound).max())
            count += got.size
        # the tensors a later launch reads by role
        p2 = name.split(".")
        if name == "z0" or (p2[0].startswith("blk") and p2[-1] in ("z", "zc")):
            latest["z"] = name
        if p2[0].startswith("blk") and p2[-1].startswith("h"):
            latest["h"] = name
        report.append(dict(name=name, kernel=kernel, ratio=worst[0], at=worst[1], abs=abs_worst, restated=r_worst, n=count))
        rs_ = "" if r_worst is None else f", float32 restatement {r_worst:.3f}"
        print(f"{tag} {name} [{kernel}]: worst err / bound {worst[0]:.3f} at (row, channel, column) {worst[1]} of {count}{rs_}")
        if not worst[0] <= 1.0:
            failures.append((tag, name, kernel, "outside the derived bound: err / bound, (row, channel, column)", worst))
        if r_worst is not None and not r_worst <= 1.0:
            failures.append((tag, name, "the float32 restatement is outside the bound: a wrong derivation", r_worst))
    for what, (e_k, e_r, cnt) in sorted(wn_sq.items()):
        rk, rr = np.sqrt(e_k / cnt), np.sqrt(e_r / cnt)
        print(f"{tag} wn_f16_kernel {what}: RMS |plane - ref64| {rk:.3e} over {cnt} elements, float32 restatement {rr:.3e} (x {rk / max(rr, 1e-300):.2f})")
        if not rk <= 4 * rr:
            failures.append((tag, f"wn_f16_kernel {what}", "wn_f16_kernel", "RMS error above 4 x the float32 restatement's: more than the f32 summation order explains", (rk / max(rr, 1e-300), None)))
    assert not pending, (tag, "planes a reference expected and no tap delivered", sorted(pending))
    assert not failures, failures
    return report, {t["kernel"] for t in taps}, c_taps
