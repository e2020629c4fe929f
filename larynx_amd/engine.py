"""One `Engine` per process per GPU: owns the C-ABI context, the resident models
and the thin numpy marshalling around the inference entry points."""
from __future__ import annotations

import ctypes as C
import json
import threading
import typing
import weakref

import numpy as np

from . import ffi
from .hparams import GlowHParams, HifiGanHParams
from .weights import build_blob


class MelBatch:
    """Device-resident mel batch handed from GlowTTS to HiFi-GAN without a host
    round trip (the reference crosses host<->runtime twice per sentence,
    `larynx/__init__.py:231-256`)."""

    def __init__(self, engine: "Engine", handle: int, durations_ld: int = 0):
        self._engine = engine
        self._h = C.c_void_p(handle)
        self._durations: typing.Optional[np.ndarray] = None  # fetched on first use
        self._durations_ld = int(durations_ld)
        engine._live_mels.add(self)
        lib = engine.lib
        self.batch = ffi.check(lib, lib.mi355tts_mel_batch(self._h))
        self.channels = ffi.check(lib, lib.mi355tts_mel_channels(self._h))
        self.max_frames = ffi.check(lib, lib.mi355tts_mel_max_frames(self._h))
        fr = (C.c_int32 * self.batch)()
        ffi.check(lib, lib.mi355tts_mel_frames(self._h, fr))
        self.frames = np.array(fr[:], dtype=np.int32)

    @property
    def handle(self) -> C.c_void_p:
        if self._h is None:
            raise ValueError("mel batch already freed")
        return self._h

    def numpy(self, which: str = "raw") -> np.ndarray:
        """[B, M, max_frames] float32; `which` is "raw" (GlowTTS output) or
        "vocoder" (after the AudioSettings transforms)."""
        out = np.zeros((self.batch, self.channels, self.max_frames), np.float32)
        if self.max_frames:
            lib = self._engine.lib
            ffi.check(lib, lib.mi355tts_mel_copy(self.handle, 0 if which == "raw" else 1, out.ctypes.data, self.max_frames))
        return out

    def plane(self, which: str = "raw") -> typing.Tuple[int, int]:
        """(device pointer, leading dimension) of a plane, [B][M][ld] float32 (`mi355tts_mel_plane`): valid until `free`."""
        p, ld = C.c_void_p(), C.c_int()
        lib = self._engine.lib
        ffi.check(lib, lib.mi355tts_mel_plane(self.handle, 0 if which == "raw" else 1, C.byref(p), C.byref(ld)))
        return int(p.value or 0), int(ld.value)

    @property
    def shape(self):
        return (self.batch, self.channels, self.max_frames)

    @property
    def durations(self) -> np.ndarray:
        """[B, P] int32: the mel frames every phoneme id occupies (the reference's `attn.sum(-1)`,
        glow_tts/models.py:350-354), zeros past a row's length; row b sums to `frames[b]`.  Only a mel made with
        `want_durations`, `id_scales` or `durations` carries them: anything else (a wrapped array) raises ValueError."""
        if self._durations is None:
            P = self._durations_ld
            out = np.zeros((self.batch, max(P, 1)), np.int32)
            lib = self._engine.lib
            if lib.mi355tts_mel_durations(self.handle, ffi.i32p(out), out.shape[1]) < 0:
                raise ValueError("this mel batch carries no durations (ask for them: want_durations=True)")
            self._durations = out[:, :P]
        return self._durations

    def __array__(self, dtype=None, copy=None):
        a = self.numpy("raw")
        return a if dtype is None else a.astype(dtype)

    def free(self):
        """Return the device blocks to the engine's pool.  A mel must not outlive its
        context: `Engine.close()` frees whatever is still alive first."""
        if self._h is not None:
            h, self._h = self._h, None
            if self._engine._ctx is not None:
                self._engine.lib.mi355tts_mel_free(h)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    def __init__(self, device: int = 0, library_path=None):
        self.lib = ffi.load_library(library_path)
        self.device = device
        h = C.c_void_p()
        ffi.check(self.lib, self.lib.mi355tts_create(device, C.byref(h)))
        self._ctx = h
        self._lock = threading.Lock()
        self._hops: typing.Dict[int, int] = {}
        self._live_mels: "weakref.WeakSet[MelBatch]" = weakref.WeakSet()
        self._kept: dict = {}
        self._kept_lock = threading.RLock()

    def kept(self, kind: str, key, make):
        """One object per (engine, kind, key), made by `make()` on first use and kept ON the engine: it lives and dies with
        the context its model id belongs to (`get_resampler`, `get_loudness`, `get_limiter`)."""
        with self._kept_lock:
            if (kind, key) not in self._kept:
                self._kept[kind, key] = make()
            return self._kept[kind, key]

    def close(self):
        if self._ctx is not None:
            for m in list(self._live_mels):  # their device blocks belong to this context
                m.free()
            self.lib.mi355tts_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights -----------------------------------------------------------
    def glow_blob(self, hp: GlowHParams, state_dict) -> np.ndarray:
        return build_blob(ffi.manifest(self.lib, ffi.glow_hparams_c(hp)), state_dict)

    def hifigan_blob(self, hp: HifiGanHParams, state_dict) -> np.ndarray:
        return build_blob(ffi.manifest(self.lib, ffi.hifigan_hparams_c(hp)), state_dict)

    def load_glow(self, hp: GlowHParams, state_dict=None, blob=None, device_ptr: int = 0) -> int:
        """Load from a reference state-dict, a prebuilt host blob, or a device
        pointer holding the blob (the receive side of the RCCL weight broadcast)."""
        hp_c = ffi.glow_hparams_c(hp)
        return self._load(self.lib.mi355tts_load_glow, hp_c, state_dict, blob, device_ptr)

    def load_hifigan(self, hp: HifiGanHParams, state_dict=None, blob=None, device_ptr: int = 0) -> int:
        hp_c = ffi.hifigan_hparams_c(hp)
        return self._load(self.lib.mi355tts_load_hifigan, hp_c, state_dict, blob, device_ptr)

    def _load(self, fn, hp_c, state_dict, blob, device_ptr) -> int:
        man = ffi.manifest(self.lib, hp_c)
        total = sum(n for _, n in man)
        if device_ptr:
            return self._loaded(fn, C.byref(hp_c), C.c_void_p(device_ptr), total, 1)
        if blob is None:
            blob = build_blob(man, state_dict)
        blob = np.ascontiguousarray(blob, np.float32)
        if blob.size != total:
            raise ValueError(f"blob has {blob.size} floats, model needs {total}")
        return self._loaded(fn, C.byref(hp_c), blob.ctypes.data, total, 0)

    def _loaded(self, fn, *args) -> int:
        """The tail of every load: `fn(ctx, *args, &model)` -> the new model's id."""
        model = C.c_int()
        ffi.check(self.lib, fn(self._ctx, *args, C.byref(model)))
        return int(model.value)

    def broadcast_weights(self, nccl_comm: int, root: int, device_ptr: int, numel: int, rccl_library: typing.Optional[str] = None):
        """`mi355tts_broadcast_weights`: ncclBroadcast of a device-resident weight blob over the caller's RCCL
        communicator (an `ncclComm_t` as an integer), in place."""
        lib_name = rccl_library.encode() if rccl_library else None
        ffi.check(self.lib, self.lib.mi355tts_broadcast_weights(self._ctx, C.c_void_p(nccl_comm), int(root), C.c_void_p(device_ptr),
                                                                int(numel), lib_name))

    def set_precision(self, model: int, precision: int):
        """`ffi.PRECISION_F32` (exact, default), `ffi.PRECISION_F16` (the reference's `half` switch: native fp16 vocoder; on a
        GlowTTS model the decoder's WaveNets in fp16) or `ffi.PRECISION_BF16X3` (split-bf16, f32-class accuracy; vocoder only).
        Returns the library's status: 0, or `ffi.PRECISION_NOOP` when the request has no effect on this GlowTTS model (it keeps
        computing in f32).  Raises when fp16 does not cover the vocoder's geometry."""
        return ffi.check(self.lib, self.lib.mi355tts_model_set_precision(self._ctx, int(model), int(precision)))

    def unload(self, model: int):
        ffi.check(self.lib, self.lib.mi355tts_unload(self._ctx, model))

    # ---- inference -----------------------------------------------------------
    def glow_infer(
        self,
        model: int,
        ids: typing.Union[np.ndarray, typing.Sequence[np.ndarray]],
        noise_scale: float = 0.667,
        length_scale: float = 1.0,
        noise: typing.Optional[np.ndarray] = None,
        seed: int = 0,
        audio_settings=None,
        row_seeds: typing.Optional[typing.Sequence[int]] = None,
        speaker_ids: typing.Union[None, int, typing.Sequence[int]] = None,
        id_scales=None,
        durations=None,
        want_durations: bool = False,
    ) -> MelBatch:
        """`ids`: one int64 vector [P] or a list of them (variable length batch).
        `speaker_ids`: a multi-speaker voice's speaker per row (one int = every row; the reference's `speaker_id`
        setting, larynx/glow_tts.py:116-130) — required there, an error for a single-speaker voice.
        `noise`: optional [B, M, >=F] (or [M, >=F] for B=1) standing in for the
        reference's `torch.randn_like` draw.  Without it the device generator draws: row b from
        the stream `row_seeds[b]` (default `seed + b`: successive BATCHED calls must advance `seed` by the batch size)
        — the field a batch-1 call with that seed draws.
        `id_scales`: a duration factor per id ([P] floats, or one vector per row): `ceil(exp(logw) * length_scale * scale)`;
        1.0 changes nothing, 0 gives the id no frames.  `durations`: the frames per id outright ([P] ints or one vector
        per row), instead of the duration predictor's.  Either of them, or `want_durations`, makes `MelBatch.durations`
        available."""
        packed, lens, B, ld = self._ids_in(ids)
        noise, nz_ptr, nz_ld = self._noise_in(noise, B)
        if row_seeds is not None and (noise is not None or len(row_seeds) != B):
            raise ValueError("row_seeds: one seed per row, and no explicit noise")
        rs = None if row_seeds is None else np.array([ffi.u64(x) for x in row_seeds], np.uint64)
        pros = keep = None
        if id_scales is not None or durations is not None or want_durations:
            pros, keep = self._prosody(lens, ld, id_scales, durations, False)
        spk = self._speaker_array(speaker_ids, B) if speaker_ids is not None else None
        out = C.c_void_p()
        head = self._glow_head((model,), packed.ctypes.data, lens, ld, noise_scale, length_scale, nz_ptr, nz_ld, seed)
        ffi.check(self.lib, self._glow_call("mi355tts_glow_infer", head, rs, spk, (ffi.audio_ref(audio_settings), 0), pros, (C.byref(out),)))
        del keep
        return MelBatch(self, out.value, durations_ld=ld if pros is not None else 0)

    @staticmethod
    def _ids_in(ids):
        """The phoneme ids of a call, one int64 vector [P] or a sequence of them (the rows of a 2-D array among them), as the
        library takes them -> (packed int64 [B, ld] with zeros behind a row's ids, lens int32 [B], B, ld = max(longest row, 1)).
        No rows, or a row without ids, is the library's to refuse."""
        rows = [np.asarray(ids, np.int64)] if isinstance(ids, np.ndarray) and ids.ndim == 1 else [np.asarray(r, np.int64) for r in ids]
        B = len(rows)
        lens = np.array([len(r) for r in rows], np.int32)
        packed = np.zeros((B, max(int(lens.max()) if B else 0, 1)), np.int64)
        for b, r in enumerate(rows):
            packed[b, : len(r)] = r
        return packed, lens, B, packed.shape[1]

    @staticmethod
    def _noise_in(noise, B: int):
        """The explicit noise of a call, [B, M, >=F] (or [M, >=F] at B = 1) or None -> (the float32 array to hold until the call
        returns, its pointer, its row stride): (None, None, 0) without noise.  A batch other than B would be read past its end."""
        if noise is None:
            return None, None, 0
        noise = np.ascontiguousarray(noise, np.float32)
        if noise.ndim == 2:
            noise = noise[None]
        if noise.shape[0] != B:
            raise ValueError("noise batch mismatch")
        return noise, noise.ctypes.data, noise.shape[2]

    def _glow_head(self, models, ids_ptr, lens: np.ndarray, ids_ld, noise_scale, length_scale, noise_ptr, noise_ld, seed) -> tuple:
        """The arguments every GlowTTS entry point starts with, context to seed; `models`: (glow,) or (glow, vocoder)."""
        return (self._ctx, *models, ids_ptr, ffi.i32p(lens), len(lens), ids_ld, float(noise_scale), float(length_scale), noise_ptr,
                noise_ld, ffi.u64(seed))

    def _glow_call(self, stem: str, head: tuple, rs, spk, tail: tuple, pros, last: tuple = ()) -> int:
        """Calls the entry point of the family `stem` ("mi355tts_glow_infer" / "mi355tts_synthesize") that the arguments given
        select, the narrowest that takes them: `_prosody` with `pros`, else `_speakers` with `spk`, else `_rows` with `rs`
        (row seeds: `glow_infer`'s family alone takes them), else the plain one.  `head`: `_glow_head`'s; `tail`: from the audio
        settings to the flags; `last`: what follows the prosody.  -> the library's status."""
        seeds = (ffi.u64p(rs),) if stem == "mi355tts_glow_infer" else ()
        if pros is not None:
            return getattr(self.lib, stem + "_prosody")(*head, *seeds, ffi.i32p(spk), *tail, C.byref(pros), *last)
        if spk is not None:
            return getattr(self.lib, stem + "_speakers")(*head, *seeds, ffi.i32p(spk), *tail, *last)
        if rs is not None:  # (no noise pointer, stride or seed: the rows' seeds stand for all three)
            return self.lib.mi355tts_glow_infer_rows(*head[:-3], *seeds, *tail, *last)
        return getattr(self.lib, stem)(*head, *tail, *last)

    def glow_infer_taps(self, model: int, ids, noise_scale: float = 0.667, length_scale: float = 1.0, noise=None, seed: int = 0,
                        speaker_ids=None, durations=None):
        """Test seam (`mi355tts_glow_infer_taps` + `mi355tts_voc_tap_copy`): one GlowTTS call with `glow_infer`'s arguments ->
        (MelBatch, taps).  `taps` lists, in launch order, every f32 plane the schedule wrote to memory: dicts with "name",
        "channels", "ld", "len" (valid columns per row), "f16" (0), "kernel" (the name the launch was counted under, "-" for
        none) and "x", the plane as float32 [B, channels, ld]."""
        packed, lens, B, ld = self._ids_in(ids)
        noise, nz_ptr, nz_ld = self._noise_in(noise, B)
        pros, keep = self._prosody(lens, ld, None, durations, False)
        spk = self._speaker_array(speaker_ids, B) if speaker_ids is not None else None
        out = C.c_void_p()
        cap = 1 << 20
        buf = C.create_string_buffer(cap)
        head = self._glow_head((model,), packed.ctypes.data, lens, ld, noise_scale, length_scale, nz_ptr, nz_ld, seed)
        ffi.check(self.lib, self.lib.mi355tts_glow_infer_taps(*head, None, ffi.i32p(spk), None, 0, C.byref(pros), C.byref(out), buf, cap))
        del keep
        return MelBatch(self, out.value, durations_ld=ld), self._taps_out(buf, B)

    def _taps_out(self, buf, B: int) -> list:
        """The tap list a `*_infer_taps` call left in `buf`, every entry with its plane "x" (`mi355tts_voc_tap_copy`)."""
        taps = json.loads(buf.value.decode("ascii"))
        for i, t in enumerate(taps):
            x = np.empty((B, t["channels"], t["ld"]), np.float32)
            ffi.check(self.lib, self.lib.mi355tts_voc_tap_copy(self._ctx, i, ffi.ptr(x), x.size))
            t["x"] = x
        return taps

    def glow_align(self, model: int, ids, mel, frames=None, speaker_ids: typing.Union[None, int, typing.Sequence[int]] = None,
                   want_latent: bool = False):
        """Forced alignment (`mi355tts_glow_align`): which frames of `mel` belong to which phoneme id.  `ids` as in
        `glow_infer`; `mel`: a `MelBatch` (its raw plane, read on the device, and its frame counts) or an array [B, M, F] / [M, F] in the GlowTTS output
        domain with `frames` valid columns per row (default: all).  Returns (durations int32 [B, P] — frames per id, zeros past
        a row's length, each row summing to its frame count cut down to a multiple of n_sqz —, scores float32 [B]) and, with
        `want_latent`, the latent z [B, M, F] as a third item.  Feed a row's durations to `glow_infer(durations=...)` to put
        this mel's timing onto another take."""
        packed, lens, B, ld = self._ids_in(ids)
        flags = 0
        if isinstance(mel, MelBatch):  # its raw plane where it lies: no host round trip
            if mel.batch != B or mel.max_frames < 1:
                raise ValueError("mel: one non-empty row per id sequence")
            if frames is None:
                frames = mel.frames
            mel_ptr, mel_ld = mel.plane("raw")
            shape, z_frames = (B, mel.channels, mel_ld), mel.max_frames
            flags = ffi.IN_DEVICE
        else:
            mel = np.ascontiguousarray(mel, np.float32)
            if mel.ndim == 2:
                mel = mel[None]
            if mel.ndim != 3 or mel.shape[0] != B or mel.shape[2] < 1:
                raise ValueError("mel: [B, M, F] with one row per id sequence")
            mel_ptr, mel_ld, shape, z_frames = mel.ctypes.data, mel.shape[2], mel.shape, mel.shape[2]
        fr = np.full(B, mel_ld, np.int32) if frames is None else np.ascontiguousarray(np.asarray(frames, np.int32).reshape(-1))
        if fr.shape != (B,):
            raise ValueError("frames: one count per row")
        spk = self._speaker_array(speaker_ids, B) if speaker_ids is not None else None
        dur = np.zeros((B, ld), np.int32)
        score = np.zeros(B, np.float32)
        z = np.zeros(shape, np.float32) if want_latent else None
        ffi.check(
            self.lib,
            self.lib.mi355tts_glow_align(
                self._ctx, model, packed.ctypes.data, ffi.i32p(lens), B, ld, mel_ptr, ffi.i32p(fr), mel_ld, ffi.i32p(spk),
                flags, ffi.i32p(dur), ld, ffi.f32p(score), ffi.ptr(z),
            ),
        )
        return (dur, score, z[:, :, :z_frames]) if want_latent else (dur, score)

    def maximum_path(self, value: np.ndarray, id_lens=None, frames=None):
        """`mi355tts_op_maximum_path`: the reference's `maximum_path` (glow_tts/utils.py:59-96) on `value` [B, P, F] (or [P, F]),
        rows `id_lens[b]` x `frames[b]` -> (durations int32 [B, P], scores float32 [B])."""
        value = np.ascontiguousarray(value, np.float32)
        if value.ndim == 2:
            value = value[None]
        B, P, F = value.shape
        pl = np.full(B, P, np.int32) if id_lens is None else np.ascontiguousarray(id_lens, np.int32)
        fr = np.full(B, F, np.int32) if frames is None else np.ascontiguousarray(frames, np.int32)
        dur = np.zeros((B, P), np.int32)
        score = np.zeros(B, np.float32)
        ffi.check(self.lib, self.lib.mi355tts_op_maximum_path(self._ctx, value.ctypes.data, B, P, F, ffi.i32p(pl), ffi.i32p(fr),
                                                             ffi.i32p(dur), P, ffi.f32p(score)))
        return dur, score

    @staticmethod
    def _prosody(lens: np.ndarray, ld: int, id_scales, durations, want_out: bool):
        """The `mi355tts_prosody` of a call and the arrays it points into (keep them alive until the call returns;
        the last one is the durations_out array or None)."""
        B = len(lens)

        def pack(v, dtype, name):
            if v is None:
                return None
            rows = [np.asarray(v, dtype)] if B == 1 and np.ndim(v[0]) == 0 else [np.asarray(r, dtype) for r in v]
            if len(rows) != B or any(r.ndim != 1 or len(r) != n for r, n in zip(rows, lens)):
                raise ValueError(f"{name}: one value per phoneme id of every row")
            out = np.zeros((B, ld), dtype)
            for b, r in enumerate(rows):
                out[b, : len(r)] = r
            return out

        sc = pack(id_scales, np.float32, "id_scales")
        din = pack(durations, np.int32, "durations")
        dout = np.zeros((B, ld), np.int32) if want_out else None
        p = ffi.ProsodyC()
        p.id_scales = ffi.f32p(sc)
        p.durations_in = ffi.i32p(din)
        p.durations_out = ffi.i32p(dout)
        p.ld = ld
        return p, (sc, din, dout)

    @staticmethod
    def _speaker_array(speaker_ids, B: int) -> np.ndarray:
        spk = np.full(B, int(speaker_ids), np.int32) if np.isscalar(speaker_ids) else np.asarray(list(speaker_ids), np.int32)
        if spk.shape != (B,):
            raise ValueError("speaker_ids: one speaker per row")
        return np.ascontiguousarray(spk)

    def glow_infer_raw(self, model, ids_ptr, lens, ids_ld, noise_scale, length_scale, noise_ptr=None, noise_ld=0,
                       seed=0, audio_settings=None, flags=0) -> MelBatch:
        """Pointer-level entry (ids/noise may be device memory with flags=ffi.IN_DEVICE)."""
        lens = np.ascontiguousarray(lens, np.int32)
        out = C.c_void_p()
        head = self._glow_head((model,), ids_ptr, lens, ids_ld, noise_scale, length_scale, noise_ptr, noise_ld, seed)
        ffi.check(self.lib, self.lib.mi355tts_glow_infer(*head, ffi.audio_ref(audio_settings), flags, C.byref(out)))
        return MelBatch(self, out.value)

    def hifigan_infer_raw(self, vocoder, mel: MelBatch, f32_ptr, i16_ptr, wav_ld, flags=0, denoiser_strength=0.0,
                          pad_before=0, pad_after=0):
        ffi.check(self.lib, self.lib.mi355tts_hifigan_infer_padded(self._ctx, vocoder, mel.handle, float(denoiser_strength),
                                                                  f32_ptr, i16_ptr, wav_ld, flags, int(pad_before), int(pad_after)))

    def synthesize_raw(self, glow, vocoder, ids_ptr, lens, ids_ld, noise_scale, length_scale, f32_ptr, i16_ptr, wav_ld,
                       noise_ptr=None, noise_ld=0, seed=0, audio_settings=None, denoiser_strength=0.0, pad_before=0,
                       pad_after=0, flags=0) -> np.ndarray:
        """Pointer-level fused call (`mi355tts_synthesize`); returns the per-row mel frame counts."""
        lens = np.ascontiguousarray(lens, np.int32)
        frames = np.zeros(len(lens), np.int32)
        head = self._glow_head((glow, vocoder), ids_ptr, lens, ids_ld, noise_scale, length_scale, noise_ptr, noise_ld, seed)
        ffi.check(
            self.lib,
            self.lib.mi355tts_synthesize(*head, ffi.audio_ref(audio_settings), float(denoiser_strength), int(pad_before), int(pad_after),
                                         ffi.i32p(frames), f32_ptr, i16_ptr, wav_ld, flags),
        )
        return frames

    def synthesize(self, glow: int, vocoder: int, ids, noise_scale: float = 0.667, length_scale: float = 1.0,
                   noise: typing.Optional[np.ndarray] = None, seed: int = 0, audio_settings=None,
                   denoiser_strength: float = 0.0, pad_before: int = 0, pad_after: int = 0, want_float: bool = False,
                   frames_per_id_guess: float = 8.0, speaker_ids: typing.Union[None, int, typing.Sequence[int]] = None,
                   id_scales=None, durations=None, return_durations: bool = False):
        """ids -> (frames [B], wav_f32 [B, n] or None, wav_i16 [B, n]) through ONE fused call; with `return_durations` a
        fourth item, the frames per phoneme id [B, P] int32 (see `glow_infer` for `id_scales` / `durations`)
        (`mi355tts_synthesize`): row b holds pad_before zeros, frames[b]*hop samples, then zeros.
        The frame count is data dependent; the output buffer is sized from a guess and the call
        is repeated once with the exact size in the rare case the guess was too small."""
        packed, lens, B, ld = self._ids_in(ids)
        noise, nz_ptr, nz_ld = self._noise_in(noise, B)
        hop = self.hop(vocoder)
        pads = int(pad_before) + int(pad_after)
        cap = int(ld * frames_per_id_guess * max(length_scale, 0.05)) * hop + pads
        pros = keep = None
        if id_scales is not None or durations is not None or return_durations:
            pros, keep = self._prosody(lens, ld, id_scales, durations, return_durations)
            if durations is not None:  # the frame count is known: no guessing
                cap = max(int(keep[1].sum(axis=1).max(initial=0)), 1) * hop + pads
        a = ffi.audio_ref(audio_settings)
        frames = np.zeros(B, np.int32)
        spk = self._speaker_array(speaker_ids, B) if speaker_ids is not None else None
        head = self._glow_head((glow, vocoder), packed.ctypes.data, lens, ld, noise_scale, length_scale, nz_ptr, nz_ld, seed)
        for attempt in range(2):
            f32 = np.empty((B, cap), np.float32) if want_float else None
            i16 = np.empty((B, cap), np.int16)
            tail = (a, float(denoiser_strength), int(pad_before), int(pad_after), ffi.i32p(frames), ffi.ptr(f32), i16.ctypes.data, cap, 0)
            rc = self._glow_call("mi355tts_synthesize", head, None, spk, tail, pros)
            n = int(frames.max(initial=0)) * hop + pads  # (no rows: the library has refused, `check` below says why)
            if rc == -4 and attempt == 0 and n > cap:  # MI355TTS_ERR_TOO_SMALL: frames_out holds the real counts
                cap = n
                continue
            ffi.check(self.lib, rc)
            res = (frames, (f32[:, :n] if f32 is not None else None), i16[:, :n])
            return res + (keep[2],) if return_durations else res
        raise AssertionError("unreachable")

    def reserve(self, workers: int, glow: int = 0, vocoder: int = 0, max_batch: int = 1, max_ids: int = 256,
                max_frames: int = 2048, denoiser: bool = False, max_pad_samples: int = 0):
        """Pre-create per-call workers and size every workspace (`mi355tts_reserve`)."""
        ffi.check(self.lib, self.lib.mi355tts_reserve(self._ctx, int(workers), int(glow), int(vocoder), int(max_batch), int(max_ids),
                                                     int(max_frames), 1 if denoiser else 0, int(max_pad_samples)))

    def ensure_workers(self, n: int):
        """At least `n` per-call workers exist and their streams' hardware queues are known (`mi355tts_reserve` without models: it
        creates the workers, measures which of their streams share a hardware queue — calls are then spread evenly over the queues —
        and leaves the workspaces to grow on first use).  Idempotent; the hosts of a sentence thread pool call it with the pool's
        size + 1 (larynx/__init__.py:146-157: one `_sentence_task` per pool thread)."""
        n = max(1, min(int(n), 64))
        if n > getattr(self, "_ensured_workers", 0):
            self.reserve(n, 0, 0, max_batch=1, max_ids=1, max_frames=1)
            self._ensured_workers = n

    def worker_queue_groups(self) -> typing.List[int]:
        """The hardware-queue group of every worker, in creation order (`mi355tts_worker_queue_groups`; -1 = not probed)."""
        buf = (C.c_int32 * 256)()
        n = self.lib.mi355tts_worker_queue_groups(self._ctx, buf, 256)
        if n < 0:
            ffi.check(self.lib, n)
        return [int(buf[i]) for i in range(min(n, 256))]

    def mel_from_numpy(self, mel: np.ndarray, frames=None, audio_settings=None) -> MelBatch:
        mel = np.ascontiguousarray(mel, np.float32)
        if mel.ndim == 2:
            mel = mel[None]
        B, M, ld = mel.shape
        return self._mel_from_buffer(mel.ctypes.data, np.full(B, ld, np.int32) if frames is None else frames, B, M, ld, audio_settings, 0)

    def mel_from_device(self, device_ptr: int, frames, channels: int, ld: int, audio_settings=None) -> MelBatch:
        """Wrap a mel that already lives in device memory ([B][channels][ld] fp32, e.g. a
        torch tensor's `data_ptr()`); `frames` gives each row's valid length."""
        fr = np.ascontiguousarray(frames, np.int32)
        return self._mel_from_buffer(C.c_void_p(int(device_ptr)), fr, len(fr), channels, ld, audio_settings, ffi.IN_DEVICE)

    def _mel_from_buffer(self, mel_ptr, frames, B: int, channels: int, ld: int, audio_settings, flags: int) -> MelBatch:
        fr = np.ascontiguousarray(frames, np.int32)
        out = C.c_void_p()
        ffi.check(self.lib, self.lib.mi355tts_mel_from_buffer(self._ctx, mel_ptr, ffi.i32p(fr), int(B), int(channels), int(ld),
                                                             ffi.audio_ref(audio_settings), flags, C.byref(out)))
        return MelBatch(self, out.value)

    def hop(self, vocoder: int) -> int:
        if vocoder not in self._hops:
            self._hops[vocoder] = ffi.check(self.lib, self.lib.mi355tts_hifigan_hop(self._ctx, vocoder))
        return self._hops[vocoder]

    def hifigan_infer(self, vocoder: int, mel: MelBatch, want_float: bool = True, want_int16: bool = True,
                      denoiser_strength: float = 0.0, pad_before: int = 0, pad_after: int = 0):
        """Returns (wav_f32 [B, N] or None, wav_i16 [B, N] or None), N = pad_before + max_frames*hop + pad_after;
        row b holds pad_before zeros, frames[b]*hop samples, then zeros (the SSML pauses of
        `larynx/__init__.py:277-283`, written by the int16 kernel instead of np.pad)."""
        n = mel.max_frames * self.hop(vocoder) + int(pad_before) + int(pad_after)
        f32 = np.empty((mel.batch, n), np.float32) if want_float else None
        i16 = np.empty((mel.batch, n), np.int16) if want_int16 else None
        ffi.check(
            self.lib,
            self.lib.mi355tts_hifigan_infer_padded(self._ctx, vocoder, mel.handle, float(denoiser_strength), ffi.ptr(f32),
                                                   ffi.ptr(i16), n, 0, int(pad_before), int(pad_after)),
        )
        return f32, i16

    def hifigan_infer_taps(self, vocoder: int, mel: MelBatch):
        """Test seam (`mi355tts_hifigan_infer_taps` + `mi355tts_voc_tap_copy`): one vocoder call without the denoiser ->
        (wav_f32 [B, N], taps).  `taps` lists, in launch order, every activation plane the schedule wrote to memory: dicts with
        "name", "channels", "ld", "len" (valid columns per row), "f16", "kernel" (the name the launch was counted under) and
        "x", the plane as float32 [B, channels, ld] (fp16 planes widened: exact)."""
        n = mel.max_frames * self.hop(vocoder)
        f32 = np.empty((mel.batch, n), np.float32)
        buf = C.create_string_buffer(1 << 16)
        ffi.check(self.lib, self.lib.mi355tts_hifigan_infer_taps(self._ctx, vocoder, mel.handle, ffi.ptr(f32), n, buf, 1 << 16))
        return f32, self._taps_out(buf, mel.batch)

    # ---- Griffin-Lim -----------------------------------------------------------
    def load_griffin_lim(self, mel_basis: np.ndarray, mel_scaling: float = 1000.0, iterations: int = 60) -> int:
        """`mi355tts_load_griffin_lim`: the weight-free vocoder (`larynx/griffin_lim.py:22-38`); `mel_basis` is
        [num_mels, 513] (`larynx_amd.audio.mel_basis`).  `unload` frees it."""
        basis = np.ascontiguousarray(mel_basis, np.float32)
        if basis.ndim != 2 or basis.shape[1] != 513:
            raise ValueError(f"mel_basis must be [num_mels, 513] (1024-point frames), got {basis.shape}")
        p = ffi.GriffinLimParamsC(int(basis.shape[0]), float(mel_scaling), int(iterations))
        return self._loaded(self.lib.mi355tts_load_griffin_lim, C.byref(p), basis.ctypes.data)

    def griffin_lim_infer(self, model: int, mel: MelBatch, phase0: typing.Optional[np.ndarray] = None, seed: int = 0,
                          iterations: int = 0, want_float: bool = True, want_int16: bool = False, want_phase: bool = False):
        """Returns (wav_f32 [B, N] or None, wav_i16 [B, N] or None, phase [B, 513, T] or None), T = max_frames - 1 and
        N = T * 256 + 1024 (0 when T = 0); row b holds (frames[b] - 1) * 256 + 1024 samples, then zeros.  `phase0`
        ([B, 513, T] or [513, T]) stands in for the reference's `np.random.rand` draw; without it the device draws from
        `seed` (row b: seed + b).  `iterations` <= 0: the model's."""
        T = max(mel.max_frames - 1, 0)
        n = T * 256 + 1024 if T else 0
        B = mel.batch
        if phase0 is not None:
            phase0 = np.ascontiguousarray(phase0, np.float32)
            if phase0.ndim == 2:
                phase0 = phase0[None]
            if phase0.shape != (B, 513, T):
                raise ValueError(f"phase0 must be [{B}, 513, {T}], got {phase0.shape}")
        f32 = np.empty((B, n), np.float32) if want_float else None
        i16 = np.empty((B, n), np.int16) if want_int16 else None
        ph = np.empty((B, 513, T), np.float32) if want_phase else None
        ffi.check(
            self.lib,
            self.lib.mi355tts_griffin_lim_infer(self._ctx, int(model), mel.handle, ffi.ptr(phase0), ffi.u64(seed),
                                                ffi.ptr(ph), ffi.ptr(f32), ffi.ptr(i16), n, int(iterations), 0),
        )
        return f32, i16, ph

    def griffin_lim_infer_raw(self, model: int, mel: MelBatch, phase0_ptr, seed, phase_out_ptr, f32_ptr, i16_ptr, wav_ld,
                              iterations=0, flags=0):
        """Pointer-level entry (`flags`: ffi.IN_DEVICE for phase0, ffi.OUT_DEVICE for phase_out and the waveforms)."""
        ffi.check(self.lib, self.lib.mi355tts_griffin_lim_infer(self._ctx, int(model), mel.handle, phase0_ptr,
                                                                ffi.u64(seed), phase_out_ptr, f32_ptr, i16_ptr,
                                                                int(wav_ld), int(iterations), int(flags)))

    # ---- mel analysis ------------------------------------------------------------
    def load_analysis(self, mel_basis: np.ndarray, framing: typing.Union[str, int] = "hifigan",
                      mag_eps: typing.Optional[float] = None) -> int:
        """`mi355tts_load_analysis`: waveform -> mel in one launch.  `mel_basis` is [num_mels, 513]
        (`larynx_amd.audio.mel_basis`); `framing` "hifigan" (the published HiFi-GAN training convention: reflect padding,
        periodic Hann) or "reference" (the reference's own `stft`: no padding, symmetric Hann); `mag_eps` goes under the
        square root of the magnitudes (default: the framing's own, 1e-9 / 0).  `unload` frees it."""
        basis = np.ascontiguousarray(mel_basis, np.float32)
        if basis.ndim != 2 or basis.shape[1] != 513:
            raise ValueError(f"mel_basis must be [num_mels, 513] (1024-point frames), got {basis.shape}")
        fr = ffi.FRAMINGS[framing] if isinstance(framing, str) else int(framing)
        if mag_eps is None:
            mag_eps = 1e-9 if fr == ffi.FRAMING_HIFIGAN else 0.0
        p = ffi.AnalysisParamsC(int(basis.shape[0]), fr, float(mag_eps))
        return self._loaded(self.lib.mi355tts_load_analysis, C.byref(p), basis.ctypes.data)

    # ---- audio in, rows out ---------------------------------------------------------
    @staticmethod
    def _audio_in(audio, samples):
        """What every call that reads audio does with it: float32 (any other type is converted) or int16, [N] or [B, N], and
        `samples` (default: all N of every row) -> (the [B, N] contiguous array, whether it was 1-D, B, N, samples int64 [B],
        the float32 pointer, the int16 pointer): exactly one pointer is set.  The pointers hold while the array is held."""
        audio = np.asarray(audio)
        if audio.dtype != np.int16:
            audio = audio.astype(np.float32, copy=False)
        audio = np.ascontiguousarray(audio)
        flat = audio.ndim == 1
        if flat:
            audio = audio[None]
        if audio.ndim != 2:
            raise ValueError("audio: [N] or [B, N]")
        B, N = audio.shape
        n = np.full(B, N, np.int64) if samples is None else Engine._samples(samples)
        if n.shape != (B,):
            raise ValueError("samples: one count per row")
        if N == 0:  # (an empty array has no address worth passing: one sample nobody reads stands in)
            audio = np.zeros((B, 1), audio.dtype)
        ptr = audio.ctypes.data
        return (audio, flat, B, N, n, None, ptr) if audio.dtype == np.int16 else (audio, flat, B, N, n, ptr, None)

    @staticmethod
    def _samples(samples) -> np.ndarray:
        """The rows' sample counts as every call that reads audio hands them to the library: int64 [B], contiguous."""
        return np.ascontiguousarray(np.asarray(samples, np.int64).reshape(-1))

    @staticmethod
    def _rows_out(flat: bool, *rows):
        """[B, N] output arrays (or None) in the shape of the call's audio: row 0 alone for a 1-D input."""
        return tuple(None if r is None else r[0] for r in rows) if flat else rows

    def mel_from_audio(self, model: int, audio: np.ndarray, samples=None, audio_settings=None) -> MelBatch:
        """`audio`: float32 (in [-1, 1]) or int16, [N] or [B, N], row b valid for `samples[b]` entries (default: all) -> the
        `MelBatch` of the recording: plane "vocoder" feeds `hifigan_infer` / `griffin_lim_infer`, plane "raw" is the
        GlowTTS domain `glow_align` expects.  `audio_settings` as everywhere; None leaves ln(max(amp, 1e-5)) in both."""
        audio, _, _, N, n, f_in, i_in = self._audio_in(audio, samples)
        return self.mel_from_audio_raw(model, f_in, i_in, n, N, audio_settings)

    def mel_from_audio_raw(self, model: int, f32_ptr, i16_ptr, samples, wav_ld: int, audio_settings=None, flags: int = 0) -> MelBatch:
        """Pointer-level entry: exactly one of the two pointers, [B][wav_ld] (device memory with flags=ffi.IN_DEVICE)."""
        n = self._samples(samples)
        out = C.c_void_p()
        ffi.check(
            self.lib,
            self.lib.mi355tts_mel_from_audio(self._ctx, int(model), f32_ptr, i16_ptr, ffi.i64p(n), len(n),
                                             int(wav_ld), ffi.audio_ref(audio_settings), int(flags), C.byref(out)),
        )
        return MelBatch(self, out.value)

    # ---- resampling ----------------------------------------------------------------
    def load_resampler(self, taps: np.ndarray, up: int, down: int) -> int:
        """`mi355tts_load_resampler`: rational resampling by `up / down` (coprime) with the symmetric prototype `taps`
        [2 H + 1] given at the up-sampled rate (`larynx_amd.resample.design_lowpass`).  `unload` frees it."""
        taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        if len(taps) % 2 != 1:
            raise ValueError(f"taps must be [2 H + 1] (a symmetric prototype around its centre), got {len(taps)}")
        p = ffi.ResamplerParamsC(int(up), int(down), len(taps) // 2)
        return self._loaded(self.lib.mi355tts_load_resampler, C.byref(p), taps.ctypes.data)

    def resample_length(self, model: int, samples: int) -> int:
        """`mi355tts_resample_length`: ceil(samples * up / down)."""
        return int(ffi.check(self.lib, self.lib.mi355tts_resample_length(self._ctx, int(model), int(samples))))

    def resample(self, model: int, audio: np.ndarray, samples=None, want_float: bool = True, want_int16: bool = False,
                 normalize: bool = False):
        """`audio`: float32 or int16 (read as s / 32768), [N] or [B, N], row b valid for `samples[b]` entries (default: all) ->
        (f32 or None, i16 or None, samples_out int64 [B]); outputs are [B, max N_out] ([N_out] for a 1-D input), rows
        zero-filled behind their N_out = ceil(N * up / down).  int16: `normalize=False` saturates
        clamp(rint(y * 32768)); `normalize=True` is the reference's `audio_float_to_int16` on each resampled row."""
        audio, flat, B, N, n, f_in, i_in = self._audio_in(audio, samples)
        if not (want_float or want_int16):
            raise ValueError("nothing asked for: want_float and / or want_int16")
        ld = max([self.resample_length(model, int(v)) for v in n if 0 <= v <= N] or [0])
        f32 = np.empty((B, ld), np.float32) if want_float else None
        i16 = np.empty((B, ld), np.int16) if want_int16 else None
        out = self.resample_raw(model, f_in, i_in, n, N, ffi.ptr(f32), ffi.ptr(i16), ld,
                                ffi.PCM_NORMALIZE if normalize else ffi.PCM_SATURATE)
        return (*self._rows_out(flat, f32, i16), out)

    def resample_raw(self, model: int, f32_ptr, i16_ptr, samples, in_ld: int, out_f32_ptr, out_i16_ptr, out_ld: int,
                     pcm_mode: int = 0, flags: int = 0) -> np.ndarray:
        """Pointer-level entry: exactly one input pointer [B][in_ld] (device memory with ffi.IN_DEVICE), at least one output
        pointer [B][out_ld] (device memory with ffi.OUT_DEVICE); returns the rows' output lengths, int64 [B]."""
        n = self._samples(samples)
        out = np.zeros(len(n), np.int64)
        ffi.check(
            self.lib,
            self.lib.mi355tts_resample(self._ctx, int(model), f32_ptr, i16_ptr, ffi.i64p(n), len(n), int(in_ld),
                                       out_f32_ptr, out_i16_ptr, int(out_ld), int(pcm_mode),
                                       ffi.i64p(out), int(flags)),
        )
        return out

    # ---- loudness ------------------------------------------------------------------
    def load_loudness(self, shelf_b, shelf_a, hp_b, hp_a, block: int, hop: int) -> int:
        """`mi355tts_load_loudness`: a BS.1770 meter from its K-weighting (two biquads: b0 b1 b2 and a1 a2 each, a0 = 1), its
        block and its hop in samples (`larynx_amd.loudness.k_weighting`).  `unload` frees it."""
        p = ffi.LoudnessParamsC()
        for name, vals, n in (("shelf_b", shelf_b, 3), ("shelf_a", shelf_a, 2), ("hp_b", hp_b, 3), ("hp_a", hp_a, 2)):
            vals = np.asarray(vals, np.float32).reshape(-1)
            if vals.shape != (n,):
                raise ValueError(f"{name}: {n} coefficients")
            setattr(p, name, (C.c_float * n)(*vals.tolist()))
        p.block, p.hop = int(block), int(hop)
        return self._loaded(self.lib.mi355tts_load_loudness, C.byref(p))

    def loudness(self, model: int, audio: np.ndarray, samples=None, target: float = float("nan"), ceiling: float = 1.0,
                 max_gain_db: float = 30.0, want_float: bool = False, want_int16: bool = False, want_weighted: bool = False) -> dict:
        """`audio`: float32 or int16 (read as s / 32768), [N] or [B, N], row b valid for `samples[b]` entries (default: all) ->
        {"lufs", "gain", "peak": float32 [B]; "f32", "i16", "weighted": [B, N] or None}.  `target` NaN measures only (gain 1);
        rows are zero-filled behind their samples.  A 1-D input gives 1-D rows (the three per-row results stay [1])."""
        audio, flat, B, N, n, f_in, i_in = self._audio_in(audio, samples)
        f32 = np.empty((B, N), np.float32) if want_float else None
        i16 = np.empty((B, N), np.int16) if want_int16 else None
        wgt = np.empty((B, N), np.float32) if want_weighted else None
        lufs, gain, peak = self.loudness_raw(model, f_in, i_in, n, N, target, ceiling, max_gain_db, ffi.ptr(f32), ffi.ptr(i16), N,
                                             ffi.ptr(wgt))
        f32, i16, wgt = self._rows_out(flat, f32, i16, wgt)
        return {"lufs": lufs, "gain": gain, "peak": peak, "f32": f32, "i16": i16, "weighted": wgt}

    def loudness_raw(self, model: int, f32_ptr, i16_ptr, samples, in_ld: int, target: float, ceiling: float, max_gain_db: float,
                     out_f32_ptr=None, out_i16_ptr=None, out_ld: int = 0, weighted_ptr=None, flags: int = 0):
        """Pointer-level entry: exactly one input pointer [B][in_ld] (device memory with ffi.IN_DEVICE); the output pointers
        [B][out_ld] and the weighted rows [B][in_ld] are optional (device memory with ffi.OUT_DEVICE); returns the rows'
        (lufs, gain, peak), float32 [B] each."""
        n = self._samples(samples)
        res = np.zeros((3, len(n)), np.float32)
        ffi.check(
            self.lib,
            self.lib.mi355tts_loudness(self._ctx, int(model), f32_ptr, i16_ptr, ffi.i64p(n), len(n), int(in_ld),
                                       float(target), float(ceiling), float(max_gain_db), out_f32_ptr, out_i16_ptr, int(out_ld),
                                       res[0].ctypes.data, res[1].ctypes.data, res[2].ctypes.data, weighted_ptr, int(flags)),
        )
        return res[0], res[1], res[2]

    # ---- limiter -------------------------------------------------------------------
    def load_limiter(self, taps, window, oversample: int, release: float) -> int:
        """`mi355tts_load_limiter`: a true-peak meter and look-ahead limiter from its interpolation prototype `taps` [2 H + 1]
        at the oversampled rate (None with `oversample` 1), its smoothing `window` [lookahead + 1] and its release, the depth's
        decay per sample (`larynx_amd.limiter`).  `unload` frees it."""
        window = np.ascontiguousarray(window, np.float32).reshape(-1)
        if len(window) < 1:
            raise ValueError("window must be [lookahead + 1]")
        half_len = 0
        if taps is not None:
            taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
            if len(taps) % 2 != 1:
                raise ValueError(f"taps must be [2 H + 1] (a symmetric prototype around its centre), got {len(taps)}")
            half_len = len(taps) // 2
        p = ffi.LimiterParamsC(int(oversample), half_len, len(window) - 1, float(release))
        return self._loaded(self.lib.mi355tts_load_limiter, C.byref(p), ffi.ptr(taps), window.ctypes.data)

    def limit(self, model: int, audio: np.ndarray, samples=None, gain=None, ceiling: float = 1.0, want_float: bool = False,
              want_int16: bool = False, want_curve: bool = False) -> dict:
        """`audio`: float32 or int16 (read as s / 32768), [N] or [B, N], row b valid for `samples[b]` entries (default: all);
        `gain`: one per row (default 1) -> {"true_peak", "min_gain": float32 [B]; "f32", "i16", "curve": [B, N] or None}.  With
        nothing asked for it is a meter call (`true_peak` of the input alone).  A 1-D input gives 1-D rows."""
        audio, flat, B, N, n, f_in, i_in = self._audio_in(audio, samples)
        g = None
        if gain is not None:
            g = np.ascontiguousarray(np.broadcast_to(np.asarray(gain, np.float32).reshape(-1), (B,)))
        f32 = np.empty((B, N), np.float32) if want_float else None
        i16 = np.empty((B, N), np.int16) if want_int16 else None
        crv = np.empty((B, N), np.float32) if want_curve else None
        tp, mg = self.limit_raw(model, f_in, i_in, n, N, g, ceiling, ffi.ptr(f32), ffi.ptr(i16), N, ffi.ptr(crv))
        f32, i16, crv = self._rows_out(flat, f32, i16, crv)
        return {"true_peak": tp, "min_gain": mg, "f32": f32, "i16": i16, "curve": crv}

    def limit_raw(self, model: int, f32_ptr, i16_ptr, samples, in_ld: int, gain, ceiling: float, out_f32_ptr=None, out_i16_ptr=None,
                  out_ld: int = 0, curve_ptr=None, flags: int = 0):
        """Pointer-level entry: exactly one input pointer [B][in_ld] (device memory with ffi.IN_DEVICE); `gain`: float32 [B] or
        None; the output pointers [B][out_ld] and the curve [B][in_ld] are optional (device memory with ffi.OUT_DEVICE); returns
        the rows' (true_peak, min_gain), float32 [B] each."""
        n = self._samples(samples)
        g = None if gain is None else np.ascontiguousarray(gain, np.float32).reshape(-1)
        if g is not None and g.shape != n.shape:
            raise ValueError("gain: one per row")
        res = np.zeros((2, len(n)), np.float32)
        ffi.check(
            self.lib,
            self.lib.mi355tts_limit(self._ctx, int(model), f32_ptr, i16_ptr, ffi.i64p(n), len(n), int(in_ld),
                                    ffi.ptr(g), float(ceiling), out_f32_ptr, out_i16_ptr, int(out_ld), res[0].ctypes.data,
                                    res[1].ctypes.data, curve_ptr, int(flags)),
        )
        return res[0], res[1]

    # ---- pitch ---------------------------------------------------------------------
    def load_pitch(self, sample_rate: int, hop: int, window: int, tau_min: int, tau_max: int, threshold: float = 0.15,
                   interpolate: bool = True) -> int:
        """`mi355tts_load_pitch`: a YIN tracker from its rate, hop, window, lag range [tau_min, tau_max], threshold on d' and
        interpolation switch (`larynx_amd.pitch.PitchTracker` derives them from a frequency range).  `unload` frees it."""
        p = ffi.PitchParamsC(int(sample_rate), int(hop), int(window), int(tau_min), int(tau_max), float(threshold), int(bool(interpolate)))
        return self._loaded(self.lib.mi355tts_load_pitch, C.byref(p))

    def pitch_frames(self, model: int, samples: int) -> int:
        """`mi355tts_pitch_frames`: floor(samples / hop)."""
        return int(ffi.check(self.lib, self.lib.mi355tts_pitch_frames(self._ctx, int(model), int(samples))))

    def pitch(self, model: int, audio: np.ndarray, samples=None, want_cmnd: int = 0) -> dict:
        """`audio`: float32 or int16 (read as s / 32768), [N] or [B, N], row b valid for `samples[b]` entries (default: all) ->
        {"f0", "periodicity", "level_db": float32 [B, F]; "cmnd": [B, F, tau_max + 1] or None; "frames": int64 [B]}, F the
        longest row's frame count, rows zero-filled behind their frames.  `want_cmnd`: tau_max + 1 of the model, to receive d'
        of every frame.  A 1-D input gives 1-D rows."""
        audio, flat, B, N, n, f_in, i_in = self._audio_in(audio, samples)
        frames = np.array([self.pitch_frames(model, int(v)) if 0 <= v <= N else 0 for v in n], np.int64)
        ld = int(frames.max(initial=0))
        f0, per, lvl = (np.empty((B, ld), np.float32) for _ in range(3))
        cmnd = np.empty((B, ld, int(want_cmnd)), np.float32) if want_cmnd else None
        self.pitch_raw(model, f_in, i_in, n, N, ffi.ptr(f0), ffi.ptr(per), ffi.ptr(lvl), ffi.ptr(cmnd), ld)
        f0, per, lvl, cmnd = self._rows_out(flat, f0, per, lvl, cmnd)
        return {"f0": f0, "periodicity": per, "level_db": lvl, "cmnd": cmnd, "frames": frames}

    def pitch_raw(self, model: int, f32_ptr, i16_ptr, samples, in_ld: int, f0_ptr=None, periodicity_ptr=None, level_ptr=None,
                  cmnd_ptr=None, out_ld: int = 0, flags: int = 0) -> None:
        """Pointer-level entry: exactly one input pointer [B][in_ld] (device memory with ffi.IN_DEVICE); the planes [B][out_ld]
        (at least one of the first three) and the d' rows [B][out_ld][tau_max + 1] (device memory with ffi.OUT_DEVICE)."""
        n = self._samples(samples)
        ffi.check(
            self.lib,
            self.lib.mi355tts_pitch(self._ctx, int(model), f32_ptr, i16_ptr, ffi.i64p(n), len(n), int(in_ld),
                                    f0_ptr, periodicity_ptr, level_ptr, cmnd_ptr, int(out_ld), int(flags)),
        )

    # ---- pitch shift and tempo ------------------------------------------------------
    def load_shift(self, up: int, down: int, window: np.ndarray, pitch: int, resampler: int = 0) -> int:
        """`mi355tts_load_shift`: a period-synchronous overlap-add stretch by `up / down` with the window `window` [N]
        (`larynx_amd.shift.ola_window`), the periods from the pitch model `pitch`; `resampler`, a resampler model by `down / up`,
        plays the stretch back at the input's duration (the PITCH mode), 0 delivers the stretch (the TEMPO mode).  The model keeps
        both alive; `unload` frees it."""
        window = np.ascontiguousarray(window, np.float32).reshape(-1)
        p = ffi.ShiftParamsC(int(up), int(down), len(window), int(pitch), int(resampler))
        return self._loaded(self.lib.mi355tts_load_shift, C.byref(p), window.ctypes.data)

    def shift_length(self, model: int, samples: int) -> int:
        """`mi355tts_shift_length`: a row's delivered length: `samples` (PITCH mode) or ceil(samples * up / down) (TEMPO)."""
        return int(ffi.check(self.lib, self.lib.mi355tts_shift_length(self._ctx, int(model), int(samples))))

    def shift(self, model: int, audio: np.ndarray, samples=None, want_float: bool = True, want_int16: bool = False,
              normalize: bool = False, positions_in=None, want_positions: typing.Optional[int] = None,
              want_f0: typing.Optional[int] = None) -> dict:
        """`audio`: float32 or int16 (read as s / 32768), [N] or [B, N], row b valid for `samples[b]` entries (default: all) ->
        {"f32", "i16": [B, longest delivered row] or None; "samples": int64 [B]; "positions": int32 [B, want_positions] or None;
        "f0": float32 [B, want_f0] or None}, rows zero-filled behind their entries; a 1-D input gives 1-D rows.
        `want_positions` / `want_f0`: the width of that output (at least the longest row's frames / pitch frames), None: not
        wanted.  `positions_in` (int32 [B, K] or [K]) replaces the tracked positions."""
        audio, flat, B, N, n, f_in, i_in = self._audio_in(audio, samples)
        if not (want_float or want_int16):
            raise ValueError("nothing asked for: want_float and / or want_int16")
        ld = max([self.shift_length(model, int(v)) for v in n if 0 <= v <= N] or [0])
        f32 = np.empty((B, ld), np.float32) if want_float else None
        i16 = np.empty((B, ld), np.int16) if want_int16 else None
        pos = np.empty((B, int(want_positions)), np.int32) if want_positions is not None else None
        f0 = np.empty((B, int(want_f0)), np.float32) if want_f0 is not None else None
        pos_ld = int(want_positions or 0)
        if positions_in is not None:
            positions_in = np.ascontiguousarray(np.asarray(positions_in, np.int32).reshape(B, -1))
            pos_ld = positions_in.shape[1]
        out = self.shift_raw(model, f_in, i_in, n, N, ffi.ptr(f32), ffi.ptr(i16), ld, ffi.PCM_NORMALIZE if normalize else ffi.PCM_SATURATE,
                             positions_in_ptr=ffi.ptr(positions_in), positions_ptr=ffi.ptr(pos), pos_ld=pos_ld, f0_ptr=ffi.ptr(f0),
                             f0_ld=int(want_f0 or 0))
        f32, i16, pos, f0 = self._rows_out(flat, f32, i16, pos, f0)
        return {"f32": f32, "i16": i16, "samples": out, "positions": pos, "f0": f0}

    def shift_raw(self, model: int, f32_ptr, i16_ptr, samples, in_ld: int, out_f32_ptr, out_i16_ptr, out_ld: int, pcm_mode: int = 0,
                  positions_in_ptr=None, positions_ptr=None, pos_ld: int = 0, f0_ptr=None, f0_ld: int = 0, flags: int = 0) -> np.ndarray:
        """Pointer-level entry: exactly one input pointer [B][in_ld] and optionally positions_in int32 [B][pos_ld] (device memory
        with ffi.IN_DEVICE); at least one output pointer [B][out_ld], optionally positions int32 [B][pos_ld] and f0 [B][f0_ld]
        (device memory with ffi.OUT_DEVICE); returns the rows' delivered lengths, int64 [B]."""
        n = self._samples(samples)
        out = np.zeros(len(n), np.int64)
        ffi.check(
            self.lib,
            self.lib.mi355tts_shift(self._ctx, int(model), f32_ptr, i16_ptr, ffi.i64p(n), len(n), int(in_ld),
                                    positions_in_ptr, out_f32_ptr, out_i16_ptr, int(out_ld), int(pcm_mode), positions_ptr, int(pos_ld),
                                    f0_ptr, int(f0_ld), ffi.i64p(out), int(flags)),
        )
        return out

    # ---- single operators ------------------------------------------------------
    def conv1d(self, x, w, bias=None, dilation=1, in_slope=1.0, out_act=0, lens=None) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        B, Cin, L = x.shape
        Cout, _, K = w.shape
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        y = np.zeros((B, Cout, L), np.float32)
        ln = None if lens is None else np.ascontiguousarray(lens, np.int32)
        ffi.check(
            self.lib,
            self.lib.mi355tts_op_conv1d(
                self._ctx, x.ctypes.data, B, Cin, L, ffi.i32p(ln),
                w.ctypes.data, ffi.ptr(b), Cout, K, int(dilation), float(in_slope), int(out_act), y.ctypes.data,
            ),
        )
        return y

    def gauss_noise(self, seed: int, B: int, channels: int, T: int) -> np.ndarray:
        """[B, channels, T] draws of the device noise generator (what `glow_infer` adds when no
        explicit noise tensor is given)."""
        out = np.empty((B, channels, T), np.float32)
        ffi.check(self.lib, self.lib.mi355tts_op_gauss_noise(self._ctx, ffi.u64(seed), B, channels, T, out.ctypes.data))
        return out

    def denoise(self, wav: np.ndarray, bias_spec: np.ndarray, strength: float) -> np.ndarray:
        wav = np.ascontiguousarray(wav, np.float32)
        if wav.ndim == 1:
            wav = wav[None]
        bias = np.ascontiguousarray(bias_spec, np.float32)
        out = np.zeros_like(wav)
        ffi.check(self.lib, self.lib.mi355tts_op_denoise(self._ctx, wav.ctypes.data, wav.shape[0], wav.shape[1], bias.ctypes.data,
                                                        float(strength), out.ctypes.data))
        return out

    def conv_transpose1d(self, x, w, bias, stride, in_slope=1.0) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        B, Cin, L = x.shape
        _, Cout, K = w.shape
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        y = np.zeros((B, Cout, L * stride), np.float32)
        ffi.check(
            self.lib,
            self.lib.mi355tts_op_conv_transpose1d(
                self._ctx, x.ctypes.data, B, Cin, L, w.ctypes.data, ffi.ptr(b), Cout, K, int(stride), float(in_slope), y.ctypes.data
            ),
        )
        return y

    def bench_conv1d(self, B, Cin, Cout, K, dilation, L, tile_shape=-1, iters=20) -> float:
        """Average ms per launch of the conv kernel on device-resident random data."""
        ms = C.c_float()
        ffi.check(self.lib, self.lib.mi355tts_bench_conv1d(self._ctx, B, Cin, Cout, K, dilation, L, tile_shape, iters, C.byref(ms)))
        return float(ms.value)

    # ---- measurement -------------------------------------------------------------
    def set_profiling(self, on: bool):
        ffi.check(self.lib, self.lib.mi355tts_set_profiling(self._ctx, 1 if on else 0))

    def set_option(self, name: str, value: int):
        ffi.check(self.lib, self.lib.mi355tts_set_option(self._ctx, name.encode("ascii"), int(value)))

    def coalesce_stats(self):
        """(passes, rows) of the shared GlowTTS passes since the context was created (see include/mi355tts.h)."""
        a, b = C.c_int64(0), C.c_int64(0)
        ffi.check(self.lib, self.lib.mi355tts_coalesce_stats(self._ctx, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def profile_reset(self):
        ffi.check(self.lib, self.lib.mi355tts_profile_reset(self._ctx))

    def profile_event_overhead_us(self, pairs: int = 64) -> float:
        """Median elapsed time of an EMPTY event pair on an idle stream (`mi355tts_profile_event_overhead`)."""
        us = C.c_double(0.0)
        ffi.check(self.lib, self.lib.mi355tts_profile_event_overhead(self._ctx, int(pairs), C.byref(us)))
        return float(us.value)

    def _json(self, fn, cap: int) -> dict:
        """What the getter `fn(ctx, buf, cap)` renders."""
        buf = C.create_string_buffer(cap)
        ffi.check(self.lib, fn(self._ctx, buf, cap))
        return json.loads(buf.value.decode("ascii"))

    def profile(self) -> dict:
        return self._json(self.lib.mi355tts_profile_json, 4096)

    def get_call_coalesce_default(self) -> int:
        """The library's built-in default of option `call_coalesce` (`mi355tts_call_coalesce_default`)."""
        return int(self.lib.mi355tts_call_coalesce_default())

    def profile_kernels(self) -> dict:
        """The profiled launches per kernel NAME and sub-key (`mi355tts_profile_kernels_json`): {class: {"name/sub": {...}}}."""
        return self._json(self.lib.mi355tts_profile_kernels_json, 32768)

    def dispatch_selfcheck(self) -> dict:
        """The one-off check of the dispatch-order assumption (`mi355tts_dispatch_selfcheck`): runs it if it has not run."""
        st, a, b = C.c_int(0), C.c_float(0.0), C.c_float(0.0)
        ffi.check(self.lib, self.lib.mi355tts_dispatch_selfcheck(self._ctx, C.byref(st), C.byref(a), C.byref(b)))
        return {"state": {0: "not run", 1: "snake order kept", 2: "snake order switched off", 3: "skipped", 4: "running"}[int(st.value)],
                "plain_us": float(a.value), "snake_us": float(b.value)}

    def kernel_counts(self) -> dict:
        """Launches per kernel name since the last `profile_reset` (`mi355tts_kernel_counts_json`; always counted)."""
        return self._json(self.lib.mi355tts_kernel_counts_json, 4096)
