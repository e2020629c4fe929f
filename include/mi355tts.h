/* mi355tts — C ABI of the MI355X-native Larynx hot path
 * (phoneme ids -> GlowTTS -> mel transform -> HiFi-GAN -> waveform).
 *
 * This is what a Larynx maintainer binds (ctypes) behind the
 * reference's own model interface.  Every entry point names the reference
 * interface it replaces (paths relative to rhasspy/larynx v1.1.0):
 *
 *   larynx/constants.py:62-72   TextToSpeechModel.phonemes_to_mels
 *   larynx/constants.py:90-100  VocoderModel.mels_to_audio
 *   larynx/glow_tts.py:109-170  GlowTextToSpeech.phonemes_to_mels  (ORT feed dict :161-168)
 *   larynx/hifi_gan.py:130-169  HiFiGanVocoder.mels_to_audio
 *   larynx/__init__.py:214-285  _sentence_task (mel transforms :242-249)
 *   larynx/audio.py:83-125      AudioSettings.denormalize/db_to_amp/
 *                               dynamic_range_compression, audio_float_to_int16
 *   glow_tts/checkpoint.py:26-68, hifi_gan/checkpoint.py:36-70   load_checkpoint
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success or a negative mi355tts_status, never throws or aborts;
 * mi355tts_last_error() gives the calling thread's last message.  All entry
 * points are re-entrant: many host threads may call into one context
 * concurrently (the reference calls its models from a ThreadPoolExecutor,
 * larynx/__init__.py:146); each call runs on its own HIP stream + workspace.
 * Tensors are row-major, channel-major like the reference's `[1, 80, F]` mels:
 * [batch][channel][time], time fastest.
 */
#ifndef MI355TTS_H
#define MI355TTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355TTS_ABI_VERSION 2 /* 2: n_speakers / gin_channels in mi355tts_glow_hparams, the *_speakers entry points */

typedef enum {
  MI355TTS_OK = 0,
  MI355TTS_ERR_INVALID = -1,   /* bad argument / unsupported hyper-parameter  */
  MI355TTS_ERR_HIP = -2,       /* a HIP runtime call failed (message has it)   */
  MI355TTS_ERR_NOMEM = -3,
  MI355TTS_ERR_TOO_SMALL = -4, /* caller-provided buffer too small             */
  MI355TTS_ERR_NO_MODEL = -5
} mi355tts_status;

typedef struct mi355tts_ctx mi355tts_ctx; /* one per process per GPU              */
typedef struct mi355tts_mel mi355tts_mel; /* device-resident mel batch             */

/* glow_tts/config.py:36-62 (ModelConfig) + audio.mel_channels */
typedef struct {
  int32_t num_symbols, hidden_channels, filter_channels, filter_channels_dp;
  int32_t kernel_size, n_blocks_dec, n_layers_enc, n_heads;
  int32_t dilation_rate, kernel_size_dec, n_block_layers, n_sqz;
  int32_t prenet, window_size, n_split, mel_channels;
  int32_t prenet_kernel_size, prenet_layers; /* glow_tts/models.py:96-97 (5, 3) */
  /* multi-speaker voices (glow_tts/config.py:56,60; models.py:304-306): n_speakers > 1 with gin_channels in [1, 1024], or a
   * single-speaker voice: n_speakers <= 1 and gin_channels = 0 */
  int32_t n_speakers, gin_channels;
} mi355tts_glow_hparams;

/* hifi_gan/config.py:29-41 (ModelConfig) */
#define MI355TTS_MAX_STAGES 8
typedef struct {
  int32_t resblock_type; /* 1 = ResBlock1, 2 = ResBlock2                       */
  int32_t num_upsamples;
  int32_t upsample_rates[MI355TTS_MAX_STAGES];
  int32_t upsample_kernel_sizes[MI355TTS_MAX_STAGES];
  int32_t upsample_initial_channel;
  int32_t num_kernels;
  int32_t resblock_kernel_sizes[MI355TTS_MAX_STAGES];
  int32_t num_dilations;
  int32_t resblock_dilations[MI355TTS_MAX_STAGES][MI355TTS_MAX_STAGES];
  int32_t num_mels;
} mi355tts_hifigan_hparams;

/* larynx/audio.py:26-50 (the fields the mel transforms read) */
typedef struct {
  int32_t signal_norm, symmetric_norm, clip_norm;
  int32_t convert_db_to_amp, do_dynamic_range_compression;
  float min_level_db, max_norm, ref_level_db, spec_gain;
} mi355tts_audio_settings;

/* flags for the inference calls */
#define MI355TTS_IN_DEVICE 1u  /* ids / noise / mel input pointers are device memory */
#define MI355TTS_OUT_DEVICE 2u /* waveform output pointers are device memory          */

int mi355tts_abi_version(void);
const char* mi355tts_last_error(void);

int mi355tts_create(int device, mi355tts_ctx** out);
void mi355tts_destroy(mi355tts_ctx* ctx);

/* ---- weights ---------------------------------------------------------------
 * A model is loaded from ONE flat fp32 blob: the reference checkpoint's tensors
 * (weight-norm folded, `remove_weight_norm` / `store_inverse` semantics) laid end
 * to end in the order the manifest enumerates.  `*_manifest` returns the i-th
 * tensor's reference state-dict name and element count (1 = past the end), so
 * the host-side converter never hard-codes the order.  `on_device` != 0 means
 * `blob` is device memory (e.g. the receive buffer of an RCCL broadcast).
 * Replaces load_checkpoint + .eval() in larynx/glow_tts.py:66-95 and
 * larynx/hifi_gan.py:71-100. */
int mi355tts_glow_manifest(const mi355tts_glow_hparams* hp, int index, char* name, int name_cap, int64_t* numel);
int mi355tts_hifigan_manifest(const mi355tts_hifigan_hparams* hp, int index, char* name, int name_cap, int64_t* numel);
int mi355tts_load_glow(mi355tts_ctx* ctx, const mi355tts_glow_hparams* hp, const float* blob, int64_t numel,
                       int on_device, int* model_out);
int mi355tts_load_hifigan(mi355tts_ctx* ctx, const mi355tts_hifigan_hparams* hp, const float* blob, int64_t numel,
                          int on_device, int* model_out);
int mi355tts_unload(mi355tts_ctx* ctx, int model);
/* Utterance-level data parallelism: the ONE collective of the path — rank `root`'s folded weight
 * blob (device memory, `numel` floats: what mi355tts_load_*(on_device = 1) ingests) is broadcast over xGMI to the
 * same-sized device buffer of every rank of the caller's RCCL communicator (`nccl_comm` is an ncclComm_t).  The
 * library does not link RCCL: ncclBroadcast is resolved from the RCCL library already loaded in the caller's
 * process (`rccl_library`: its path or soname, NULL = "librccl.so.1").  The reference is a single process and has
 * no counterpart; a Python host broadcasts with torch.distributed instead (larynx_amd/sharding.py). */
int mi355tts_broadcast_weights(mi355tts_ctx* ctx, void* nccl_comm, int root, float* device_blob, int64_t numel,
                               const char* rccl_library);
/* The reference's `half` switch (TextToSpeechModelConfig.half / VocoderModelConfig.half,
 * larynx/constants.py:58,85; `.half()` at larynx/glow_tts.py:90-91, larynx/hifi_gan.py:96-97).
 * MI355TTS_PRECISION_F32 (default): exact f32 MFMA everywhere — the parity mode.
 * MI355TTS_PRECISION_F16: the native 16-bit mode, the analogue of the reference's `.half()` on the generator (hifi_gan/models.py
 * :186-202 under half weights and activations): fp16 weights, fp16 activation planes in HBM between ALL layers of the vocoder
 * (conv_pre, upsamplers, every ResBlock conv of every stage, conv_post), ONE v_mfma_f32_32x32x16_f16 per product, f32 accumulation;
 * bias, residual and activation are applied to the f32 accumulator before its one rounding to fp16 (csrc/conv_f16.h,
 * csrc/hifigan_f16.h).  Accuracy is that of a half-precision forward (tests compare with the reference's own generator run
 * under .half() / .bfloat16()).  Returns MI355TTS_ERR_INVALID with the reason when the vocoder's geometry is not covered
 * (channel counts not multiples of 8, upsampler kernel != 2 x stride, taps outside 3 / 5 / 7 / 11).
 * MI355TTS_PRECISION_BF16X3: the accurate reduced mode — the HiFi-GAN ResBlock convs and upsamplers run on the bf16 matrix cores
 * with split operands (x = hi + lo, three bf16 MFMAs per product, f32 accumulate, f32 planes): ~1e-5 relative error per layer.
 * MI355TTS_PRECISION_BF16: the BF16X3 kernels with ONE bf16 MFMA per product (kept for A/B runs).
 * GlowTTS models (the reference calls `.half()` on the whole FlowGenerator, larynx/glow_tts.py:90-91): MI355TTS_PRECISION_F16
 * puts the decoder's WaveNets — every gate conv and res_skip of every coupling block (glow_tts/layers.py:138-162): 84 % of the
 * acoustic model's FLOPs and 97 of its ~140 launches — on the fp16 matrix cores, ONE launch per block (csrc/wn_f16.h: fp16 weights,
 * hidden state and gated activations, f32 accumulation, f32 skip sum).  The encoder, the duration predictor (so the FRAME COUNTS
 * are the f32 model's: the reference's whole-model .half() changes them on 3 of 8 golden cases), the start / end convs, the
 * affine coupling, InvConvNear and ActNorm stay f32.  Accuracy: the mel within the error of the reference's own decoder under
 * .half() (tests/golden/glow_half_reference.json, made by oracle/make_golden_glow_half.py).  The kernel covers hidden_channels
 * 192 (the released voices; 32 for tests), kernel_size_dec 5, dilation_rate 1, single-speaker models; on any other GlowTTS
 * geometry, and for the split-bf16 requests on every GlowTTS model, the request changes nothing and returns
 * MI355TTS_PRECISION_NOOP (= 1, a positive status: not an error, not a silent success).  MI355TTS_PRECISION_F32 returns 0. */
#define MI355TTS_PRECISION_F32 0
#define MI355TTS_PRECISION_BF16X3 1
#define MI355TTS_PRECISION_BF16 2
#define MI355TTS_PRECISION_F16 3
#define MI355TTS_PRECISION_NOOP 1 /* return value: accepted, no effect on this model */
int mi355tts_model_set_precision(mi355tts_ctx* ctx, int model, int precision);

/* ---- GlowTTS: replaces GlowTextToSpeech.phonemes_to_mels --------------------
 * ids [B][ids_ld] int64 (row b valid for id_lens[b] entries; the reference's
 * "input" / "input_lengths"), scales as in the reference's "scales" input.
 * noise: optional N(0,1) tensor [B][mel_channels][noise_ld] standing in for
 * torch.randn_like (glow_tts/models.py:348) — parity mode; NULL draws from a
 * counter-based generator keyed by `seed` (row b of a batch: the stream seed + b — a batched call consumes the B
 * consecutive streams seed .. seed + B - 1, so successive batched calls must advance `seed` by at least B, or pass explicit
 * per-row seeds to mi355tts_glow_infer_rows, to draw independent fields).  `audio` (optional) additionally
 * produces the vocoder-input mel (the three numpy transforms of _sentence_task).
 * The frame count is data dependent; the result stays on the device. */
int mi355tts_glow_infer(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                        float noise_scale, float length_scale, const float* noise, int noise_ld, uint64_t seed,
                        const mi355tts_audio_settings* audio, uint32_t flags, mi355tts_mel** out);

/* The same with one noise-stream seed PER ROW (host array [B]) for the device generator: row b draws the field a
 * batch-1 call with seed = row_seeds[b] draws, so a work list cut into micro-batches (the utterance shards of
 * larynx/__init__.py:146-157 run as padded batches) gives every utterance the audio it gets on its own.
 * (mi355tts_glow_infer's rows use seed + b.) */
int mi355tts_glow_infer_rows(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                             float noise_scale, float length_scale, const uint64_t* row_seeds,
                             const mi355tts_audio_settings* audio, uint32_t flags, mi355tts_mel** out);

/* Multi-speaker voices: the reference's `speaker_id` setting (larynx/glow_tts.py:116-130 -> `g` of
 * FlowGenerator.forward, glow_tts/models.py:318-319: g = F.normalize(emb_g(speaker)), which conditions every WaveNet
 * layer of the decoder, layers.py:141-154, and is concatenated to the duration predictor's input, models.py:128-132).
 * `speaker_ids` (host array [B], one speaker per row, each in [0, n_speakers)) is REQUIRED for a model loaded with
 * n_speakers > 1 and must be NULL for a single-speaker model — the reference fails on both mismatches too (no emb_g /
 * a duration predictor that expects hidden + gin input channels).  mi355tts_glow_infer / _rows / mi355tts_synthesize on
 * a multi-speaker model return MI355TTS_ERR_INVALID.  Everything else as in mi355tts_glow_infer; `row_seeds` (optional,
 * host [B]) as in mi355tts_glow_infer_rows (then `seed` is ignored). */
int mi355tts_glow_infer_speakers(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                                 float noise_scale, float length_scale, const float* noise, int noise_ld, uint64_t seed,
                                 const uint64_t* row_seeds, const int32_t* speaker_ids, const mi355tts_audio_settings* audio,
                                 uint32_t flags, mi355tts_mel** out);

/* Phoneme timings out, per-id timing control in (glow_tts/models.py:323-335: w, w_ceil, generate_path; :350-354: the `attn`
 * FlowGenerator.forward returns next to the mel — attn[b, 0, t, :].sum() is the number of mel frames id t occupies).
 * All three arrays are HOST memory [B][ld] whatever `flags` says, ld >= the longest row; entries past a row's length are
 * not read (inputs) and written as 0 (output).
 *   id_scales     a rate per id: w = (exp(logw) * length_scale) * id_scales[t] in f32, in this order, then ceil as in the
 *                 reference.  Finite and >= 0.  Exactly 1.0f gives the duration of a call without it (an all-ones array is
 *                 bit-identical to no prosody); 0 gives the id no frames (generate_path handles zero durations).
 *   durations_in  stands in for ceil(w) altogether, each in [0, 2^28]: logw, length_scale and id_scales are not read for the
 *                 durations; the cumulative sum, the frame count and everything behind them are unchanged.  Excludes id_scales.
 *   durations_out what every id got.  TRUNCATION RULE: the row's frame count F is max(sum, 1) cut down to a multiple of n_sqz,
 *                 and the reference masks the path to F frames (sequence_mask(y_lengths) in attn_mask, models.py:329-335), so
 *                 durations_out[t] = min(cum[t], F) - min(cum[t-1], F), not simply ceil(w): when the sum is odd at n_sqz = 2
 *                 the last id that has frames loses one.  The row sums to F (except: every duration 0 at n_sqz = 1, where
 *                 F = 1 and the sum is 0).  All durations 0 at n_sqz = 2 gives F = 0: an empty mel.
 * ROUND TRIP: feeding a call's durations_out back as durations_in, with the same noise or seed, reproduces its mel bit for
 * bit and the same durations.
 * mi355tts_glow_infer_prosody: the arguments of mi355tts_glow_infer_speakers (speaker_ids NULL for a single-speaker voice, same
 * rules as there), then `prosody`.  NULL behaves exactly like that call.  Otherwise the mel keeps the per-id durations
 * (mi355tts_mel_durations), and durations_out, when given, receives them as well.
 * A call without prosody pays nothing: same launches, copies and host synchronisations as before; with it, the same launches
 * (the durations are written by the launch that computes them) and one more small copy each way.
 * Added in ABI version 2 (additive: the version number is unchanged). */
typedef struct {
  const float* id_scales;     /* host [B][ld] or NULL */
  const int32_t* durations_in; /* host [B][ld] or NULL; excludes id_scales */
  int32_t* durations_out;     /* host [B][ld] or NULL */
  int32_t ld;
} mi355tts_prosody;
int mi355tts_glow_infer_prosody(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                                float noise_scale, float length_scale, const float* noise, int noise_ld, uint64_t seed,
                                const uint64_t* row_seeds, const int32_t* speaker_ids, const mi355tts_audio_settings* audio,
                                uint32_t flags, const mi355tts_prosody* prosody, mi355tts_mel** out);
/* dst host [B][ld], ld >= the ld the call was made with (columns past it: 0).  MI355TTS_ERR_INVALID for a mel that has no
 * durations: one wrapped by mi355tts_mel_from_buffer, or made by a call without prosody. */
int mi355tts_mel_durations(const mi355tts_mel* mel, int32_t* dst, int ld);

/* ---- forced alignment: which frames of a given mel belong to which phoneme id ------
 * Glow-TTS's own training-time alignment (the reference carries the pieces: FlowSpecDecoder.forward with reverse=False,
 * glow_tts/models.py:191-209; the reverse=False branches of ActNorm, InvConvNear and CouplingBlock, layers.py:192-197, :238-272,
 * attentions.py:119-142; maximum_path, glow_tts/utils.py:59-96), per batch row (row b of a batch equals its own batch-1 call):
 *   1. F = (frames[b] / n_sqz) * n_sqz, later frames are ignored (FlowGenerator.preprocess, models.py:356-363); F >= id_lens[b].
 *   2. the encoder exactly as in mi355tts_glow_infer: x_m [M][P] (and the speaker vector of a multi-speaker voice).
 *   3. z = decoder(mel, reverse=False): squeeze; per flow block ActNorm (bias + exp(logs) x), InvConvNear with the forward
 *      weight (the inverse, computed in double at load time, of the weight_inv the blob carries), coupling z1 = m + exp(logs) x1;
 *      unsqueeze; masked to F.  Always f32, whatever mi355tts_model_set_precision says.  No log-determinant.
 *   4. scores (Glow-TTS's likelihood with x_logs = 0 — mean_only voices, the only ones loaded; not a line of the reference):
 *        logp[t][j] = -0.5 M ln(2 pi) - 0.5 sum_c z[c][j]^2 + sum_c x_m[c][t] z[c][j] - 0.5 sum_c x_m[c][t]^2
 *      every sum over c ascending in f32 (one fma per term), combined as ((c0 - 0.5 zz) + xz) - 0.5 xx.
 *   5. the best monotonic path as maximum_path computes it in float32: v = 0; per frame j: v0[t] = v[t-1] (-inf at t = 0),
 *      stay = v[t] >= v0[t] (a tie stays), v[t] = max(v[t], v0[t]) + logp[t][j] for t <= j, else -inf; backtrack from t = P - 1
 *      at j = F - 1.  One max and one add per cell: v is numpy's bit for bit.
 * ids / id_lens / speaker_ids as in mi355tts_glow_infer_speakers (HOST memory; speaker_ids NULL for a single-speaker voice).
 * mel: host [B][M][mel_ld] (device with MI355TTS_IN_DEVICE), in the GlowTTS output domain (plane 0 of mi355tts_mel_copy, before
 * the AudioSettings transforms), frames[b] <= mel_ld valid columns.  durations_out: host [B][dur_ld], dur_ld >= the longest
 * row: frames per id, each >= 1, row sum F, entries past id_lens[b] zero.  score_out: host [B] or NULL, the path's total
 * v[P - 1].  z_out: host (device with MI355TTS_OUT_DEVICE) [B][M][mel_ld] or NULL, zero past F.
 * MI355TTS_ERR_INVALID with the reason: F < id_lens[b], more than 2048 ids in a row (the path kernel's registers), dur_ld too
 * small, speaker ids missing or superfluous, null pointers.  Durations from here go into mi355tts_prosody.durations_in
 * ("the timing of one take onto another").  Added in ABI version 2 (additive: the version number is unchanged). */
int mi355tts_glow_align(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                        const float* mel, const int32_t* frames, int mel_ld, const int32_t* speaker_ids, uint32_t flags,
                        int32_t* durations_out, int dur_ld, float* score_out, float* z_out);

int mi355tts_mel_batch(const mi355tts_mel* mel);
int mi355tts_mel_channels(const mi355tts_mel* mel);
int mi355tts_mel_max_frames(const mi355tts_mel* mel);
int mi355tts_mel_frames(const mi355tts_mel* mel, int32_t* frames /* [B] */);
/* which: 0 = raw GlowTTS output, 1 = vocoder input.  dst is host [B][M][ld], ld >= max_frames */
int mi355tts_mel_copy(const mi355tts_mel* mel, int which, float* dst, int ld);
void mi355tts_mel_free(mi355tts_mel* mel); /* must precede mi355tts_destroy() of the owning context */
/* Wrap a host (or device) mel [B][M][ld]; apply the mel transforms iff `audio` != NULL. */
int mi355tts_mel_from_buffer(mi355tts_ctx* ctx, const float* mel, const int32_t* frames, int B, int M, int ld,
                             const mi355tts_audio_settings* audio, uint32_t flags, mi355tts_mel** out);

/* ---- HiFi-GAN: replaces HiFiGanVocoder.mels_to_audio ------------------------
 * Consumes the vocoder-input mel; writes per row frames[b]*hop samples (tail up
 * to wav_ld zero-filled).  wav_f32 (optional) is the generator output before
 * audio_float_to_int16; wav_i16 (optional) after it.  wav_ld >= max_frames*hop.
 * denoiser_strength > 0 additionally runs the reference's spectral-subtraction
 * denoiser (larynx/hifi_gan.py:152-203, STFT helpers larynx/audio.py:232-306) on
 * the device before the int16 conversion; its bias spectrum is computed once per
 * vocoder from an all-zero mel, as `maybe_init_denoiser` does. */
int mi355tts_hifigan_hop(mi355tts_ctx* ctx, int vocoder);
int mi355tts_hifigan_infer(mi355tts_ctx* ctx, int vocoder, const mi355tts_mel* mel, float denoiser_strength,
                           float* wav_f32, int16_t* wav_i16, int64_t wav_ld, uint32_t flags);

/* The same call with the SSML pause padding `_sentence_task` applies on the host with np.pad
 * (larynx/__init__.py:277-283) done by the int16 kernel: per row `pad_before` zero samples,
 * the audio, then zeros (at least `pad_after`) up to wav_ld.  wav_ld >= pad_before +
 * max_frames*hop + pad_after. */
int mi355tts_hifigan_infer_padded(mi355tts_ctx* ctx, int vocoder, const mi355tts_mel* mel, float denoiser_strength,
                                  float* wav_f32, int16_t* wav_i16, int64_t wav_ld, uint32_t flags, int32_t pad_before,
                                  int32_t pad_after);

/* ---- Griffin-Lim: replaces GriffinLimVocoder.mels_to_audio -------------------
 * (larynx/griffin_lim.py:22-76 on the STFT helpers of larynx/audio.py:232-306): a vocoder without weights.  The
 * magnitudes are exp(mel) @ mel_basis * mel_scaling with the last mel frame dropped, the phase starts uniform and
 * `iterations` rounds of transform + inverse refine it — 1024-point frames every 256 samples, symmetric Hann window on
 * analysis and synthesis, no window-sum normalisation: the reference's hard-wired conventions (fft and hop are NOT
 * parameters: audio.py:284,297; a voice whose filter_length / hop_length differ is rejected by the Python wrapper).
 * `mel_basis` is the host array [num_mels][513] (larynx_amd.audio.mel_basis builds the reference's Slaney filter bank).
 * mi355tts_unload frees the model.  Added in ABI version 2 (additive: the version number is unchanged). */
typedef struct {
  int32_t num_mels;    /* 1 .. 256 */
  float mel_scaling;   /* the reference's 1000.0 */
  int32_t iterations;  /* the reference's 60; >= 0 */
} mi355tts_griffin_lim_params;
int mi355tts_load_griffin_lim(mi355tts_ctx* ctx, const mi355tts_griffin_lim_params* params, const float* mel_basis,
                              int* model_out);
/* A mel row of F frames gives T = F - 1 STFT frames and (F - 1) * 256 + 1024 samples (F < 2: an empty signal); the row's
 * tail up to wav_ld is zero-filled; wav_ld >= (max_frames - 1) * 256 + 1024.  The mel is the vocoder-input plane of `mel`
 * (ln domain, what dynamic_range_decompression expects).
 * phase0 (optional): the initial phase [B][513][max_frames - 1] standing in for the reference's np.random.rand draw
 *   (griffin_lim.py:68) — parity mode.  NULL draws it on the device: u = a 24-bit uniform from the counter hash of the
 *   noise generator keyed by (`seed` + row, bin, frame), phase = np.angle(np.exp(2j pi u)) in (-pi, pi).
 * phase_out (optional, same shape): the initial phase the call used; a call that injects it as phase0 reproduces the
 *   seeded call bit for bit.  Entries past a row's T frames are zero.
 * wav_f32 (optional): the float signal (the reference returns it as float64; this is float32).  wav_i16 (optional): its
 *   audio_float_to_int16 (larynx/audio.py:118-125), computed on the device.
 * iterations <= 0: the model's.  One launch per iteration; the signal lives as overlapping synthesis frames in between
 *   (csrc/griffin_lim.h).  flags: MI355TTS_IN_DEVICE — phase0 is device memory; MI355TTS_OUT_DEVICE — phase_out and the
 *   waveform pointers are.  All arithmetic is f32: a mel whose magnitudes leave the f32 range (one that is not in the ln
 *   domain: spectra beyond ~1e30) is out of scope — the result is then unspecified, not an error. */
int mi355tts_griffin_lim_infer(mi355tts_ctx* ctx, int model, const mi355tts_mel* mel, const float* phase0, uint64_t seed,
                               float* phase_out, float* wav_f32, int16_t* wav_i16, int64_t wav_ld, int iterations,
                               uint32_t flags);

/* ---- mel analysis: a recording into the voice's own mel domain -----------------
 * waveform -> mi355tts_mel, the inverse direction of the transforms above, in ONE launch (csrc/mel_analysis.h): 1024-point
 * frames every 256 samples (fft and hop are not parameters, as for Griffin-Lim), mag[k] = sqrt(re^2 + im^2 + mag_eps) in f32,
 * amp[m] = sum_k mel_basis[m][k] mag[k] (k ascending, one fma per term, over the row's non-zero band), then
 *   vocoder plane (1): ln(max(amp, 1e-5)) with do_dynamic_range_compression (AudioSettings.dynamic_range_compression,
 *                      larynx/audio.py:106-108), else amp;
 *   raw plane (0):     the inverse of the mel transforms, switch by switch: convert_db_to_amp gives spec_gain * log10(max(1e-5,
 *                      amp)) (amp_to_db, audio.py:55-56), otherwise the vocoder plane's value; signal_norm then applies
 *                      AudioSettings.normalize (audio.py:65-81) in its operation order, both clip variants;
 *   audio == NULL:     both planes ln(max(amp, 1e-5)).
 * The reference carries these functions and never calls them on its inference path; it has no framing of a recording for a
 * VOICE at all.  The two framings offered, and what each one is:
 *   MI355TTS_FRAMING_HIFIGAN (0)    the published HiFi-GAN training convention — not a line of the reference: the signal is
 *       reflect-padded by 384 samples on each side (frame t reads 256 t - 384 + i; an index < 0 maps to -idx, one >= N to
 *       2 (N - 1) - idx), periodic Hann window 0.5 - 0.5 cos(2 pi i / 1024).  N samples give N / 256 frames (floor) for
 *       N >= 385, none below (one reflection would not be enough).  Frame t is centred on hop t: the "frame j <-> samples
 *       [j hop, (j + 1) hop)" relation of the phoneme spans.
 *   MI355TTS_FRAMING_REFERENCE (1)  the reference's own stft (audio.py:232-249: what transform() and its Griffin-Lim vocoder
 *       use): no padding, frame t reads x[256 t : 256 t + 1024), symmetric np.hanning(1024).  ceil((N - 1024) / 256) frames for
 *       N > 1024, none below.  (mi355tts_griffin_lim_infer on an F-frame mel comes back as F - 1 such frames.)
 * Which of them — if either — equals what a given released voice was trained with is not known to this library: the choice
 * is the caller's.  Both windows are computed in double precision and rounded once.
 * mi355tts_load_analysis: mel_basis is the host array [num_mels][513]; mi355tts_unload frees the model.
 * mi355tts_mel_from_audio: exactly one of wav_f32 / wav_i16 [B][wav_ld] (host, or device with MI355TTS_IN_DEVICE); int16 samples
 * are converted as s * 2^-15 (exact) inside the same launch; row b holds samples[b] <= wav_ld samples (host array, each
 * <= 2^30).  The mel's leading dimension is the longest row's frame count rounded up to 4, columns past a row's frames are zero
 * in both planes, row b of a batch is bit-identical to its own batch-1 call, a batch whose rows all have 0 frames is a valid
 * empty mel (max_frames 0), and the mel has no durations (like one from mi355tts_mel_from_buffer).  Inputs are expected in
 * [-1, 1] (|X| <= 1024: nothing is rescaled before the square).
 * MI355TTS_ERR_INVALID with the reason: null pointers, both or neither waveform, samples[b] outside [0, wav_ld], num_mels
 * outside [1, 256], a negative or non-finite mag_eps, an unknown framing.
 * Added in ABI version 2 (additive: the version number is unchanged). */
#define MI355TTS_FRAMING_HIFIGAN 0
#define MI355TTS_FRAMING_REFERENCE 1
typedef struct {
  int32_t num_mels; /* 1 .. 256 */
  int32_t framing;  /* MI355TTS_FRAMING_* */
  float mag_eps;    /* >= 0; 1e-9 in the HiFi-GAN convention, 0 in the reference's */
} mi355tts_analysis_params;
int mi355tts_load_analysis(mi355tts_ctx* ctx, const mi355tts_analysis_params* params, const float* mel_basis, int* model_out);
int mi355tts_mel_from_audio(mi355tts_ctx* ctx, int model, const float* wav_f32, const int16_t* wav_i16, const int64_t* samples,
                            int B, int64_t wav_ld, const mi355tts_audio_settings* audio, uint32_t flags, mi355tts_mel** out);
/* The device planes of a mel (which: 0 = raw, 1 = vocoder input; [B][M][*ld] floats, valid until mi355tts_mel_free), so that a
 * mel can feed mi355tts_glow_align with MI355TTS_IN_DEVICE without a host round trip. */
int mi355tts_mel_plane(const mi355tts_mel* mel, int which, const float** device_ptr, int* ld);

/* ---- resampling: the delivered rows at another sample rate --------------------
 * Every voice produces 22 050 Hz audio; this delivers 8 / 16 / 24 / 44.1 / 48 kHz (or any other rational ratio) where the samples
 * already are: ONE launch behind the vocoder, TWO with MI355TTS_PCM_NORMALIZE (csrc/resample.h).  The reference has no such
 * step (larynx/server.py:211-217 writes whatever AudioSettings.sample_rate says).
 * Rational resampling by up / down (coprime) with a caller-supplied symmetric prototype filter: only up, down and the
 * prototype's half-length are parameters, the design is the caller's (larynx_amd.resample.design_lowpass: a Kaiser-windowed
 * sinc) and the taps are passed in like any other table.
 *   Prototype:     host array taps[2 H + 1], centre H (= half_len), given at the up-sampled rate.
 *   Output length: a row of N input samples gives N_out = ceil(N * up / down) outputs; N = 0 gives 0.
 *   Definition:    with c = n * down + H,
 *                    y[n] = sum over i in [0, N) with 0 <= c - i * up <= 2 H of x[i] * taps[c - i * up].
 *                  Samples outside [0, N) are zero: each row starts and ends from silence, with no state across calls.  Output n
 *                  sits at input time n * down / up: zero delay, y[0] is aligned with x[0].  This is
 *                  scipy.signal.resample_poly(x, up, down, window=taps / up).
 *   Arithmetic:    all f32, one fma per term, one accumulator per output, starting from +0.  Term order: i DESCENDING from
 *                  c div up, i.e. prototype index c mod up + t * up for t = 0, 1, .. ascending (the polyphase row of phase
 *                  c mod up, T = ceil((2 H + 1) / up) taps, walked from its first entry).  Terms outside the row or the
 *                  prototype add exact zeros.  Row b of a batch is bit-identical to its own batch-1 call; int16 input is
 *                  converted as s * 2^-15 (exact) inside the launch and gives the bits of the equal f32 input; host and device
 *                  pointers give the same bits.
 * mi355tts_load_resampler: lays the prototype out as the polyphase table [phase][t] on the device; mi355tts_unload frees the model.
 * mi355tts_resample_length: ceil(samples * up / down) for 0 <= samples <= 2^24; a negative status on error.
 * mi355tts_resample: exactly one of in_f32 / in_i16 [B][in_ld] (host, or device with MI355TTS_IN_DEVICE) and at least one of
 * out_f32 / out_i16 [B][out_ld] (host, or device with MI355TTS_OUT_DEVICE), as in mi355tts_mel_from_audio and
 * mi355tts_griffin_lim_infer.  Row b holds samples[b] <= in_ld input samples (host array); every output row is zero-filled from
 * its N_out up to out_ld; samples_out (host [B], or NULL) receives the rows' N_out.  The workspace grows on demand
 * (mi355tts_reserve does not cover this call).
 * int16 output (pcm_mode):
 *   MI355TTS_PCM_SATURATE (0)   clamp(rintf(y * 32768), -32768, 32767).  The filter overshoots: a full-scale input saturates,
 *                               so a delivered int16 stream (whose peak sits at 32767) re-sampled in this mode MAY CLIP.
 *   MI355TTS_PCM_NORMALIZE (1)  the reference's audio_float_to_int16 (larynx/audio.py:118-125) applied to the row's N_out resampled
 *                               samples: scale 32767 / max(0.01, max|y|), clip to +-32767, truncate toward zero — the rule and
 *                               rounding the vocoder's own int16 rows get.  The mode of the sentence path: resample the FLOAT
 *                               signal, then normalise; the peak lands on 32767 at the new rate and nothing clips.
 * MI355TTS_ERR_INVALID with the reason (MI355TTS_ERR_NO_MODEL for an unknown id): null pointers; both inputs or neither; no
 * output; up or down outside [1, 1024], or not coprime; half_len < 0; more than 128 taps per phase (ceil((2 H + 1) / up)); a
 * non-finite tap; samples[b] outside [0, in_ld] or above 2^24; out_ld below the longest row's N_out; an unknown pcm_mode.
 * Added in ABI version 2 (additive: the version number is unchanged). */
typedef struct {
  int32_t up, down; /* 1 .. 1024, coprime */
  int32_t half_len; /* H >= 0: the prototype has 2 H + 1 taps, at most 128 per phase */
} mi355tts_resampler_params;
int mi355tts_load_resampler(mi355tts_ctx* ctx, const mi355tts_resampler_params* params, const float* taps, int* model_out);
int64_t mi355tts_resample_length(mi355tts_ctx* ctx, int model, int64_t samples);
#define MI355TTS_PCM_SATURATE 0
#define MI355TTS_PCM_NORMALIZE 1
int mi355tts_resample(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                      int64_t in_ld, float* out_f32, int16_t* out_i16, int64_t out_ld, int pcm_mode, int64_t* samples_out,
                      uint32_t flags);

/* ---- loudness: a level target for the delivered rows ---------------------------
 * The int16 rows the library delivers are peak-normalised sentence by sentence (the reference's rule, and the default).  This
 * measures a row's ITU-R BS.1770-4 integrated loudness (mono) where the samples already are and delivers it at a target level
 * under a sample-peak ceiling: FIVE launches measure, a SIXTH delivers, whatever N and B are (csrc/loudness.h).  The reference
 * has no such step.
 *   K-weighting:   two biquads in series, first the shelf and then the high-pass, each
 *                    y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2],
 *                  every row from zero state, no state across calls.  The ten coefficients are the caller's, passed in like any
 *                  other table (larynx_amd.loudness.k_weighting(fs): the standard's 48 kHz filters re-derived for fs).
 *   Blocks:        block j covers weighted samples [j hop, j hop + block) for every j with j hop + block <= N; z_j is their mean
 *                  square, l_j = -0.691 + 10 log10 z_j.  block = round(0.4 fs) and hop = round(0.1 fs) are the caller's too.
 *                  A row with 0 < N < block has ONE block, made of its N samples: BS.1770 gives such a row no value, and a
 *                  sentence can be 0.3 s long.  This is this library's rule, not the standard's.
 *   Gates:         absolute, l_j > -70; relative, l_j > -0.691 + 10 log10(mean of the absolutely gated z_j) - 10.  Both are
 *                  decided on z itself: z_j > 10^((-70 + 0.691) / 10), and z_j > 0.1 x that mean.
 *   Integrated:    L = -0.691 + 10 log10(mean of the z_j past both gates); -inf when no block passes the absolute gate or N = 0.
 *   Gain:          g = 1 when target_lufs is NaN (measure only) or L = -inf.  Else g = 10^((target_lufs - L) / 20), then
 *                  g = min(g, 10^(max_gain_db / 20)), then g = min(g, peak_ceiling / max|x|) when max|x| > 0; computed in f64,
 *                  rounded to f32 once, and stepped down by an ulp where that rounding would carry max|x| * g past
 *                  peak_ceiling.  The ceiling is on the SAMPLE peak, not the true peak: the signal between the samples may
 *                  pass it.
 *   Outputs:       out_f32[n] = x[n] * g (one f32 multiply); out_i16[n] = clamp(rintf(out_f32[n] * 32768), -32768, 32767), the
 *                  rule of MI355TTS_PCM_SATURATE; every output row is zero-filled from its N up to out_ld.
 *                  lufs_out / gain_out / peak_out (host [B], each or NULL): L, the linear g that was applied, max|x|.
 *                  weighted_out ([B][in_ld], or NULL; a device pointer with MI355TTS_OUT_DEVICE, like out_f32 / out_i16): the
 *                  K-weighted signal itself, N samples | zeros up to in_ld, so that a test can compare every sample.
 *   Arithmetic:    the recurrence runs in f64 on the caller's f32 coefficients (widened), exactly decomposed: chunks of 64
 *                  samples from zero state, their 4-element states carried across the chunk seams with the powers of the chunk
 *                  transition matrix (computed at load time in double), then every chunk again from its true state.  The
 *                  weighted samples are rounded to f32; the sums of their squares are f64, per hop-sized segment in a fixed
 *                  order, a block is the sum of its segments; z_j and L are f32 values, g is computed in f64 and rounded once.
 *                  The order of every sum is fixed by the row alone, not by the grid or B; no sum uses an atomic.  Row b of a
 *                  batch gives the bits of its own batch-1 call; int16 input is converted as s * 2^-15 (exact) inside the launch
 *                  and gives the bits of the equal f32 input; host and device pointers give the same bits.
 * mi355tts_load_loudness: computes the transition-matrix powers and keeps them on the device; mi355tts_unload frees the model.
 * mi355tts_loudness: exactly one of in_f32 / in_i16 [B][in_ld] (host, or device with MI355TTS_IN_DEVICE); row b holds samples[b]
 * <= in_ld samples (host array).  out_f32 / out_i16 [B][out_ld] (host, or device with MI355TTS_OUT_DEVICE) are optional: a call
 * with no output pointer at all is valid and measures only.  The workspace grows on demand (mi355tts_reserve does not cover this
 * call).
 * MI355TTS_ERR_INVALID with the reason (MI355TTS_ERR_NO_MODEL for an unknown id): null pointers; both inputs or neither; a
 * non-finite coefficient; block < 1; hop < 1 or hop > block; samples[b] outside [0, in_ld] or above 2^24; out_ld below the
 * longest row (when an output is asked for); peak_ceiling outside (0, 1]; a non-finite max_gain_db.
 * Added in ABI version 2 (additive: the version number is unchanged). */
typedef struct {
  float shelf_b[3], shelf_a[2]; /* b0 b1 b2, a1 a2 (a0 = 1) */
  float hp_b[3], hp_a[2];
  int32_t block, hop;           /* 1 <= hop <= block */
} mi355tts_loudness_params;
int mi355tts_load_loudness(mi355tts_ctx* ctx, const mi355tts_loudness_params* params, int* model_out);
int mi355tts_loudness(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                      int64_t in_ld, float target_lufs, float peak_ceiling, float max_gain_db, float* out_f32, int16_t* out_i16,
                      int64_t out_ld, float* lufs_out, float* gain_out, float* peak_out, float* weighted_out, uint32_t flags);

/* ---- limiter: a true-peak meter and a look-ahead limiter for the delivered rows --
 * mi355tts_loudness delivers a row at ONE gain, capped by peak_ceiling / max|x|: a row with a high peak-to-loudness ratio comes
 * out under its target.  This measures a row's TRUE peak (ITU-R BS.1770-4 Annex 2: the peak of the oversampled signal) and
 * delivers the row at the full gain G with only the neighbourhood of each peak turned down, where the samples already are:
 * TWO launches for a meter call, SIX for a limited row, whatever N and B are (csrc/limiter.h).  The reference has no such step.
 * Per row x[0 .. N); everything outside the row is silence; no state is kept across calls.
 *   Parameters (fixed at load time): oversample os in 1 .. 8 (BS.1770 uses 4); a symmetric interpolation prototype
 *                  taps[2 H + 1] at the oversampled rate, at most 128 taps per phase, the caller's
 *                  (larynx_amd.limiter.design_interpolator); lookahead la in 0 .. 1024 samples; release a in [0, 1): the depth
 *                  decays by a per sample; a smoothing window w[la + 1], finite, non-negative, its sum (in double) within 1e-6
 *                  of 1 (larynx_amd.limiter.smoothing_window).
 *   Per call:      a gain G[b] per row (host array; NULL: 1) and ceiling in (0, 1].
 *   1 Interpolation  u[m] = sum_i x[i] taps[m + H - i os] for m in [0, N os): the arithmetic and term order of mi355tts_resample
 *                  with up = os, down = 1 (f32, one fma per term, the polyphase row of phase (m + H) mod os walked from its
 *                  first entry, one accumulator from +0), so max|u| equals, bit for bit, the maximum over that call's output.
 *   2 True peak    tp[n] = max(|x[n]|, max over p < os of |u[n os + p]|); the row's TP = max_n tp[n].  With os = 1 no taps are
 *                  read and tp = |x|.
 *   3 Required gain  c[n] = 1 where tp[n] * G <= ceiling (one f32 product), else ceiling / (tp[n] * G), one correctly rounded
 *                  f32 division.  Outside [0, N), c = 1.
 *   4 Hold         m[k] = min(c[k - 1], .., c[k + la]) for k = -la .. N - 1 (the k - 1 term: a peak between samples k - 1 and
 *                  k turns both down).
 *   5 Release      d[-la - 1] = 0, d[k] = max(1 - m[k], a d[k - 1]): the depth, f32.
 *   6 Smoothing    s[n] = max(0, 1 - sum over j = 0 .. la of w[j] d[n - j]), j ascending, one fma per term from +0, then one
 *                  subtraction.  (With r = 1 - d this is sum_j w[j] r[n - j] for a window that sums to 1; it is taken on the
 *                  depth so that a row that needs no limiting has s = 1 and s <= 1 holds for every window, both exactly.)  Every
 *                  d[n - j] >= 1 - m[n - j] >= 1 - min(c[n], c[n - 1]), so s[n] <= min(c[n], c[n - 1]) up to the window's
 *                  distance from sum 1 and f32 round-off: the property that makes it a limiter.
 *   7 Delivery     out_f32[n] = clamp((x[n] * G) * s[n], -ceiling, +ceiling) (the clamp catches the round-off above);
 *                  out_i16[n] = clamp(rintf(out_f32[n] * 32768), -32768, 32767), the rule of MI355TTS_PCM_SATURATE; every output
 *                  row is zero-filled from its N up to out_ld.
 *   Outputs (each optional): out_f32 / out_i16 [B][out_ld] and curve_out [B][in_ld] (s itself, zeros behind N: for tests, like
 *                  weighted_out), host, or device with MI355TTS_OUT_DEVICE; true_peak_out [B] (host): TP of the INPUT, before
 *                  G; min_gain_out [B] (host): min_n s[n] (1 for an empty row).  A call with no waveform output and no curve is a
 *                  METER CALL: it runs only the two launches TP needs, and min_gain_out receives 1.
 *   Arithmetic:    all f32.  The release is the one recurrence; its operator (max, x a^len) is associative, so it is decomposed:
 *                  chunks of 16 positions from d = 0, the chunks' end states scanned inside a workgroup of 256 chunks, the
 *                  workgroups' end states carried in sequence, every position resolved from its true start state, with the
 *                  powers a^0 .. a^4096 computed in double at load time and rounded to f32 once.  With a = 0 every step is the
 *                  sequential definition bit for bit; with a > 0 a carried term is a^len * d in ONE product where the sequential
 *                  form multiplies len times.  No atomics; every order is fixed by the row alone.  Row b of a batch gives the
 *                  bits of its own batch-1 call; int16 input is converted as s * 2^-15 (exact) inside the launch and gives the
 *                  bits of the equal f32 input; host and device pointers give the same bits.
 * mi355tts_load_limiter: lays out the polyphase table and the powers on the device; taps may be NULL with oversample 1;
 * mi355tts_unload frees the model.
 * mi355tts_limit: exactly one of in_f32 / in_i16 [B][in_ld] (host, or device with MI355TTS_IN_DEVICE); row b holds samples[b]
 * <= in_ld <= 2^24 samples (host array).  The workspace grows on demand (mi355tts_reserve does not cover this call).
 * MI355TTS_ERR_INVALID with the reason (MI355TTS_ERR_NO_MODEL for an unknown id): null pointers; oversample outside [1, 8];
 * half_len < 0; more than 128 taps per phase; a non-finite tap; lookahead outside [0, 1024]; release outside [0, 1); a
 * non-finite or negative window entry; a window sum further than 1e-6 from 1; both inputs or neither; samples[b] outside
 * [0, in_ld] or above 2^24; out_ld below the longest row (when a waveform output is asked for); ceiling outside (0, 1]; a
 * non-finite or negative G[b].
 * Added in ABI version 2 (additive: the version number is unchanged). */
typedef struct {
  int32_t oversample; /* 1 .. 8 */
  int32_t half_len;   /* H >= 0: the prototype has 2 H + 1 taps, at most 128 per phase (ignored with oversample 1) */
  int32_t lookahead;  /* 0 .. 1024 samples */
  float release;      /* [0, 1): the depth's decay per sample */
} mi355tts_limiter_params;
int mi355tts_load_limiter(mi355tts_ctx* ctx, const mi355tts_limiter_params* params, const float* taps, const float* window,
                          int* model_out);
int mi355tts_limit(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                   int64_t in_ld, const float* gain, float ceiling, float* out_f32, int16_t* out_i16, int64_t out_ld,
                   float* true_peak_out, float* min_gain_out, float* curve_out, uint32_t flags);

/* ---- pitch: a YIN F0 tracker for the delivered rows, or any recording -----------
 * Timing (mi355tts_mel_durations, mi355tts_glow_align) and level (mi355tts_loudness) can be read; this reads the third part of
 * prosody: the fundamental frequency per frame, with how periodic the frame is and how loud.  YIN (de Cheveigne & Kawahara
 * 2002) steps 1-5, without the best-local-estimate step; ONE launch per call, whatever N and B are (csrc/pitch.h).  The
 * reference has no such step.
 *   Parameters (fixed at load time): sample_rate; hop; window W, a multiple of 4 in [64, 2048]; the lag range 1 <= tau_min <=
 *                  tau_max <= 1024 with W + tau_max <= 3072; threshold theta in (0, 1]; interpolate (0 / 1).
 *   Frames:        a row of N samples has F = floor(N / hop) frames (none for N < hop); frame t starts at s = t hop - W / 2, so
 *                  it is centred on hop t like a frame of mi355tts_mel_from_audio; x[i] = 0 for i outside [0, N); int16
 *                  samples are s * 2^-15 (exact).  No state across calls.
 *   1 Difference   d(tau) = sum_{j < W} (x[s + j] - x[s + j + tau])^2 for tau = 1 .. tau_max, in f32, in the DIFFERENCE FORM:
 *                  one subtraction, then one fma per term (never r(0) - 2 r(tau)), so a signal with an integer period P has
 *                  d(P) == 0 exactly.  Order: four accumulators from +0, accumulator m takes the terms j = m (mod 4) with j
 *                  ascending; d = (a0 + a1) + (a2 + a3).
 *   2 Level        r0 = sum_j x[s + j]^2: 256 accumulators from +0, accumulator i takes j = i, i + 256, .. ascending, one fma
 *                  per term; the accumulators 64 w .. 64 w + 63 are summed by a butterfly (v[l] += v[l ^ m] for m = 32, 16, ..
 *                  1), and r0 = (p0 + p1) + (p2 + p3) over the four results.  level_db = 10 log10f(r0 / W) where r0 / W >
 *                  1e-10, else -100 (= 10 log10 of the floor 1e-10).
 *   3 Normalise    c(tau) = sum_{k <= tau} d(k); d'(0) = 1; d'(tau) = c(tau) > 0 ? (d(tau) * tau) / c(tau) : 1 (one f32
 *                  product, one correctly rounded f32 division).  Order of c: the lags 1 .. 1024 (d = 0 behind tau_max) in
 *                  256 groups of four, l1 .. l4 the running sums inside a group in sequence; an inclusive Hillis-Steele scan
 *                  of l4 over each 64 groups (v[i] += v[i - st] for i >= st, st = 1, 2, .. 32); the four scans' totals added in
 *                  sequence, T0, T0 + T1, (T0 + T1) + T2; c = (offset of the 64 groups + the scan value of the group before,
 *                  0 for the first) + l_m.
 *   4 Pick         tau_p = the smallest tau in [tau_min, tau_max] with d'(tau) < theta, advanced while tau_p + 1 <= tau_max
 *                  and d'(tau_p + 1) < d'(tau_p).  No such tau: the frame is UNVOICED, f0 = 0, and tau_p is the first
 *                  minimiser of d' over the range.
 *   5 Outputs      periodicity = max(0, 1 - d'(tau_p)).  Voiced: f0 = sample_rate / tau*, tau* = tau_p + (0.5 (a - c)) /
 *                  ((a - 2 b) + c) on a, b, c = d'(tau_p - 1), d'(tau_p), d'(tau_p + 1) when interpolate is set, tau_p - 1 >=
 *                  1, tau_p + 1 <= tau_max and the denominator is > 0; else tau* = tau_p.  All f32, in this order.
 *   Outputs:       f0_out / periodicity_out / level_db_out [B][out_ld], each optional but at least one given; out_ld >= the
 *                  longest row's frame count; entries behind a row's frames are written 0.  cmnd_out (optional) [B][out_ld]
 *                  [tau_max + 1]: d' of every frame (zeros behind a row's frames), so that a test can see the whole kernel.
 *                  Host, or device with MI355TTS_OUT_DEVICE; the input host, or device with MI355TTS_IN_DEVICE.
 *   Arithmetic:    every order above is fixed by the frame alone.  No atomics.  Row b of a batch gives the bits of its own
 *                  batch-1 call; int16 input gives the bits of the equal f32 input; host and device pointers give the same
 *                  bits.  A batch whose rows all have no frame is valid, writes the zeros and launches nothing.
 * mi355tts_load_pitch: checks and keeps the parameters; mi355tts_unload frees the model.  mi355tts_pitch_frames: floor(samples /
 * hop).  mi355tts_pitch: exactly one of in_f32 / in_i16 [B][in_ld]; row b holds samples[b] <= in_ld samples (host array).  The
 * workspace grows on demand (mi355tts_reserve does not cover this call).
 * MI355TTS_ERR_INVALID with the reason (MI355TTS_ERR_NO_MODEL for an unknown id): null pointers; sample_rate < 1; hop outside
 * [1, 4096]; window not a multiple of 4 in [64, 2048]; not 1 <= tau_min <= tau_max <= 1024; window + tau_max > 3072; threshold
 * outside (0, 1]; both inputs or neither; no result plane; samples[b] outside [0, in_ld] or above 2^30; out_ld below the longest
 * row's frame count.
 * Added in ABI version 2 (additive: the version number is unchanged). */
typedef struct {
  int32_t sample_rate, hop, window, tau_min, tau_max;
  float threshold;
  int32_t interpolate;
} mi355tts_pitch_params;
int mi355tts_load_pitch(mi355tts_ctx* ctx, const mi355tts_pitch_params* params, int* model_out);
int64_t mi355tts_pitch_frames(mi355tts_ctx* ctx, int model, int64_t samples);
int mi355tts_pitch(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                   int64_t in_ld, float* f0_out, float* periodicity_out, float* level_db_out, float* cmnd_out, int64_t out_ld,
                   uint32_t flags);

/* ---- pitch shift and tempo: a period-synchronous overlap-add stretch ------------
 * Timing and level can be set (durations, id_length_scales; mi355tts_loudness, mi355tts_limit); this sets the third part of
 * prosody.  A pitch shift by rho = up / down is a time stretch by rho followed by resampling by down / up; only the stretch is
 * new: an overlap-add of windowed frames, each frame's read position moved by a whole number of local pitch periods (the period
 * from mi355tts_pitch's f0 of the same row), so that overlapping frames stay in phase.  Time domain, no transcendental function;
 * csrc/shift.h.  The reference has no such step.  This is resampling, NOT PSOLA: the formants move with the pitch, so the PITCH
 * mode is meant for about +-4 semitones.  One ratio per model and per call.
 *   Parameters (fixed at load time): up, down coprime, each in [1, 64]; window = N, a multiple of 4 in [64, 2048], Hs = N / 2; the
 *                  window w[N], the caller's (finite values; larynx_amd.shift.ola_window: a periodic Hann whose halves sum to 1);
 *                  pitch = the id of a loaded pitch model (its sample_rate, hop = hop_p and lag range are used); resampler = the
 *                  id of a loaded resampler whose (up, down) is this model's (down, up), or 0.  A resampler gives the PITCH mode
 *                  (same duration, pitch x up / down), 0 the TEMPO mode (duration x up / down, pitch unchanged).  The model pins
 *                  both: unloading their ids later does not break it.
 *   1 Periods      f0[j], j < Fp = floor(n / hop_p): exactly what mi355tts_pitch gives for the row (the same launch).
 *   2 Positions    L = ceil(n up / down); K = L > 0 ? (L - 1) / Hs + 2 : 0 frames; for k < K: c_k = floor(k Hs down / up) (64-bit),
 *                  a_k = c_k - Hs.  s_0 = a_0.  For k >= 1: j = min(Fp - 1, (c_k + hop_p / 2) / hop_p); Fp == 0 or f0[j] == 0
 *                  (unvoiced): s_k = a_k; else T = (float)sample_rate / f0[j] (one correctly rounded f32 division), e = (s_(k-1)
 *                  + Hs) - a_k, q = rintf((float)e / T), m = rintf(q * T) (one f32 product, nothing fused), s_k = a_k + (e -
 *                  (int)m).  rintf rounds half to even.  Integers are 32-bit but c_k.
 *   3 Overlap-add  for t in [0, L): k1 = t / Hs, i2 = t - k1 Hs, i1 = i2 + Hs,
 *                  y[t] = rn(rn(w[i1] x[s_k1 + i1]) + rn(w[i2] x[s_(k1+1) + i2])): two f32 products and one f32 add, each rounded
 *                  by itself, NO fused multiply-add; x[i] = 0 outside [0, n); int16 samples are s * 2^-15 (exact).
 *   4 Delivery     TEMPO: y, L samples.  PITCH: the first n samples of what mi355tts_resample defines for y (a row of L samples)
 *                  with the pinned resampler — it would yield ceil(L down / up) >= n; only n are computed — in mi355tts_resample's
 *                  arithmetic and term order.
 *   Outputs:       mi355tts_resample's: out_f32 and / or out_i16 [B][out_ld], pcm_mode MI355TTS_PCM_SATURATE or _NORMALIZE (the peak
 *                  is that of the row's delivered samples); entries behind a row's samples are written 0; samples_out[b]
 *                  (optional) = the row's delivered length.  positions_out (optional) int32 [B][pos_ld]: the s_k, zeros behind a
 *                  row's K, so that a test can see the whole kernel; f0_out (optional) [B][f0_ld]: the plane of step 1.  Outputs
 *                  are host, or device with MI355TTS_OUT_DEVICE; the input (and positions_in) host, or device with
 *                  MI355TTS_IN_DEVICE.
 *   positions_in   (optional) int32 [B][pos_ld]: replaces steps 1 and 2 by the caller's positions, any values (reads outside the
 *                  row are zeros).  A call's own positions_out fed back reproduce its output bit for bit.  Not together with
 *                  positions_out / f0_out.
 *   Arithmetic:    every order above is fixed by the row alone.  No atomics.  Row b of a batch gives the bits of its own batch-1
 *                  call; int16 input gives the bits of the equal f32 input; host and device pointers give the same bits.
 *   Launches:      pitch_kernel, shift_mark_kernel (one wave per row: the recurrence is serial in k), shift_ola_kernel, then PITCH:
 *                  the resampler's one launch, two with MI355TTS_PCM_NORMALIZE; TEMPO: that second launch alone with
 *                  MI355TTS_PCM_NORMALIZE.  With positions_in the first two are not run; pitch_kernel is not run where no row holds a pitch
 *                  frame (every n < hop_p).  A batch whose rows are all empty launches
 *                  nothing and writes zeros.
 * mi355tts_load_shift: checks the parameters, pins the two models, uploads the window; mi355tts_unload frees the model.
 * mi355tts_shift_length: the delivered length of a row of `samples`: samples (PITCH) or ceil(samples up / down) (TEMPO), for 0 <=
 * samples <= 2^24.  mi355tts_shift: exactly one of in_f32 / in_i16 [B][in_ld], at least one of out_f32 / out_i16.  The workspace
 * grows on demand (mi355tts_reserve does not cover this call).
 * MI355TTS_ERR_INVALID with the reason (MI355TTS_ERR_NO_MODEL for an unknown id): null pointers; up / down outside [1, 64] or not
 * coprime; window not a multiple of 4 in [64, 2048]; a window value that is not finite; a resampler whose ratio is not (down, up);
 * up == down together with a resampler; both inputs or neither; no output; an unknown pcm_mode; samples[b] outside [0, in_ld] or
 * above 2^24; out_ld below the longest row's delivered length; pos_ld below the longest row's K (with positions_in or
 * positions_out); f0_ld below the longest row's Fp (with f0_out); positions_in together with positions_out or f0_out.
 * Added in ABI version 2 (additive: the version number is unchanged). */
typedef struct {
  int32_t up, down, window;
  int32_t pitch, resampler; /* model ids; resampler 0 = TEMPO mode */
} mi355tts_shift_params;
int mi355tts_load_shift(mi355tts_ctx* ctx, const mi355tts_shift_params* params, const float* window, int* model_out);
int64_t mi355tts_shift_length(mi355tts_ctx* ctx, int model, int64_t samples);
int mi355tts_shift(mi355tts_ctx* ctx, int model, const float* in_f32, const int16_t* in_i16, const int64_t* samples, int B,
                   int64_t in_ld, const int32_t* positions_in, float* out_f32, int16_t* out_i16, int64_t out_ld, int pcm_mode,
                   int32_t* positions_out, int64_t pos_ld, float* f0_out, int64_t f0_ld, int64_t* samples_out, uint32_t flags);

/* ---- fused call: replaces the model half of _sentence_task -------------------
 * (larynx/__init__.py:229-283: phonemes_to_mels -> mel transforms -> mels_to_audio -> pause
 * padding) with ONE call on one stream: arguments as in mi355tts_glow_infer +
 * mi355tts_hifigan_infer_padded.  `frames_out[b]` receives each row's mel frame count (row b
 * of the output holds pad_before + frames_out[b]*hop samples of padding + audio, then zeros).
 * The frame count is data dependent: if `wav_ld` turns out too small the call returns
 * MI355TTS_ERR_TOO_SMALL with frames_out filled, and the caller retries with a larger buffer.
 * MI355TTS_IN_DEVICE applies to ids / noise, MI355TTS_OUT_DEVICE to the waveform pointers. */
int mi355tts_synthesize(mi355tts_ctx* ctx, int glow, int vocoder, const int64_t* ids, const int32_t* id_lens, int B,
                        int ids_ld, float noise_scale, float length_scale, const float* noise, int noise_ld, uint64_t seed,
                        const mi355tts_audio_settings* audio, float denoiser_strength, int32_t pad_before,
                        int32_t pad_after, int32_t* frames_out, float* wav_f32, int16_t* wav_i16, int64_t wav_ld,
                        uint32_t flags);

/* mi355tts_synthesize for a multi-speaker voice: `speaker_ids` as in mi355tts_glow_infer_speakers. */
int mi355tts_synthesize_speakers(mi355tts_ctx* ctx, int glow, int vocoder, const int64_t* ids, const int32_t* id_lens, int B,
                                 int ids_ld, float noise_scale, float length_scale, const float* noise, int noise_ld,
                                 uint64_t seed, const int32_t* speaker_ids, const mi355tts_audio_settings* audio,
                                 float denoiser_strength, int32_t pad_before, int32_t pad_after, int32_t* frames_out,
                                 float* wav_f32, int16_t* wav_i16, int64_t wav_ld, uint32_t flags);

/* The fused call with mi355tts_prosody (see mi355tts_glow_infer_prosody): the arguments of mi355tts_synthesize_speakers
 * (speaker_ids NULL for a single-speaker voice), then `prosody`; NULL, or a struct with three NULL arrays, behaves exactly like
 * that call.  durations_out is filled before the call returns, also when it returns MI355TTS_ERR_TOO_SMALL, like frames_out.
 * A call that passes any of the three arrays runs on its own (like one with explicit noise, it never shares a coalesced pass). */
int mi355tts_synthesize_prosody(mi355tts_ctx* ctx, int glow, int vocoder, const int64_t* ids, const int32_t* id_lens, int B,
                                int ids_ld, float noise_scale, float length_scale, const float* noise, int noise_ld,
                                uint64_t seed, const int32_t* speaker_ids, const mi355tts_audio_settings* audio,
                                float denoiser_strength, int32_t pad_before, int32_t pad_after, int32_t* frames_out,
                                float* wav_f32, int16_t* wav_i16, int64_t wav_ld, uint32_t flags,
                                const mi355tts_prosody* prosody);

/* Serving set-up (the reference warms its model caches the same way, larynx/__init__.py:290,412):
 * pre-create `workers` per-call workers (stream, side streams, pinned staging) and size
 * their workspaces and the result-block pool for calls of up to max_batch rows x max_ids ids
 * x max_frames mel frames (+ max_pad_samples of pause padding; denoiser != 0 also sizes the
 * STFT scratch), so that no steady-state call allocates device memory.  glow / vocoder may
 * be 0 to size for one model only.  With a GlowTTS model the workspaces also cover mi355tts_glow_align on the same shapes
 * (its [F][P] score matrix and direction bits; a mel_ld up to max_frames rounded up to 4). */
int mi355tts_reserve(mi355tts_ctx* ctx, int workers, int glow, int vocoder, int max_batch, int max_ids, int max_frames,
                     int denoiser, int max_pad_samples);
/* Measurement: the hardware-queue group of every worker of the context, in creation order (groups[i] for worker i; -1 = not probed:
 * a worker created on demand after the last mi355tts_reserve).  The HIP runtime deals its few hardware queues (4) to streams as
 * they are first used, and two streams of one queue run their kernels one after the other; mi355tts_reserve measures which of its
 * worker streams share a queue (one kernel waits for a host flag on stream A while another raises a flag on stream B: if B's does
 * not come up, B sits behind A) and a call then takes the free worker whose queue carries the fewest calls.  Which worker a call
 * gets never changes its result.  Returns the number of workers (only `capacity` entries are written).  MI355TTS_NO_QUEUE_PROBE=1
 * skips the measurement (every worker -1: the most recently released free worker is taken, as before round 6).
 * MI355TTS_QUEUE_POLICY=1: an idle queue first, otherwise the BUSIEST one (as many calls as there are queues get a queue to
 * themselves, the rest share one) instead of the least busy one: measured better only for long runs of the fp16 mode, whose calls
 * are launch-latency chains (1228 against 1166 utterances/s in 200-utterance regions; 1134 against 1149 in the 20-utterance
 * regions; f32: 289 against 294 / 296.6 both) — profiles/r06_queue_map.txt.  No reference
 * counterpart (the reference has one model instance and Python threads: larynx/__init__.py:146-157). */
int mi355tts_worker_queue_groups(mi355tts_ctx* ctx, int32_t* groups, int capacity);

/* ---- single operators (kernel-level parity tests, drop-in conv) ------------- */
/* y[B][Cout][L] = act_out(bias + conv1d(lrelu_slope(x[B][Cin][L]), w[Cout][Cin][K], dilation, "same" padding)) */
int mi355tts_op_conv1d(mi355tts_ctx* ctx, const float* x, int B, int Cin, int L, const int32_t* lens, const float* w,
                       const float* bias, int Cout, int K, int dilation, float in_slope, int out_act, float* y);
/* y[B][Cout][L*stride] = bias + conv_transpose1d(lrelu_slope(x), w[Cin][Cout][K], stride, padding=(K-stride)/2) */
int mi355tts_op_conv_transpose1d(mi355tts_ctx* ctx, const float* x, int B, int Cin, int L, const float* w,
                                 const float* bias, int Cout, int K, int stride, float in_slope, float* y);

/* out[B][N] = denoise(wav[B][N], bias_spec[513], strength): the STFT kernels alone
 * (host buffers), N a multiple of 256 and > 1024 */
int mi355tts_op_denoise(mi355tts_ctx* ctx, const float* wav, int B, int64_t N, const float* bias_spec, float strength,
                        float* out);

/* out[B][C][T] (host) = the device noise generator's N(0,1) draw for (seed, row, channel, frame) —
 * the stand-in for torch.randn_like (glow_tts/models.py:348) that mi355tts_glow_infer uses when
 * `noise` is NULL; exposed so its distribution can be tested. */
int mi355tts_op_gauss_noise(mi355tts_ctx* ctx, uint64_t seed, int B, int C, int T, float* out);

/* maximum_path alone (glow_tts/utils.py:59-96): value host [B][P_ld][F_ld] (the reference's layout), row b is
 * id_lens[b] x frames[b] with frames[b] >= id_lens[b], at most 2048 ids; durations_out host [B][dur_ld] (the path's row sums,
 * zero past id_lens[b]); score_out host [B] or NULL */
int mi355tts_op_maximum_path(mi355tts_ctx* ctx, const float* value, int B, int P_ld, int F_ld, const int32_t* id_lens,
                             const int32_t* frames, int32_t* durations_out, int dur_ld, float* score_out);

/* Test seam: the activation planes of ONE vocoder call.  Runs the generator once on `mel` in the precision the model is switched
 * to and with the context's options, without the denoiser, and writes the float rows wav_f32[B][wav_ld] as
 * mi355tts_hifigan_infer does (same launches, same bits).  A copy of every plane the schedule wrote to memory is taken in
 * stream order right behind the launch that wrote it and kept by the context until the next such call.  `json` receives the
 * taps in launch order: [{"name", "channels", "ld", "len": [valid columns per row], "f16": 0 | 1, "kernel": the name the launch
 * was counted under}, ...].  Names: "mel" (the generator's input as the first conv reads it: the packed plane in fp16), "pre",
 * "up{i}", "rb{i}.{j}.{d}.t" (conv1's stored output, where the schedule materialises it), "rb{i}.{j}.{d}", "stage{i}" (where a
 * kernel writes the MRF average; "stage{i}.sum{m}": the two partial sums of the one-launch narrow stages), "wav".  Refused with a
 * reason when the copies would exceed 256 MB, and for the forked schedule ("mrf_group" = 0 outside fp16), whose side streams a
 * copy cannot be ordered behind.  The other entry points pay host-side tests of a null pointer for this (one where a launch is
 * named, one where a plane would be copied) and nothing on the device. */
int mi355tts_hifigan_infer_taps(mi355tts_ctx* ctx, int vocoder, const mi355tts_mel* mel, float* wav_f32, int64_t wav_ld, char* json,
                                int cap);
/* Tap `index` of the last mi355tts_hifigan_infer_taps as float32 dst[B][channels][ld] (host, `cap` floats); fp16 octet planes are
 * un-permuted and widened, which is exact. */
int mi355tts_voc_tap_copy(mi355tts_ctx* ctx, int index, float* dst, int64_t cap);
/* The acoustic model's twin of that seam: ONE GlowTTS call with the arguments of mi355tts_glow_infer_prosody (same launches, same
 * bits, same mel) that keeps a copy of every f32 plane [B][channels][ld] its schedule wrote, each queued right behind the launch
 * that wrote it — the passes rewrite their planes in place, so every launch's input is some earlier tap.  `json` as above ("f16" is
 * always 0; "kernel" is "-" for a launch counted under no name); mi355tts_voc_tap_copy then serves this call's taps (it serves
 * whichever call tapped last).  A launch that writes two planes leaves two taps.  Names, in launch order: "emb", "pre.{i}",
 * "pre.proj", per encoder layer "enc{l}.qkv" (and "enc{l}.x0", the stored normalised input, from the second layer on),
 * "enc{l}.att", "enc{l}.x1", "enc{l}.ffn", "enc{l}.t1", then "enc.out", "xm", ("dp.spk",) "dp.1", "dp.2", "logw", "z0", per flow
 * block in reverse order "blk{b}.h" (its start conv), "blk{b}.acts{j}", "blk{b}.h{j}" / "blk{b}.skip{j}", "blk{b}.z", and "mel"
 * (the raw mel).  The un-fused forms ("glow_fuse" = 0) file the same names where the same tensor exists and their extra
 * intermediates as "{name}.ln" (a separate LayerNorm's output), "enc{l}.o", "logw.ln", "blk{b}.zc" (the coupling before the
 * mix).  Integer results (frames, durations) are the mel's.  Refused with a reason when the copies would exceed 256 MB; the rows
 * of a coalesced pass are never tapped (only the fused synthesize calls coalesce).  The other entry points pay a host-side test
 * of a null pointer per launch for this and nothing on the device. */
int mi355tts_glow_infer_taps(mi355tts_ctx* ctx, int glow, const int64_t* ids, const int32_t* id_lens, int B, int ids_ld,
                             float noise_scale, float length_scale, const float* noise, int noise_ld, uint64_t seed,
                             const uint64_t* row_seeds, const int32_t* speaker_ids, const mi355tts_audio_settings* audio,
                             uint32_t flags, const mi355tts_prosody* prosody, mi355tts_mel** out, char* json, int cap);

/* Kernel micro-benchmark: `iters` back-to-back launches of the conv kernel on
 * device-resident random data of the given geometry (tile_shape -1 = the
 * launcher's own choice, 0/1/2 = pinned), timed with HIP events on the launch
 * stream; *ms_per_launch receives the average. */
int mi355tts_bench_conv1d(mi355tts_ctx* ctx, int B, int Cin, int Cout, int K, int dilation, int L, int tile_shape,
                          int iters, float* ms_per_launch);

/* ---- measurement -------------------------------------------------------------
 * With profiling on, every kernel launch is bracketed by HIP events on the
 * call's own stream and accumulated per kernel class.  `mi355tts_profile_json`
 * writes {"class": {"launches": n, "ms": t, "flop": f}, ...}. */
int mi355tts_set_profiling(mi355tts_ctx* ctx, int enabled);
/* Options, by what they may change in a RESULT.
 *
 * (1) Schedule options that compute THE SAME BITS under every setting (the same tiles run the same arithmetic; only which
 * launch, stream or workgroup order carries them changes):
 *   "serial_branches" (0/1, default 0) — the three MRF ResBlock chains of a HiFi-GAN stage one after another, one conv per
 *     launch (per-kernel timing); "mrf_group" (0/1, default 1) — the same-geometry launches of the three chains as one grouped
 *     launch; "adaptive_schedule" (0/1, default 0) — while other calls are in flight, launch the members of a group one by one;
 *   "rb_conv" (0/1, default 1) — the grouped 128-row ResBlock launches on the continuous-stream tile of rb_conv.h (0 = the
 *     chunked tile of conv_mfma.h);
 *   "rb_dil" (0/1, default 1) — the grouped ResBlock launches of rb_conv.h / rb_pair.h whose members share a dilation of 1, 3
 *     or 5 on the kernel compiled for that dilation (operand offsets as instruction immediates; 0 = the kernel that reads the
 *     dilation from its arguments, which every other dilation takes anyway);
 *   "group_snake" (0/1, default 1) — the workgroup ORDER of fully resident grouped launches (a snake over the dispatcher's
 *     rounds).  The one option the library may change by itself: mi355tts_dispatch_selfcheck switches it off on a device where
 *     the order does not win;
 *   "gate16_wide" (default 512) — gate convs / 1 x 1 convs of passes with at least this many 16-row tiles (padded batches) take
 *     two / four row tiles per workgroup from one staged input tile (0 = never).
 *   Not an option, the same class: while ANOTHER call holds a worker of the context, a batch-1 grouped ResBlock launch with more
 *     128-column tiles than the chip holds at once runs on them (rb_group_kernel<11, 7, 3, 4>) instead of on 64-column tiles — the
 *     same chain per output element, so which one a call gets depends on the load and its result does not (environment
 *     MI355TTS_RB_NB4_MIN_TILES pins the threshold whatever the load; 0 = never).
 * (2) Tile options: another tile = another f32 SUMMATION ORDER; results equal to f32 round-off, never changed by the library
 * itself (a timing never picks a tile):
 *   "gate16", "glow_fuse", "mrf_small" (0/1, default 1) — the small-launch kernels of gate16.h / coltile.h / mrf_small.h
 *     (0 = the generic tiles);
 *   "rb_pair" (0/1, default 1) — the fused ResBlock steps of the 64- / 32-channel stages on the 4-wave tile without a k-split
 *     (rb_pair.h; 0 = the 8-wave k-split tile of resblock_pair.h).  In the fp16 mode: conv1 + conv2 of a ResBlock1 step as ONE launch
 *     (pair_f16.h; 0 = two launches — there the two forms give the SAME bits);
 *   "group_promote" (0/1, default 1) — at batch 1 the same-geometry ResBlock convs of a step that are too short for the 128-row
 *     tile's own threshold move to it when the round-robin deal of their (all resident) workgroups stays balanced: decided from
 *     the device's CU count and the launch geometry alone (0 = they keep the 64 x 32 k-split tile);
 *   "voc_out" (0/1, default 1) — conv_post + tanh + the rows' peaks as one dedicated launch and the delivery of the rows (pause |
 *     samples | zeros) as one more (voc_out.h; 0 = the generic conv tile, zero_tail, absmax, to_int16 and a copy / fill per
 *     piece of every row: float rows equal to f32 round-off, int16 within 1 LSB).
 * (0) "sync_mode" (0-3, default 3 or MI355TTS_SYNC_MODE; process-wide) — how a caller thread waits for its stream: 0 =
 * hipStreamSynchronize (spins a core), 1 = a blocking event, 2 = hipStreamQuery + 20 us sleeps, 3 = 60 us of polling, then
 * query + 20 us sleeps with the calling thread's timer slack lowered to 1 us FOR THE DURATION OF THE WAIT (prctl
 * PR_SET_TIMERSLACK on the caller's own thread, restored before the call returns; skipped where prctl is denied).
 * (3) "call_coalesce" / "call_coalesce_window_us" (below): with it on, WHICH tiles compute a batch-1 call depends on the calls
 * that happened to share its pass — results equal to f32 round-off across loads, not bit-reproducible. */
int mi355tts_set_option(mi355tts_ctx* ctx, const char* name, int value);
/* Option "call_coalesce" (lanes; 0 = off; the built-in default: mi355tts_call_coalesce_default): concurrent batch-1
 * mi355tts_synthesize calls (the reference's per-sentence thread pool, larynx/__init__.py:146-157, 187-190) become the rows of
 * fused padded calls — acoustic pass AND vocoder — with at most `lanes` such passes in flight: the callers waiting when a lane
 * frees ride one pass, each row with its own seed's noise stream, its own pause padding and its own output buffers.  A lone
 * caller never waits (its pass is its solitary call, same bits); a caller that finds a lane free while other passes are in
 * flight gathers followers for at most "call_coalesce_window_us" (default 300).  Calls with explicit noise, speaker ids,
 * B > 1 or more than 768 ids always run alone.  A row of a padded batch is computed by other tiles than its solitary call:
 * equal to f32 round-off (frames identical, int16 within 1 LSB), not bit-identical.  Counters since the context was created:
 * fused passes run, rows they carried. */
int mi355tts_call_coalesce_default(void);
int mi355tts_coalesce_stats(mi355tts_ctx* ctx, int64_t* passes, int64_t* rows);
/* One-off check of the dispatcher rule the batch-1 ResBlock schedule relies on (grouped launches whose workgroups are all
 * resident go out in a "snake" order that assumes workgroup i lands on CU i mod #CUs; the promotion of a step to the 128-row
 * tile relies on that order): the grouped launch of a 256-channel ResBlock step in the plain and in the snake order, timed on
 * this device.  Runs by itself on the first load of a vocoder with a >= 256-channel stage; where the snake is not at least as
 * fast (2 % margin) the ORDER option "group_snake" is switched off for the context — results are the same bits either way; the
 * promotion rule ("group_promote": a tile choice) is never touched by a timing.  state: 1 = kept, 2 = switched off, 3 = skipped
 * (MI355TTS_NO_SELFCHECK, unsuitable CU count), 4 = running on another thread; times in microseconds per launch.  No
 * reference counterpart. */
int mi355tts_dispatch_selfcheck(mi355tts_ctx* ctx, int* state, float* plain_us, float* snake_us);
int mi355tts_profile_reset(mi355tts_ctx* ctx);
int mi355tts_profile_json(mi355tts_ctx* ctx, char* buf, int cap);
/* The same sums per kernel NAME and launch sub-key (the output rows of a conv launch / the channels of a fused ResBlock step):
 * {"class": {"rb_group_kernel.snake/256": {"launches": n, "ms": t, "flop": f}, ...}, ...}; kernels without a counted name are
 * filed under "-".  No reference counterpart (bench.py's `roofline.by_kernel`). */
int mi355tts_profile_kernels_json(mi355tts_ctx* ctx, char* buf, int cap);
/* Launches per kernel NAME since the last mi355tts_profile_reset, {"rb_group_kernel": n, ...}; counted whether profiling is
 * on or not.  The class counters cannot tell a kernel from the fallback that would silently take its place (same launch count,
 * same bits by design): the device tests assert on these.  The first 44 keys and their order are fixed and always present,
 * zero or not; the names of later entry points (the six loudness_*_kernel, the five limiter_*_kernel, pitch_kernel,
 * shift_mark_kernel, shift_ola_kernel) follow them once they have launched since the last reset.  No reference counterpart (measurement only). */
int mi355tts_kernel_counts_json(mi355tts_ctx* ctx, char* buf, int cap);
/* Median elapsed time (microseconds) of `pairs` EMPTY event pairs on an idle stream: what the two hipEventRecord calls around a
 * profiled launch add to its event-timed duration (rocprofv3's kernel durations do not contain it). */
int mi355tts_profile_event_overhead(mi355tts_ctx* ctx, int pairs, double* us_out);

#ifdef __cplusplus
}
#endif
#endif /* MI355TTS_H */
