/* A plain C99 program on the pitch-shift entry points of include/mi355tts.h: a ragged batch of five rows (an empty row and a row
 * shorter than one pitch hop included, unsorted) through a PITCH-mode model (6 / 5 with a resampler by 5 / 6) and a TEMPO-mode
 * model, every output asked for, float and int16 input; each row again as its own batch-1 call and with its own positions fed
 * back, compared bit for bit.  Prints one line per row and mode and "ok" at the end.  Stand-alone so that it can also be built
 * with the host sanitizers (-fsanitize=address,undefined) against the library's CPU-emulator flavour: profiles/shift.md has the
 * command. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355tts.h"

#define ROWS 5
#define FS 22050.0
#define HOP 256
#define N_WIN 1024
#define UP 6
#define DOWN 5
#define HALF 48 /* the resampler's prototype: 97 taps at the rate x 5 */
static const int64_t LEN[ROWS] = {2561, 0, 5000, 255, 300};
static const double F0[ROWS] = {110.0, 0.0, 196.0, 150.0, 300.0};
#define IN_LD 5040
#define OUT_LD 6011 /* past the longest row's 6000 stretched samples */
#define POS_LD 16   /* past the longest row's 5999 / 512 + 2 = 13 frames */
#define F0_LD 21    /* past the longest row's 19 pitch frames */

static void die(const char* what) {
  fprintf(stderr, "%s: %s\n", what, mi355tts_last_error());
  exit(1);
}

int main(int argc, char** argv) {
  const int device = argc > 1 ? atoi(argv[1]) : 0;
  const double pi = 3.14159265358979323846;
  mi355tts_ctx* ctx = NULL;
  mi355tts_pitch_params pp;
  mi355tts_resampler_params rp;
  mi355tts_shift_params sp;
  int pitch = -1, rs = -1, model[2] = {-1, -1}, b, mode;
  int64_t i;
  float taps[2 * HALF + 1];
  float* win = (float*)malloc(sizeof(float) * N_WIN);
  float* x = (float*)malloc(sizeof(float) * ROWS * IN_LD);
  int16_t* s = (int16_t*)malloc(sizeof(int16_t) * ROWS * IN_LD);
  float* y = (float*)malloc(sizeof(float) * ROWS * OUT_LD);
  int16_t* pcm = (int16_t*)malloc(sizeof(int16_t) * ROWS * OUT_LD);
  int32_t* pos = (int32_t*)malloc(sizeof(int32_t) * ROWS * POS_LD);
  float* f0 = (float*)malloc(sizeof(float) * ROWS * F0_LD);
  float* y1 = (float*)malloc(sizeof(float) * OUT_LD);
  int16_t* pcm1 = (int16_t*)malloc(sizeof(int16_t) * OUT_LD);
  int32_t* pos1 = (int32_t*)malloc(sizeof(int32_t) * POS_LD);
  float* f01 = (float*)malloc(sizeof(float) * F0_LD);
  float* y2 = (float*)malloc(sizeof(float) * ROWS * OUT_LD);
  int64_t got[ROWS];
  uint32_t st = 2002u;
  if (!win || !x || !s || !y || !pcm || !pos || !f0 || !y1 || !pcm1 || !pos1 || !f01 || !y2) return 2;
  if (mi355tts_create(device, &ctx)) die("create");
  pp.sample_rate = (int32_t)FS;
  pp.hop = HOP;
  pp.window = 896;
  pp.tau_min = 45;
  pp.tau_max = 441;
  pp.threshold = 0.15f;
  pp.interpolate = 1;
  if (mi355tts_load_pitch(ctx, &pp, &pitch)) die("load_pitch");
  for (i = -HALF; i <= HALF; ++i) { /* a Hann-windowed sinc with its cutoff at the lower Nyquist rate, gain up = 5 */
    const double u = (double)i / UP, sinc = i ? sin(pi * u) / (pi * u) : 1.0;
    taps[i + HALF] = (float)((double)DOWN / UP * sinc * (0.5 + 0.5 * cos(pi * (double)i / (HALF + 1))));
  }
  rp.up = DOWN;
  rp.down = UP;
  rp.half_len = HALF;
  if (mi355tts_load_resampler(ctx, &rp, taps, &rs)) die("load_resampler");
  for (i = 0; i < N_WIN / 2; ++i) {
    win[i] = (float)(0.5 - 0.5 * cos(2.0 * pi * (double)i / N_WIN));
    win[i + N_WIN / 2] = 1.0f - win[i];
  }
  sp.up = UP;
  sp.down = DOWN;
  sp.window = N_WIN;
  sp.pitch = pitch;
  sp.resampler = rs;
  if (mi355tts_load_shift(ctx, &sp, win, &model[0])) die("load_shift, pitch mode");
  sp.resampler = 0;
  if (mi355tts_load_shift(ctx, &sp, win, &model[1])) die("load_shift, tempo mode");
  sp.resampler = rs;
  sp.up = DOWN;
  if (mi355tts_load_shift(ctx, &sp, win, &b) != MI355TTS_ERR_INVALID) return 7; /* 5 / 5 */
  /* the shift models pin what they run: the ids may go first */
  if (mi355tts_unload(ctx, pitch) || mi355tts_unload(ctx, rs)) die("unload");
  for (b = 0; b < ROWS; ++b)
    for (i = 0; i < IN_LD; ++i) {
      float v = 0.25f; /* what lies past a row's samples must not be read */
      if (i < LEN[b]) {
        const double ph = 2.0 * pi * F0[b] * (double)i / FS;
        st = st * 1664525u + 1013904223u;
        v = (float)(0.3 * sin(ph) + 0.15 * sin(2.0 * ph) + 0.1 * sin(3.0 * ph)) + 0.002f * ((float)(st >> 8) / 8388608.0f - 1.0f);
      }
      x[(size_t)b * IN_LD + i] = v;
      s[(size_t)b * IN_LD + i] = (int16_t)lrintf(v * 32767.0f);
    }
  for (mode = 0; mode < 2; ++mode) {
    const int m = model[mode];
    memset(y, 0x55, sizeof(float) * ROWS * OUT_LD);
    memset(pcm, 0x55, sizeof(int16_t) * ROWS * OUT_LD);
    memset(pos, 0x55, sizeof(int32_t) * ROWS * POS_LD);
    memset(f0, 0x55, sizeof(float) * ROWS * F0_LD);
    if (mi355tts_shift(ctx, m, x, NULL, LEN, ROWS, IN_LD, NULL, y, pcm, OUT_LD, MI355TTS_PCM_NORMALIZE, pos, POS_LD, f0, F0_LD, got, 0)) die("shift");
    for (b = 0; b < ROWS; ++b) {
      const int64_t n = LEN[b], L = (n * UP + DOWN - 1) / DOWN, K = L > 0 ? (L - 1) / (N_WIN / 2) + 2 : 0, F = n / HOP;
      const int64_t out = mode == 0 ? n : L;
      const float* row = y + (size_t)b * OUT_LD;
      int64_t one = -1;
      int moved = 0, peak = 0;
      if (got[b] != out || mi355tts_shift_length(ctx, m, n) != out) return 3;
      if (mi355tts_shift(ctx, m, x + (size_t)b * IN_LD, NULL, &n, 1, n, NULL, y1, pcm1, OUT_LD, MI355TTS_PCM_NORMALIZE, pos1, POS_LD, f01, F0_LD, &one, 0))
        die("shift, one row");
      if (one != out || memcmp(row, y1, sizeof(float) * OUT_LD) || memcmp(pcm + (size_t)b * OUT_LD, pcm1, sizeof(int16_t) * OUT_LD) ||
          memcmp(pos + (size_t)b * POS_LD, pos1, sizeof(int32_t) * POS_LD) || memcmp(f0 + (size_t)b * F0_LD, f01, sizeof(float) * F0_LD)) {
        fprintf(stderr, "mode %d row %d differs from its batch-1 call\n", mode, b);
        return 1;
      }
      for (i = out; i < OUT_LD; ++i)
        if (row[i] != 0.f || pcm[(size_t)b * OUT_LD + i] != 0) return 3;
      for (i = K; i < POS_LD; ++i)
        if (pos[(size_t)b * POS_LD + i] != 0) return 3;
      for (i = F; i < F0_LD; ++i)
        if (f0[(size_t)b * F0_LD + i] != 0.f) return 3;
      for (i = 0; i < K; ++i) /* a_k = floor(k Hs down / up) - Hs */
        if (pos[(size_t)b * POS_LD + i] != (int32_t)(i * (N_WIN / 2) * DOWN / UP - N_WIN / 2)) ++moved;
      for (i = 0; i < out; ++i) {
        const int a = abs((int)pcm[(size_t)b * OUT_LD + i]);
        if (a > peak) peak = a;
      }
      if (n && peak < 32766) return 4; /* normalised: the peak lands on 32767 (the scaling truncates: or 32766) */
      if (F >= 8 && moved < 2) return 4; /* the long rows are voiced: their frames move by whole periods */
      /* the row's own positions fed back: the same bits */
      if (mi355tts_shift(ctx, m, x + (size_t)b * IN_LD, NULL, &n, 1, n, pos1, y1, NULL, OUT_LD, MI355TTS_PCM_SATURATE, NULL, POS_LD, NULL, 0, NULL, 0))
        die("shift, positions_in");
      if (memcmp(row, y1, sizeof(float) * OUT_LD)) return 5;
      printf("mode %d row %d n %lld out %lld frames %lld moved %d peak %d\n", mode, b, (long long)n, (long long)out, (long long)K, moved, peak);
    }
    /* int16 input: the float rows hold the int16 values' neighbours, so the result is near, not equal */
    if (mi355tts_shift(ctx, m, NULL, s, LEN, ROWS, IN_LD, NULL, y2, NULL, OUT_LD, MI355TTS_PCM_SATURATE, NULL, 0, NULL, 0, got, 0)) die("shift, int16");
    for (b = 0; b < ROWS; ++b)
      for (i = 0; i < OUT_LD; ++i)
        if (i >= got[b] && y2[(size_t)b * OUT_LD + i] != 0.f) return 6;
    /* no sample in any row: valid, zeros */
    {
      const int64_t none[3] = {0, 0, 0};
      memset(y, 0x55, sizeof(float) * 3 * OUT_LD);
      memset(pos, 0x55, sizeof(int32_t) * 3 * POS_LD);
      if (mi355tts_shift(ctx, m, x, NULL, none, 3, IN_LD, NULL, y, NULL, OUT_LD, MI355TTS_PCM_SATURATE, pos, POS_LD, NULL, 0, got, 0)) die("shift, empty");
      for (i = 0; i < 3 * (int64_t)OUT_LD; ++i)
        if (y[i] != 0.f) return 6;
      for (i = 0; i < 3 * POS_LD; ++i)
        if (pos[i] != 0) return 6;
    }
    if (mi355tts_shift(ctx, m, x, NULL, LEN, ROWS, IN_LD, NULL, y, NULL, 100, 0, NULL, 0, NULL, 0, NULL, 0) != MI355TTS_ERR_INVALID) return 7;
    if (mi355tts_shift(ctx, m, x, s, LEN, ROWS, IN_LD, NULL, y, NULL, OUT_LD, 0, NULL, 0, NULL, 0, NULL, 0) != MI355TTS_ERR_INVALID) return 7;
    if (mi355tts_shift(ctx, m, x, NULL, LEN, ROWS, IN_LD, NULL, y, NULL, OUT_LD, 0, pos, 12, NULL, 0, NULL, 0) != MI355TTS_ERR_INVALID) return 7;
    if (mi355tts_unload(ctx, m)) die("unload");
  }
  mi355tts_destroy(ctx);
  free(win); free(x); free(s); free(y); free(pcm); free(pos); free(f0); free(y1); free(pcm1); free(pos1); free(f01); free(y2);
  printf("ok\n");
  return 0;
}
