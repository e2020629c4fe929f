/* A plain C99 program on the pitch entry points of include/mi355tts.h: a ragged batch of five rows (an empty row and a row
 * shorter than one hop included, unsorted), every output asked for, float and int16 input, and each row again as its own batch-1
 * call, compared bit for bit.  Prints one line per row (frames, voiced frames, the bits of the last voiced f0) and "ok" at
 * the end.  Stand-alone so that it can also be built with the host sanitizers (-fsanitize=address,undefined) against the
 * library's CPU-emulator flavour: profiles/pitch.md has the command. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355tts.h"

#define ROWS 5
#define FS 22050.0
#define HOP 256
#define TAU_MAX 441
#define T1 (TAU_MAX + 1)
static const int64_t LEN[ROWS] = {2561, 0, 5000, 255, 300};
static const double F0[ROWS] = {110.0, 0.0, 196.0, 150.0, 300.0};
#define IN_LD 5040
#define OUT_LD 23 /* past the longest row's 19 frames */

static void die(const char* what) {
  fprintf(stderr, "%s: %s\n", what, mi355tts_last_error());
  exit(1);
}

static uint32_t bits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}

int main(int argc, char** argv) {
  const int device = argc > 1 ? atoi(argv[1]) : 0;
  const double pi = 3.14159265358979323846;
  mi355tts_ctx* ctx = NULL;
  mi355tts_pitch_params p;
  int model = -1, b, k;
  int64_t i;
  float* x = (float*)malloc(sizeof(float) * ROWS * IN_LD);
  int16_t* s = (int16_t*)malloc(sizeof(int16_t) * ROWS * IN_LD);
  float* out = (float*)malloc(sizeof(float) * 3 * ROWS * OUT_LD);
  float* cm = (float*)malloc(sizeof(float) * ROWS * OUT_LD * T1);
  float* out1 = (float*)malloc(sizeof(float) * 3 * OUT_LD);
  float* cm1 = (float*)malloc(sizeof(float) * OUT_LD * T1);
  float* out2 = (float*)malloc(sizeof(float) * 3 * ROWS * OUT_LD);
  uint32_t st = 2002u;
  if (!x || !s || !out || !cm || !out1 || !cm1 || !out2) return 2;
  if (mi355tts_create(device, &ctx)) die("create");
  p.sample_rate = (int32_t)FS;
  p.hop = HOP;
  p.window = 1024;
  p.tau_min = 45;
  p.tau_max = TAU_MAX;
  p.threshold = 0.15f;
  p.interpolate = 1;
  if (mi355tts_load_pitch(ctx, &p, &model)) die("load_pitch");
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
  memset(out, 0x55, sizeof(float) * 3 * ROWS * OUT_LD);
  memset(cm, 0x55, sizeof(float) * ROWS * OUT_LD * T1);
  if (mi355tts_pitch(ctx, model, x, NULL, LEN, ROWS, IN_LD, out, out + ROWS * OUT_LD, out + 2 * ROWS * OUT_LD, cm, OUT_LD, 0)) die("pitch");
  for (b = 0; b < ROWS; ++b) {
    const int64_t n = LEN[b], F = mi355tts_pitch_frames(ctx, model, n);
    int voiced = 0;
    float last = 0.f;
    if (F != n / HOP) return 3;
    if (mi355tts_pitch(ctx, model, x + (size_t)b * IN_LD, NULL, &n, 1, n, out1, out1 + OUT_LD, out1 + 2 * OUT_LD, cm1, OUT_LD, 0)) die("pitch, one row");
    for (k = 0; k < 3; ++k) {
      const float* row = out + ((size_t)k * ROWS + (size_t)b) * OUT_LD;
      if (memcmp(row, out1 + (size_t)k * OUT_LD, sizeof(float) * OUT_LD)) {
        fprintf(stderr, "row %d plane %d differs from its batch-1 call\n", b, k);
        return 1;
      }
      for (i = F; i < OUT_LD; ++i)
        if (row[i] != 0.f) return 3;
    }
    if (memcmp(cm + (size_t)b * OUT_LD * T1, cm1, sizeof(float) * OUT_LD * T1)) return 1;
    for (i = (int64_t)F * T1; i < (int64_t)OUT_LD * T1; ++i)
      if (cm[(size_t)b * OUT_LD * T1 + (size_t)i] != 0.f) return 3;
    for (i = 0; i < F; ++i) {
      const float f0 = out[(size_t)b * OUT_LD + i];
      if (cm[((size_t)b * OUT_LD + (size_t)i) * T1] != 1.0f) return 3; /* d'(0) */
      if (f0 > 0.f) {
        ++voiced;
        last = f0;
      }
    }
    if (F >= 8 && (voiced < F / 2 || fabs(last / F0[b] - 1.0) > 0.02)) return 4; /* the long rows are tracked */
    printf("row %d n %lld frames %lld voiced %d f0 %08x\n", b, (long long)n, (long long)F, voiced, (unsigned)bits(last));
  }
  /* int16 input, two planes alone: the float rows hold the int16 values' neighbours, so only the voicing is compared */
  memset(out2, 0x55, sizeof(float) * 3 * ROWS * OUT_LD);
  if (mi355tts_pitch(ctx, model, NULL, s, LEN, ROWS, IN_LD, out2, NULL, out2 + 2 * ROWS * OUT_LD, NULL, OUT_LD, 0)) die("pitch, int16");
  for (b = 0; b < ROWS; ++b)
    for (i = 0; i < OUT_LD; ++i) {
      const int64_t F = LEN[b] / HOP;
      const float a = out[(size_t)b * OUT_LD + i], c = out2[(size_t)b * OUT_LD + i];
      if (i >= F ? c != 0.f : (F >= 8 && a > 0.f && fabs(c / a - 1.0) > 0.01)) return 5;
    }
  /* no frame in any row: valid, zeros */
  {
    const int64_t none[3] = {0, 255, 17};
    memset(out, 0x55, sizeof(float) * 3 * OUT_LD);
    memset(cm, 0x55, sizeof(float) * 3 * OUT_LD * T1);
    if (mi355tts_pitch(ctx, model, x, NULL, none, 3, IN_LD, out, NULL, NULL, cm, OUT_LD, 0)) die("pitch, empty");
    for (i = 0; i < 3 * OUT_LD; ++i)
      if (out[i] != 0.f) return 6;
    for (i = 0; i < 3 * (int64_t)OUT_LD * T1; ++i)
      if (cm[i] != 0.f) return 6;
  }
  if (mi355tts_pitch(ctx, model, x, NULL, LEN, ROWS, IN_LD, out, NULL, NULL, NULL, 3, 0) != MI355TTS_ERR_INVALID) return 7;
  if (mi355tts_pitch(ctx, model, x, s, LEN, ROWS, IN_LD, out, NULL, NULL, NULL, OUT_LD, 0) != MI355TTS_ERR_INVALID) return 7;
  if (mi355tts_unload(ctx, model)) die("unload");
  mi355tts_destroy(ctx);
  free(x); free(s); free(out); free(cm); free(out1); free(cm1); free(out2);
  printf("ok\n");
  return 0;
}
