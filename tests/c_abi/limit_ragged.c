/* A plain C99 program on the limiter entry points of include/mi355tts.h: a ragged batch of eight rows (zero-length rows
 * included, lengths at the edges of a tile, a chunk and a workgroup, unsorted), a gain per row, every output asked for, float and
 * int16 input, a meter call, and each row again as its own batch-1 call, compared bit for bit.  Prints one line per row (the bits
 * of the true peak, the smallest gain and the delivered peak) and "ok" at the end.  Stand-alone so that it can also be built with
 * the host sanitizers (-fsanitize=address,undefined) against the library's CPU-emulator flavour: profiles/limiter.md has the
 * command. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355tts.h"

#define ROWS 8
#define FS 22050.0
#define OS 4
#define HALF 64 /* 16 zero crossings at 4 x */
#define LA 33
static const int64_t LEN[ROWS] = {257, 0, 9000, 1, 4063, 0, 33, 4097};
static const float GAIN[ROWS] = {2.0f, 1.0f, 2.5f, 3.0f, 2.0f, 7.0f, 0.5f, 1.7f};
#define IN_LD 9040
#define OUT_LD 9061

static void die(const char* what) {
  fprintf(stderr, "%s: %s\n", what, mi355tts_last_error());
  exit(1);
}

static double bessel_i0(double x) {
  double s = 1.0, t = 1.0;
  int k;
  for (k = 1; k < 60; ++k) {
    t *= (x / (2.0 * k)) * (x / (2.0 * k));
    s += t;
  }
  return s;
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
  mi355tts_limiter_params p;
  int model = -1, b, j;
  int64_t i;
  const float ceiling = 0.8912509f;
  float taps[2 * HALF + 1], win[LA + 1];
  double wsum = 0;
  float* x = (float*)malloc(sizeof(float) * ROWS * IN_LD);
  int16_t* s = (int16_t*)malloc(sizeof(int16_t) * ROWS * IN_LD);
  float* of = (float*)malloc(sizeof(float) * ROWS * OUT_LD);
  int16_t* oi = (int16_t*)malloc(sizeof(int16_t) * ROWS * OUT_LD);
  float* oc = (float*)malloc(sizeof(float) * ROWS * IN_LD);
  float* f1 = (float*)malloc(sizeof(float) * IN_LD);
  int16_t* i1 = (int16_t*)malloc(sizeof(int16_t) * IN_LD);
  float* c1 = (float*)malloc(sizeof(float) * IN_LD);
  float tp[ROWS], mn[ROWS], tp2[ROWS], mn2[ROWS];
  uint32_t st = 2025u;
  if (!x || !s || !of || !oi || !oc || !f1 || !i1 || !c1) return 2;
  if (mi355tts_create(device, &ctx)) die("create");
  for (j = -HALF; j <= HALF; ++j) { /* a Kaiser-windowed sinc, beta 9 */
    const double t = (double)j / OS, r = (double)j / HALF;
    const double sinc = j ? sin(pi * t) / (pi * t) : 1.0;
    taps[j + HALF] = (float)(sinc * bessel_i0(9.0 * sqrt(1.0 - r * r)) / bessel_i0(9.0));
  }
  for (j = 0; j <= LA; ++j) wsum += 0.5 - 0.5 * cos(2.0 * pi * (j + 1) / (LA + 2)); /* a Hann window without its zero ends */
  for (j = 0; j <= LA; ++j) win[j] = (float)((0.5 - 0.5 * cos(2.0 * pi * (j + 1) / (LA + 2))) / wsum);
  p.oversample = OS;
  p.half_len = HALF;
  p.lookahead = LA;
  p.release = (float)exp(-1.0 / (50.0 * FS / 1000.0));
  if (mi355tts_load_limiter(ctx, &p, taps, win, &model)) die("load_limiter");
  for (b = 0; b < ROWS; ++b)
    for (i = 0; i < IN_LD; ++i) {
      float v = 0.25f; /* what lies past a row's samples must not be read */
      if (i < LEN[b]) {
        st = st * 1664525u + 1013904223u;
        v = 0.3f * (float)sin(2.0 * pi * 140.0 * (double)(b + 1) * (double)i / FS) + 0.02f * ((float)(st >> 8) / 8388608.0f - 1.0f);
        if (i % 1000 == 0 || i == LEN[b] - 1) v = (i & 1) ? -0.9f : 0.9f; /* clicks, one at either end */
      }
      x[(size_t)b * IN_LD + i] = v;
      s[(size_t)b * IN_LD + i] = (int16_t)lrintf(v * 32767.0f);
    }
  memset(of, 0x55, sizeof(float) * ROWS * OUT_LD);
  memset(oi, 0x55, sizeof(int16_t) * ROWS * OUT_LD);
  memset(oc, 0x55, sizeof(float) * ROWS * IN_LD);
  if (mi355tts_limit(ctx, model, x, NULL, LEN, ROWS, IN_LD, GAIN, ceiling, of, oi, OUT_LD, tp, mn, oc, 0)) die("limit");
  for (b = 0; b < ROWS; ++b) {
    const int64_t n = LEN[b];
    float t1, m1, peak = 0.f;
    if (mi355tts_limit(ctx, model, x + (size_t)b * IN_LD, NULL, &n, 1, n, GAIN + b, ceiling, f1, i1, n, &t1, &m1, c1, 0)) die("limit, one row");
    if (bits(t1) != bits(tp[b]) || bits(m1) != bits(mn[b]) || memcmp(f1, of + (size_t)b * OUT_LD, sizeof(float) * (size_t)n) ||
        memcmp(i1, oi + (size_t)b * OUT_LD, sizeof(int16_t) * (size_t)n) || memcmp(c1, oc + (size_t)b * IN_LD, sizeof(float) * (size_t)n)) {
      fprintf(stderr, "row %d differs from its batch-1 call\n", b);
      return 1;
    }
    for (i = 0; i < n; ++i) peak = fmaxf(peak, fabsf(of[(size_t)b * OUT_LD + i]));
    for (i = n; i < OUT_LD; ++i)
      if (of[(size_t)b * OUT_LD + i] != 0.f || oi[(size_t)b * OUT_LD + i] != 0) return 3;
    for (i = n; i < IN_LD; ++i)
      if (oc[(size_t)b * IN_LD + i] != 0.f) return 3;
    printf("row %d n %lld tp %08x min %08x peak %08x\n", b, (long long)n, (unsigned)bits(tp[b]), (unsigned)bits(mn[b]), (unsigned)bits(peak));
  }
  /* a meter call: no output pointer at all, NULL gains */
  if (mi355tts_limit(ctx, model, x, NULL, LEN, ROWS, IN_LD, NULL, 1.0f, NULL, NULL, 0, tp2, mn2, NULL, 0)) die("limit, meter");
  for (b = 0; b < ROWS; ++b)
    if (bits(tp2[b]) != bits(tp[b]) || mn2[b] != 1.0f) return 4;
  /* int16 input, the int16 rows alone */
  if (mi355tts_limit(ctx, model, NULL, s, LEN, ROWS, IN_LD, GAIN, ceiling, NULL, oi, OUT_LD, tp2, NULL, NULL, 0)) die("limit, int16");
  for (b = 0; b < ROWS; ++b)
    if ((LEN[b] > 0) != (tp2[b] > 0.f)) return 4;
  /* every row empty */
  {
    const int64_t none[2] = {0, 0};
    memset(of, 0x55, sizeof(float) * 2 * OUT_LD);
    if (mi355tts_limit(ctx, model, x, NULL, none, 2, IN_LD, NULL, ceiling, of, NULL, OUT_LD, tp2, mn2, oc, 0)) die("limit, empty");
    for (i = 0; i < 2 * OUT_LD; ++i)
      if (of[i] != 0.f) return 6;
    if (tp2[0] != 0.f || mn2[1] != 1.0f) return 6;
  }
  if (mi355tts_limit(ctx, model, x, NULL, LEN, ROWS, IN_LD, GAIN, 1.5f, NULL, NULL, 0, tp2, NULL, NULL, 0) != MI355TTS_ERR_INVALID) return 5;
  if (mi355tts_unload(ctx, model)) die("unload");
  mi355tts_destroy(ctx);
  free(x); free(s); free(of); free(oi); free(oc); free(f1); free(i1); free(c1);
  printf("ok\n");
  return 0;
}
