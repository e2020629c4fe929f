/* A plain C99 program on the loudness entry points of include/mi355tts.h: a ragged batch of eight rows (lengths at the edges
 * of a block, a hop, a chunk and a workgroup, unsorted), every output asked for, float and int16 input, and each row again as
 * its own batch-1 call, compared bit for bit.  Prints one line per row (the bits of lufs / gain / peak) for the Python side to
 * compare with its own binding, and "ok" at the end.  Stand-alone so that it can also be built with the host sanitizers
 * (-fsanitize=address,undefined) against the library's CPU-emulator flavour: profiles/loudness.md has the command. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mi355tts.h"

#define ROWS 8
#define FS 22050.0
static const int64_t LEN[ROWS] = {8820, 0, 60000, 65, 1, 11024, 129, 8819};
#define IN_LD 60040
#define OUT_LD 60061

static void die(const char* what) {
  fprintf(stderr, "%s: %s\n", what, mi355tts_last_error());
  exit(1);
}

static void k_weighting(double fs, mi355tts_loudness_params* p) {
  const double pi = 3.14159265358979323846;
  double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
  double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
  p->shelf_b[0] = (float)((Vh + Vb * K / Q + K * K) / a0);
  p->shelf_b[1] = (float)(2.0 * (K * K - Vh) / a0);
  p->shelf_b[2] = (float)((Vh - Vb * K / Q + K * K) / a0);
  p->shelf_a[0] = (float)(2.0 * (K * K - 1.0) / a0);
  p->shelf_a[1] = (float)((1.0 - K / Q + K * K) / a0);
  f0 = 38.13547087602444;
  Q = 0.5003270373238773;
  K = tan(pi * f0 / fs);
  a0 = 1.0 + K / Q + K * K;
  p->hp_b[0] = 1.0f;
  p->hp_b[1] = -2.0f;
  p->hp_b[2] = 1.0f;
  p->hp_a[0] = (float)(2.0 * (K * K - 1.0) / a0);
  p->hp_a[1] = (float)((1.0 - K / Q + K * K) / a0);
  p->block = (int32_t)floor(0.4 * fs + 0.5);
  p->hop = (int32_t)floor(0.1 * fs + 0.5);
}

static uint32_t bits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}

int main(int argc, char** argv) {
  const int device = argc > 1 ? atoi(argv[1]) : 0;
  mi355tts_ctx* ctx = NULL;
  mi355tts_loudness_params p;
  int model = -1, b;
  int64_t i;
  const float ceiling = 0.8912509f;
  float* x = (float*)malloc(sizeof(float) * ROWS * IN_LD);
  int16_t* s = (int16_t*)malloc(sizeof(int16_t) * ROWS * IN_LD);
  float* of = (float*)malloc(sizeof(float) * ROWS * OUT_LD);
  int16_t* oi = (int16_t*)malloc(sizeof(int16_t) * ROWS * OUT_LD);
  float* ow = (float*)malloc(sizeof(float) * ROWS * IN_LD);
  float* f1 = (float*)malloc(sizeof(float) * IN_LD);
  int16_t* i1 = (int16_t*)malloc(sizeof(int16_t) * IN_LD);
  float* w1 = (float*)malloc(sizeof(float) * IN_LD);
  float lufs[ROWS], gain[ROWS], peak[ROWS];
  uint32_t st = 2024u;
  if (!x || !s || !of || !oi || !ow || !f1 || !i1 || !w1) return 2;
  if (mi355tts_create(device, &ctx)) die("create");
  k_weighting(FS, &p);
  if (mi355tts_load_loudness(ctx, &p, &model)) die("load_loudness");
  for (b = 0; b < ROWS; ++b)
    for (i = 0; i < IN_LD; ++i) {
      float v = 0.25f; /* what lies past a row's samples must not be read */
      if (i < LEN[b]) {
        st = st * 1664525u + 1013904223u;
        v = 0.3f * (float)sin(2.0 * 3.14159265358979323846 * 140.0 * (double)(b + 1) * (double)i / FS) +
            0.02f * ((float)(st >> 8) / 8388608.0f - 1.0f);
      }
      x[(size_t)b * IN_LD + i] = v;
      s[(size_t)b * IN_LD + i] = (int16_t)lrintf(v * 32767.0f);
    }
  memset(of, 0x55, sizeof(float) * ROWS * OUT_LD);
  memset(oi, 0x55, sizeof(int16_t) * ROWS * OUT_LD);
  memset(ow, 0x55, sizeof(float) * ROWS * IN_LD);
  if (mi355tts_loudness(ctx, model, x, NULL, LEN, ROWS, IN_LD, -20.0f, ceiling, 30.0f, of, oi, OUT_LD, lufs, gain, peak, ow, 0)) die("loudness");
  for (b = 0; b < ROWS; ++b) {
    const int64_t n = LEN[b];
    float l1, g1, p1;
    if (mi355tts_loudness(ctx, model, x + (size_t)b * IN_LD, NULL, &n, 1, n, -20.0f, ceiling, 30.0f, f1, i1, n, &l1, &g1, &p1, w1, 0))
      die("loudness, one row");
    if (bits(l1) != bits(lufs[b]) || bits(g1) != bits(gain[b]) || bits(p1) != bits(peak[b]) ||
        memcmp(f1, of + (size_t)b * OUT_LD, sizeof(float) * (size_t)n) || memcmp(i1, oi + (size_t)b * OUT_LD, sizeof(int16_t) * (size_t)n) ||
        memcmp(w1, ow + (size_t)b * IN_LD, sizeof(float) * (size_t)n)) {
      fprintf(stderr, "row %d differs from its batch-1 call\n", b);
      return 1;
    }
    for (i = n; i < OUT_LD; ++i)
      if (of[(size_t)b * OUT_LD + i] != 0.f || oi[(size_t)b * OUT_LD + i] != 0) return 3;
    for (i = n; i < IN_LD; ++i)
      if (ow[(size_t)b * IN_LD + i] != 0.f) return 3;
    printf("row %d n %lld lufs %08x gain %08x peak %08x\n", b, (long long)n, (unsigned)bits(lufs[b]), (unsigned)bits(gain[b]), (unsigned)bits(peak[b]));
  }
  /* int16 input, measuring only: no output pointer at all */
  if (mi355tts_loudness(ctx, model, NULL, s, LEN, ROWS, IN_LD, NAN, 1.0f, 30.0f, NULL, NULL, 0, lufs, gain, NULL, NULL, 0)) die("loudness, int16");
  for (b = 0; b < ROWS; ++b)
    if (gain[b] != 1.0f || (LEN[b] > 0 && !(lufs[b] > -40.f && lufs[b] < 0.f))) return 4;
  if (mi355tts_loudness(ctx, model, x, NULL, LEN, ROWS, IN_LD, -20.0f, 1.5f, 30.0f, NULL, NULL, 0, lufs, NULL, NULL, NULL, 0) != MI355TTS_ERR_INVALID)
    return 5;
  if (mi355tts_unload(ctx, model)) die("unload");
  mi355tts_destroy(ctx);
  free(x); free(s); free(of); free(oi); free(ow); free(f1); free(i1); free(w1);
  printf("ok\n");
  return 0;
}
