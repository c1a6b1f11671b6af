// ijg_check.cpp -- runs the arithmetic of encoding as libjpeg does
// (csrc/mij_ijg_math.h, the code k_ijg_fdct calls) on the host, for
// tests/test_ijg_model.py:
//   - the colour conversion over all 2^24 colours against the closed forms
//     in 64-bit arithmetic, with FIX() computed here from the real constants
//   - both downsamplers over every input
//   - the quantiser against `/` for every q in 1..255 and |c| <= 2^15
//   - the table scaling for Q = 1..100 against the model's tables
//   - the two DCT passes and the quantiser on blocks dumped by the model
//   - that no intermediate of the DCT leaves int32: the passes run a second
//     time over a 64-bit type that checks every result
// Input file (int32): 100 x (luma[64], chroma[64]) natural order for Q =
// 1..100; n; then n x (samples[64], q[64], expected[64]) natural order.
// Prints the largest DCT intermediate and exits 0 when everything agrees.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mij_ijg_math.h"

static long long g_max = 0;
static int g_over = 0;

// an integer that holds 64 bits and notes how far any value goes
struct Wide {
  long long v;
  Wide() : v(0) {}
  Wide(int x) : v(x) { note(); }
  Wide(long long x, int) : v(x) { note(); }
  void note() const {
    const long long a = v < 0 ? -v : v;
    if (a > g_max) g_max = a;
    if (v > 2147483647LL || v < -2147483648LL) g_over = 1;
  }
};
static Wide operator+(Wide a, Wide b) { return Wide(a.v + b.v, 0); }
static Wide operator-(Wide a, Wide b) { return Wide(a.v - b.v, 0); }
static Wide operator*(Wide a, Wide b) { return Wide(a.v * b.v, 0); }
static Wide operator>>(Wide a, int n) { return Wide(a.v >> n, 0); }

static long long fix(double x) { return (long long)floor(x * 65536.0 + 0.5); }

#define FAIL(...)                 \
  do {                            \
    fprintf(stderr, __VA_ARGS__); \
    fprintf(stderr, "\n");        \
    return 1;                     \
  } while (0)

static int check_colour() {
  const long long yr = fix(.299), yg = fix(.587), yb = fix(.114), br = fix(.168735892), bg = fix(.331264108),
                  half = fix(.5), rg = fix(.418687589), rb = fix(.081312411);
  for (int r = 0; r < 256; r++)
    for (int g = 0; g < 256; g++)
      for (int b = 0; b < 256; b++) {
        const long long y = (yr * r + yg * g + yb * b + 32768) >> 16;
        const long long cb = (-br * r - bg * g + half * b + (128LL << 16) + 32767) >> 16;
        const long long cr = (half * r - rg * g - rb * b + (128LL << 16) + 32767) >> 16;
        if (y < 0 || y > 255 || cb < 0 || cb > 255 || cr < 0 || cr > 255) FAIL("colour %d %d %d out of a byte", r, g, b);
        if (mij::ijg_y(r, g, b) != (uint32_t)y || mij::ijg_cb(r, g, b) != (uint32_t)cb ||
            mij::ijg_cr(r, g, b) != (uint32_t)cr)
          FAIL("colour %d %d %d", r, g, b);
      }
  return 0;
}

static int check_downsamplers() {
  for (int x = 0; x < 4; x++) {
    for (int a = 0; a < 256; a++)
      for (int b = 0; b < 256; b++)
        if (mij::ijg_h2v1(a, b, x) != (uint32_t)((a + b + (x % 2 ? 1 : 0)) / 2)) FAIL("h2v1 %d %d %d", a, b, x);
    for (int s = 0; s <= 1020; s++)
      if (mij::ijg_h2v2(s, x) != (uint32_t)((s + (x % 2 ? 2 : 1)) / 4)) FAIL("h2v2 %d %d", s, x);
  }
  return 0;
}

static int check_quantiser() {
  for (int q = 1; q <= 255; q++) {
    const mij::IjgQ m = mij::ijg_qmagic(q);
    const int d = 8 * q;
    for (int c = 0; c <= 32768; c++) {
      const int want = (c + (d >> 1)) / d;
      if (mij::ijg_quant(c, m) != want || mij::ijg_quant(-c, m) != -want) FAIL("quant q %d c %d", q, c);
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> tabs(100 * 128);
  int32_t n = 0;
  if (fread(tabs.data(), 4, tabs.size(), f) != tabs.size() || fread(&n, 4, 1, f) != 1 || n < 1) return 2;
  std::vector<int32_t> blocks((size_t)n * 192);
  if (fread(blocks.data(), 4, blocks.size(), f) != blocks.size()) return 2;
  fclose(f);
  if (check_colour() || check_downsamplers() || check_quantiser()) return 1;
  for (int q = 1; q <= 100; q++) {
    int lq[64], cq[64];
    mij::ijg_tables(q, lq, cq);
    for (int i = 0; i < 64; i++)
      if (lq[i] != tabs[(q - 1) * 128 + i] || cq[i] != tabs[(q - 1) * 128 + 64 + i]) FAIL("tables at Q %d entry %d", q, i);
  }
  for (int b = 0; b < n; b++) {
    const int32_t *smp = &blocks[(size_t)b * 192], *q = smp + 64, *want = smp + 128;
    int32_t w[8][8];
    Wide s[8][8];
    for (int y = 0; y < 8; y++) {  // rows first
      Wide e[8];
      for (int x = 0; x < 8; x++) {
        w[y][x] = smp[y * 8 + x] - 128;
        e[x] = Wide(smp[y * 8 + x] - 128);
      }
      mij::ijg_fdct_pass<true>(w[y]);
      mij::ijg_fdct_pass<true>(e);
      for (int x = 0; x < 8; x++) s[y][x] = e[x];
    }
    for (int u = 0; u < 8; u++) {  // then columns
      int32_t d[8];
      Wide e[8];
      for (int y = 0; y < 8; y++) {
        d[y] = w[y][u];
        e[y] = s[y][u];
      }
      mij::ijg_fdct_pass<false>(d);
      mij::ijg_fdct_pass<false>(e);
      for (int v = 0; v < 8; v++) {
        if (d[v] != e[v].v) FAIL("block %d (%d, %d): int32 %d, 64-bit %lld", b, v, u, d[v], e[v].v);
        const int got = mij::ijg_quant(d[v], mij::ijg_qmagic(q[v * 8 + u]));
        if (got != want[v * 8 + u]) FAIL("block %d (%d, %d): %d, the model has %d", b, v, u, got, want[v * 8 + u]);
        if (got > 1024 || got < -1024) FAIL("block %d (%d, %d): %d past 1024", b, v, u, got);
      }
    }
  }
  if (g_over) FAIL("a DCT intermediate left int32: %lld", g_max);
  printf("max_intermediate %lld\n", g_max);
  return 0;
}
