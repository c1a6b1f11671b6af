// mij_resize.h -- the arithmetic of the separable resampler:
// Pillow's 8-bit Image.resize (src/libImaging/Resample.c) for BOX, BILINEAR
// and BICUBIC, stated once:
//
//   rs_build_axis   (host) one axis' table: per output index the first source
//                   index and the tap count, then the 22-bit fixed-point
//                   weights, computed in double arithmetic in Pillow's order
//                   of operations.  Must be compiled with -ffp-contract=off
//                   wherever it is compiled: a fused multiply-add changes the
//                   last bit of a coefficient and with it a rounded weight.
//   rs_tap / rs_clip (host and device) one output byte: acc = 1 << 21, plus
//                   source byte x weight per tap, arithmetic shift by 22,
//                   clipped to 0..255.
//
// Shared by k_rs_h / k_rs_v (mij_resize.hip) and the host check
// tests/resize_check.cpp, so the CPU suite runs the very arithmetic the GPU
// runs.  Plain C++: no HIP, nothing but the standard headers.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MIJ_RS_HD __host__ __device__ __forceinline__
#else
#define MIJ_RS_HD inline
#endif

namespace mij {

enum { RS_BOX = 0, RS_BILINEAR = 1, RS_BICUBIC = 2, RS_FILTERS = 3 };
constexpr int RS_BITS = 22;              // Pillow's PRECISION_BITS: 32 - 8 - 2
constexpr int RS_MAX_SIDE = 65535;

inline double rs_support(int filter) { return filter == RS_BOX ? 0.5 : filter == RS_BILINEAR ? 1.0 : 2.0; }

inline double rs_filter(int filter, double x) {
  if (filter == RS_BOX) return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
  if (x < 0.0) x = -x;
  if (filter == RS_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// taps a table row holds: 2 * ceil(support) + 1
inline int rs_ksize(int in, int out, int filter) {
  double filterscale = (double)in / out;
  if (filterscale < 1.0) filterscale = 1.0;
  return (int)ceil(rs_support(filter) * filterscale) * 2 + 1;
}

// int32 words of one axis' table: {xmin, count} per output index, then
// `out` rows of ksize weights
inline long long rs_table_words(int in, int out, int filter) { return 2LL * out + (long long)out * rs_ksize(in, out, filter); }

// Fills tab[0 .. rs_table_words).  k is scratch for ksize doubles.  Returns
// the largest sum of |weight| over the output indices: 255 times it, plus
// 1 << 21, is the bound of the accumulator.
inline long long rs_build_axis(int in, int out, int filter, int32_t *tab, double *k) {
  const int ksize = rs_ksize(in, out, filter);
  int32_t *bounds = tab, *wt = tab + 2LL * out;
  double scale, filterscale;
  scale = filterscale = (double)in / out;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = rs_support(filter) * filterscale;
  const double ss = 1.0 / filterscale;
  long long worst = 0;
  for (int xx = 0; xx < out; xx++) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    for (int x = 0; x < xmax; x++) {
      const double w = rs_filter(filter, (x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    int32_t *row = wt + (long long)xx * ksize;
    long long sum = 0;
    for (int x = 0; x < ksize; x++) {
      double v = 0.0;
      if (x < xmax) v = ww != 0.0 ? k[x] / ww : k[x];
      row[x] = v < 0 ? (int)(-0.5 + v * (1 << RS_BITS)) : (int)(0.5 + v * (1 << RS_BITS));
      sum += row[x] < 0 ? -(long long)row[x] : row[x];
    }
    if (sum > worst) worst = sum;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return worst;
}

// the accumulator stays inside int32 for every source byte
inline bool rs_sum_fits(long long worst) { return 255 * worst + (1LL << (RS_BITS - 1)) <= 0x7FFFFFFFLL; }

constexpr int32_t RS_ACC0 = 1 << (RS_BITS - 1);

MIJ_RS_HD int32_t rs_tap(int32_t acc, uint32_t byte, int32_t weight) { return acc + (int32_t)byte * weight; }

MIJ_RS_HD uint32_t rs_clip(int32_t acc) {
  const int32_t v = acc >> RS_BITS;  // arithmetic
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// One pass of one channel byte on the host (the check program and the
// reference for the kernels): dst[i * dstep] for i < out from src[j * sstep].
inline void rs_pass_host(const uint8_t *src, long long sstep, uint8_t *dst, long long dstep, int out, const int32_t *tab,
                         int ksize) {
  const int32_t *wt = tab + 2LL * out;
  for (int i = 0; i < out; i++) {
    const int xmin = tab[2 * i], n = tab[2 * i + 1];
    int32_t acc = RS_ACC0;
    for (int x = 0; x < n; x++) acc = rs_tap(acc, src[(long long)(xmin + x) * sstep], wt[(long long)i * ksize + x]);
    dst[(long long)i * dstep] = (uint8_t)rs_clip(acc);
  }
}

}  // namespace mij
