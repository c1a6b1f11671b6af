// mij_ijg_math.h -- the arithmetic of encoding as libjpeg does (DESIGN.md
// §4n): its fixed-point colour conversion, its two downsamplers, the "islow"
// forward DCT (jfdctint: CONST_BITS 13, PASS1_BITS 2), the quantiser that
// rounds the magnitude, and the IJG scaling of the Annex K tables.  Integer
// only, plain C++: shared by k_ijg_fdct (mij_ijg.hip) and the host check
// tests/ijg_check.cpp, so the CPU suite runs the very code the GPU runs.  The
// DCT passes are templates over the integer type: the kernel takes int32_t,
// the host check also a 64-bit type that records how far every intermediate
// goes.
#pragma once
#include <stdint.h>

#include "mij_divmagic.h"

#ifdef __HIPCC__
#define MIJ_IJG_HD __host__ __device__ __forceinline__
#else
#define MIJ_IJG_HD inline
#endif

namespace mij {

// ---- tables: Annex K, scaled as jpeg_quality_scaling / jpeg_add_quant_table
// with force_baseline do; natural order ------------------------------------
#define MIJ_IJG_LUMA_Q                                                                                 \
  {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,    \
   69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,   \
   81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92, 95,  98,  112, 100, 103, 99}
#define MIJ_IJG_CHROMA_Q                                                                               \
  {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,             \
   99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,             \
   99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}

// the percentage a quality of 1..100 scales the base tables by
MIJ_IJG_HD int ijg_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }
// one table entry: (base * scale + 50) / 100 in 1..255
MIJ_IJG_HD int ijg_qentry(int base, int scale) {
  const int v = (base * scale + 50) / 100;
  return v < 1 ? 1 : v > 255 ? 255 : v;
}
// both tables of a quality, natural order
inline void ijg_tables(int quality, int lq[64], int cq[64]) {
  const int lb[64] = MIJ_IJG_LUMA_Q, cb[64] = MIJ_IJG_CHROMA_Q;
  const int s = ijg_scale(quality);
  for (int i = 0; i < 64; i++) {
    lq[i] = ijg_qentry(lb[i], s);
    cq[i] = ijg_qentry(cb[i], s);
  }
}

// ---- colour (jccolor.c): FIX(x) = floor(x * 65536 + 0.5) --------------------
constexpr int32_t IJG_Y_R = 19595, IJG_Y_G = 38470, IJG_Y_B = 7471;     // FIX(.299) FIX(.587) FIX(.114)
constexpr int32_t IJG_CB_R = 11058, IJG_CB_G = 21710, IJG_HALF = 32768;  // FIX(.168735892) FIX(.331264108) FIX(.5)
constexpr int32_t IJG_CR_G = 27439, IJG_CR_B = 5329;                     // FIX(.418687589) FIX(.081312411)
constexpr int32_t IJG_C_OFF = (128 << 16) + 32767;                       // CBCR_OFFSET + ONE_HALF - 1

MIJ_IJG_HD uint32_t ijg_y(int32_t r, int32_t g, int32_t b) {
  return (uint32_t)((IJG_Y_R * r + IJG_Y_G * g + IJG_Y_B * b + 32768) >> 16);
}
MIJ_IJG_HD uint32_t ijg_cb(int32_t r, int32_t g, int32_t b) {
  return (uint32_t)((-IJG_CB_R * r - IJG_CB_G * g + IJG_HALF * b + IJG_C_OFF) >> 16);
}
MIJ_IJG_HD uint32_t ijg_cr(int32_t r, int32_t g, int32_t b) {
  return (uint32_t)((IJG_HALF * r - IJG_CR_G * g - IJG_CR_B * b + IJG_C_OFF) >> 16);
}

// ---- downsampling (jcsample.c, no smoothing); x is the output column -------
// h2v1: a, b the two samples of the pair; the bias alternates 0, 1, 0, 1, ...
MIJ_IJG_HD uint32_t ijg_h2v1(uint32_t a, uint32_t b, int x) { return (a + b + (uint32_t)(x & 1)) >> 1; }
// h2v2: sum4 the four samples of the square; the bias alternates 1, 2, 1, 2, ...
MIJ_IJG_HD uint32_t ijg_h2v2(uint32_t sum4, int x) { return (sum4 + 1u + (uint32_t)(x & 1)) >> 2; }

// ---- forward DCT (jfdctint.c) ----------------------------------------------
// One 1-D pass over d[0..7] in place.  ROWS: the first pass, on samples - 128;
// its even outputs 0 and 4 are left scaled by 4 (PASS1_BITS), the others are
// descaled by 11 bits.  !ROWS: the second pass, down a column of first-pass
// results; outputs 0 and 4 are descaled by 2 bits, the others by 15.  Every
// descale is (x + (1 << (n - 1))) >> n with an arithmetic shift.  Both passes
// together give 8 times the true DCT.  Bounds (T = int32_t is enough): §4n.
template <bool ROWS, class T>
MIJ_IJG_HD void ijg_fdct_pass(T d[8]) {
  constexpr int SH = ROWS ? 11 : 15;
  const T rnd = T(1 << (SH - 1));
  const T t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const T t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const T t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (ROWS) {
    d[0] = (t10 + t11) * T(4);
    d[4] = (t10 - t11) * T(4);
  } else {
    d[0] = (t10 + t11 + T(2)) >> 2;
    d[4] = (t10 - t11 + T(2)) >> 2;
  }
  const T e = (t12 + t13) * T(4433);
  d[2] = (e + t13 * T(6270) + rnd) >> SH;
  d[6] = (e - t12 * T(15137) + rnd) >> SH;
  const T z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const T z5 = (z3 + z4) * T(9633);
  const T p4 = t4 * T(2446), p5 = t5 * T(16819), p6 = t6 * T(25172), p7 = t7 * T(12299);
  const T q1 = z1 * T(-7373), q2 = z2 * T(-20995);
  const T q3 = z3 * T(-16069) + z5, q4 = z4 * T(-3196) + z5;
  d[7] = (p4 + q1 + q3 + rnd) >> SH;
  d[5] = (p5 + q2 + q4 + rnd) >> SH;
  d[3] = (p6 + q2 + q3 + rnd) >> SH;
  d[1] = (p7 + q1 + q4 + rnd) >> SH;
}

// ---- quantisation (jcdctmgr.c): the magnitude rounded, the sign restored ----
// The divisor of coefficient c (8 times the true one) is d = 8 q; m, s are
// div_magic(d), half = d >> 1.  |c| + half < 2^31 is all div_by needs.
struct IjgQ {
  uint32_t m;
  uint16_t half;
  uint16_t s;
};
inline IjgQ ijg_qmagic(int q) {
  IjgQ r;
  uint32_t m, s;
  div_magic((uint32_t)(8 * q), m, s);
  r.m = m;
  r.s = (uint16_t)s;
  r.half = (uint16_t)(8 * q >> 1);
  return r;
}
MIJ_IJG_HD int32_t ijg_quant(int32_t c, IjgQ q) {
  const uint32_t a = (uint32_t)(c < 0 ? -c : c) + q.half;
  const int32_t r = (int32_t)div_by(a, q.m, q.s);
  return c < 0 ? -r : r;
}

}  // namespace mij
