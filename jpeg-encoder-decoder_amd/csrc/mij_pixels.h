// mij_pixels.h -- the decoder's pixel arithmetic (DESIGN.md "Decode to
// pixels"): libjpeg's "islow" IDCT, h2v2 "fancy" upsampling and fixed-point
// colour conversion, integer only.  Shared by the kernels of mij_decode.hip
// and the host check tests/pixels_check.cpp, so the CPU suite runs the very
// code the GPU runs.  The IDCT's products and sums are taken modulo 2^32
// (uint32_t): a stream no 8-bit image produces wraps instead of overflowing
// a signed type; encoder-made streams never come near the limit.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MIJ_HD __host__ __device__ __forceinline__
#define MIJ_UNROLL _Pragma("unroll")
#else
#define MIJ_HD inline
#define MIJ_UNROLL
#endif

namespace mij {

// natural position of zigzag index z
#define MIJ_ZIGZAG                                                                                    \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,            \
   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,            \
   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

MIJ_HD uint32_t clamp255(int32_t v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// the 1-D pass of the "islow" IDCT (CONST_BITS 13), outputs descaled by SH
template <int SH>
MIJ_HD void idct8(uint32_t i0, uint32_t i1, uint32_t i2, uint32_t i3, uint32_t i4, uint32_t i5, uint32_t i6,
                  uint32_t i7, int32_t o[8]) {
  uint32_t z1 = (i2 + i6) * 4433u;
  const uint32_t t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
  const uint32_t t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t o0 = i7, o1 = i5, o2 = i3, o3 = i1;
  z1 = o0 + o3;
  uint32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  o0 *= 2446u;
  o1 *= 16819u;
  o2 *= 25172u;
  o3 *= 12299u;
  z1 *= (uint32_t)-7373;
  z2 *= (uint32_t)-20995;
  z3 = z3 * (uint32_t)-16069 + z5;
  z4 = z4 * (uint32_t)-3196 + z5;
  o0 += z1 + z3;
  o1 += z2 + z4;
  o2 += z2 + z3;
  o3 += z1 + z4;
  constexpr uint32_t R = 1u << (SH - 1);
  o[0] = (int32_t)(t10 + o3 + R) >> SH;
  o[1] = (int32_t)(t11 + o2 + R) >> SH;
  o[2] = (int32_t)(t12 + o1 + R) >> SH;
  o[3] = (int32_t)(t13 + o0 + R) >> SH;
  o[4] = (int32_t)(t13 - o0 + R) >> SH;
  o[5] = (int32_t)(t12 - o1 + R) >> SH;
  o[6] = (int32_t)(t11 - o2 + R) >> SH;
  o[7] = (int32_t)(t10 - o3 + R) >> SH;
}

// One 8x8 block: c = its 64 zigzag-ordered quantised coefficients (c[0] is
// ignored: dc is the absolute DC), qz = the quantiser in zigzag order.
// rows[r] = the 8 samples of row r, little-endian in two words.  Every index
// is a compile-time constant once unrolled, so on the GPU all arrays are
// registers.
MIJ_HD void idct_block(const int16_t *c, uint32_t dc, const int32_t *qz, uint32_t rows[8][2]) {
  constexpr uint8_t zz[64] = MIJ_ZIGZAG;
  uint32_t d[64];
  d[0] = dc * (uint32_t)qz[0];
  MIJ_UNROLL
  for (int z = 1; z < 64; z++) d[zz[z]] = (uint32_t)(int32_t)c[z] * (uint32_t)qz[z];
  int32_t ws[64];
  MIJ_UNROLL
  for (int col = 0; col < 8; col++) {  // down each column, descale 11
    int32_t o[8];
    idct8<11>(d[col], d[8 + col], d[16 + col], d[24 + col], d[32 + col], d[40 + col], d[48 + col], d[56 + col], o);
  MIJ_UNROLL
    for (int k = 0; k < 8; k++) ws[8 * k + col] = o[k];
  }
  MIJ_UNROLL
  for (int r = 0; r < 8; r++) {  // along each row, descale 18, level shift, clamp
    int32_t o[8];
    idct8<18>(ws[8 * r], ws[8 * r + 1], ws[8 * r + 2], ws[8 * r + 3], ws[8 * r + 4], ws[8 * r + 5], ws[8 * r + 6],
              ws[8 * r + 7], o);
    rows[r][0] = clamp255(o[0] + 128) | clamp255(o[1] + 128) << 8 | clamp255(o[2] + 128) << 16 |
                 clamp255(o[3] + 128) << 24;
    rows[r][1] = clamp255(o[4] + 128) | clamp255(o[5] + 128) << 8 | clamp255(o[6] + 128) << 16 |
                 clamp255(o[7] + 128) << 24;
  }
}

// 16 upsampled chroma samples (0..255) of one output row.  p = chroma
// samples c0-1 .. c0+8 of the chroma row itself, nb = the same columns of its
// upper (for the upper output row) or lower neighbour; the caller replicates
// the plane's edge rows and columns (jdsample.c h2v2_fancy_upsample)
MIJ_HD void upsample16(const int p[10], const int nb[10], int out[16]) {
  int s[10];
  MIJ_UNROLL
  for (int k = 0; k < 10; k++) s[k] = 3 * p[k] + nb[k];
  MIJ_UNROLL
  for (int k = 0; k < 8; k++) {
    out[2 * k] = (3 * s[k + 1] + s[k] + 8) >> 4;
    out[2 * k + 1] = (3 * s[k + 1] + s[k + 2] + 7) >> 4;
  }
}

// 16 pixels -> 48 packed bytes in 12 little-endian words; y = 16 luma bytes in
// 4 words, cb / cr = upsample16's output; rgb: R,G,B order, else B,G,R.
// jdcolor.c's R = Y + ((91881 * (Cr - 128) + 32768) >> 16) and so on, the
// - 128 folded into the rounding constant (sums of integers: the same value)
MIJ_HD void colour16(const uint32_t y[4], const int cb[16], const int cr[16], int rgb, uint32_t wd[12]) {
  MIJ_UNROLL
  for (int k = 0; k < 12; k++) wd[k] = 0;
  MIJ_UNROLL
  for (int p = 0; p < 16; p++) {
    const int yy = (int)((y[p >> 2] >> (8 * (p & 3))) & 255);
    const uint32_t R = clamp255(yy + ((91881 * cr[p] + (32768 - 128 * 91881)) >> 16));
    const uint32_t G = clamp255(yy + ((-22554 * cb[p] - 46802 * cr[p] + (32768 + 128 * (22554 + 46802))) >> 16));
    const uint32_t B = clamp255(yy + ((116130 * cb[p] + (32768 - 128 * 116130)) >> 16));
    const uint32_t ch[3] = {rgb ? R : B, G, rgb ? B : R};
  MIJ_UNROLL
    for (int k = 0; k < 3; k++) wd[(3 * p + k) >> 2] |= ch[k] << (8 * ((3 * p + k) & 3));
  }
}

// aligned 8- and 16-byte moves (one load or store instruction each on the GPU)
struct alignas(8) W2 {
  uint32_t x, y;
};
struct alignas(16) W4 {
  uint32_t x, y, z, w;
};
template <class T>
MIJ_HD T load_as(const uint8_t *p) {
  T v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, alignof(T)), sizeof(T));
  return v;
}
template <class T>
MIJ_HD void store_as(uint8_t *p, const T &v) {
  __builtin_memcpy(__builtin_assume_aligned(p, alignof(T)), &v, sizeof(T));
}

// chroma samples c0-1 .. c0+8 of a row (c0 % 8 == 0; cl / cr: the two halo
// columns, already clamped to the plane)
MIJ_HD void chroma10(const uint8_t *row, int c0, int cl, int cr, int v[10]) {
  const W2 m = load_as<W2>(row + c0);
  v[0] = row[cl];
  MIJ_UNROLL
  for (int k = 0; k < 4; k++) {
    v[1 + k] = (int)((m.x >> (8 * k)) & 255);
    v[5 + k] = (int)((m.y >> (8 * k)) & 255);
  }
  v[9] = row[cr];
}

// ---------------------------------------------------------------------------
// The colour stage for every layout the decoder accepts (DESIGN.md "Decoding
// ordinary baseline files"): greyscale, 4:4:4, 4:2:2 and 4:2:0 at any size,
// on planes padded to whole MCUs (the encoder's own frames, multiples of 16,
// have no padding).  libjpeg's rules: the chroma edges are those of the
// component's real size, ceil(w / 2) x ceil(h / 2) (downsampled_width /
// _height), not of the padded plane; the "fancy" upsamplers only run when
// that width is > 2, else each sample is replicated (jdsample.c).
//
// 4:4:0 (luma 1x2) is the transposed 4:2:2: chroma of the
// frame's width and ceil(h / 2) rows, PIX_H1V2 (h1v2_fancy_upsample: each
// sample with its upper or lower neighbour, no horizontal ones, hence no
// small-width exception) or PIX_H1V2_REP (each row twice, at 1/8 scale).
// ---------------------------------------------------------------------------
enum {
  PIX_GREY = 0,
  PIX_444 = 1,
  PIX_H2V1 = 2,
  PIX_H2V1_REP = 3,
  PIX_H2V2 = 4,
  PIX_H2V2_REP = 5,
  PIX_H1V2 = 6,
  PIX_H1V2_REP = 7
};

struct PixGeom {
  int w, h;         // the frame's real size
  int mode;         // PIX_*
  int yp, cp;       // bytes between rows of the padded luma / chroma planes (multiples of 8)
  int cw, ch;       // the chroma planes' real size
  long long pitch;  // bytes between pixel rows: 3 * w rounded up to 16
};

// (the modes from PIX_H2V2 on are the two-row ones: a mode added after them must be one too, or this test changes)
MIJ_HD int pix_rows_per_lane(int mode) { return mode >= PIX_H2V2 ? 2 : 1; }

// 16 samples at columns x0 .. x0 + 15 (x0 % 16 == 0) of a padded row whose
// length is a multiple of 8: the second 8 may lie past it (then never shown)
MIJ_HD void row16(const uint8_t *row, int x0, int rowlen, uint32_t wd[4]) {
  const W2 a = load_as<W2>(row + x0);
  W2 b = {0, 0};
  if (x0 + 8 < rowlen) b = load_as<W2>(row + x0 + 8);
  wd[0] = a.x;
  wd[1] = a.y;
  wd[2] = b.x;
  wd[3] = b.y;
}

// chroma10 on a padded row of real width cw: columns past cw - 1 replicate it
MIJ_HD void chroma10_edge(const uint8_t *row, int c0, int cw, int v[10]) {
  const int cl = c0 > 0 ? c0 - 1 : 0, cr = c0 + 8 < cw ? c0 + 8 : cw - 1;
  chroma10(row, c0, cl, cr, v);
  if (c0 + 8 > cw) {
    const int last = row[cw - 1];
  MIJ_UNROLL
    for (int k = 1; k < 9; k++)
      if (c0 - 1 + k >= cw) v[k] = last;
  }
}

// jdsample.c h2v1_fancy_upsample: p = chroma samples c0-1 .. c0+8
MIJ_HD void upsample16_h2v1(const int p[10], int out[16]) {
  MIJ_UNROLL
  for (int k = 0; k < 8; k++) {
    out[2 * k] = (3 * p[k + 1] + p[k] + 1) >> 2;
    out[2 * k + 1] = (3 * p[k + 1] + p[k + 2] + 2) >> 2;
  }
}

MIJ_HD void replicate16(const int p[10], int out[16]) {
  MIJ_UNROLL
  for (int k = 0; k < 8; k++) out[2 * k] = out[2 * k + 1] = p[k + 1];
}

// jdsample.c h1v2_fancy_upsample: 16 samples of a chroma row (mid) and of its
// upper and lower neighbours (the plane's edge rows replicated), four to a
// word -> the two output rows they make
MIJ_HD void upsample16_h1v2(const uint32_t mid[4], const uint32_t up[4], const uint32_t dn[4], int top[16],
                            int bot[16]) {
  MIJ_UNROLL
  for (int p = 0; p < 16; p++) {
    const int sh = 8 * (p & 3);
    const int m = (int)((mid[p >> 2] >> sh) & 255);
    top[p] = (3 * m + (int)((up[p >> 2] >> sh) & 255) + 1) >> 2;
    bot[p] = (3 * m + (int)((dn[p >> 2] >> sh) & 255) + 2) >> 2;
  }
}

// up to three aligned 16-byte stores of one output row's 16-pixel group; the
// row is G.pitch bytes long (a multiple of 16), so a store that begins inside
// it ends inside it.  Bytes between 3 * w and the pitch receive anything.
MIJ_HD void store_group(uint8_t *rowp, int g, long long pitch, const uint32_t wd[12]) {
  MIJ_UNROLL
  for (int j = 0; j < 3; j++)
    if (48LL * g + 16 * j < pitch) store_as(rowp + 48LL * g + 16 * j, W4{wd[4 * j], wd[4 * j + 1], wd[4 * j + 2], wd[4 * j + 3]});
}

// Unit u, group g: output columns 16g .. 16g+15 of row u (one-row modes) or of
// rows 2u and 2u+1 (h2v2 and h1v2 modes; the second only if < h).  g <
// ceil(w / 16), u < h or ceil(h / 2).  Reads stay inside the padded planes
// (their rows are yp / cp long and there are at least h, resp. ch, of them);
// stores stay inside rows < h of the frame's pixel slot.
//
// The h1v2 modes: the chroma planes are as wide as the frame (cw == w <= cp, a
// multiple of 8), so group g's row16 begins at byte 16g < w <= cp, its first 8
// bytes end at 16g + 8 <= cp and its second 8 are loaded only if 16g + 8 <
// cp: inside the row, as for luma.  The rows read are u and its neighbours
// clamped to 0 .. ch - 1, with u < ceil(h / 2) == ch <= the padded plane's
// rows.  Output rows 2u and 2u + 1 pass the same y < h test as the h2v2
// modes' before their luma load and their stores.
MIJ_HD void colour_tile_any(const uint8_t *Y, const uint8_t *Cb, const uint8_t *Cr, const PixGeom &G, int u, int g,
                            int rgb, uint8_t *pix) {
  const int nrows = pix_rows_per_lane(G.mode);
  int cb[2][16], crv[2][16];
  if (G.mode == PIX_444) {
    uint32_t a[4], b[4];
    row16(Cb + (long long)u * G.cp, 16 * g, G.cp, a);
    row16(Cr + (long long)u * G.cp, 16 * g, G.cp, b);
  MIJ_UNROLL
    for (int p = 0; p < 16; p++) {
      cb[0][p] = (int)((a[p >> 2] >> (8 * (p & 3))) & 255);
      crv[0][p] = (int)((b[p >> 2] >> (8 * (p & 3))) & 255);
    }
  } else if (G.mode == PIX_H2V2) {
    const int ru = u > 0 ? u - 1 : 0, rd = u + 1 < G.ch ? u + 1 : G.ch - 1;
    int mid[10], nb[10];
    chroma10_edge(Cb + (long long)u * G.cp, 8 * g, G.cw, mid);
    chroma10_edge(Cb + (long long)ru * G.cp, 8 * g, G.cw, nb);
    upsample16(mid, nb, cb[0]);
    chroma10_edge(Cb + (long long)rd * G.cp, 8 * g, G.cw, nb);
    upsample16(mid, nb, cb[1]);
    chroma10_edge(Cr + (long long)u * G.cp, 8 * g, G.cw, mid);
    chroma10_edge(Cr + (long long)ru * G.cp, 8 * g, G.cw, nb);
    upsample16(mid, nb, crv[0]);
    chroma10_edge(Cr + (long long)rd * G.cp, 8 * g, G.cw, nb);
    upsample16(mid, nb, crv[1]);
  } else if (G.mode == PIX_H1V2 || G.mode == PIX_H1V2_REP) {
    // _REP: both neighbours are the row itself, (3 m + m + 1 or 2) >> 2 == m
    const int ru = G.mode == PIX_H1V2 && u > 0 ? u - 1 : u, rd = G.mode == PIX_H1V2 && u + 1 < G.ch ? u + 1 : u;
    uint32_t mid[4], up[4], dn[4];
    row16(Cb + (long long)u * G.cp, 16 * g, G.cp, mid);
    row16(Cb + (long long)ru * G.cp, 16 * g, G.cp, up);
    row16(Cb + (long long)rd * G.cp, 16 * g, G.cp, dn);
    upsample16_h1v2(mid, up, dn, cb[0], cb[1]);
    row16(Cr + (long long)u * G.cp, 16 * g, G.cp, mid);
    row16(Cr + (long long)ru * G.cp, 16 * g, G.cp, up);
    row16(Cr + (long long)rd * G.cp, 16 * g, G.cp, dn);
    upsample16_h1v2(mid, up, dn, crv[0], crv[1]);
  } else if (G.mode != PIX_GREY) {
    int p[10];
    chroma10_edge(Cb + (long long)u * G.cp, 8 * g, G.cw, p);
    if (G.mode == PIX_H2V1) upsample16_h2v1(p, cb[0]);
    else replicate16(p, cb[0]);
    chroma10_edge(Cr + (long long)u * G.cp, 8 * g, G.cw, p);
    if (G.mode == PIX_H2V1) upsample16_h2v1(p, crv[0]);
    else replicate16(p, crv[0]);
  MIJ_UNROLL
    for (int k = 0; k < 16; k++) {
      cb[1][k] = cb[0][k];
      crv[1][k] = crv[0][k];
    }
  }
  MIJ_UNROLL
  for (int row = 0; row < 2; row++) {
    const long long y = (long long)nrows * u + row;
    if (row >= nrows || y >= G.h) break;
    uint32_t yw[4], wd[12];
    row16(Y + y * G.yp, 16 * g, G.yp, yw);
    if (G.mode == PIX_GREY) {
  MIJ_UNROLL
      for (int k = 0; k < 12; k++) wd[k] = 0;
  MIJ_UNROLL
      for (int p = 0; p < 16; p++) {
        const uint32_t v = (yw[p >> 2] >> (8 * (p & 3))) & 255;
  MIJ_UNROLL
        for (int k = 0; k < 3; k++) wd[(3 * p + k) >> 2] |= v << (8 * ((3 * p + k) & 3));
      }
    } else {
      colour16(yw, cb[row], crv[row], rgb, wd);
    }
    store_group(pix + y * G.pitch, g, G.pitch, wd);
  }
}

// ---------------------------------------------------------------------------
// Decoding at 1/2, 1/4 and 1/8 scale: libjpeg's reduced IDCTs
// (jidctred.c), which give a 4x4, 2x2 or 1x1 block from the low frequencies,
// and the geometry that goes with them.  Products and sums modulo 2^32 as in
// idct8.
// ---------------------------------------------------------------------------
template <int SH>
MIJ_HD void idct4_1d(uint32_t i0, uint32_t i1, uint32_t i2, uint32_t i3, uint32_t i5, uint32_t i6, uint32_t i7,
                     int32_t o[4]) {
  const uint32_t t0 = i0 << 14, t2 = i2 * 15137u - i6 * 6270u;
  const uint32_t t10 = t0 + t2, t12 = t0 - t2;
  const uint32_t a = i5 * 11893u + i1 * 8697u - i7 * 1730u - i3 * 17799u;
  const uint32_t b = i3 * 7373u + i1 * 20995u - i7 * 4176u - i5 * 4926u;
  constexpr uint32_t R = 1u << (SH - 1);
  o[0] = (int32_t)(t10 + b + R) >> SH;
  o[1] = (int32_t)(t12 + a + R) >> SH;
  o[2] = (int32_t)(t12 - a + R) >> SH;
  o[3] = (int32_t)(t10 - b + R) >> SH;
}

// One block at 1/2 scale: c, dc, qz as idct_block; rows[r] = the 4 samples of
// row r in one little-endian word.  Column 4 and row 4 of the block are never
// used (jpeg_idct_4x4).
MIJ_HD void idct4_block(const int16_t *c, uint32_t dc, const int32_t *qz, uint32_t rows[4]) {
  constexpr uint8_t zz[64] = MIJ_ZIGZAG;
  uint32_t d[64];
  d[0] = dc * (uint32_t)qz[0];
  MIJ_UNROLL
  for (int z = 1; z < 64; z++) d[zz[z]] = (uint32_t)(int32_t)c[z] * (uint32_t)qz[z];
  int32_t ws[4][8];
  MIJ_UNROLL
  for (int col = 0; col < 8; col++) {  // down each column but 4, descale 12
    int32_t o[4] = {0, 0, 0, 0};
    if (col != 4) idct4_1d<12>(d[col], d[8 + col], d[16 + col], d[24 + col], d[40 + col], d[48 + col], d[56 + col], o);
  MIJ_UNROLL
    for (int k = 0; k < 4; k++) ws[k][col] = o[k];
  }
  MIJ_UNROLL
  for (int r = 0; r < 4; r++) {  // along each row, descale 19, level shift, clamp
    int32_t o[4];
    idct4_1d<19>(ws[r][0], ws[r][1], ws[r][2], ws[r][3], ws[r][5], ws[r][6], ws[r][7], o);
    rows[r] = clamp255(o[0] + 128) | clamp255(o[1] + 128) << 8 | clamp255(o[2] + 128) << 16 |
              clamp255(o[3] + 128) << 24;
  }
}

template <int SH>
MIJ_HD void idct2_1d(uint32_t i0, uint32_t i1, uint32_t i3, uint32_t i5, uint32_t i7, int32_t o[2]) {
  const uint32_t t10 = i0 << 15;
  const uint32_t t0 = i5 * 6967u + i1 * 29692u - i7 * 5906u - i3 * 10426u;
  constexpr uint32_t R = 1u << (SH - 1);
  o[0] = (int32_t)(t10 + t0 + R) >> SH;
  o[1] = (int32_t)(t10 - t0 + R) >> SH;
}

// One block at 1/4 scale: rows[r] = the 2 samples of row r in the low 16 bits.
// Only rows and columns 0, 1, 3, 5, 7 of the block are used (jpeg_idct_2x2).
MIJ_HD void idct2_block(const int16_t *c, uint32_t dc, const int32_t *qz, uint32_t rows[2]) {
  constexpr uint8_t zz[64] = MIJ_ZIGZAG;
  uint32_t d[64];
  d[0] = dc * (uint32_t)qz[0];
  MIJ_UNROLL
  for (int z = 1; z < 64; z++) d[zz[z]] = (uint32_t)(int32_t)c[z] * (uint32_t)qz[z];
  int32_t ws[2][8];
  MIJ_UNROLL
  for (int col = 0; col < 8; col++) {  // down columns 0, 1, 3, 5, 7, descale 13
    int32_t o[2] = {0, 0};
    if (col < 2 || (col & 1)) idct2_1d<13>(d[col], d[8 + col], d[24 + col], d[40 + col], d[56 + col], o);
    ws[0][col] = o[0];
    ws[1][col] = o[1];
  }
  MIJ_UNROLL
  for (int r = 0; r < 2; r++) {  // along each row, descale 20, level shift, clamp
    int32_t o[2];
    idct2_1d<20>(ws[r][0], ws[r][1], ws[r][3], ws[r][5], ws[r][7], o);
    rows[r] = clamp255(o[0] + 128) | clamp255(o[1] + 128) << 8;
  }
}

// One block at 1/8 scale: the DC alone (jpeg_idct_1x1)
MIJ_HD uint32_t idct1_block(uint32_t dc, int32_t q0) {
  return clamp255(((int32_t)(dc * (uint32_t)q0 + 4u) >> 3) + 128);
}

// The geometry of a frame decoded at 1/denom (denom 1, 2, 4 or 8), libjpeg's
// rules (jdmaster.c): s = 8 / denom output samples per 8 input samples; a
// component's IDCT size S starts at s and doubles while it stays <= 8 and
// the component would otherwise be upsampled by a multiple of 2 both across
// and down, so 4:2:0 chroma is scaled up inside its IDCT and needs no
// upsampler, 4:2:2 keeps its horizontal one and 4:4:0 its vertical one (fx ==
// 1, fy == 2 at every scale).  Shared by the host
// planner, the kernels' job tables and tests/scaled_check.cpp.
struct ScaledComp {
  int S;       // the IDCT's output size: S x S samples per block
  int cw, ch;  // the component's real size in samples
  int pitch;   // bytes between rows of its padded plane: S * blocks across, rounded up to 8
  int rows;    // rows of the padded plane: S * blocks down
};

struct ScaledGeom {
  int ow, oh;  // the output's size
  int mode;    // PIX_* for colour_tile_any on the scaled planes
  ScaledComp c[3];
};

// hs / vs / bw / bh: per component sampling factors and padded plane in
// blocks (a single component: 1 x 1)
MIJ_HD void scaled_geometry(int w, int h, int ncomp, const int *hs, const int *vs, const int *bw, const int *bh,
                            int denom, ScaledGeom &G) {
  const int s = 8 / denom;
  int hmax = 1, vmax = 1;
  for (int c = 0; c < ncomp; c++) {
    hmax = hs[c] > hmax ? hs[c] : hmax;
    vmax = vs[c] > vmax ? vs[c] : vmax;
  }
  G.ow = (int)(((long long)w * s + 7) / 8);
  G.oh = (int)(((long long)h * s + 7) / 8);
  int fx = 1, fy = 1;
  for (int c = 0; c < 3; c++) {
    ScaledComp &C = G.c[c];
    if (c >= ncomp) {
      C = G.c[0];
      continue;
    }
    int S = s;
    while (S < 8 && (hmax * s) % (hs[c] * S * 2) == 0 && (vmax * s) % (vs[c] * S * 2) == 0) S *= 2;
    C.S = S;
    C.cw = (int)(((long long)w * hs[c] * S + hmax * 8LL - 1) / (hmax * 8LL));
    C.ch = (int)(((long long)h * vs[c] * S + vmax * 8LL - 1) / (vmax * 8LL));
    C.pitch = (S * bw[c] + 7) / 8 * 8;
    C.rows = S * bh[c];
    if (c) {
      fx = hmax * s / (hs[c] * S);
      fy = vmax * s / (vs[c] * S);
    }
  }
  if (ncomp == 1) G.mode = PIX_GREY;
  else if (fx == 1 && fy == 1) G.mode = PIX_444;
  else if (fy == 1) G.mode = (G.c[1].cw > 2 && s > 1) ? PIX_H2V1 : PIX_H2V1_REP;  // libjpeg: no fancy upsampling at IDCT size 1
  else if (fx == 1) G.mode = s > 1 ? PIX_H1V2 : PIX_H1V2_REP;  // (no small-width exception: no horizontal neighbours)
  else G.mode = (G.c[1].cw > 2 && s > 1) ? PIX_H2V2 : PIX_H2V2_REP;
}

// what colour_tile_any needs of it
MIJ_HD PixGeom pix_geometry(const ScaledGeom &G) {
  return PixGeom{G.ow, G.oh, G.mode, G.c[0].pitch, G.c[1].pitch, G.c[1].cw, G.c[1].ch, (3LL * G.ow + 15) / 16 * 16};
}

}  // namespace mij
