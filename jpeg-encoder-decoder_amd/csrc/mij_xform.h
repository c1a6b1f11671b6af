// mij_xform.h -- the index and sign mapping of the lossless geometric
// transforms: flip, transpose, rotation and MCU-aligned crop
// of a plane of 8x8 blocks of zigzag coefficients, ordered by DESTINATION:
//
//   (plane geometry, operation, destination block, zigzag position)
//       -> (source block, source zigzag position, sign)
//
// Shared by k_xf_blocks (mij_transform.hip) and the host check
// tests/xform_check.cpp, so the CPU suite runs the very mapping the GPU runs.
// Plain C++: no HIP, nothing but <stdint.h>.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MIJ_XF_HD __host__ __device__ __forceinline__
#else
#define MIJ_XF_HD inline
#endif

namespace mij {

// what an operation is made of, applied in this order to the cropped plane
enum { XF_T = 1,    // transpose
       XF_FH = 2,   // then mirror the OUTPUT left-right
       XF_FV = 4 }; // and / or top-bottom

// bits of the public operations MIJ_XF_NONE .. MIJ_XF_ROT270 (jpegtran's JXFORM order)
constexpr int XF_OPS = 8;
MIJ_XF_HD int xf_op_bits(int op) {
  // none, flip_h, flip_v, transpose, transverse, rot90 (clockwise), rot180, rot270
  constexpr int bits[XF_OPS] = {0, XF_FH, XF_FV, XF_T, XF_T | XF_FH | XF_FV, XF_T | XF_FH, XF_FH | XF_FV, XF_T | XF_FV};
  return op >= 0 && op < XF_OPS ? bits[op] : 0;
}

// One component's planes.  The source is a raster of sbw blocks across; the
// part that is kept starts ox blocks in and oy blocks down (the crop) and is
// dbw x dbh blocks after the operation (dbh x dbw before a transposing one).
struct XfGeo {
  int sbw;       // source plane: blocks across
  int dbw, dbh;  // destination plane: blocks across and down
  int ox, oy;    // the crop's offset in the source plane, in blocks
  int bits;      // XF_T | XF_FH | XF_FV
};

// raster index in the source plane of the block that lands on destination
// block (by, bx), 0 <= by < dbh, 0 <= bx < dbw
MIJ_XF_HD int xf_src_block(const XfGeo &g, int by, int bx) {
  if (g.bits & XF_FH) bx = g.dbw - 1 - bx;
  if (g.bits & XF_FV) by = g.dbh - 1 - by;
  const int sy = g.bits & XF_T ? bx : by, sx = g.bits & XF_T ? by : bx;
  return (g.oy + sy) * g.sbw + g.ox + sx;
}

// zigzag position of the transposed coefficient: C[v][u] of position z is
// C[u][v] of position XF_TZ[z].  An involution that keeps every anti-diagonal.
#define MIJ_XF_TZ                                                                                     \
  {0,  2,  1,  5,  4,  3,  9,  8,  7,  6,  14, 13, 12, 11, 10, 20, 19, 18, 17, 16, 15, 27,            \
   26, 25, 24, 23, 22, 21, 35, 34, 33, 32, 31, 30, 29, 28, 42, 41, 40, 39, 38, 37, 36, 48,            \
   47, 46, 45, 44, 43, 53, 52, 51, 50, 49, 57, 56, 55, 54, 60, 59, 58, 62, 61, 63}
// zigzag positions whose horizontal frequency u (XF_ODD_U) or vertical
// frequency v (XF_ODD_V) is odd: bit z.  The DC's bit is clear in both.
constexpr uint64_t XF_ODD_U = 0xb56aad55554aa952ull;
constexpr uint64_t XF_ODD_V = 0xd6ab555aa5552a94ull;

// positions of the DESTINATION block whose coefficient changes sign:
// s_h = (-1)^u with a left-right mirror, s_v = (-1)^v with a top-bottom one
MIJ_XF_HD uint64_t xf_neg_mask(int bits) {
  return (bits & XF_FH ? XF_ODD_U : 0) ^ (bits & XF_FV ? XF_ODD_V : 0);
}

MIJ_XF_HD int xf_src_pos(int bits, int z) {
  constexpr uint8_t tz[64] = MIJ_XF_TZ;
  return bits & XF_T ? tz[z] : z;
}

namespace xf_detail {
// the tables above, derived again from the zigzag scan at compile time
constexpr bool tables_ok() {
  constexpr int zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  constexpr uint8_t tz[64] = MIJ_XF_TZ;
  for (int z = 0; z < 64; z++) {
    const int v = zz[z] >> 3, u = zz[z] & 7;
    if (zz[tz[z]] != u * 8 + v) return false;
    if (((XF_ODD_U >> z) & 1) != (uint64_t)(u & 1) || ((XF_ODD_V >> z) & 1) != (uint64_t)(v & 1)) return false;
  }
  return true;
}
static_assert(tables_ok(), "XF_TZ / XF_ODD_U / XF_ODD_V do not match the zigzag scan");
}  // namespace xf_detail

}  // namespace mij
