// mij_transform.hip -- the gfx950 kernel of the lossless geometric transforms
// (DESIGN.md §4i): flip, transpose, rotation by 90/180/270 and MCU-aligned
// crop in the coefficient domain, one stage between k_tc_abs and k_tc_hist
// (mij_transcode.hip).  It writes the transformed planes and absolute DCs;
// the k_tc_* stages then code them as they code any TcFrame.
//
//   k_xf_blocks   ordered by destination: 8 lanes x 16 bytes store one whole
//                 aligned 128-byte block, 8 blocks per wave instruction; the
//                 block is gathered from the source as one whole 128-byte
//                 block wherever it lies (xf_src_block, mij_xform.h).  A
//                 group of 8 lanes owns XF_PER blocks and loads them all
//                 before it uses the first, for bytes in flight.  Without a
//                 transpose a lane keeps its 8 zigzag positions and flips the
//                 signs its constant mask names.  With one the block goes
//                 through LDS and comes back by the constant permutation
//                 XF_TZ.  Every index is bounded by the host's geometry
//                 (XfGeo), none by stream contents.
#include "mij_transform.h"

namespace mij {

// LDS row of one block: 32 dwords and one of padding, so that the blocks a
// half-wave holds start on different banks
constexpr int XF_ROW = 33;
constexpr int XF_GROUPS = 32;                      // 8-lane groups of a workgroup
constexpr int XF_PER = XF_WG_BLOCKS / XF_GROUPS;   // blocks per group

__global__ __launch_bounds__(256) void k_xf_blocks(const XfFrame *frames) {
  __shared__ uint32_t tile[XF_WG_BLOCKS][XF_ROW];
  const XfFrame &F = frames[blockIdx.y];
  if ((long long)blockIdx.x * XF_WG_BLOCKS >= F.nblk) return;  // (the whole workgroup)
  const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
  const int bits = F.c[0].g.bits;  // the same in every component and frame of a call
  bool live[XF_PER];
  int d[XF_PER], sblk[XF_PER], comp[XF_PER];
  uint32_t w[XF_PER][4];
#pragma unroll
  for (int k = 0; k < XF_PER; k++) {
    const int i = blockIdx.x * XF_WG_BLOCKS + k * XF_GROUPS + g;
    live[k] = i < F.nblk;
    const int c = F.ncomp > 1 && i >= F.c[1].blk0 ? (F.ncomp > 2 && i >= F.c[2].blk0 ? 2 : 1) : 0;
    const XfComp &C = F.c[c];
    comp[k] = c;
    d[k] = sblk[k] = 0;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (live[k]) {
      const XfGeo geo = C.g;
      d[k] = i - C.blk0;  // < dbw * dbh
      const int by = d[k] / geo.dbw, bx = d[k] - by * geo.dbw;
      sblk[k] = xf_src_block(geo, by, bx);  // inside the source plane: the host checked the crop against it
      v = *(const uint4 *)(C.src + 64LL * sblk[k] + 8 * l);
    }
    w[k][0] = v.x, w[k][1] = v.y, w[k][2] = v.z, w[k][3] = v.w;
  }
  if (bits & XF_T) {
    constexpr uint8_t tz[64] = MIJ_XF_TZ;
#pragma unroll
    for (int k = 0; k < XF_PER; k++)
#pragma unroll
      for (int j = 0; j < 4; j++) tile[k * XF_GROUPS + g][4 * l + j] = w[k][j];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < XF_PER; k++) {
      const uint16_t *row = (const uint16_t *)tile[k * XF_GROUPS + g];
#pragma unroll
      for (int j = 0; j < 4; j++)
        w[k][j] = (uint32_t)row[tz[8 * l + 2 * j]] | ((uint32_t)row[tz[8 * l + 2 * j + 1]] << 16);
    }
  }
  const uint32_t neg = (uint32_t)(xf_neg_mask(bits) >> (8 * l)) & 255u;
#pragma unroll
  for (int k = 0; k < XF_PER; k++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t lo = w[k][j] & 0xFFFFu, hi = w[k][j] >> 16;
      if (neg & (1u << (2 * j))) lo = (0u - lo) & 0xFFFFu;
      if (neg & (2u << (2 * j))) hi = (0u - hi) & 0xFFFFu;
      w[k][j] = lo | (hi << 16);
    }
    if (!live[k]) continue;
    const XfComp &C = F.c[comp[k]];
    *(uint4 *)(C.dst + 64LL * d[k] + 8 * l) = make_uint4(w[k][0], w[k][1], w[k][2], w[k][3]);
    if (l == 0) C.dst_abs[d[k]] = C.src_abs[sblk[k]];
  }
}

hipError_t launch_xf_blocks(const XfFrame *frames, int nframes, int max_nblk, hipStream_t s) {
  const unsigned wgs = (unsigned)((max_nblk + XF_WG_BLOCKS - 1) / XF_WG_BLOCKS);
  hipLaunchKernelGGL(k_xf_blocks, dim3(wgs, nframes), dim3(256), 0, s, frames);
  return hipGetLastError();
}

}  // namespace mij
