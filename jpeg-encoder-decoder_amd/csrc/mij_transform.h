// mij_transform.h -- lossless geometric transforms: what
// mij_transform.hip (the kernel) and mij_decode.hip (host) share.  Not public.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mij_xform.h"

namespace mij {

// blocks per workgroup of k_xf_blocks: 32 groups of 8 lanes x 16 bytes, 4 blocks each
constexpr int XF_WG_BLOCKS = 128;

struct XfComp {
  const int16_t *src;      // the decoded padded plane: raster blocks of 64 zigzag coefficients
  const int16_t *src_abs;  // its absolute DCs (k_tc_abs)
  int16_t *dst;            // the transformed plane, g.dbw x g.dbh blocks
  int16_t *dst_abs;        // its absolute DCs
  XfGeo g;
  int blk0;                // the component's first block among the frame's destination blocks
  int pad;
};

struct XfFrame {
  XfComp c[3];
  int ncomp;
  int nblk;  // destination blocks of all components
};

// every frame's planes and absolute DCs, transformed: grid row = frame
hipError_t launch_xf_blocks(const XfFrame *frames, int nframes, int max_nblk, hipStream_t s);

}  // namespace mij
