// mij_ijg.h -- encoding as libjpeg does: what mij_ijg.hip
// (the front-end kernel) and mij_api.hip (host) share.  Not public.
#pragma once
#include "mij_sampled.h"
// (after the HIP runtime's headers: __forceinline__, __umulhi)
#include "mij_ijg_math.h"

namespace mij {

// k_ijg_fdct's tile is k_samp_dct's: SAMP_TW x SAMP_TH pixels of a padded
// slot = 32 luma blocks; with them 8 + 8 chroma blocks at 4:2:0, 16 + 16 at
// 4:2:2, 32 + 32 at 4:4:4, none for greyscale.

// Real blocks across and down of component c: ceil(w_c / 8) x ceil(h_c / 8)
// with w_c = ceil(w H_c / Hmax), h_c = ceil(h V_c / Vmax); the rest of the
// MCU-padded plane (SampGrid::bw x bh) are dummy blocks.
__host__ __device__ inline void ijg_real_blocks(int w, int h, const SampGrid &g, int c, int &rbw, int &rbh) {
  const int wc = (w * g.hs[c] + g.hmax - 1) / g.hmax, hc = (h * g.vs[c] + g.vmax - 1) / g.vmax;
  rbw = (wc + 7) >> 3;
  rbh = (hc + 7) >> 3;
}

// A frame of the launch: SampFrame (planes in TcComp's layout, MCU-padded
// extents, the slot's padded extent, tiles) and what libjpeg's edge rules
// need beside it.
struct IjgFrame {
  SampFrame s;
  int w, h;            // the frame's true size
  int rbw[3], rbh[3];  // real blocks across and down, per component
};

// per table (0 luma, 1 chroma) and natural position: the quantiser's magic
struct IjgQuant {
  IjgQ q[2][64];
};

struct IjgArgs {
  const uint8_t *in;  // slot 0: B, G, R bytes, rows `pitch` apart (16-byte aligned)
  long long in_fs;    // bytes between slots
  int pitch;
  int sampling;       // MIJ_SAMP_*
  const IjgFrame *fr;
  const IjgQuant *qt;
};

hipError_t launch_ijg_fdct(const IjgArgs &a, int nframes, int max_tiles, hipStream_t s);

}  // namespace mij
