// mij_sampled.h -- encoding at a chosen chroma sampling:
// what mij_sampled.hip (the front-end kernel) and mij_api.hip (host) share.
// Not public.
#pragma once
#include "mij_internal.h"

namespace mij {

// A workgroup's tile of k_samp_dct: SAMP_TW x SAMP_TH pixels of a padded slot
// = 32 luma blocks (two block rows of 16); with them the tile's chroma
// blocks: 32 + 32 at 4:4:4, 16 + 16 at 4:2:2, none for greyscale.
constexpr int SAMP_TW = 128;
constexpr int SAMP_TH = 16;

// Blocks across and down of each component of a w x h frame at a sampling
// (MIJ_SAMP_*): the frame padded to whole MCUs of 8 Hmax x 8 Vmax pixels.
struct SampGrid {
  int ncomp, hmax, vmax, mcus_x, mcus_y;
  int hs[3], vs[3], bw[3], bh[3];
  long long nblk;  // blocks of all components
};
__host__ __device__ inline SampGrid samp_grid(int w, int h, int sampling) {
  SampGrid g;
  g.ncomp = sampling == 3 ? 1 : 3;
  g.hmax = sampling <= 1 ? 2 : 1;
  g.vmax = sampling == 0 ? 2 : 1;
  g.mcus_x = (w + 8 * g.hmax - 1) / (8 * g.hmax);
  g.mcus_y = (h + 8 * g.vmax - 1) / (8 * g.vmax);
  g.nblk = 0;
  for (int c = 0; c < 3; c++) {
    g.hs[c] = c ? 1 : g.hmax;
    g.vs[c] = c ? 1 : g.vmax;
    g.bw[c] = c < g.ncomp ? g.mcus_x * g.hs[c] : 0;
    g.bh[c] = c < g.ncomp ? g.mcus_y * g.vs[c] : 0;
    g.nblk += (long long)g.bw[c] * g.bh[c];
  }
  return g;
}

// A frame of the launch: where its planes go (TcComp's layout: raster blocks
// of 64 zigzag coefficients, DC absolute; one absolute DC per block beside
// them) and how much of its slot holds padded pixels.
struct SampFrame {
  int16_t *plane[3];
  int16_t *abs[3];
  int bw[3], bh[3];
  int w16, h16;          // the slot's padded extent (multiples of 16)
  int tiles_x, ntiles;   // tiles across, tiles of the frame
};

struct SampArgs {
  const uint8_t *in;     // slot 0: B, G, R bytes, rows `pitch` apart (16-byte aligned)
  long long in_fs;       // bytes between slots
  int pitch;
  int sampling;          // MIJ_SAMP_422 / _444 / _GRAY
  const SampFrame *fr;
  const Tables *tab;
};

hipError_t launch_samp_dct(const SampArgs &a, int nframes, int max_tiles, hipStream_t s);

}  // namespace mij
