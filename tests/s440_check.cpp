// s440_check.cpp -- runs the arithmetic of decoding a 4:4:0 frame (DESIGN.md
// §4r) at full size and at 1/2, 1/4, 1/8 scale on the host: scaled_geometry,
// the block IDCTs of every size and colour_tile_any in the modes PIX_H1V2 and
// PIX_H1V2_REP (csrc/mij_pixels.h, the code k_dec_idct<S> and k_dec_colour
// call), for tests/test_s440_model.py to compare with the numpy model.  Built
// with -fsanitize=address,undefined: every plane and the pixels are heap
// vectors of exactly the size the decoder gives them, so a load or store past
// them stops the run.
// Input file: int32 w, h, ncomp, denom, then hs, vs, bw, bh and q[64] (zigzag
// order) per component, then per component its padded int16 coefficient plane
// (blocks in raster order, DC absolute).  Output file: int32 mode, then ow, oh,
// ncomp and S, cw, ch, pitch, rows per component (mij_decoder_scaled_layout's
// list), the padded planes, the packed R,G,B pixels, the packed B,G,R pixels.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mij_pixels.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 1;
  int32_t hdr[4];
  if (fread(hdr, sizeof hdr, 1, f) != 1) return 1;
  const int w = hdr[0], h = hdr[1], nc = hdr[2], denom = hdr[3];
  if (w < 1 || h < 1 || nc != 3 || (denom != 1 && denom != 2 && denom != 4 && denom != 8)) return 1;
  int32_t geo[3][4 + 64];
  if (fread(geo, sizeof geo[0], nc, f) != (size_t)nc) return 1;
  int hs[3], vs[3], bw[3], bh[3];
  for (int c = 0; c < nc; c++) {
    hs[c] = geo[c][0];
    vs[c] = geo[c][1];
    bw[c] = geo[c][2];
    bh[c] = geo[c][3];
  }
  mij::ScaledGeom SG;
  mij::scaled_geometry(w, h, nc, hs, vs, bw, bh, denom, SG);
  if (SG.mode != (denom < 8 ? mij::PIX_H1V2 : mij::PIX_H1V2_REP)) {
    fprintf(stderr, "mode %d for a frame given as 4:4:0 at 1/%d\n", SG.mode, denom);
    return 3;
  }
  std::vector<uint8_t> plane[3];
  for (int c = 0; c < nc; c++) {
    const mij::ScaledComp &C = SG.c[c];
    std::vector<int16_t> coef((size_t)64 * bw[c] * bh[c]);
    if (fread(coef.data(), 2, coef.size(), f) != coef.size()) return 1;
    plane[c].assign((size_t)C.pitch * C.rows, 0);
    const int32_t *q = geo[c] + 4;
    for (int b = 0; b < bw[c] * bh[c]; b++) {
      const int16_t *blk = &coef[64 * (size_t)b];
      const uint32_t dc = (uint32_t)(int32_t)blk[0];
      const int by = b / bw[c], bx = b % bw[c];
      uint8_t *dst = &plane[c][(size_t)C.S * by * C.pitch + (size_t)C.S * bx];
      uint32_t r8[8][2], r4[4], r2[2];
      switch (C.S) {
        case 8:
          mij::idct_block(blk, dc, q, r8);
          for (int r = 0; r < 8; r++) mij::store_as(dst + (size_t)r * C.pitch, mij::W2{r8[r][0], r8[r][1]});
          break;
        case 4:
          mij::idct4_block(blk, dc, q, r4);
          for (int r = 0; r < 4; r++)
            for (int k = 0; k < 4; k++) dst[(size_t)r * C.pitch + k] = (uint8_t)(r4[r] >> (8 * k));
          break;
        case 2:
          mij::idct2_block(blk, dc, q, r2);
          for (int r = 0; r < 2; r++)
            for (int k = 0; k < 2; k++) dst[(size_t)r * C.pitch + k] = (uint8_t)(r2[r] >> (8 * k));
          break;
        default:
          dst[0] = (uint8_t)mij::idct1_block(dc, q[0]);
      }
    }
  }
  fclose(f);
  const mij::PixGeom G = mij::pix_geometry(SG);
  const int rows = mij::pix_rows_per_lane(G.mode);
  if (rows != 2) return 3;
  const int units = (SG.oh + rows - 1) / rows, groups = (SG.ow + 15) / 16;
  f = fopen(argv[2], "wb");
  if (!f) return 1;
  std::vector<int32_t> lay = {SG.mode, SG.ow, SG.oh, nc};
  for (int c = 0; c < nc; c++)
    for (int v : {SG.c[c].S, SG.c[c].cw, SG.c[c].ch, SG.c[c].pitch, SG.c[c].rows}) lay.push_back(v);
  if (fwrite(lay.data(), 4, lay.size(), f) != lay.size()) return 1;
  for (int c = 0; c < nc; c++)
    if (fwrite(plane[c].data(), 1, plane[c].size(), f) != plane[c].size()) return 1;
  for (int rgb = 1; rgb >= 0; rgb--) {
    std::vector<uint8_t> px((size_t)G.pitch * SG.oh, 0xA5);
    for (int u = 0; u < units; u++)
      for (int g = 0; g < groups; g++)
        mij::colour_tile_any(plane[0].data(), plane[1].data(), plane[2].data(), G, u, g, rgb, px.data());
    for (int y = 0; y < SG.oh; y++)
      if (fwrite(&px[(size_t)y * G.pitch], 1, 3 * (size_t)SG.ow, f) != 3 * (size_t)SG.ow) return 1;
  }
  return fclose(f) ? 1 : 0;
}
