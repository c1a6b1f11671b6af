// foreign_pixels_check.cpp -- runs the decoder's pixel arithmetic for every
// accepted layout (csrc/mij_pixels.h: idct_block and colour_tile_any, the code
// k_dec_idct<8> and k_dec_colour call) on the host, unit by unit as the kernels do,
// for tests/test_foreign_model.py to compare with the numpy model.
// Input file: int32 w, h, ncomp, mode (PIX_*), then bw, bh and q[64] (zigzag
// order) per component, then per component its padded int16 coefficient plane
// (blocks in raster order, DC absolute).  Output file: the padded sample
// planes, the packed R,G,B pixels, the packed B,G,R pixels.
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
  const int w = hdr[0], h = hdr[1], nc = hdr[2], mode = hdr[3];
  if (w < 1 || h < 1 || (nc != 1 && nc != 3)) return 1;
  int32_t geo[3][2 + 64];
  if (fread(geo, sizeof geo[0], nc, f) != (size_t)nc) return 1;
  std::vector<uint8_t> plane[3];
  for (int c = 0; c < nc; c++) {
    const int bw = geo[c][0], bh = geo[c][1];
    std::vector<int16_t> coef((size_t)64 * bw * bh);
    if (fread(coef.data(), 2, coef.size(), f) != coef.size()) return 1;
    plane[c].assign((size_t)64 * bw * bh, 0);
    for (int b = 0; b < bw * bh; b++) {
      const int16_t *blk = &coef[64 * (size_t)b];
      uint32_t rows[8][2];
      mij::idct_block(blk, (uint32_t)(int32_t)blk[0], geo[c] + 2, rows);
      const int by = b / bw, bx = b % bw;
      for (int r = 0; r < 8; r++)
        mij::store_as(&plane[c][((size_t)8 * by + r) * 8 * bw + 8 * bx], mij::W2{rows[r][0], rows[r][1]});
    }
  }
  fclose(f);
  mij::PixGeom G;
  G.w = w;
  G.h = h;
  G.mode = mode;
  G.yp = 8 * geo[0][0];
  G.cp = nc == 3 ? 8 * geo[1][0] : 0;
  const int fx = mode >= mij::PIX_H2V1 ? 2 : 1, fy = mode >= mij::PIX_H2V2 ? 2 : 1;
  G.cw = (w + fx - 1) / fx;
  G.ch = (h + fy - 1) / fy;
  G.pitch = (3LL * w + 15) / 16 * 16;
  const int units = (h + fy - 1) / fy, groups = (w + 15) / 16;
  std::vector<uint8_t> pix[2];
  f = fopen(argv[2], "wb");
  if (!f) return 1;
  for (int c = 0; c < nc; c++)
    if (fwrite(plane[c].data(), 1, plane[c].size(), f) != plane[c].size()) return 1;
  for (int rgb = 1; rgb >= 0; rgb--) {
    std::vector<uint8_t> px((size_t)G.pitch * h, 0xA5);
    const uint8_t *cb = nc == 3 ? plane[1].data() : nullptr, *cr = nc == 3 ? plane[2].data() : nullptr;
    for (int u = 0; u < units; u++)
      for (int g = 0; g < groups; g++) mij::colour_tile_any(plane[0].data(), cb, cr, G, u, g, rgb, px.data());
    for (int y = 0; y < h; y++)
      if (fwrite(&px[(size_t)y * G.pitch], 1, 3 * (size_t)w, f) != 3 * (size_t)w) return 1;
  }
  return fclose(f) ? 1 : 0;
}
