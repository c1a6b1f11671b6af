// pixels_check.cpp -- runs the decoder's pixel arithmetic (csrc/mij_pixels.h,
// the code the kernels of mij_decode.hip call) on the host, tile by tile as
// the kernels do, for tests/test_decode_model.py to compare with the numpy
// model.  Input file: int32 w, h, luma q[64], chroma q[64] (zigzag order),
// then the int16 coefficient planes Y[w*h], Cb[w*h/4], Cr[w*h/4] (DC as the
// coded difference).  Output file: the planes (w*h*3/2 bytes), the R,G,B
// pixels, the B,G,R pixels.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mij_pixels.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 1;
  int32_t hdr[2 + 128];
  if (fread(hdr, sizeof hdr, 1, f) != 1) return 1;
  const int w = hdr[0], h = hdr[1];
  if (w < 16 || h < 16 || w % 16 || h % 16) return 1;
  const size_t ny = (size_t)w * h, ns = ny * 3 / 2;
  std::vector<int16_t> coef(ns);
  if (fread(coef.data(), 2, ns, f) != ns) return 1;
  fclose(f);
  std::vector<uint8_t> planes(ns), rgb(3 * ny), bgr(3 * ny);
  const size_t off[3] = {0, ny, ny + ny / 4};
  for (int c = 0; c < 3; c++) {
    const int bw = c ? w / 16 : w / 8, nblocks = (int)((c ? ny / 4 : ny) / 64);
    uint32_t dc = 0;  // k_dec_dc on a one-component scan: running sum modulo 2^32 in raster order
    for (int b = 0; b < nblocks; b++) {
      const int16_t *blk = &coef[off[c] + 64 * (size_t)b];
      dc += (uint32_t)(int32_t)blk[0];
      uint32_t rows[8][2];
      mij::idct_block(blk, dc, hdr + 2 + (c ? 64 : 0), rows);
      const int by = b / bw, bx = b % bw;
      for (int r = 0; r < 8; r++)
        mij::store_as(&planes[off[c] + ((size_t)8 * by + r) * 8 * bw + 8 * bx], mij::W2{rows[r][0], rows[r][1]});
    }
  }
  // the frame's geometry as the decoder computes it: 4:2:0 at full size
  const int hs[3] = {2, 1, 1}, vs[3] = {2, 1, 1}, bw[3] = {w / 8, w / 16, w / 16}, bh[3] = {h / 8, h / 16, h / 16};
  mij::ScaledGeom S;
  mij::scaled_geometry(w, h, 3, hs, vs, bw, bh, 1, S);
  const mij::PixGeom G = mij::pix_geometry(S);
  for (int r = 0; r < h / 2; r++)
    for (int g = 0; g < w / 16; g++) {
      mij::colour_tile_any(&planes[0], &planes[ny], &planes[ny + ny / 4], G, r, g, 1, rgb.data());
      mij::colour_tile_any(&planes[0], &planes[ny], &planes[ny + ny / 4], G, r, g, 0, bgr.data());
    }
  f = fopen(argv[2], "wb");
  if (!f || fwrite(planes.data(), 1, ns, f) != ns || fwrite(rgb.data(), 1, 3 * ny, f) != 3 * ny ||
      fwrite(bgr.data(), 1, 3 * ny, f) != 3 * ny || fclose(f))
    return 1;
  return 0;
}
