// resize_check.cpp -- runs the resampler's arithmetic (csrc/mij_resize.h:
// rs_build_axis, rs_tap, rs_clip, the code k_rs_h and k_rs_v call and the
// tables the library uploads) on the host, for tests/test_resize_model.py to
// compare with the numpy model.  Built with -ffp-contract=off, as the library
// is.
// Input file: int32 w, h, out_w, out_h, filter, then w * h packed 3-byte
// pixels.  Output file: out_w * out_h packed pixels, then per axis that has a
// pass (horizontal first) its table as rs_build_axis lays it out, then int64
// the largest sum of |weight| of the tables.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mij_resize.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 1;
  int32_t hdr[5];
  if (fread(hdr, sizeof hdr, 1, f) != 1) return 1;
  const int w = hdr[0], h = hdr[1], ow = hdr[2], oh = hdr[3], filter = hdr[4];
  if (w < 1 || h < 1 || ow < 1 || oh < 1 || w > mij::RS_MAX_SIDE || h > mij::RS_MAX_SIDE || ow > mij::RS_MAX_SIDE ||
      oh > mij::RS_MAX_SIDE || filter < 0 || filter >= mij::RS_FILTERS)
    return 1;
  std::vector<uint8_t> src((size_t)3 * w * h);
  if (fread(src.data(), 1, src.size(), f) != src.size()) return 1;
  fclose(f);

  std::vector<int32_t> htab, vtab;
  std::vector<double> k;
  long long worst = 0;
  // horizontal first, to an intermediate of h rows x ow pixels; a pass whose sizes are equal is skipped
  std::vector<uint8_t> mid;
  const std::vector<uint8_t> *cur = &src;
  if (ow != w) {
    const int ks = mij::rs_ksize(w, ow, filter);
    htab.resize((size_t)mij::rs_table_words(w, ow, filter));
    k.resize(ks);
    worst = mij::rs_build_axis(w, ow, filter, htab.data(), k.data());
    mid.resize((size_t)3 * ow * h);
    for (int y = 0; y < h; y++)
      for (int c = 0; c < 3; c++)
        mij::rs_pass_host(src.data() + (size_t)3 * w * y + c, 3, mid.data() + (size_t)3 * ow * y + c, 3, ow, htab.data(), ks);
    cur = &mid;
  }
  std::vector<uint8_t> out;
  if (oh != h) {
    const int ks = mij::rs_ksize(h, oh, filter);
    vtab.resize((size_t)mij::rs_table_words(h, oh, filter));
    k.resize(ks);
    const long long s = mij::rs_build_axis(h, oh, filter, vtab.data(), k.data());
    if (s > worst) worst = s;
    out.resize((size_t)3 * ow * oh);
    for (int b = 0; b < 3 * ow; b++) mij::rs_pass_host(cur->data() + b, 3LL * ow, out.data() + b, 3LL * ow, oh, vtab.data(), ks);
    cur = &out;
  }
  if (!mij::rs_sum_fits(worst)) return 3;

  f = fopen(argv[2], "wb");
  if (!f) return 1;
  const int64_t w64 = worst;
  if (fwrite(cur->data(), 1, cur->size(), f) != cur->size() ||
      fwrite(htab.data(), 4, htab.size(), f) != htab.size() || fwrite(vtab.data(), 4, vtab.size(), f) != vtab.size() ||
      fwrite(&w64, 8, 1, f) != 1 || fclose(f))
    return 1;
  return 0;
}
