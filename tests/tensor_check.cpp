// tensor_check.cpp -- builds the four tables of the pixels-to-tensor stage
// with csrc/mij_tensor.h (tz_build_lut: what the library uploads and
// k_tensorize looks up) on the host, for tests/test_tensor_model.py to compare
// with the numpy model.  Built with -ffp-contract=off, as the library is.
// Arguments: the bit patterns of mean[0..2] and std[0..2] (float32) in hex.
// Output: per dtype (uint8, float16, bfloat16, float32) one line "dtype N"
// followed by one line of 768 hex elements, channel-major.
#include <stdio.h>
#include <stdlib.h>

#include "mij_tensor.h"

int main(int argc, char **argv) {
  if (argc != 7) return 2;
  float mean[3], std[3];
  for (int c = 0; c < 3; c++) {
    const uint32_t m = (uint32_t)strtoul(argv[1 + c], nullptr, 16), s = (uint32_t)strtoul(argv[4 + c], nullptr, 16);
    memcpy(&mean[c], &m, 4);
    memcpy(&std[c], &s, 4);
  }
  for (int dtype = 0; dtype < mij::TZ_DTYPES; dtype++) {
    uint32_t lut[3 * 256];
    const int es = mij::tz_esize(dtype);
    mij::tz_build_lut(dtype, mean, std, lut);
    printf("dtype %d\n", dtype);
    for (int i = 0; i < 3 * 256; i++) {
      const uint32_t e = es == 1 ? ((const uint8_t *)lut)[i] : es == 2 ? ((const uint16_t *)lut)[i] : lut[i];
      printf("%x%c", e, i == 3 * 256 - 1 ? '\n' : ' ');
    }
  }
  return mij::tz_esize(mij::TZ_DTYPES) == 0 && mij::tz_src_channel(0, 1) == 2 && mij::tz_src_channel(1, 1) == 1 ? 0 : 3;
}
