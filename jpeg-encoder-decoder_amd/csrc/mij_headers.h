// mij_headers.h -- the JFIF frame headers, shared by the three-scan assembly
// (mij_kernels.hip k_emit_scan, k_band_join) and the interleaved one
// (mij_interleave.hip).  Device code only.
#pragma once
#include "mij_internal.h"

namespace mij {

// Frame headers (encoder.c:549-600) into out[0, hlen); returns hlen.  Called
// by a whole workgroup (s_n: 4 ints of LDS; one barrier inside).
__device__ __forceinline__ int emit_headers(const EntArgs &a, int f, uint8_t *out, int *s_n) {
  const int tid = threadIdx.x;
  const HuffCode *hc = a.hc + (long long)f * 4;
  // headers, one byte per thread (a single thread's byte loop is a chain of
  // dependent loads and stores: 40 us per launch): APP0 20 + DQT 2 x 69 +
  // DHT 4 x (21 + n_t) + SOF0 19
  {
    int hn = tid < 64 ? hc[tid >> 4].code_len_freq[1 + (tid & 15)] : 0;
    for (int o = 8; o; o >>= 1) hn += __shfl_xor(hn, o);  // sums over 16 lanes
    if (tid < 64 && (tid & 15) == 0) s_n[tid >> 4] = hn;
  }
  __syncthreads();
  int doff[5];  // DHT t starts at doff[t]; SOF0 at doff[4]
  doff[0] = 20 + 2 * 69;
  for (int t = 0; t < 4; t++) doff[t + 1] = doff[t] + 21 + s_n[t];
  const int hlen = doff[4] + 19;
  {
    const FGeom fg = frame_geom(a.g, a.fdims, f);
    const int W = fg.w, H = fg.h;
    auto hbyte = [&](int i) -> uint8_t {
      if (i < 20) {
        const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 0x4A, 0x46, 0x49, 0x46,
                                  0x00, 0x01, 0x01, 0x00, 0x00, 0x48, 0x00, 0x48, 0x00, 0x00};
        return app0[i];
      }
      if (i < doff[0]) {  // DQT (encoder.c:559-571)
        const int t = (i - 20) / 69, k = (i - 20) - 69 * t;
        const uint8_t m[5] = {0xFF, 0xDB, 0x00, 0x43, (uint8_t)t};
        return k < 5 ? m[k] : (uint8_t)a.tab->dqt[t][k - 5];
      }
      if (i < doff[4]) {  // DHT (encoder.c:504-532)
        const int t = i >= doff[3] ? 3 : i >= doff[2] ? 2 : i >= doff[1] ? 1 : 0;
        const int k = i - doff[t], len = 19 + s_n[t];
        const uint8_t m[5] = {0xFF, 0xC4, (uint8_t)(len >> 8), (uint8_t)len, (uint8_t)((t & 1) << 4 | (t >> 1))};
        return k < 5 ? m[k] : k < 21 ? (uint8_t)hc[t].code_len_freq[k - 4] : (uint8_t)hc[t].sym_sorted[k - 21];
      }
      // SOF0 (encoder.c:573-600)
      const uint8_t sof[19] = {0xFF, 0xC0, 0x00, 0x11, 0x08, (uint8_t)(H >> 8), (uint8_t)H,
                               (uint8_t)(W >> 8), (uint8_t)W, 0x03, 0x01, 0x22, 0x00,
                               0x02, 0x11, 0x01, 0x03, 0x11, 0x01};
      return sof[i - doff[4]];
    };
    // a thread's first HB bytes all computed before any is stored: their
    // loads then go out together instead of each waiting behind the store
    // before it (hlen = 261 + the four tables' symbols: <= 768 whenever the
    // tables hold <= 507 symbols in all -- 2 x 162 AC + 2 x 12 DC at most in
    // practice; the loop after covers the rest)
    constexpr int HB = 3;
    uint8_t hv[HB];
#pragma unroll
    for (int hb = 0; hb < HB; hb++) hv[hb] = tid + 256 * hb < hlen ? hbyte(tid + 256 * hb) : (uint8_t)0;
#pragma unroll
    for (int hb = 0; hb < HB; hb++)
      if (tid + 256 * hb < hlen) out[tid + 256 * hb] = hv[hb];
    for (int i = tid + 256 * HB; i < hlen; i += 256) out[i] = hbyte(i);
  }
  return hlen;
}

}  // namespace mij
