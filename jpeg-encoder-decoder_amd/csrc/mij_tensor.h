// mij_tensor.h -- the arithmetic of the pixels-to-tensor stage (DESIGN.md
// §4o), stated once: torchvision's to_tensor followed by normalize on one
// source byte, in IEEE single precision, round to nearest even:
//
//   t = (float)v / 255.0f;   t = t - mean[c];   t = t / std[c];
//
// float32 stores t, float16 and bfloat16 store t rounded to nearest even (what
// tensor.to(torch.float16 / torch.bfloat16) gives), uint8 stores v.
//
//   tz_build_lut    (host) lut[3][256] in the output dtype: entry [c][v] is
//                   the element tensor channel c gets for source byte v.  The
//                   kernel only looks values up, so the result does not
//                   depend on how the device divides.  Must be compiled with
//                   -ffp-contract=off wherever it is compiled, like the rest
//                   of the library (no expression here can contract, the flag
//                   keeps that true).
//   tz_src_channel  (host and device) the pixel byte tensor channel c reads.
//
// Shared by k_tensorize (mij_tensor.hip) and the host check
// tests/tensor_check.cpp.  Plain C++: no HIP, nothing but the standard headers.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define MIJ_TZ_HD __host__ __device__ __forceinline__
#else
#define MIJ_TZ_HD inline
#endif

namespace mij {

enum { TZ_U8 = 0, TZ_F16 = 1, TZ_BF16 = 2, TZ_F32 = 3, TZ_DTYPES = 4 };  // MIJ_T_*
enum { TZ_NCHW = 0, TZ_NHWC = 1, TZ_LAYOUTS = 2 };
constexpr int TZ_MAX_SIDE = 65535;
// k_tensorize's tile: TZ_ROWS rows of TZ_SEG pixels per workgroup
constexpr int TZ_SEG = 256;
constexpr int TZ_ROWS = 8;

// bytes of an element; 0 for an unknown dtype
MIJ_TZ_HD int tz_esize(int dtype) { return dtype == TZ_U8 ? 1 : dtype == TZ_F16 || dtype == TZ_BF16 ? 2 : dtype == TZ_F32 ? 4 : 0; }

// swap: tensor channel c reads pixel byte 2 - c (BGR pixels, RGB tensor)
MIJ_TZ_HD int tz_src_channel(int c, int swap) { return swap ? 2 - c : c; }

inline uint32_t tz_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

inline float tz_value(int v, float mean, float std) {
  float t = (float)v / 255.0f;
  t = t - mean;
  t = t / std;
  return t;
}

// IEEE binary16 of f, round to nearest even; overflow gives infinity
inline uint16_t tz_f16(float f) {
  uint32_t x = tz_bits(f);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
  x &= 0x7FFFFFFFu;
  if (x >= 0x7F800000u) return (uint16_t)(sign | (x > 0x7F800000u ? 0x7E00u : 0x7C00u));
  const int e = (int)(x >> 23);
  if (e < 113) {  // under 2^-14: a binary16 subnormal, in units of 2^-24
    const int s = 126 - e;
    if (s > 24) return sign;  // under 2^-25: nearer to 0 than to the smallest subnormal
    const uint32_t m = (x & 0x7FFFFFu) | 0x800000u;
    uint32_t r = m >> s;
    const uint32_t rem = m & ((1u << s) - 1), half = 1u << (s - 1);
    if (rem > half || (rem == half && (r & 1))) r++;
    return (uint16_t)(sign | r);
  }
  uint32_t r = ((uint32_t)(e - 112) << 10) | ((x & 0x7FFFFFu) >> 13);
  const uint32_t rem = x & 0x1FFFu;
  if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) r++;  // may carry into the exponent, up to infinity
  return (uint16_t)(sign | (r > 0x7C00u ? 0x7C00u : r));
}

// bfloat16 of f, round to nearest even
inline uint16_t tz_bf16(float f) {
  uint32_t x = tz_bits(f);
  if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((x >> 16) | 0x40u);
  x += 0x7FFFu + ((x >> 16) & 1u);
  return (uint16_t)(x >> 16);
}

// lut: 3 * 256 elements of tz_esize(dtype) bytes, channel-major
inline void tz_build_lut(int dtype, const float mean[3], const float std[3], void *lut) {
  for (int c = 0; c < 3; c++)
    for (int v = 0; v < 256; v++) {
      const int i = 256 * c + v;
      if (dtype == TZ_U8) {
        ((uint8_t *)lut)[i] = (uint8_t)v;
        continue;
      }
      const float t = tz_value(v, mean[c], std[c]);
      if (dtype == TZ_F16) ((uint16_t *)lut)[i] = tz_f16(t);
      else if (dtype == TZ_BF16) ((uint16_t *)lut)[i] = tz_bf16(t);
      else ((uint32_t *)lut)[i] = tz_bits(t);
    }
}

}  // namespace mij
