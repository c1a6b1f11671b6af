// mij_colour_f64.h -- the reference's colour expressions in FP64, shared by
// k_fix_blocks (mij_kernels.hip) and the sampled front end (mij_sampled.hip).
// Not public.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mij {

// The reference's colour expressions in FP64, operation for operation
// (encoder.c:133-135: left to right, no contraction), truncated to uint8_t
// (k_fix_blocks' recomputation of listed blocks; every pixel of k_samp_dct).
__device__ __forceinline__ int y_f64(uint32_t R, uint32_t G, uint32_t B) {
  const double y = __dadd_rn(__dadd_rn(__dmul_rn(0.299, (double)R), __dmul_rn(0.587, (double)G)),
                             __dmul_rn(0.114, (double)B));
  return (int)(uint8_t)(int)y;
}
__device__ __forceinline__ int cb_f64(uint32_t R, uint32_t G, uint32_t B) {
  const double v = __dadd_rn(__dadd_rn(__dadd_rn(128.0, -__dmul_rn(0.168736, (double)R)),
                                       -__dmul_rn(0.331264, (double)G)),
                             __dmul_rn(0.5, (double)B));
  return (int)(uint8_t)(int)v;
}
__device__ __forceinline__ int cr_f64(uint32_t R, uint32_t G, uint32_t B) {
  const double v = __dadd_rn(__dadd_rn(__dadd_rn(128.0, __dmul_rn(0.5, (double)R)),
                                       -__dmul_rn(0.418688, (double)G)),
                             -__dmul_rn(0.081312, (double)B));
  return (int)(uint8_t)(int)v;
}

}  // namespace mij
