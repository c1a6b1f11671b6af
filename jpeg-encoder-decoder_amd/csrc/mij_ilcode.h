// mij_ilcode.h -- device helpers of the one-scan entropy coders: the
// interleaved output format (mij_interleave.hip) and lossless
// transcoding (mij_transcode.hip, §4h) code blocks, sum over a workgroup and
// count 0xFF bytes the same way.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mij {

__device__ __forceinline__ int il_class(int v) {  // encoder.c:303-313
  v = v < 0 ? -v : v;
  return 32 - __clz(v);
}
__device__ __forceinline__ uint32_t il_mag(int v, int cls) {  // encoder.c:442-444
  uint32_t id = (uint32_t)(v < 0 ? -v : v);
  if (v < 0) id = ~id;
  return id & ((1u << cls) - 1u);
}

// One block's symbols in coding order: emit(table 0 DC / 1 AC, symbol,
// value, value bits).  blk: its 64 zigzag coefficients (128-byte aligned).
template <class Emit>
__device__ __forceinline__ void il_walk(const int16_t *blk, int diff, const Emit &emit) {
  unsigned long long nz = 0;
  const uint4 *q = (const uint4 *)blk;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint4 v = q[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (w[j] & 0xFFFFu) nz |= 1ull << (8 * i + 2 * j);
      if (w[j] >> 16) nz |= 1ull << (8 * i + 2 * j + 1);
    }
  }
  const int dcls = il_class(diff);
  emit(0, dcls, diff, dcls);
  const bool eob = !(nz >> 63);
  nz &= ~1ull;
  int prev = 0;
  while (nz) {
    const int p = __ffsll((long long)nz) - 1;
    nz &= nz - 1ull;
    int run = p - prev - 1;
    for (; run >= 16; run -= 16) emit(1, 0xF0, 0, 0);
    const int v = blk[p], cls = il_class(v);
    emit(1, ((run << 4) & 0xF0) | (cls & 15), v, cls & 15);
    prev = p;
  }
  if (eob) emit(1, 0x00, 0, 0);
}

// inclusive prefix sum over a 256-thread workgroup; total in every thread
template <class T>
__device__ __forceinline__ T il_scan256(T v, T *red /* [4] */, T &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  __syncthreads();  // (red: the call before has read it)
  if (lane == 63) red[wave] = v;
  __syncthreads();
  T before = 0;
  total = 0;
  for (int q = 0; q < 4; q++) {
    if (q < wave) before += red[q];
    total += red[q];
  }
  return v + before;
}

// 0xFF bytes among the first lim bytes (big-endian order) of a scan word
__device__ __forceinline__ int il_ff(uint32_t w, int lim) {
  int n = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) n += j < lim && ((w >> (24 - 8 * j)) & 255u) == 255u;
  return n;
}

}  // namespace mij
