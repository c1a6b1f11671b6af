// mij_sampled.hip -- gfx950 front end of encoding at a chosen chroma sampling
// (DESIGN.md §4k): padded B, G, R slots -> quantised coefficient planes at
// 4:4:4, 4:2:2 or greyscale, in the layout the transcoder's entropy coder
// takes (TcComp, mij_transcode.h).  4:2:0 stays with K1.
//
//   k_samp_dct   colour conversion, optional horizontal averaging, FP64 DCT,
//                truncating quantisation, clip, zigzag; planes and absolute DCs
//
// Every operation that decides a bit is the reference's, in its order
// (encoder.c:133-135 colour, :137-138 averaging in its two-sample form,
// :81-112 DCT and quantisation), written with __dmul_rn / __dadd_rn /
// __ddiv_rn: there is no fast path and so nothing to replay.  This is
// k_fix_blocks' arithmetic (mij_kernels.hip) in another shape: a workgroup
// takes a SAMP_TW x SAMP_TH pixel tile, eight lanes take a block, and a lane
// holds a whole column (pass 1) and then a whole row (pass 2) in registers.
#include "mij_colour_f64.h"
#include "mij_pixels.h"
#include "mij_sampled.h"

namespace mij {

namespace {

constexpr double SAMP_SQRT1_2 = 0.70710678118654752440;  // <math.h> M_SQRT1_2
// doubles between the column-pass results of two blocks: 64 + 8, so that the
// eight blocks of a wave start 64 bytes apart modulo the 256-byte bank row
constexpr int SAMP_INNER = 72;
constexpr int SAMP_LINES = SAMP_TW * 3 / 16;  // 16-byte lines per tile row

struct SampIzz {
  uint8_t v[64];
};
constexpr SampIzz samp_izz() {  // zigzag index of natural position n
  constexpr uint8_t zz[64] = MIJ_ZIGZAG;
  SampIzz r = {};
  for (int z = 0; z < 64; z++) r.v[zz[z]] = (uint8_t)z;
  return r;
}
__constant__ SampIzz c_samp_izz = samp_izz();

// LDS written by some lanes of a wave, read by others of the same wave
__device__ __forceinline__ void samp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// floor((a + b) / 2) of each byte pair
__device__ __forceinline__ uint32_t avg_bytes(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) >> 1) & 0x7F7F7F7Fu); }

}  // namespace

// grid (tiles of the largest frame, frames); 256 threads
__global__ __launch_bounds__(256) void k_samp_dct(SampArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[SAMP_TH][SAMP_TW * 3];
  // sample planes, one 64-byte block after another, a block column-major
  // (byte xt * 8 + yt): blocks 0..31 luma (by * 16 + bx), then Cb, then Cr
  __shared__ __attribute__((aligned(16))) uint8_t s_smp[96 * 64];
  __shared__ __attribute__((aligned(16))) double s_inner[32 * SAMP_INNER];  // per block [yf][xt]
  __shared__ __attribute__((aligned(16))) int16_t s_out[32 * 64];           // per block, zigzag
  __shared__ double s_cos[64];
  __shared__ double s_q[2][64];  // natural order
  __shared__ uint8_t s_izz[64];
  const int tid = threadIdx.x, f = blockIdx.y;
  const SampFrame &F = a.fr[f];
  if ((int)blockIdx.x >= F.ntiles) return;
  const int ty = blockIdx.x / F.tiles_x, tx = blockIdx.x - ty * F.tiles_x;
  if (tid < 64) {
    s_cos[tid] = a.tab->cosd[tid];
    s_izz[tid] = c_samp_izz.v[tid];
  }
  if (tid < 128) {  // qint is in zigzag order
    const int c = tid >> 6, n = tid & 63;
    s_q[c][n] = (double)a.tab->qint[c][c_samp_izz.v[n]];
  }
  // the tile's rows, as 16-byte lines; lines past the padded frame stay zero
  {
    const uint8_t *slot = a.in + (long long)f * a.in_fs;
    for (int i = tid; i < SAMP_TH * SAMP_LINES; i += 256) {
      const int row = i / SAMP_LINES, l = i - row * SAMP_LINES;
      const int y = ty * SAMP_TH + row, xb = tx * SAMP_TW * 3 + 16 * l;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (y < F.h16 && xb + 16 <= F.w16 * 3) v = *(const uint4 *)(slot + (long long)y * a.pitch + xb);
      *(uint4 *)&s_raw[row][16 * l] = v;
    }
  }
  __syncthreads();
  const bool grey = a.sampling == 3, h2 = a.sampling == 1;
  // colour: a thread takes eight pixels of a column, one block's column
  {
    const int x = tid & 127, half = tid >> 7;
    uint32_t yv[2] = {0u, 0u}, bv[2] = {0u, 0u}, rv[2] = {0u, 0u};
#pragma unroll
    for (int yt = 0; yt < 8; yt++) {
      const uint8_t *px = &s_raw[half * 8 + yt][x * 3];
      const uint32_t B = px[0], G = px[1], R = px[2];
      yv[yt >> 2] |= (uint32_t)y_f64(R, G, B) << (8 * (yt & 3));
      if (!grey) {
        bv[yt >> 2] |= (uint32_t)cb_f64(R, G, B) << (8 * (yt & 3));
        rv[yt >> 2] |= (uint32_t)cr_f64(R, G, B) << (8 * (yt & 3));
      }
    }
    *(uint2 *)&s_smp[(half * 16 + (x >> 3)) * 64 + (x & 7) * 8] = make_uint2(yv[0], yv[1]);
    if (!grey) {
      if (h2) {  // (a + b) / 2 over the truncated samples of a horizontal pair
        const uint32_t b0 = __shfl_down(bv[0], 1), b1 = __shfl_down(bv[1], 1);
        const uint32_t r0 = __shfl_down(rv[0], 1), r1 = __shfl_down(rv[1], 1);
        if (!(x & 1)) {
          const int cx = x >> 1;
          const int o = (half * 8 + (cx >> 3)) * 64 + (cx & 7) * 8;
          *(uint2 *)&s_smp[32 * 64 + o] = make_uint2(avg_bytes(bv[0], b0), avg_bytes(bv[1], b1));
          *(uint2 *)&s_smp[48 * 64 + o] = make_uint2(avg_bytes(rv[0], r0), avg_bytes(rv[1], r1));
        }
      } else {
        const int o = (half * 16 + (x >> 3)) * 64 + (x & 7) * 8;
        *(uint2 *)&s_smp[32 * 64 + o] = make_uint2(bv[0], bv[1]);
        *(uint2 *)&s_smp[64 * 64 + o] = make_uint2(rv[0], rv[1]);
      }
    }
  }
  __syncthreads();
  // 32 blocks per pass, eight lanes a block: the eight are lanes of one wave
  // and s_inner / s_out are the block's own, so from here on what one lane
  // writes only lanes of its wave read, and a wave-level barrier orders it
  const int nc = grey ? 0 : h2 ? 16 : 32;  // chroma blocks per plane and tile
  const int npass = (32 + 2 * nc) / 32;
  const int lb = tid >> 3, k = tid & 7;
  for (int p = 0; p < npass; p++) {
    const int j = p * 32 + lb;
    int c = 0, by = j >> 4, bx = j & 15, tbw = 16;
    if (j >= 32) {
      const int jj = j - 32, r = jj >= nc ? jj - nc : jj;
      c = jj >= nc ? 2 : 1;
      tbw = nc >> 1;
      by = r / tbw;
      bx = r - by * tbw;
    }
    const int gbx = tx * tbw + bx, gby = ty * 2 + by;
    const bool valid = gbx < F.bw[c] && gby < F.bh[c];
    if (valid) {  // column pass: lane = column xt = k, summed from 0 in y_t order
      const uint2 sv = *(const uint2 *)&s_smp[j * 64 + k * 8];
      double d[8];
#pragma unroll
      for (int yt = 0; yt < 8; yt++)
        d[yt] = (double)((int)(((yt < 4 ? sv.x : sv.y) >> (8 * (yt & 3))) & 255u) - 128);
#pragma unroll
      for (int yf = 0; yf < 8; yf++) {
        double in = 0.0;
#pragma unroll
        for (int yt = 0; yt < 8; yt++) in = __dadd_rn(in, __dmul_rn(d[yt], s_cos[yt * 8 + yf]));
        s_inner[lb * SAMP_INNER + yf * 8 + k] = in;
      }
    }
    samp_wave_sync();
    if (valid) {  // row pass: lane = vertical frequency v = k, summed from 0 in x_t order;
                  // then the 1/sqrt2 factors (u first), /4, quantisation, clip
      const int v = k;
      double in[8];
#pragma unroll
      for (int xt = 0; xt < 8; xt++) in[xt] = s_inner[lb * SAMP_INNER + v * 8 + xt];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        double freq = 0.0;
#pragma unroll
        for (int xt = 0; xt < 8; xt++) freq = __dadd_rn(freq, __dmul_rn(in[xt], s_cos[xt * 8 + u]));
        if (u == 0) freq = __dmul_rn(freq, SAMP_SQRT1_2);
        if (v == 0) freq = __dmul_rn(freq, SAMP_SQRT1_2);
        freq = __dmul_rn(freq, 0.25);
        int o = (int)__ddiv_rn(freq, s_q[c ? 1 : 0][v * 8 + u]);
        o = o < -2048 ? -2048 : (o > 2047 ? 2047 : o);
        s_out[lb * 64 + s_izz[v * 8 + u]] = (int16_t)o;
      }
    }
    samp_wave_sync();
    if (valid) {  // whole 16-byte lines: lane k stores coefficients 8k .. 8k + 7 of its block
      const long long blk = (long long)gby * F.bw[c] + gbx;
      *(uint4 *)(F.plane[c] + blk * 64 + k * 8) = *(const uint4 *)&s_out[lb * 64 + k * 8];
      if (k == 0) F.abs[c][blk] = s_out[lb * 64];
    }
  }
}

hipError_t launch_samp_dct(const SampArgs &a, int nframes, int max_tiles, hipStream_t s) {
  hipLaunchKernelGGL(k_samp_dct, dim3((unsigned)max_tiles, (unsigned)nframes), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace mij
