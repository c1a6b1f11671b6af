// mij_ijg.hip -- gfx950 front end of encoding as libjpeg does (DESIGN.md
// §4n): padded B, G, R slots -> quantised coefficient planes at 4:2:0, 4:2:2,
// 4:4:4 or greyscale, in the layout the transcoder's entropy coder takes
// (TcComp, mij_transcode.h).  It sits where k_samp_dct sits.
//
//   k_ijg_fdct   libjpeg's fixed-point colour conversion, its h2v1 / h2v2
//                downsampling, the "islow" forward DCT, the quantiser that
//                rounds the magnitude, zigzag; planes and absolute DCs, the
//                dummy blocks of the MCU padding included
//
// All of it is int32 arithmetic from mij_ijg_math.h, which tests/
// ijg_check.cpp runs on the host.  A workgroup takes a SAMP_TW x SAMP_TH
// pixel tile, eight lanes take a block: a lane holds a whole row (pass 1) and
// then a whole column (pass 2) in registers.
#include "mij_ijg.h"
#include "mij_pixels.h"

namespace mij {

namespace {

// ints between the row-pass results of two blocks: 64 + 8, so that the column
// reads of a 32-lane half (four blocks, eight columns each, one row) fall on
// 32 different banks
constexpr int IJG_INNER = 72;
constexpr int IJG_LINES = SAMP_TW * 3 / 16;  // 16-byte lines per tile row

struct IjgIzz {
  uint8_t v[64];
};
constexpr IjgIzz ijg_izz() {  // zigzag index of natural position n
  constexpr uint8_t zz[64] = MIJ_ZIGZAG;
  IjgIzz r = {};
  for (int z = 0; z < 64; z++) r.v[zz[z]] = (uint8_t)z;
  return r;
}
__constant__ IjgIzz c_ijg_izz = ijg_izz();

// LDS written by some lanes of a wave, read by others of the same wave
__device__ __forceinline__ void ijg_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// eight B, G, R pixels of a tile row, 24 bytes from an 8-byte aligned address
struct Px8 {
  uint32_t w[6];
  __device__ __forceinline__ int32_t byte(int i) const { return (int32_t)((w[i >> 2] >> (8 * (i & 3))) & 255u); }
  __device__ __forceinline__ int32_t b(int j) const { return byte(3 * j); }
  __device__ __forceinline__ int32_t g(int j) const { return byte(3 * j + 1); }
  __device__ __forceinline__ int32_t r(int j) const { return byte(3 * j + 2); }
};
__device__ __forceinline__ Px8 load_px8(const uint8_t *p) {
  const uint2 a = *(const uint2 *)p, b = *(const uint2 *)(p + 8), c = *(const uint2 *)(p + 16);
  return Px8{{a.x, a.y, b.x, b.y, c.x, c.y}};
}

}  // namespace

// grid (tiles of the largest frame, frames); 256 threads
__global__ __launch_bounds__(256) void k_ijg_fdct(IjgArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[SAMP_TH][SAMP_TW * 3];
  // sample planes, one 64-byte block after another, a block row-major (byte
  // yt * 8 + xt): blocks 0..31 luma (by * 16 + bx), then Cb, then Cr
  __shared__ __attribute__((aligned(16))) uint8_t s_smp[96 * 64];
  __shared__ __attribute__((aligned(16))) int32_t s_inner[32 * IJG_INNER];  // per block [yt][u]
  __shared__ __attribute__((aligned(16))) int16_t s_out[32 * 64];           // per block, zigzag
  __shared__ IjgQ s_q[2][64];  // natural order
  __shared__ uint8_t s_izz[64];
  __shared__ int16_t s_dc[32];  // the tile's luma DCs, for its dummy blocks
  const int tid = threadIdx.x, f = blockIdx.y;
  const IjgFrame &F = a.fr[f];
  if ((int)blockIdx.x >= F.s.ntiles) return;
  const int ty = blockIdx.x / F.s.tiles_x, tx = blockIdx.x - ty * F.s.tiles_x;
  if (tid < 64) s_izz[tid] = c_ijg_izz.v[tid];
  if (tid < 128) s_q[tid >> 6][tid & 63] = a.qt->q[tid >> 6][tid & 63];
  // the tile's rows, as 16-byte lines; lines past the padded frame stay zero
  {
    const uint8_t *slot = a.in + (long long)f * a.in_fs;
    for (int i = tid; i < SAMP_TH * IJG_LINES; i += 256) {
      const int row = i / IJG_LINES, l = i - row * IJG_LINES;
      const int y = ty * SAMP_TH + row, xb = tx * SAMP_TW * 3 + 16 * l;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (y < F.s.h16 && xb + 16 <= F.s.w16 * 3) v = *(const uint4 *)(slot + (long long)y * a.pitch + xb);
      *(uint4 *)&s_raw[row][16 * l] = v;
    }
  }
  __syncthreads();
  const bool grey = a.sampling == 3, s444 = a.sampling == 2, s422 = a.sampling == 1, s420 = a.sampling == 0;
  // colour: a thread takes eight pixels of a row, one block's row
  {
    const int row = tid >> 4, xb = tid & 15;
    const Px8 P = load_px8(&s_raw[row][xb * 24]);
    uint32_t yv[2] = {0u, 0u}, bv[2] = {0u, 0u}, rv[2] = {0u, 0u};
    uint32_t cb[8], cr[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      yv[j >> 2] |= ijg_y(P.r(j), P.g(j), P.b(j)) << (8 * (j & 3));
      if (s444 || s422) {
        cb[j] = ijg_cb(P.r(j), P.g(j), P.b(j));
        cr[j] = ijg_cr(P.r(j), P.g(j), P.b(j));
      }
    }
    const int o = ((row >> 3) * 16 + xb) * 64 + (row & 7) * 8;
    *(uint2 *)&s_smp[o] = make_uint2(yv[0], yv[1]);
    if (s444) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        bv[j >> 2] |= cb[j] << (8 * (j & 3));
        rv[j >> 2] |= cr[j] << (8 * (j & 3));
      }
      *(uint2 *)&s_smp[32 * 64 + o] = make_uint2(bv[0], bv[1]);
      *(uint2 *)&s_smp[64 * 64 + o] = make_uint2(rv[0], rv[1]);
    } else if (s422) {  // output columns xb * 4 + j: the bias follows j
#pragma unroll
      for (int j = 0; j < 4; j++) {
        bv[0] |= ijg_h2v1(cb[2 * j], cb[2 * j + 1], j) << (8 * j);
        rv[0] |= ijg_h2v1(cr[2 * j], cr[2 * j + 1], j) << (8 * j);
      }
      const int oc = ((row >> 3) * 8 + (xb >> 1)) * 64 + (row & 7) * 8 + (xb & 1) * 4;
      *(uint32_t *)&s_smp[32 * 64 + oc] = bv[0];
      *(uint32_t *)&s_smp[48 * 64 + oc] = rv[0];
    }
  }
  if (s420) {
    // waves 0, 1: Cb, waves 2, 3: Cr; a thread takes four samples of a chroma
    // row.  Below the frame's last chroma row that row is repeated (libjpeg
    // replicates sample rows there, not pixel rows): it lies in this tile
    const int plane = tid >> 7, r = (tid >> 4) & 7, g = tid & 15;
    const int last = ((F.h + 1) >> 1) - 1 - ty * 8;
    const int rs = r < last ? r : last;
    const Px8 P0 = load_px8(&s_raw[2 * rs][g * 24]), P1 = load_px8(&s_raw[2 * rs + 1][g * 24]);
    uint32_t v = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t sum;
      if (plane)
        sum = ijg_cr(P0.r(2 * j), P0.g(2 * j), P0.b(2 * j)) + ijg_cr(P0.r(2 * j + 1), P0.g(2 * j + 1), P0.b(2 * j + 1)) +
              ijg_cr(P1.r(2 * j), P1.g(2 * j), P1.b(2 * j)) + ijg_cr(P1.r(2 * j + 1), P1.g(2 * j + 1), P1.b(2 * j + 1));
      else
        sum = ijg_cb(P0.r(2 * j), P0.g(2 * j), P0.b(2 * j)) + ijg_cb(P0.r(2 * j + 1), P0.g(2 * j + 1), P0.b(2 * j + 1)) +
              ijg_cb(P1.r(2 * j), P1.g(2 * j), P1.b(2 * j)) + ijg_cb(P1.r(2 * j + 1), P1.g(2 * j + 1), P1.b(2 * j + 1));
      v |= ijg_h2v2(sum, j) << (8 * j);
    }
    *(uint32_t *)&s_smp[(32 + plane * 8 + (g >> 1)) * 64 + r * 8 + (g & 1) * 4] = v;
  }
  __syncthreads();
  // 32 blocks per pass, eight lanes a block: the eight are lanes of one wave
  // and s_inner / s_out are the block's own, so inside a pass what one lane
  // writes only lanes of its wave read, and a wave-level barrier orders it
  const int nc = grey ? 0 : s420 ? 8 : s422 ? 16 : 32;  // chroma blocks per plane and tile
  const int nblocks = 32 + 2 * nc, npass = (nblocks + 31) / 32;
  const int lb = tid >> 3, k = tid & 7;
  for (int p = 0; p < npass; p++) {
    const int j = p * 32 + lb;
    int c = 0, by = (j >> 4) & 1, bx = j & 15, tbw = 16, tbh = 2;
    if (j >= 32) {
      const int jj = j - 32, r = jj >= nc ? jj - nc : jj;
      c = jj >= nc ? 2 : 1;
      tbw = s420 ? 8 : nc >> 1;
      tbh = s420 ? 1 : 2;
      by = r / tbw;
      bx = r - by * tbw;
    }
    const int gbx = tx * tbw + bx, gby = ty * tbh + by;
    const bool real = j < nblocks && gbx < F.rbw[c] && gby < F.rbh[c];
    if (real) {  // row pass: lane = row yt = k
      const uint2 sv = *(const uint2 *)&s_smp[j * 64 + k * 8];
      int32_t d[8];
#pragma unroll
      for (int xt = 0; xt < 8; xt++) d[xt] = (int32_t)(((xt < 4 ? sv.x : sv.y) >> (8 * (xt & 3))) & 255u) - 128;
      ijg_fdct_pass<true>(d);
      *(int4 *)&s_inner[lb * IJG_INNER + k * 8] = make_int4(d[0], d[1], d[2], d[3]);
      *(int4 *)&s_inner[lb * IJG_INNER + k * 8 + 4] = make_int4(d[4], d[5], d[6], d[7]);
    }
    ijg_wave_sync();
    if (real) {  // column pass: lane = horizontal frequency u = k; then quantisation
      int32_t d[8];
#pragma unroll
      for (int yt = 0; yt < 8; yt++) d[yt] = s_inner[lb * IJG_INNER + yt * 8 + k];
      ijg_fdct_pass<false>(d);
#pragma unroll
      for (int v = 0; v < 8; v++)
        s_out[lb * 64 + s_izz[v * 8 + k]] = (int16_t)ijg_quant(d[v], s_q[c ? 1 : 0][v * 8 + k]);
    }
    ijg_wave_sync();
    if (real) {  // whole 16-byte lines: lane k stores coefficients 8k .. 8k + 7 of its block
      const long long blk = (long long)gby * F.s.bw[c] + gbx;
      *(uint4 *)(F.s.plane[c] + blk * 64 + k * 8) = *(const uint4 *)&s_out[lb * 64 + k * 8];
      if (k == 0) {
        F.s.abs[c][blk] = s_out[lb * 64];
        if (p == 0) s_dc[lb] = s_out[lb * 64];
      }
    }
    if (p == 0 && a.sampling <= 1) {
      // dummy blocks (luma only, one column and one row at the most): no AC,
      // the DC of the block before them in the MCU, which is in this tile
      __syncthreads();
      if (!real && gbx < F.s.bw[0] && gby < F.s.bh[0]) {
        int donor;
        if (gby < F.rbh[0]) {
          donor = by * 16 + bx - 1;
        } else {  // the MCU's last block in the row above, or the block left of that dummy
          const int lastreal = F.rbw[0] - 1 - tx * 16;
          donor = (bx | 1) < lastreal ? (bx | 1) : lastreal;
        }
        const int16_t dc = s_dc[donor];
        const long long blk = (long long)gby * F.s.bw[0] + gbx;
        *(uint4 *)(F.s.plane[0] + blk * 64 + k * 8) = make_uint4(k == 0 ? (uint32_t)(uint16_t)dc : 0u, 0u, 0u, 0u);
        if (k == 0) F.s.abs[0][blk] = dc;
      }
    }
  }
}

hipError_t launch_ijg_fdct(const IjgArgs &a, int nframes, int max_tiles, hipStream_t s) {
  hipLaunchKernelGGL(k_ijg_fdct, dim3((unsigned)max_tiles, (unsigned)nframes), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace mij
