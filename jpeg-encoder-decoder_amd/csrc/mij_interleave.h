// mij_interleave.h -- the interleaved output format: what
// mij_interleave.hip (kernels) and mij_api.hip (host) share.  Not public.
#pragma once
#include "mij_internal.h"

namespace mij {

// entropy bytes per stuffing chunk: 256 threads x 16 bytes (one uint4 of scan words each)
constexpr int IL_CH = 4096;

// Per-frame arrays are laid out for the canvas (Geom g): block and MCU arrays
// nblk / nC apart, row arrays il_rows(g) + 1 apart, chunk arrays il_chunks(g).
__host__ __device__ inline int il_rows(const Geom &g) { return g.h >> 4; }
__host__ __device__ inline long long il_chunks(const Geom &g) { return (g.raw_fs * 4 + IL_CH - 1) / IL_CH; }

struct IlArgs {
  Geom g;
  int nframes;
  int restart_rows;         // MCU rows per restart interval, 0: none
  const int2 *pdims;        // per frame: the padded size K1 encoded (multiples of 16)
  const int2 *tdims;        // per frame: the true size (SOF0)
  const int16_t *coef;      // K1's planes: per frame Y[nY*64] Cb[nC*64] Cr[nC*64], zigzag
  const int16_t *dc;        // raw DC per block, plane order
  uint32_t *hist;           // per frame [4][257]: DC-Y, AC-Y, DC-C, AC-C
  const uint32_t *ehuf;     // per frame [4][256] = len << 16 | code
  const HuffCode *hc;       // per frame [4]
  const Tables *tab;
  uint16_t *blk_bits;       // per block in MCU order (MCU m, block k: m * 6 + k)
  uint32_t *mcu_off;        // per MCU: its bit offset inside its MCU row
  uint32_t *row_bits;       // per MCU row
  unsigned long long *row_pre;        // per MCU row: bits of the rows before it, unpadded; [rows] = all
  unsigned long long *ival_off;       // per interval: its first bit in the entropy data; [nint] = all
  unsigned long long *row_off;        // per MCU row: its first bit in the entropy data; [rows] = all
  uint32_t *raw;            // per frame g.raw_fs big-endian words: the unstuffed entropy data
  uint32_t *ffc;            // per IL_CH chunk: its 0xFF bytes, then those of the chunks before it
  int *hdr;                 // per frame: bytes before the entropy data
  uint8_t *out;             // per frame g.out_cap bytes
  uint64_t *out_len;
  int *err;
};

struct IlPadArgs {
  uint8_t *dst;             // slot 0 of the launch
  long long slot_bytes;
  int pitch;                // canvas row pitch (multiple of 16)
  const uint8_t *src;       // frame 0 of the launch, any alignment
  long long src_fs;         // bytes between source frames
  long long src_pitch;
  const int2 *tdims;        // per slot true size
  int swap;                 // source in R, G, B order: written as B, G, R
  int cw, ch;               // canvas
};

hipError_t launch_il_pad(const IlPadArgs &a, int n, hipStream_t s);
hipError_t launch_il_hist(const IlArgs &a, hipStream_t s);
// after the tables: bits, offsets, packing, stuffed write
hipError_t launch_il_entropy(const IlArgs &a, hipStream_t s);

}  // namespace mij
