// mij_decode.hip -- baseline JPEG decoder: streams -> quantized coefficient
// planes -> pixels on the GPU (the reference has no
// decoder, func_tester.c:1262-1309 checks its output with libjpeg).
//
// Scope: baseline sequential DCT (SOF0, 8-bit, Huffman) in two shapes.
// (a) The streams this library and the reference write (encoder.c:549-644):
// 3 components Y 2x2 / Cb 1x1 / Cr 1x1, three non-interleaved scans, no
// restart markers, sizes multiples of 16.  Their output is the encoder's own
// coefficient layout (encoder.c:158-178): per component, blocks in raster
// order, 64 zigzag-ordered coefficients per block, the DC as the coded
// difference -- so decode(encode(x)) can be compared bit-exactly with
// rgb_to_dct(x) at any size.  (b) What libjpeg, cameras and browsers write:
// one interleaved scan (a greyscale file's single scan included), greyscale
// or YCbCr with luma 1x1 / 2x1 / 2x2 and chroma 1x1, any size from 1x1,
// arbitrary component ids, DQT ids 0..3, restart intervals.  Their planes are
// padded to whole MCUs and live in an arena of their own (k_il_* kernels;
// DESIGN.md "Decoding ordinary baseline files").  Refused with MIJ_EJPEG and
// the reason: SOF1..15, 12-bit samples, 16-bit DQT, 2 or 4 components, Adobe
// RGB / YCCK, other sampling, further scans, Ss/Se/AhAl other than 0/63/0,
// missing tables, restart markers missing or out of order.
//
// Host: marker parsing (SOI, APPn, DQT, DHT, DRI, SOF0, SOS, EOI), canonical
// Huffman tables with a 9-bit lookahead, and the scans copied unstuffed
// into one pinned staging blob.  Device: every scan is cut into 512-bit
// chunks, one lane per chunk.  Entropy decoding is sequential by
// construction, so the chunks' entry states (bit position, coefficient
// index) are found by self-synchronisation: each chunk first decodes from
// its own first bit as if a block began there, then repeatedly from the
// exit state of its predecessor until no entry changes (2-3 passes).  A
// per-scan prefix sum of the blocks each chunk starts gives every chunk its
// output block, and a final pass writes the nonzero coefficients into the
// zeroed planes.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "mij_host.h"
#include "mij_pixels.h"
#include "mij_transcode.h"
#include "mij_transform.h"

#define HIP_TRY(x)                                                                 \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess)                                                          \
      return mij_fail(MIJ_EHIP, "%s failed: %s", #x, hipGetErrorString(e_));       \
  } while (0)

namespace mij {

constexpr int LOOK = 9;

// One canonical Huffman table (ISO/IEC 10918-1 F.2.2.3 decoding procedure).
struct DecTab {
  uint16_t look[1 << LOOK];  // (length << 8) | symbol, 0 = longer than LOOK
  int32_t maxcode[18];       // largest code of each length, -1 if none
  int32_t valoff[17];        // index of the first symbol of a length - its code
  uint8_t val[256];
};

struct DecJob {
  long long data;   // byte offset of the UNSTUFFED scan in the blob (8-aligned)
  long long nbits;  // its length in bits (the pad bits included)
  long long out;    // first int16 of the component's plane
  int nblocks;
  int dc, ac;       // table indices
  int chunk0, nchunks;  // global ids of the scan's chunks
};

// chunk c of a scan covers bits [c*CHUNK, (c+1)*CHUNK): a symbol belongs to
// the chunk its first bit lies in.  512: measured against 1024 / 2048 / 4096
// on 256 config-3 streams, 16.3 / 17.7 / 21.1 / 23.9 ms per decode call.
constexpr int CHUNK = 512;

// MSB-first bit window over an unstuffed, 8-byte aligned, zero-padded scan
struct Bits {
  const unsigned long long *w;
  long long cw = -2;  // index of the word pair held (none yet)
  unsigned long long hi = 0, lo = 0;
  __device__ unsigned long long window(long long pos) {
    const long long i = pos >> 6;
    if (i != cw) {
      if (i == cw + 1) {
        hi = lo;
        lo = __builtin_bswap64(w[i + 1]);
      } else {
        hi = __builtin_bswap64(w[i]);
        lo = __builtin_bswap64(w[i + 1]);
      }
      cw = i;
    }
    const int sh = pos & 63;
    return sh ? (hi << sh) | (lo >> (64 - sh)) : hi;
  }
};

// one symbol (+ its magnitude bits) at pos; returns bits consumed, or 0 on
// an invalid code.  F.2.2.3 DECODE with a LOOK-bit table, F.2.2.1 EXTEND
__device__ __forceinline__ int decode_one(Bits &br, long long pos, const DecTab &t, int &sym, int &val) {
  const unsigned long long win = br.window(pos);
  int len;
  const uint32_t e = t.look[win >> (64 - LOOK)];
  if (e) {
    len = e >> 8;
    sym = e & 255;
  } else {
    len = 0;
    for (int l = LOOK + 1; l <= 16; l++) {
      const int32_t code = (int32_t)(win >> (64 - l));
      if (code <= t.maxcode[l]) {
        len = l;
        sym = t.val[t.valoff[l] + code];
        break;
      }
    }
    if (!len) return 0;
  }
  const int s = sym & 15;
  if (s) {
    // magnitude bits follow the code; the window holds >= 64 - 16 bits
    const int v = (int)((win << len) >> (64 - s));
    val = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;  // negatives are ~|v| (encoder.c:442-444)
  } else {
    val = 0;
  }
  return len + s;
}

// Decodes from (pos, k) until pos reaches `stop` or `blocks_left` blocks
// have ended.  k = next coefficient index (0 = a DC symbol is next).
// Returns the number of blocks started; pos/k are the state after the last
// symbol.  WRITE: coefficients go to out[64*blk + zigzag index] (nonzeros
// only; the planes are zeroed first).  *bad = invalid code met.
template <bool WRITE>
__device__ int decode_span(Bits &br, long long &pos, int &k, long long stop, const DecTab &dc,
                           const DecTab &ac, int16_t *out, long long blk, long long blocks_left,
                           bool *bad) {
  int started = 0;
  *bad = false;
  while (pos < stop) {
    int sym, val;
    if (k == 0) {
      if (blocks_left <= 0) break;
      const int n = decode_one(br, pos, dc, sym, val);
      if (!n || sym > 15) {
        *bad = true;
        break;
      }
      pos += n;
      if (WRITE && val) out[64 * blk] = (int16_t)val;
      started++;
      k = 1;
    } else {
      const int n = decode_one(br, pos, ac, sym, val);
      if (!n) {
        *bad = true;
        break;
      }
      pos += n;
      const int r = sym >> 4;
      if (sym & 15) {
        k += r;
        if (k > 63) {
          *bad = true;
          break;
        }
        if (WRITE) out[64 * blk + k] = (int16_t)val;
        k++;
      } else if (r == 15) {
        k += 16;  // ZRL
      } else {
        k = 64;   // EOB
      }
    }
    if (k >= 64) {
      k = 0;
      blk++;
      blocks_left--;
    }
  }
  return started;
}

__device__ __forceinline__ int job_of(const DecJob *jobs, int njobs, int c) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].chunk0 <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Self-synchronising pass (Weissenberger & Schmidt, ICPP 2018): chunk c
// decodes from its entry state to its end.  First pass: every chunk starts
// at its first bit as if a block began there (exact for chunk 0 of a
// scan).  Later passes: the entry of chunk c is the exit of chunk c-1 from
// the previous pass; a chunk whose entry did not change keeps its result.
// Huffman streams resynchronise within a few symbols, so 2-3 passes settle.
struct SyncArgs {
  const uint8_t *blob;
  const DecJob *jobs;
  int njobs, nchunks;
  const DecTab *tabs;
  long long *entry_pos, *exit_in, *exit_out;  // pos * 64 + k packed
  int *nblk;
  int *changed;
  int first;
};

__device__ __forceinline__ long long pack_state(long long pos, int k) { return pos * 64 + k; }

__global__ __launch_bounds__(256) void k_dec_sync(SyncArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.nchunks) return;
  const DecJob &job = a.jobs[job_of(a.jobs, a.njobs, c)];
  const int lc = c - job.chunk0;
  long long entry;
  if (a.first || lc == 0) {
    entry = pack_state((long long)lc * CHUNK, 0);
    if (!a.first) {
      a.exit_out[c] = a.exit_in[c];
      return;
    }
  } else {
    entry = a.exit_in[c - 1];
    if (entry < 0) entry = pack_state((long long)lc * CHUNK, 0);  // predecessor met a bad code
    if (entry == a.entry_pos[c]) {
      a.exit_out[c] = a.exit_in[c];
      return;
    }
    *a.changed = 1;
  }
  a.entry_pos[c] = entry;
  Bits br{(const unsigned long long *)(a.blob + job.data)};
  long long pos = entry >> 6;
  int k = (int)(entry & 63);
  const long long stop = min((long long)(lc + 1) * CHUNK, job.nbits);
  bool bad;
  const int n = decode_span<false>(br, pos, k, stop, a.tabs[job.dc], a.tabs[job.ac], nullptr, 0,
                                   (long long)job.nblocks, &bad);
  a.nblk[c] = n;
  a.exit_out[c] = bad ? -1 : pack_state(pos, k);
}

// per scan: exclusive scan of the chunks' block counts (one workgroup per
// scan, sequential over 256-chunk tiles) and the total check
__global__ __launch_bounds__(256) void k_dec_scan(const DecJob *jobs, const int *nblk, long long *base,
                                                  int *status) {
  __shared__ long long part[256];
  const DecJob job = jobs[blockIdx.x];
  long long carry = 0;
  for (int t0 = 0; t0 < job.nchunks; t0 += 256) {
    const int t = t0 + threadIdx.x;
    const long long v = t < job.nchunks ? nblk[job.chunk0 + t] : 0;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const long long add = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    if (t < job.nchunks) base[job.chunk0 + t] = carry + part[threadIdx.x] - v;
    const long long tot = part[255];
    __syncthreads();
    carry += tot;
  }
  // a chunk that decodes the last block may go on through the pad bits
  // (and count garbage blocks there); fewer blocks than the frame needs is
  // a truncated stream
  if (threadIdx.x == 0) status[blockIdx.x] = carry >= job.nblocks ? 0 : 5;
}

// final pass: every chunk decodes from its settled entry and writes.  A
// lane assembles each block in its own LDS slot (128 B) and stores it whole
// (8 x 16 B, zeros included: no memset of the planes).  A block split
// between two chunks is stored in halves with 2-byte stores: the lane that
// started it writes positions [first, k_exit), the next lane [k_entry, 64)
// -- the settled states make k_exit == k_entry.
__global__ __launch_bounds__(256) void k_dec_write(SyncArgs a, const long long *base, int16_t *coefs,
                                                   int *status) {
  __shared__ int4 slot[256][8];
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.nchunks) return;
  const int j = job_of(a.jobs, a.njobs, c);
  const DecJob &job = a.jobs[j];
  const int lc = c - job.chunk0;
  const long long entry = a.entry_pos[c];
  long long pos = entry >> 6;
  int k = (int)(entry & 63);
  // the block in progress at the entry was started by an earlier chunk
  long long blk = base[c] - (k ? 1 : 0);
  if (blk >= job.nblocks) return;  // pad bits after the last block
  Bits br{(const unsigned long long *)(a.blob + job.data)};
  const long long stop = min((long long)(lc + 1) * CHUNK, job.nbits);
  const DecTab &dc = a.tabs[job.dc], &ac = a.tabs[job.ac];
  int4 *sl = slot[threadIdx.x];
  int16_t *b16 = (int16_t *)sl;
  int16_t *out = coefs + job.out;
#pragma unroll
  for (int q = 0; q < 8; q++) sl[q] = int4{0, 0, 0, 0};
  int first = k;
  bool bad = false;
  while (pos < stop && blk < job.nblocks) {
    int sym, val;
    const int n = decode_one(br, pos, k ? ac : dc, sym, val);
    if (!n) {
      bad = true;
      break;
    }
    pos += n;
    if (k == 0) {
      if (sym > 15) {
        bad = true;
        break;
      }
      b16[0] = (int16_t)val;
      k = 1;
    } else {
      const int r = sym >> 4;
      if (sym & 15) {
        k += r;
        if (k > 63) {
          bad = true;
          break;
        }
        b16[k++] = (int16_t)val;
      } else {
        k = r == 15 ? k + 16 : 64;  // ZRL / EOB
      }
    }
    if (k >= 64) {  // block complete: store it, clear the slot
      int16_t *o = out + 64 * blk;
      if (first == 0) {
#pragma unroll
        for (int q = 0; q < 8; q++) ((int4 *)o)[q] = sl[q];
      } else {
        for (int t = first; t < 64; t++) o[t] = b16[t];
      }
#pragma unroll
      for (int q = 0; q < 8; q++) sl[q] = int4{0, 0, 0, 0};
      first = 0;
      k = 0;
      blk++;
    }
  }
  if (!bad && k && blk < job.nblocks) {  // block continues in the next chunk
    int16_t *o = out + 64 * blk;
    for (int t = first; t < k; t++) o[t] = b16[t];
  }
  if (bad) atomicMax(&status[j], 6);
}

// ---------------------------------------------------------------------------
// Pixels (DESIGN.md "Decode to pixels"): libjpeg's "islow" IDCT, h2v2 "fancy"
// upsampling and fixed-point colour conversion, integer only, in two passes
// through uint8 planes: k_dec_dc + k_dec_dcbase (absolute DCs), k_dec_idct
// (coefficients -> Y / Cb / Cr samples), k_dec_colour (samples -> packed
// 3-byte pixels).  The arithmetic itself is mij_pixels.h.
// The IDCT's sums run in uint32_t: streams no 8-bit image produces wrap
// instead of overflowing a signed type; encoder-made streams never wrap.
// ---------------------------------------------------------------------------
struct RecJob {     // one component of one frame
  long long off;    // first int16 of its coefficient plane == first byte of its sample plane
  int nblocks, bw;  // 8x8 blocks, and blocks per row
  int wg0;          // its first workgroup in k_dec_idct's grid
  int qt;           // its quantiser: 64 ints (zigzag order) at q + 64 * qt
  int tile0;        // its first workgroup in k_dec_dc's grid == its first entry of the tile bases
  int pad;
};

struct RecFrame {
  long long planes;  // first byte of the Y plane; Cb at + w*h, Cr at + w*h*5/4
  long long pix;     // first byte of the pixels, rows 3*w bytes apart
  int w, h;
  int wg0;           // its first workgroup in k_dec_colour's grid
  int pad;
};

// Absolute DCs in two levels.  A plane's blocks are cut into tiles of
// DC_TILE; k_dec_dc, one 1024-lane workgroup per tile (so luma and chroma
// planes load the chip alike), writes every block's DC relative to its tile
// (each lane DC_PER consecutive blocks, a shuffle scan per wave, the waves'
// totals through LDS) to dc[off / 64 + block] and the tile's total to
// tile[blockIdx.x]; k_dec_dcbase, one lane per plane, turns the totals into
// each tile's base.  k_dec_idct adds the two.  All sums modulo 2^32.
constexpr int DC_T = 1024, DC_PER = 8, DC_TILE = DC_T * DC_PER;

template <class J>
__device__ __forceinline__ int rec_tile_job(const J *jobs, int njobs, int tile) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].tile0 <= tile) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(DC_T) void k_dec_dc(const RecJob *jobs, int njobs, const int16_t *coefs, int32_t *dc,
                                                 uint32_t *tile) {
  __shared__ uint32_t wsum[DC_T / 64];
  const RecJob job = jobs[rec_tile_job(jobs, njobs, blockIdx.x)];
  const int16_t *src = coefs + job.off;
  int32_t *dst = dc + job.off / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b0 = ((int)blockIdx.x - job.tile0) * DC_TILE + (int)threadIdx.x * DC_PER;
  uint32_t v[DC_PER], s = 0;
#pragma unroll
  for (int i = 0; i < DC_PER; i++) {
    if (b0 + i < job.nblocks) s += (uint32_t)(int32_t)src[64LL * (b0 + i)];
    v[i] = s;
  }
  uint32_t x = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  uint32_t base = x - s, tot = 0;
#pragma unroll
  for (int k = 0; k < DC_T / 64; k++) {
    const uint32_t t = wsum[k];
    if (k < wave) base += t;
    tot += t;
  }
#pragma unroll
  for (int i = 0; i < DC_PER; i++)
    if (b0 + i < job.nblocks) dst[b0 + i] = (int32_t)(base + v[i]);
  if (threadIdx.x == 0) tile[blockIdx.x] = tot;
}

// tile totals -> exclusive prefix within each plane (a 3840x2160 luma plane
// has 16 tiles)
template <class J>
__global__ __launch_bounds__(64) void k_dec_dcbase(const J *jobs, int njobs, uint32_t *tile) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= njobs) return;
  const int t0 = jobs[j].tile0, nt = (jobs[j].nblocks + DC_TILE - 1) / DC_TILE;
  uint32_t run = 0;
  for (int t = 0; t < nt; t++) {
    const uint32_t v = tile[t0 + t];
    tile[t0 + t] = run;
    run += v;
  }
}

template <class J>
__device__ __forceinline__ int rec_job_of(const J *jobs, int njobs, int wg) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].wg0 <= wg) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One lane per 8x8 block, 256 blocks of one component per workgroup.  The
// workgroup's 32 KiB of coefficients come in with coalesced 16-byte loads
// and are staged in LDS, a block's 8 int4 in a slot of 9 (a lane's 16-byte
// reads then fall on distinct bank groups); the lane dequantises into
// natural order (all indices compile-time: registers), runs the column pass
// (descale 11) and the row pass (descale 18), and stores 8 bytes per row.
__global__ __launch_bounds__(256) void k_dec_idct(const RecJob *jobs, int njobs, const int16_t *coefs,
                                                  const int32_t *dc, const uint32_t *tile, const int32_t *q,
                                                  uint8_t *planes) {
  __shared__ int4 stage[256 * 9];
  const RecJob job = jobs[rec_job_of(jobs, njobs, blockIdx.x)];
  const int first = ((int)blockIdx.x - job.wg0) * 256;
  const int nb = min(256, job.nblocks - first);
  const int4 *src = (const int4 *)(coefs + job.off + 64LL * first);
  for (int i = threadIdx.x; i < nb * 8; i += 256) stage[(i >> 3) * 9 + (i & 7)] = src[i];
  __syncthreads();
  if ((int)threadIdx.x >= nb) return;
  const int blk = first + threadIdx.x;
  union {
    int4 v[8];
    int16_t c[64];
  } in;
#pragma unroll
  for (int k = 0; k < 8; k++) in.v[k] = stage[threadIdx.x * 9 + k];
  uint32_t rows[8][2];
  const uint32_t dc_abs = (uint32_t)dc[job.off / 64 + blk] + tile[job.tile0 + blk / DC_TILE];
  idct_block(in.c, dc_abs, q + 64 * job.qt, rows);
  const int by = blk / job.bw, bx = blk - by * job.bw;
  const long long pitch = 8LL * job.bw;
  uint8_t *dst = planes + job.off + 8LL * by * pitch + 8 * bx;
#pragma unroll
  for (int r = 0; r < 8; r++)  // 8-byte aligned: off % 64 == 0, pitch % 8 == 0
    store_as(dst + r * pitch, W2{rows[r][0], rows[r][1]});
}

template <class F>
__device__ __forceinline__ int rec_frame_of(const F *fr, int n, int wg) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (fr[mid].wg0 <= wg) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One lane per 16 x 2 output pixels (colour_tile, mij_pixels.h), a frame's
// tiles in raster order, 256 per workgroup; no workgroup spans two frames.
__global__ __launch_bounds__(256) void k_dec_colour(const RecFrame *frames, int nframes, const uint8_t *planes,
                                                    uint8_t *pix, int rgb) {
  const RecFrame fr = frames[rec_frame_of(frames, nframes, blockIdx.x)];
  const int groups = fr.w >> 4;
  const int idx = ((int)blockIdx.x - fr.wg0) * 256 + (int)threadIdx.x;
  if (idx >= (fr.h >> 1) * groups) return;
  const int r = idx / groups, g = idx - r * groups;
  const uint8_t *Y = planes + fr.planes;
  const uint8_t *Cb = Y + (long long)fr.w * fr.h, *Cr = Cb + ((long long)fr.w * fr.h >> 2);
  colour_tile(Y, Cb, Cr, fr.w, fr.h, r, g, rgb, pix + fr.pix);
}

// ---------------------------------------------------------------------------
// Interleaved scans (DESIGN.md "Decoding ordinary baseline files"): one scan
// holds MCUs of up to 6 blocks, cut into restart intervals.  An interval is
// what a scan is above: its own zero-padded slot of the blob, its own chunks,
// an exact entry (first bit, k 0, slot 0) for its first chunk.  A chunk's
// state is (bit position, coefficient index k, block slot within the MCU);
// the Huffman tables follow the slot.
//
// Bounds, whatever the bits say.  Reads: a window is taken only at pos <
// stop <= nbits and covers words pos/64 and pos/64 + 1, i.e. at most 15
// bytes past the interval's last byte; every slot ends in >= 16 zero bytes.
// States: k leaves a span in 0..63 (a run past 63 is "bad", ZRL / EOB end
// the block), slot in 0..bpm-1 (only ever stepped modulo bpm), and a state
// is only ever produced by these kernels.  Stores: k_il_write stores block
// b of interval i only while b < nmcus_i * bpm, to MCU mcu0_i + b / bpm <
// the frame's MCU count (the host checks mcu0_i + nmcus_i <= mcus_x *
// mcus_y before any launch), at a position inside that MCU (slot_x < h_c,
// slot_y < v_c), hence inside the component's padded plane; b itself comes
// from the prefix sum and is checked >= 0 and congruent to the entry slot
// first.  A stream that breaks any of this ends in a status code.
// ---------------------------------------------------------------------------
struct IlFrame {
  long long off[3];  // first int16 of each component's padded plane
  int ncomp, bpm;    // blocks per MCU
  int mcus_x, nmcus;
  int chunk0, nchunks;  // all chunks of the frame's intervals, contiguous
  int hs[3], vs[3], bw[3];
  int dc[3], ac[3];  // table indices per component
  int slot_comp[6], slot_x[6], slot_y[6];
};

struct IlJob {          // one restart interval (a whole scan without DRI)
  long long data, nbits;  // as DecJob
  int frame;            // index into the IlFrame table
  int mcu0, nmcus;
  int chunk0, nchunks;
  int pad;
};

struct IlArgs {
  const uint8_t *blob;
  const IlJob *jobs;
  const IlFrame *frames;
  int njobs, nchunks;
  const DecTab *tabs;
  long long *entry_pos, *exit_in, *exit_out;  // (pos * 8 + slot) * 64 + k
  int *nblk;
  int *changed;
  int first;
};

__device__ __forceinline__ long long il_pack(long long pos, int slot, int k) { return (pos * 8 + slot) * 64 + k; }

__device__ __forceinline__ int il_job_of(const IlJob *jobs, int njobs, int c) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].chunk0 <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// k_dec_sync for intervals: the same passes, the state one field wider.  A
// chunk decodes again only when its predecessor's exit state, slot included,
// changed.
__global__ __launch_bounds__(256) void k_il_sync(IlArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.nchunks) return;
  const IlJob &job = a.jobs[il_job_of(a.jobs, a.njobs, c)];
  const int lc = c - job.chunk0;
  long long entry;
  if (a.first || lc == 0) {
    entry = il_pack((long long)lc * CHUNK, 0, 0);
    if (!a.first) {
      a.exit_out[c] = a.exit_in[c];
      return;
    }
  } else {
    entry = a.exit_in[c - 1];
    if (entry < 0) entry = il_pack((long long)lc * CHUNK, 0, 0);  // predecessor met a bad code
    if (entry == a.entry_pos[c]) {
      a.exit_out[c] = a.exit_in[c];
      return;
    }
    *a.changed = 1;
  }
  a.entry_pos[c] = entry;
  const IlFrame &F = a.frames[job.frame];
  Bits br{(const unsigned long long *)(a.blob + job.data)};
  long long pos = entry >> 9;
  int slot = (int)(entry >> 6) & 7, k = (int)(entry & 63);
  const long long stop = min((long long)(lc + 1) * CHUNK, job.nbits);
  long long blocks_left = (long long)job.nmcus * F.bpm;
  int comp = F.slot_comp[slot];
  const DecTab *dc = a.tabs + F.dc[comp], *ac = a.tabs + F.ac[comp];
  int started = 0;
  bool bad = false;
  while (pos < stop) {
    int sym, val;
    if (k == 0) {
      if (blocks_left <= 0) break;
      const int n = decode_one(br, pos, *dc, sym, val);
      if (!n || sym > 15) {
        bad = true;
        break;
      }
      pos += n;
      started++;
      k = 1;
    } else {
      const int n = decode_one(br, pos, *ac, sym, val);
      if (!n) {
        bad = true;
        break;
      }
      pos += n;
      const int r = sym >> 4;
      if (sym & 15) {
        k += r;
        if (k > 63) {
          bad = true;
          break;
        }
        k++;
      } else {
        k = r == 15 ? k + 16 : 64;  // ZRL / EOB
      }
    }
    if (k >= 64) {
      k = 0;
      blocks_left--;
      slot = slot + 1 == F.bpm ? 0 : slot + 1;
      comp = F.slot_comp[slot];
      dc = a.tabs + F.dc[comp];
      ac = a.tabs + F.ac[comp];
    }
  }
  a.nblk[c] = started;
  a.exit_out[c] = bad ? -1 : il_pack(pos, slot, k);
}

// per frame (not per interval: a file may hold thousands of one-MCU
// intervals): exclusive scan of its chunks' block counts across all its
// intervals.  k_il_write takes differences against its interval's first chunk.
__global__ __launch_bounds__(256) void k_il_scan(const IlFrame *frames, const int *nblk, long long *base) {
  __shared__ long long part[256];
  const int chunk0 = frames[blockIdx.x].chunk0, nchunks = frames[blockIdx.x].nchunks;
  long long carry = 0;
  for (int t0 = 0; t0 < nchunks; t0 += 256) {
    const int t = t0 + threadIdx.x;
    const long long v = t < nchunks ? nblk[chunk0 + t] : 0;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const long long add = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    if (t < nchunks) base[chunk0 + t] = carry + part[threadIdx.x] - v;
    const long long tot = part[255];
    __syncthreads();
    carry += tot;
  }
}

// k_dec_write for intervals.  Scan-order block b of the interval lies in MCU
// mcu0 + b / bpm at slot b % bpm; its place is that component's padded plane,
// block row my * v_c + slot_y, block column mx * h_c + slot_x.  status: one
// int per frame; 5 = an interval holds fewer blocks than its MCUs need, 6 =
// invalid code, 7 = the prefix sum and the settled slot disagree.
__global__ __launch_bounds__(256) void k_il_write(IlArgs a, const long long *base, int16_t *coefs, int *status) {
  __shared__ int4 slotbuf[256][8];
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.nchunks) return;
  const IlJob &job = a.jobs[il_job_of(a.jobs, a.njobs, c)];
  const IlFrame &F = a.frames[job.frame];
  const int lc = c - job.chunk0;
  const long long nblocks = (long long)job.nmcus * F.bpm;
  const long long lb = base[c] - base[job.chunk0];  // blocks the interval's earlier chunks started
  if (lc == job.nchunks - 1 && lb + a.nblk[c] < nblocks) atomicMax(&status[job.frame], 5);
  const long long entry = a.entry_pos[c];
  long long pos = entry >> 9;
  int slot = (int)(entry >> 6) & 7, k = (int)(entry & 63);
  // the block in progress at the entry was started by an earlier chunk
  long long blk = lb - (k ? 1 : 0);
  if (blk >= nblocks) return;  // pad bits after the last block
  if (blk < 0 || (int)(blk % F.bpm) != slot) {
    atomicMax(&status[job.frame], 7);
    return;
  }
  int mcu = job.mcu0 + (int)(blk / F.bpm);
  Bits br{(const unsigned long long *)(a.blob + job.data)};
  const long long stop = min((long long)(lc + 1) * CHUNK, job.nbits);
  int4 *sl = slotbuf[threadIdx.x];
  int16_t *b16 = (int16_t *)sl;
#pragma unroll
  for (int q = 0; q < 8; q++) sl[q] = int4{0, 0, 0, 0};
  int first = k;
  bool bad = false;
  while (pos < stop && blk < nblocks) {
    const int comp = F.slot_comp[slot];
    int sym, val;
    const int n = decode_one(br, pos, a.tabs[k ? F.ac[comp] : F.dc[comp]], sym, val);
    if (!n) {
      bad = true;
      break;
    }
    pos += n;
    if (k == 0) {
      if (sym > 15) {
        bad = true;
        break;
      }
      b16[0] = (int16_t)val;
      k = 1;
    } else {
      const int r = sym >> 4;
      if (sym & 15) {
        k += r;
        if (k > 63) {
          bad = true;
          break;
        }
        b16[k++] = (int16_t)val;
      } else {
        k = r == 15 ? k + 16 : 64;  // ZRL / EOB
      }
    }
    if (k >= 64) {  // block complete: store it, clear the slot
      const int my = mcu / F.mcus_x, mx = mcu - my * F.mcus_x;
      int16_t *o = coefs + F.off[comp] +
                   64 * ((long long)(my * F.vs[comp] + F.slot_y[slot]) * F.bw[comp] + mx * F.hs[comp] + F.slot_x[slot]);
      if (first == 0) {
#pragma unroll
        for (int q = 0; q < 8; q++) ((int4 *)o)[q] = sl[q];
      } else {
        for (int t = first; t < 64; t++) o[t] = b16[t];
      }
#pragma unroll
      for (int q = 0; q < 8; q++) sl[q] = int4{0, 0, 0, 0};
      first = 0;
      k = 0;
      blk++;
      if (++slot == F.bpm) {
        slot = 0;
        mcu++;
      }
    }
  }
  if (!bad && k && blk < nblocks) {  // block continues in the next chunk
    const int comp = F.slot_comp[slot];
    const int my = mcu / F.mcus_x, mx = mcu - my * F.mcus_x;
    int16_t *o = coefs + F.off[comp] +
                 64 * ((long long)(my * F.vs[comp] + F.slot_y[slot]) * F.bw[comp] + mx * F.hs[comp] + F.slot_x[slot]);
    for (int t = first; t < k; t++) o[t] = b16[t];
  }
  if (bad) atomicMax(&status[job.frame], 6);
}

// Reconstruction for these frames.  DC prediction runs per component in scan
// order (inside an MCU left-right, top-bottom, then the next MCU) and starts
// again at 0 every restart interval, i.e. every `seg` blocks of the
// component.  k_il_dc is k_dec_dc over scan-order index s instead of raster
// order: dc[off / 64 + s] = the sum of differences 0..s relative to the tile,
// tile totals as before, k_dec_dcbase unchanged.  With P(s) = dc + tile base,
// block s has absolute DC P(s) - P(first block of its segment - 1): two loads
// in k_il_idct, no segmented scan.  All modulo 2^32.
struct IlRec {      // one component of one frame
  long long off;    // as RecJob
  int nblocks, bw;  // padded plane: blocks, and blocks per row (mcus_x * h_c)
  int wg0, qt, tile0;
  int hs, vs, mcus_x;
  int seg;          // blocks between DC resets: Ri * h_c * v_c, nblocks without DRI
  int pad;
};

// scan-order index -> raster index in the padded plane, and back
__device__ __forceinline__ int il_raster(const IlRec &j, int s) {
  const int hv = j.hs * j.vs, m = s / hv, i = s - m * hv;
  const int my = m / j.mcus_x, mx = m - my * j.mcus_x, iy = i / j.hs, ix = i - iy * j.hs;
  return (my * j.vs + iy) * j.bw + mx * j.hs + ix;
}
__device__ __forceinline__ int il_scan_index(const IlRec &j, int blk) {
  const int by = blk / j.bw, bx = blk - by * j.bw;
  const int my = by / j.vs, iy = by - my * j.vs, mx = bx / j.hs, ix = bx - mx * j.hs;
  return (my * j.mcus_x + mx) * (j.hs * j.vs) + iy * j.hs + ix;
}

__global__ __launch_bounds__(DC_T) void k_il_dc(const IlRec *jobs, int njobs, const int16_t *coefs, int32_t *dc,
                                                uint32_t *tile) {
  __shared__ uint32_t wsum[DC_T / 64];
  const IlRec job = jobs[rec_tile_job(jobs, njobs, blockIdx.x)];
  const int16_t *src = coefs + job.off;
  int32_t *dst = dc + job.off / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b0 = ((int)blockIdx.x - job.tile0) * DC_TILE + (int)threadIdx.x * DC_PER;
  uint32_t v[DC_PER], s = 0;
#pragma unroll
  for (int i = 0; i < DC_PER; i++) {
    if (b0 + i < job.nblocks) s += (uint32_t)(int32_t)src[64LL * il_raster(job, b0 + i)];
    v[i] = s;
  }
  uint32_t x = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  uint32_t base = x - s, tot = 0;
#pragma unroll
  for (int k = 0; k < DC_T / 64; k++) {
    const uint32_t t = wsum[k];
    if (k < wave) base += t;
    tot += t;
  }
#pragma unroll
  for (int i = 0; i < DC_PER; i++)
    if (b0 + i < job.nblocks) dst[b0 + i] = (int32_t)(base + v[i]);
  if (threadIdx.x == 0) tile[blockIdx.x] = tot;
}

// k_dec_idct with the component's own quantiser and the DC rule above
__global__ __launch_bounds__(256) void k_il_idct(const IlRec *jobs, int njobs, const int16_t *coefs, const int32_t *dc,
                                                 const uint32_t *tile, const int32_t *q, uint8_t *planes) {
  __shared__ int4 stage[256 * 9];
  const IlRec job = jobs[rec_job_of(jobs, njobs, blockIdx.x)];
  const int first = ((int)blockIdx.x - job.wg0) * 256;
  const int nb = min(256, job.nblocks - first);
  const int4 *src = (const int4 *)(coefs + job.off + 64LL * first);
  for (int i = threadIdx.x; i < nb * 8; i += 256) stage[(i >> 3) * 9 + (i & 7)] = src[i];
  __syncthreads();
  if ((int)threadIdx.x >= nb) return;
  const int blk = first + threadIdx.x;
  union {
    int4 v[8];
    int16_t c[64];
  } in;
#pragma unroll
  for (int k = 0; k < 8; k++) in.v[k] = stage[threadIdx.x * 9 + k];
  const int s = il_scan_index(job, blk), s0 = s / job.seg * job.seg;
  const int32_t *pd = dc + job.off / 64;
  uint32_t dc_abs = (uint32_t)pd[s] + tile[job.tile0 + s / DC_TILE];
  if (s0 > 0) dc_abs -= (uint32_t)pd[s0 - 1] + tile[job.tile0 + (s0 - 1) / DC_TILE];
  uint32_t rows[8][2];
  idct_block(in.c, dc_abs, q + 64 * job.qt, rows);
  const int by = blk / job.bw, bx = blk - by * job.bw;
  const long long pitch = 8LL * job.bw;
  uint8_t *dst = planes + job.off + 8LL * by * pitch + 8 * bx;
#pragma unroll
  for (int r = 0; r < 8; r++) store_as(dst + r * pitch, W2{rows[r][0], rows[r][1]});
}

struct IlPix {
  long long y, cb, cr;  // first byte of each padded sample plane
  long long pix;        // first byte of the pixels, rows G.pitch apart
  PixGeom G;
  int groups, units;    // 16-pixel groups per row; rows or row pairs (colour_tile_any)
  int wg0, pad;
};

__global__ __launch_bounds__(256) void k_il_colour(const IlPix *frames, int nframes, const uint8_t *planes,
                                                   uint8_t *pix, int rgb) {
  const IlPix fr = frames[rec_frame_of(frames, nframes, blockIdx.x)];
  const long long idx = ((long long)blockIdx.x - fr.wg0) * 256 + (int)threadIdx.x;
  if (idx >= (long long)fr.units * fr.groups) return;
  const int u = (int)(idx / fr.groups), g = (int)(idx - (long long)u * fr.groups);
  colour_tile_any(planes + fr.y, planes + fr.cb, planes + fr.cr, fr.G, u, g, rgb, pix + fr.pix);
}

// ---------------------------------------------------------------------------
// Decoding at 1/2, 1/4 and 1/8 scale.  The absolute DCs come
// from the kernels above, unchanged; a component whose blocks become S x S
// samples (mij_pixels.h scaled_geometry) goes through k_sc_idct<S> into a
// plane whose rows are S * bw rounded up to 8 bytes apart, at the place its
// full-size plane would take; k_il_colour then runs on the scaled geometry.
// Frames of the encoder's own shape take the same path as any 4:2:0 frame.
//
// Bounds.  A lane owns strip t < bh * spr of its component: block row by =
// t / spr, blocks bx0 = (8 / S) * sx .. of which only those < bw are read.
// Its S stores of 8 bytes go to rows S * by .. S * by + S - 1 < S * bh at
// byte 8 * sx, and 8 * sx + 8 <= 8 * spr == pitch, so each stays inside its
// row of the plane, which is pitch * S * bh <= 64 * bw * bh bytes: inside the
// slot of the full-size plane.  In LDS a workgroup's block b < nb <= 256
// has its staging slot at 9 * b int4 and its rows at words 256 * r + b,
// r < S <= 4: both inside the 256 * 9 int4.  Nothing is addressed from data.
// ---------------------------------------------------------------------------
struct ScJob {      // one component of one frame
  long long off;    // as RecJob
  int nblocks, bw, bh;
  int wg0, qt, tile0;
  int hs, vs, mcus_x, seg;  // as IlRec (il only)
  int il;           // the DC rule: 1 = k_il_idct's (scan order, segments), 0 = k_dec_idct's (raster)
  int pitch;        // bytes between the scaled plane's rows
  int spr;          // strips of 8 samples per block row: ceil(bw * S / 8)
  int pad;
};

__device__ __forceinline__ uint32_t sc_dc(const ScJob &j, const int32_t *pd, const uint32_t *tile, int blk) {
  if (!j.il) return (uint32_t)pd[blk] + tile[j.tile0 + blk / DC_TILE];
  const int by = blk / j.bw, bx = blk - by * j.bw;
  const int my = by / j.vs, iy = by - my * j.vs, mx = bx / j.hs, ix = bx - mx * j.hs;
  const int s = (my * j.mcus_x + mx) * (j.hs * j.vs) + iy * j.hs + ix, s0 = s / j.seg * j.seg;
  uint32_t v = (uint32_t)pd[s] + tile[j.tile0 + s / DC_TILE];
  if (s0 > 0) v -= (uint32_t)pd[s0 - 1] + tile[j.tile0 + (s0 - 1) / DC_TILE];
  return v;
}

// One lane stores a strip: the 8 / S horizontally adjacent blocks of one
// block row that make 8 output samples, so every row leaves as one aligned
// 8-byte store.  A workgroup takes 256 * S / 8 consecutive strips, i.e. at
// most 256 blocks, consecutive in raster order also where a block row ends
// in a partial strip; all 256 lanes stage their coefficients through LDS as
// k_il_idct does.  For S == 4 and 2 every lane then runs the IDCT of one
// block (so none idles), leaves its S rows in LDS, in the staging area once
// every lane has read its coefficients, and the strip lanes gather them.
// S == 8 is k_il_idct itself with the job's DC rule (4:2:0 chroma at 1/2);
// S == 1 reads the DC buffers alone, 8 blocks per lane.
template <int S>
__global__ __launch_bounds__(256) void k_sc_idct(const ScJob *jobs, int njobs, const int16_t *coefs, const int32_t *dc,
                                                 const uint32_t *tile, const int32_t *q, uint8_t *planes) {
  constexpr int PER = 8 / S, LANES = 256 / PER;
  __shared__ int4 stage[S > 1 ? 256 * 9 : 1];
  const ScJob job = jobs[rec_job_of(jobs, njobs, blockIdx.x)];
  const int nstrips = job.bh * job.spr;
  const int t0 = ((int)blockIdx.x - job.wg0) * LANES, t1 = min(t0 + LANES, nstrips);
  const int by0 = t0 / job.spr, first = by0 * job.bw + (t0 - by0 * job.spr) * PER;
  const int32_t *pd = dc + job.off / 64;
  const int32_t *qz = q + 64 * job.qt;
  int nb = 0;  // the workgroup's blocks: <= 256
  if (S > 1) {
    const int by1 = t1 / job.spr, last = t1 == nstrips ? job.nblocks : by1 * job.bw + (t1 - by1 * job.spr) * PER;
    nb = last - first;
    const int4 *src = (const int4 *)(coefs + job.off + 64LL * first);
    for (int i = threadIdx.x; i < nb * 8; i += 256) stage[(i >> 3) * 9 + (i & 7)] = src[i];
    __syncthreads();
  }
  uint32_t *res = (uint32_t *)stage;  // S == 4, 2: row r of the workgroup's block b at res[256 * r + b]
  if constexpr (S == 4 || S == 2) {
    uint32_t rows[S];
    const bool have = (int)threadIdx.x < nb;
    if (have) {
      union {
        int4 v[8];
        int16_t c[64];
      } in;
#pragma unroll
      for (int j = 0; j < 8; j++) in.v[j] = stage[threadIdx.x * 9 + j];
      const uint32_t dc_abs = sc_dc(job, pd, tile, first + (int)threadIdx.x);
      if constexpr (S == 4) idct4_block(in.c, dc_abs, qz, rows);
      else idct2_block(in.c, dc_abs, qz, rows);
    }
    __syncthreads();  // every lane holds its coefficients in registers: the staging area is free
    if (have) {
#pragma unroll
      for (int r = 0; r < S; r++) res[256 * r + threadIdx.x] = rows[r];
    }
    __syncthreads();
  }
  const int t = t0 + (int)threadIdx.x;
  if ((int)threadIdx.x >= LANES || t >= t1) return;
  const int by = t / job.spr, sx = t - by * job.spr;
  const int blk0 = by * job.bw + sx * PER, nbl = min(PER, job.bw - sx * PER);
  uint32_t out[S][2];
#pragma unroll
  for (int r = 0; r < S; r++) out[r][0] = out[r][1] = 0;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    if (k >= nbl) break;
    const int blk = blk0 + k;
    if constexpr (S == 1) {
      out[0][k >> 2] |= idct1_block(sc_dc(job, pd, tile, blk), qz[0]) << (8 * (k & 3));
    } else if constexpr (S == 8) {
      union {
        int4 v[8];
        int16_t c[64];
      } in;
#pragma unroll
      for (int j = 0; j < 8; j++) in.v[j] = stage[(blk - first) * 9 + j];
      idct_block(in.c, sc_dc(job, pd, tile, blk), qz, out);
    } else if constexpr (S == 4) {
#pragma unroll
      for (int r = 0; r < 4; r++) out[r][k] = res[256 * r + blk - first];
    } else {
#pragma unroll
      for (int r = 0; r < 2; r++) out[r][k >> 1] |= res[256 * r + blk - first] << (16 * (k & 1));
    }
  }
  uint8_t *dst = planes + job.off + (long long)S * by * job.pitch + 8 * sx;
#pragma unroll
  for (int r = 0; r < S; r++)  // 8-byte aligned: off % 64 == 0, pitch % 8 == 0
    store_as(dst + (long long)r * job.pitch, W2{out[r][0], out[r][1]});
}

}  // namespace mij

// ---------------------------------------------------------------------------
// host: JFIF parsing
// ---------------------------------------------------------------------------
namespace {

struct Parsed {
  int w = 0, h = 0;
  int ncomp = 0;
  // components in SOF order; a single component is 1x1 whatever it declares
  int cid[3] = {0, 0, 0}, hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1}, tq[3] = {0, 0, 0};
  uint8_t decl_hv[3] = {0x11, 0x11, 0x11};  // SOF0's H/V bytes as declared (transcoding writes them back)
  int hmax = 1, vmax = 1, mcus_x = 0, mcus_y = 0;
  int bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};  // padded planes, in blocks
  int ri = 0;       // restart interval in MCUs, 0 = none
  int adobe = -1;   // APP14 transform, -1 = no such segment
  bool legacy = false;       // the encoder's shape: three one-component scans, 4:2:0, multiples of 16
  bool interleaved = false;  // one scan holding every component
  uint8_t dqt[4][64];
  bool have_dqt[4] = {false, false, false, false};
  mij::DecTab tab[4];  // DC0, AC0, DC1, AC1: index 2*Th + Tc
  bool have_tab[4] = {false, false, false, false};
  struct Scan {
    int comp, td, ta;
    long long data, end;
  } scan[3];        // legacy: the three scans
  int nscans = 0;
  int comp_seen = 0;  // components that already have a scan (bit c)
  int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};  // interleaved: tables per component
  struct Ivl {
    long long data, end;  // raw bytes of one restart interval
  };
  std::vector<Ivl> ivl;
  char err[200] = "";
  long long units() const {  // int16 coefficients == sample bytes of all padded planes
    long long u = 0;
    for (int c = 0; c < ncomp; c++) u += 64LL * bw[c] * bh[c];
    return u;
  }
  long long pitch() const { return (3LL * w + 15) / 16 * 16; }
};

int be16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

int build_table(mij::DecTab &t, const uint8_t counts[16], const uint8_t *syms, int nsyms) {
  memset(&t, 0, sizeof t);
  memcpy(t.val, syms, nsyms);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; l++) {
    const int c = counts[l - 1];
    t.valoff[l] = k - code;
    t.maxcode[l] = c ? code + c - 1 : -1;
    for (int i = 0; i < c; i++, k++, code++) {
      if (l <= mij::LOOK) {
        const int sh = mij::LOOK - l;
        for (int f = 0; f < (1 << sh); f++) t.look[(code << sh) | f] = (uint16_t)((l << 8) | syms[k]);
      }
    }
    if (code > (1 << l)) return -1;  // over-subscribed
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  return 0;
}

// Host only (no device use): the message goes to P.err, since streams are
// parsed on worker threads; the caller reports it.
int parse(const uint8_t *s, size_t n, Parsed &P, int frame) {
#define BAD(...)                                  \
  do {                                            \
    snprintf(P.err, sizeof P.err, __VA_ARGS__);   \
    return MIJ_EJPEG;                             \
  } while (0)
  if (n < 4 || s[0] != 0xFF || s[1] != 0xD8) BAD("stream %d: no SOI", frame);
  size_t i = 2;
  while (i + 4 <= n) {
    if (s[i] != 0xFF) BAD("stream %d: marker expected at byte %zu", frame, i);
    const int m = s[i + 1];
    if (m == 0xFF) {  // fill byte
      i++;
      continue;
    }
    if (m == 0xD9) break;  // EOI
    if (m >= 0xD0 && m <= 0xD7) BAD("stream %d: restart marker RST%d without a restart interval in force", frame, m - 0xD0);
    const int len = be16(s + i + 2);
    if (len < 2 || i + 2 + len > n) BAD("stream %d: segment 0x%02X length %d", frame, m, len);
    const uint8_t *q = s + i + 4;
    const int body = len - 2;
    if (m == 0xDB) {  // DQT, 8-bit, possibly several tables
      for (int o = 0; o < body; o += 65) {
        const int tq = q[o] & 15;
        if (q[o] >> 4) BAD("stream %d: 16-bit DQT (Pq %d) is not baseline 8-bit", frame, q[o] >> 4);
        if (tq > 3 || o + 65 > body) BAD("stream %d: DQT Tq %d / length", frame, tq);
        memcpy(P.dqt[tq], q + o + 1, 64);
        P.have_dqt[tq] = true;
      }
    } else if (m == 0xC4) {  // DHT, possibly several tables
      int o = 0;
      while (o + 17 <= body) {
        const int tc = q[o] >> 4, th = q[o] & 15;
        if (tc > 1 || th > 1) BAD("stream %d: DHT Tc/Th %02X", frame, q[o]);
        int nsym = 0;
        for (int l = 0; l < 16; l++) nsym += q[o + 1 + l];
        if (nsym > 256 || o + 17 + nsym > body) BAD("stream %d: DHT symbol count %d", frame, nsym);
        if (build_table(P.tab[2 * th + tc], q + o + 1, q + o + 17, nsym))
          BAD("stream %d: DHT code over-subscribed", frame);
        P.have_tab[2 * th + tc] = true;
        o += 17 + nsym;
      }
    } else if (m == 0xC0) {  // SOF0
      if (P.ncomp) BAD("stream %d: second SOF0", frame);
      if (body < 6) BAD("stream %d: SOF0 length", frame);
      if (q[0] != 8) BAD("stream %d: %d-bit samples (only 8-bit)", frame, q[0]);
      const int nc = q[5];
      if (nc != 1 && nc != 3) BAD("stream %d: %d components (only greyscale and YCbCr)", frame, nc);
      if (body < 6 + 3 * nc) BAD("stream %d: SOF0 length", frame);
      P.h = be16(q + 1);
      P.w = be16(q + 3);
      if (P.w <= 0 || P.h <= 0) BAD("stream %d: %dx%d", frame, P.w, P.h);
      for (int c = 0; c < nc; c++) {
        const uint8_t *e = q + 6 + 3 * c;
        P.cid[c] = e[0];
        P.decl_hv[c] = e[1];
        P.hs[c] = e[1] >> 4;
        P.vs[c] = e[1] & 15;
        P.tq[c] = e[2];
        if (P.hs[c] < 1 || P.hs[c] > 4 || P.vs[c] < 1 || P.vs[c] > 4 || P.tq[c] > 3)
          BAD("stream %d: SOF0 component %d sampling %dx%d / Tq %d", frame, c, P.hs[c], P.vs[c], P.tq[c]);
        for (int b = 0; b < c; b++)
          if (P.cid[b] == P.cid[c]) BAD("stream %d: SOF0 repeats component id %d", frame, P.cid[c]);
      }
      if (nc == 1) {
        P.hs[0] = P.vs[0] = 1;
      } else {
        if (P.hs[1] != 1 || P.vs[1] != 1 || P.hs[2] != 1 || P.vs[2] != 1)
          BAD("stream %d: chroma sampling %dx%d / %dx%d (only 1x1)", frame, P.hs[1], P.vs[1], P.hs[2], P.vs[2]);
        if (!(P.hs[0] <= 2 && P.vs[0] <= P.hs[0]))
          BAD("stream %d: luma sampling %dx%d (only 1x1, 2x1, 2x2)", frame, P.hs[0], P.vs[0]);
      }
      P.ncomp = nc;
      P.hmax = P.hs[0];
      P.vmax = P.vs[0];
      P.mcus_x = (P.w + 8 * P.hmax - 1) / (8 * P.hmax);
      P.mcus_y = (P.h + 8 * P.vmax - 1) / (8 * P.vmax);
      for (int c = 0; c < nc; c++) {
        P.bw[c] = P.mcus_x * P.hs[c];
        P.bh[c] = P.mcus_y * P.vs[c];
      }
    } else if (m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xCF && m != 0xC8 && m != 0xCC)) {
      BAD("stream %d: SOF 0x%02X is not baseline", frame, m);
    } else if (m == 0xDD) {  // DRI
      if (body != 2) BAD("stream %d: DRI length", frame);
      P.ri = be16(q);
    } else if (m == 0xEE) {  // APP14: Adobe's colour transform flag
      if (body >= 12 && !memcmp(q, "Adobe", 5)) P.adobe = q[11];
    } else if (m == 0xDA) {  // SOS + entropy data
      if (!P.ncomp) BAD("stream %d: SOS before SOF0", frame);
      if (body < 1 || body != 4 + 2 * q[0]) BAD("stream %d: SOS length", frame);
      const int ns = q[0];
      const uint8_t *tail = q + 1 + 2 * ns;
      if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0) BAD("stream %d: SOS Ss/Se/AhAl (only 0, 63, 0)", frame);
      if (P.interleaved) BAD("stream %d: more than one scan after an interleaved scan", frame);
      const bool il = ns == P.ncomp;
      if (il) {
        if (P.nscans) BAD("stream %d: interleaved scan after one-component scans", frame);
        for (int c = 0; c < ns; c++) {
          if (q[1 + 2 * c] != P.cid[c]) BAD("stream %d: SOS selectors are not the SOF0 components in order", frame);
          P.td[c] = q[2 + 2 * c] >> 4;
          P.ta[c] = q[2 + 2 * c] & 15;
          if (P.td[c] > 1 || P.ta[c] > 1) BAD("stream %d: SOS table ids", frame);
          if (!P.have_tab[2 * P.td[c]] || !P.have_tab[2 * P.ta[c] + 1])
            BAD("stream %d: Huffman table of component %d missing before its scan", frame, c);
        }
        P.interleaved = true;
      } else {
        // one-component scans: only the encoder's own shape.  Such scans of
        // other samplings or sizes cover ceil(w_c / 8) x ceil(h_c / 8) blocks,
        // not the padded plane, and nothing at hand writes them to test with.
        if (ns != 1 || P.ncomp != 3 || P.hs[0] != 2 || P.vs[0] != 2 || P.w % 16 || P.h % 16 || P.ri ||
            P.tq[1] != P.tq[2])
          BAD("stream %d: SOS of %d components in a %d-component %dx%d frame (non-interleaved scans only as three "
              "scans of a 4:2:0 frame, multiples of 16, no restarts)", frame, ns, P.ncomp, P.w, P.h);
        if (P.nscans >= 3) BAD("stream %d: more than three scans", frame);
        Parsed::Scan &sc = P.scan[P.nscans++];
        sc.comp = -1;
        for (int c = 0; c < 3; c++)
          if (q[1] == P.cid[c]) sc.comp = c;
        sc.td = q[2] >> 4;
        sc.ta = q[2] & 15;
        if (sc.comp < 0 || sc.td > 1 || sc.ta > 1) BAD("stream %d: SOS component", frame);
        // each component exactly once: a repeated scan would leave another
        // component's plane unwritten (it keeps the previous call's values)
        if (P.comp_seen & (1 << sc.comp)) BAD("stream %d: SOS repeats component %d", frame, sc.comp + 1);
        P.comp_seen |= 1 << sc.comp;
      }
      size_t e = i + 2 + len;
      long long start = (long long)e;
      const long long nm = (long long)P.mcus_x * P.mcus_y;
      const long long want = il && P.ri ? (nm + P.ri - 1) / P.ri : 1;
      // entropy data ends at the next marker: a 0xFF followed by neither
      // 0x00 (stuffing) nor 0xFF.  The reference never stuffs its end-of-scan
      // pad byte (encoder.c:425-432), so "FF FF xx" is a pad byte that still
      // holds the scan's last bits, then the marker: the first FF is kept as
      // data.  On a standard stream those are fill bytes before a marker;
      // kept, they are trailing one-bits after the last block, and decoding
      // stops at the block count, so the same rule serves every stream.
      // FF D0..D7 bound an interval only while a restart interval is in
      // force; otherwise they end the scan and the marker loop refuses them.
      for (;;) {
        const uint8_t *f = (const uint8_t *)memchr(s + e, 0xFF, n - e);
        if (!f || (size_t)(f - s) + 1 >= n) BAD("stream %d: scan %d runs to the end", frame, P.nscans + (il ? 1 : 0));
        e = f - s;
        const int b = s[e + 1];
        if (b == 0x00) {
          e += 2;
          continue;
        }
        if (b == 0xFF) {
          e += 1;
          continue;
        }
        if (b >= 0xD0 && b <= 0xD7 && il && P.ri) {
          const int k = (int)P.ivl.size();
          if (b != 0xD0 + (k & 7))
            BAD("stream %d: restart marker RST%d where RST%d is due (interval %d)", frame, b - 0xD0, k & 7, k);
          if (k + 1 >= want) BAD("stream %d: more restart markers than its %lld intervals need", frame, want);
          P.ivl.push_back({start, (long long)e});
          e += 2;
          start = (long long)e;
          continue;
        }
        break;
      }
      if (il) {
        P.ivl.push_back({start, (long long)e});
        if ((long long)P.ivl.size() != want)
          BAD("stream %d: %zu restart intervals, %lld expected (%lld MCUs, interval %d)", frame, P.ivl.size(), want,
              nm, P.ri);
      } else {
        P.scan[P.nscans - 1].data = start;
        P.scan[P.nscans - 1].end = (long long)e;
      }
      i = e;
      continue;
    }
    i += 2 + len;  // APPn, COM, anything else: skipped
  }
  if (!P.ncomp) BAD("stream %d: no SOF0", frame);
  // Adobe transform 0 on three components is RGB, 2 is YCCK; on a single
  // component the flag says nothing
  if (P.ncomp == 3 && (P.adobe == 0 || P.adobe == 2))
    BAD("stream %d: Adobe APP14 transform %d (RGB / YCCK), only YCbCr", frame, P.adobe);
  if (P.interleaved) {
    for (int c = 0; c < P.ncomp; c++)
      if (!P.have_dqt[P.tq[c]]) BAD("stream %d: DQT %d of component %d missing", frame, P.tq[c], c);
    return MIJ_OK;
  }
  if (P.nscans != 3) BAD("stream %d: missing scans (%d)", frame, P.nscans);
  for (int k = 0; k < 3; k++) {
    const auto &sc = P.scan[k];
    if (!P.have_tab[2 * sc.td] || !P.have_tab[2 * sc.ta + 1]) BAD("stream %d: scan %d table missing", frame, k);
  }
  P.legacy = true;
  return MIJ_OK;
#undef BAD
}

// where a frame of the last decode lives
struct FrameLoc {
  bool foreign = false;  // in the arena of padded planes, not in its legacy slot
  long long off[3] = {0, 0, 0};  // first int16 / sample byte of each component's plane
  long long pix = 0;     // first byte of its pixels (legacy: d_pix, else f_pix)
};

template <class T>
int grow(T *&p, size_t &cap, size_t need) {
  if (need <= cap) return MIJ_OK;
  hipFree(p);  // waits for the device
  p = nullptr;
  cap = 0;
  HIP_TRY(hipMalloc((void **)&p, need * sizeof(T)));
  cap = need;
  return MIJ_OK;
}

}  // namespace

struct mij_decoder {
  int dev = 0;
  hipStream_t stream = nullptr;
  int max_w = 0, max_h = 0, cap = 0;
  size_t blob_cap = 0;
  uint8_t *d_blob = nullptr, *h_blob = nullptr;
  int16_t *d_coef = nullptr;
  mij::DecTab *d_tabs = nullptr;
  mij::DecJob *d_jobs = nullptr;
  int *d_status = nullptr;
  int *d_changed = nullptr;
  long long *d_entry = nullptr, *d_exit[2] = {nullptr, nullptr}, *d_base = nullptr;
  int *d_nblk = nullptr;
  int chunk_cap = 0, job_cap = 1 << 30, last_passes = 0;
  std::vector<Parsed> parsed;
  std::vector<FrameLoc> loc;
  long long plane_px = 0;  // max_w * max_h: Y plane; Cb/Cr a quarter each
  int n = 0;
  // pixels (mij_decoder_reconstruct): allocated on its first call
  bool rec_ready = false;  // the legacy frames' buffers exist
  bool rec_valid = false;  // they hold the last decode's frames
  uint8_t *d_planes = nullptr, *d_pix = nullptr;
  int32_t *d_dc = nullptr, *d_recq = nullptr;
  uint32_t *d_tile = nullptr;
  mij::RecJob *d_rjobs = nullptr;
  mij::RecFrame *d_rframes = nullptr;
  std::vector<mij::RecJob> h_rjobs;  // kept: the uploads are asynchronous
  std::vector<mij::RecFrame> h_rframes;
  std::vector<int32_t> h_recq;
  hipEvent_t rec_ev[3] = {nullptr, nullptr, nullptr};
  // Frames that are not of the legacy shape live in an arena of their own,
  // packed frame after frame in the order of the call and grown (freed and
  // allocated again) when a call needs more: a decoder that only ever sees
  // legacy streams allocates none of it.
  int16_t *f_coef = nullptr;
  uint8_t *f_planes = nullptr, *f_pix = nullptr;
  int32_t *f_dc = nullptr, *f_recq = nullptr;
  uint32_t *f_tile = nullptr;
  mij::IlJob *f_jobs = nullptr;
  mij::IlFrame *f_frames = nullptr;
  int *f_status = nullptr;
  mij::IlRec *f_rjobs = nullptr;
  mij::IlPix *f_rpix = nullptr;
  size_t f_coef_cap = 0, f_planes_cap = 0, f_pix_cap = 0, f_dc_cap = 0, f_recq_cap = 0, f_tile_cap = 0,
         f_jobs_cap = 0, f_frames_cap = 0, f_status_cap = 0, f_rjobs_cap = 0, f_rpix_cap = 0;
  long long f_pix_bytes = 0;  // of the last decode's frames
  std::vector<mij::IlRec> h_irec;
  std::vector<mij::IlPix> h_ipix;
  std::vector<int32_t> h_irecq;
  // decoding at 1/2, 1/4, 1/8 scale (mij_decoder_reconstruct_scaled, DESIGN.md
  // §4j): the job tables only; planes and pixels take the places of the
  // full-size ones
  int rec_denom = 1;  // of the last reconstruct
  std::vector<mij::ScaledGeom> sgeom;  // per frame, when rec_denom > 1
  mij::ScJob *s_jobs = nullptr;
  mij::IlPix *s_pix = nullptr;
  size_t s_jobs_cap = 0, s_pix_cap = 0;
  std::vector<mij::ScJob> h_sjobs;
  std::vector<mij::IlPix> h_spix;
  // lossless transcoding (mij_decoder_transcode): everything allocated at its
  // first call and grown like the arena.  It keeps its own DC prefix sums, so
  // that it and reconstruct may run in either order, or alone.
  bool tc_valid = false;  // the streams below are the last decode's
  hipEvent_t tc_ev[2] = {nullptr, nullptr};
  int32_t *t_dcl = nullptr, *t_dcf = nullptr;  // prefix sums of the legacy slots' / the arena's DCs
  uint32_t *t_tile = nullptr;
  mij::IlRec *t_rec = nullptr;
  mij::TcDc *t_dcjobs = nullptr;
  int16_t *t_abs = nullptr;
  mij::TcFrame *t_frames = nullptr;
  mij::TcOut *t_outs = nullptr;
  uint32_t *t_hist = nullptr, *t_ehuf = nullptr;
  mij::HuffCode *t_hc = nullptr;
  uint16_t *t_blk_bits = nullptr;
  uint32_t *t_mcu_off = nullptr, *t_row_bits = nullptr;
  unsigned long long *t_row_pre = nullptr, *t_ival = nullptr, *t_row_off = nullptr, *t_bits = nullptr;
  uint32_t *t_raw = nullptr, *t_ffc = nullptr;
  int *t_hdr = nullptr, *t_err = nullptr;
  uint8_t *t_out = nullptr;
  uint64_t *t_len = nullptr;
  size_t t_dcl_cap = 0, t_dcf_cap = 0, t_tile_cap = 0, t_rec_cap = 0, t_dcjobs_cap = 0, t_abs_cap = 0,
         t_frames_cap = 0, t_outs_cap = 0, t_hist_cap = 0, t_ehuf_cap = 0, t_hc_cap = 0, t_blk_bits_cap = 0,
         t_mcu_off_cap = 0, t_row_bits_cap = 0, t_row_pre_cap = 0, t_ival_cap = 0, t_row_off_cap = 0,
         t_bits_cap = 0, t_raw_cap = 0, t_ffc_cap = 0, t_hdr_cap = 0, t_err_cap = 0, t_out_cap = 0, t_len_cap = 0;
  std::vector<mij::IlRec> h_trec;  // kept: the uploads are asynchronous
  std::vector<mij::TcDc> h_tdc;
  std::vector<mij::TcFrame> h_tframes;
  std::vector<mij::TcOut> h_touts;
  std::vector<uint64_t> tc_len;    // per frame of the last transcode or transform
  std::vector<int> tc_err;
  // lossless transforms (mij_decoder_transform): the
  // transformed planes and absolute DCs, allocated at the first transform
  int16_t *x_plane = nullptr, *x_abs = nullptr;
  mij::XfFrame *x_frames = nullptr;
  size_t x_plane_cap = 0, x_abs_cap = 0, x_frames_cap = 0;
  std::vector<mij::XfFrame> h_xframes;
};

static void decoder_free(mij_decoder *d) {
  if (!d) return;
  hipSetDevice(d->dev);
  if (d->stream) hipStreamSynchronize(d->stream);
  hipFree(d->d_blob);
  hipFree(d->d_coef);
  hipFree(d->d_tabs);
  hipFree(d->d_jobs);
  hipFree(d->d_status);
  hipFree(d->d_changed);
  hipFree(d->d_entry);
  hipFree(d->d_exit[0]);
  hipFree(d->d_exit[1]);
  hipFree(d->d_nblk);
  hipFree(d->d_base);
  hipFree(d->d_planes);
  hipFree(d->d_pix);
  hipFree(d->d_dc);
  hipFree(d->d_recq);
  hipFree(d->d_tile);
  hipFree(d->d_rjobs);
  hipFree(d->d_rframes);
  hipFree(d->f_coef);
  hipFree(d->f_planes);
  hipFree(d->f_pix);
  hipFree(d->f_dc);
  hipFree(d->f_recq);
  hipFree(d->f_tile);
  hipFree(d->f_jobs);
  hipFree(d->f_frames);
  hipFree(d->f_status);
  hipFree(d->f_rjobs);
  hipFree(d->f_rpix);
  hipFree(d->s_jobs);
  hipFree(d->s_pix);
  for (void *p : {(void *)d->t_dcl, (void *)d->t_dcf, (void *)d->t_tile, (void *)d->t_rec, (void *)d->t_dcjobs,
                  (void *)d->t_abs, (void *)d->t_frames, (void *)d->t_outs, (void *)d->t_hist, (void *)d->t_ehuf,
                  (void *)d->t_hc, (void *)d->t_blk_bits, (void *)d->t_mcu_off, (void *)d->t_row_bits,
                  (void *)d->t_row_pre, (void *)d->t_ival, (void *)d->t_row_off, (void *)d->t_bits, (void *)d->t_raw,
                  (void *)d->t_ffc, (void *)d->t_hdr, (void *)d->t_err, (void *)d->t_out, (void *)d->t_len,
                  (void *)d->x_plane, (void *)d->x_abs, (void *)d->x_frames})
    hipFree(p);
  for (hipEvent_t e : d->rec_ev)
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : d->tc_ev)
    if (e) hipEventDestroy(e);
  if (d->h_blob) hipHostFree(d->h_blob);
  if (d->stream) hipStreamDestroy(d->stream);
  delete d;
}

extern "C" mij_decoder *mij_decoder_create(int device, int max_w, int max_h, int max_frames) {
  mij_clear_error();
  if (max_w < 16 || max_h < 16 || max_w % 16 || max_h % 16 || max_frames < 1) {
    mij_fail(MIJ_EINVAL, "decoder_create: %dx%d x%d", max_w, max_h, max_frames);
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    mij_fail(MIJ_ENODEV, "no HIP device %d (the HIP path has no CPU fallback)", device);
    return nullptr;
  }
  auto *d = new mij_decoder();
  d->dev = device;
  d->max_w = max_w;
  d->max_h = max_h;
  d->cap = max_frames;
  d->plane_px = (long long)max_w * max_h;
  auto init = [&]() -> int {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    HIP_TRY(hipMalloc((void **)&d->d_coef, (size_t)max_frames * d->plane_px * 3 / 2 * sizeof(int16_t)));
    HIP_TRY(hipMalloc((void **)&d->d_tabs, (size_t)max_frames * 4 * sizeof(mij::DecTab)));
    HIP_TRY(hipMalloc((void **)&d->d_jobs, (size_t)max_frames * 3 * sizeof(mij::DecJob)));
    HIP_TRY(hipMalloc((void **)&d->d_status, (size_t)max_frames * 3 * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&d->d_changed, sizeof(int)));
    return MIJ_OK;
  };
  if (init()) {
    decoder_free(d);
    return nullptr;
  }
  return d;
}

extern "C" void mij_decoder_destroy(mij_decoder *d) { decoder_free(d); }

static int decoder_stage(mij_decoder *d, size_t total) {
  if (total <= d->blob_cap) return MIJ_OK;
  hipFree(d->d_blob);
  if (d->h_blob) hipHostFree(d->h_blob);
  d->d_blob = nullptr;
  d->h_blob = nullptr;
  d->blob_cap = 0;
  const size_t cap = total + total / 4 + 4096;
  HIP_TRY(hipMalloc((void **)&d->d_blob, cap));
  HIP_TRY(hipHostMalloc((void **)&d->h_blob, cap));
  d->blob_cap = cap;
  return MIJ_OK;
}

// Unstuffed copy of scan bytes [b, e) of stream s into dst; returns bytes
static size_t unstuff(uint8_t *dst, const uint8_t *s, size_t b, size_t e) {
  size_t o = 0;
  while (b < e) {
    const uint8_t *f = (const uint8_t *)memchr(s + b, 0xFF, e - b);
    const size_t stop = f ? (size_t)(f - s) + 1 : e;  // through the 0xFF
    memcpy(dst + o, s + b, stop - b);
    o += stop - b;
    b = stop;
    if (f && b < e && s[b] == 0x00) b++;  // stuffed zero (B.1.1.5)
  }
  return o;
}

static int decoder_buffers(mij_decoder *d, int nchunks, int njobs) {
  if (nchunks <= d->chunk_cap && njobs <= d->job_cap) return MIJ_OK;
  // null each pointer once freed: a failed hipMalloc below must not leave
  // one dangling for the next call or decoder_free to free again
  for (void **p : {(void **)&d->d_entry, (void **)&d->d_exit[0], (void **)&d->d_exit[1], (void **)&d->d_nblk,
                   (void **)&d->d_base}) {
    hipFree(*p);
    *p = nullptr;
  }
  d->chunk_cap = 0;
  const size_t n = (size_t)nchunks + nchunks / 4 + 1024;
  HIP_TRY(hipMalloc((void **)&d->d_entry, n * sizeof(long long)));
  HIP_TRY(hipMalloc((void **)&d->d_exit[0], n * sizeof(long long)));
  HIP_TRY(hipMalloc((void **)&d->d_exit[1], n * sizeof(long long)));
  HIP_TRY(hipMalloc((void **)&d->d_nblk, n * sizeof(int)));
  HIP_TRY(hipMalloc((void **)&d->d_base, n * sizeof(long long)));
  d->chunk_cap = (int)n;
  return MIJ_OK;
}

// the legacy frames' scans: jobs[3 * i + k] belongs to frame leg[i]
static int decode_legacy(mij_decoder *d, std::vector<mij::DecJob> &jobs, const std::vector<int> &leg, int *passes_out) {
  int nchunks = 0, max_chunks = 1;
  for (auto &j : jobs) {
    j.chunk0 = nchunks;
    nchunks += j.nchunks;
    max_chunks = std::max(max_chunks, j.nchunks);
  }
  const int nj = (int)jobs.size();
  HIP_TRY(hipMemcpyAsync(d->d_jobs, jobs.data(), jobs.size() * sizeof(mij::DecJob), hipMemcpyHostToDevice,
                         d->stream));
  HIP_TRY(hipMemsetAsync(d->d_status, 0, nj * sizeof(int), d->stream));
  mij::SyncArgs a{d->d_blob, d->d_jobs, nj, nchunks, d->d_tabs, d->d_entry, d->d_exit[1], d->d_exit[0],
                  d->d_nblk, d->d_changed, 1};
  const dim3 grid((nchunks + 255) / 256);
  hipLaunchKernelGGL(mij::k_dec_sync, grid, dim3(256), 0, d->stream, a);
  HIP_TRY(hipGetLastError());
  int cur = 0, passes = 1;
  for (;; passes++) {
    // every pass settles at least one more chunk of each scan, so this bound
    // is never reached by a valid stream (badly synchronising content, e.g.
    // Q=100 noise with blocks longer than a chunk, only costs more passes)
    if (passes > max_chunks + 1) return mij_fail(MIJ_EJPEG, "decoder: chunk states did not settle");
    HIP_TRY(hipMemsetAsync(d->d_changed, 0, sizeof(int), d->stream));
    a.first = 0;
    a.exit_in = d->d_exit[cur];
    a.exit_out = d->d_exit[!cur];
    hipLaunchKernelGGL(mij::k_dec_sync, grid, dim3(256), 0, d->stream, a);
    HIP_TRY(hipGetLastError());
    cur = !cur;
    int changed = 0;
    HIP_TRY(hipMemcpyAsync(&changed, d->d_changed, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    if (!changed) break;
  }
  *passes_out = passes;
  hipLaunchKernelGGL(mij::k_dec_scan, dim3(nj), dim3(256), 0, d->stream, d->d_jobs, d->d_nblk, d->d_base,
                     d->d_status);
  hipLaunchKernelGGL(mij::k_dec_write, grid, dim3(256), 0, d->stream, a, d->d_base, d->d_coef, d->d_status);
  HIP_TRY(hipGetLastError());
  std::vector<int> st(nj);
  HIP_TRY(hipMemcpyAsync(st.data(), d->d_status, nj * sizeof(int), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  for (int j = 0; j < nj; j++)
    if (st[j]) return mij_fail(MIJ_EJPEG, "stream %d scan %d: corrupt entropy data (%d)", leg[j / 3], j % 3, st[j]);
  return MIJ_OK;
}

// the other frames' restart intervals; their chunk arrays start at chunk `c0`
// of the decoder's (behind the legacy scans')
static int decode_interleaved(mij_decoder *d, std::vector<mij::IlJob> &jobs, std::vector<mij::IlFrame> &frames,
                              const std::vector<int> &fgn, int c0, int *passes_out) {
  const int nj = (int)jobs.size(), nf = (int)frames.size();
  int nchunks = 0, max_chunks = 1;
  for (auto &j : jobs) {
    mij::IlFrame &F = frames[j.frame];
    if (F.nchunks == 0) F.chunk0 = nchunks;
    j.chunk0 = nchunks;
    nchunks += j.nchunks;
    F.nchunks += j.nchunks;
    max_chunks = std::max(max_chunks, j.nchunks);
  }
  if (int rc = grow(d->f_jobs, d->f_jobs_cap, (size_t)nj)) return rc;
  if (int rc = grow(d->f_frames, d->f_frames_cap, (size_t)nf)) return rc;
  if (int rc = grow(d->f_status, d->f_status_cap, (size_t)nf)) return rc;
  HIP_TRY(hipMemcpyAsync(d->f_jobs, jobs.data(), nj * sizeof(mij::IlJob), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->f_frames, frames.data(), nf * sizeof(mij::IlFrame), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemsetAsync(d->f_status, 0, nf * sizeof(int), d->stream));
  mij::IlArgs a{d->d_blob, d->f_jobs, d->f_frames, nj, nchunks, d->d_tabs, d->d_entry + c0, d->d_exit[1] + c0,
                d->d_exit[0] + c0, d->d_nblk + c0, d->d_changed, 1};
  const dim3 grid((nchunks + 255) / 256);
  hipLaunchKernelGGL(mij::k_il_sync, grid, dim3(256), 0, d->stream, a);
  HIP_TRY(hipGetLastError());
  int cur = 0, passes = 1;
  for (;;) {
    // as above: each pass settles one more chunk of every interval.  The
    // slot makes interleaved scans settle later than one-component scans (a
    // chunk may find the right bit and the wrong luma slot, which only the
    // next chroma block exposes), and a pass in which nothing changes costs
    // little, so after the first two the host looks only every fourth pass.
    const int group = passes < 3 ? 1 : 4;
    if (passes > max_chunks + 1 + group) return mij_fail(MIJ_EJPEG, "decoder: chunk states did not settle");
    HIP_TRY(hipMemsetAsync(d->d_changed, 0, sizeof(int), d->stream));
    a.first = 0;
    for (int g = 0; g < group; g++, passes++) {
      a.exit_in = d->d_exit[cur] + c0;
      a.exit_out = d->d_exit[!cur] + c0;
      hipLaunchKernelGGL(mij::k_il_sync, grid, dim3(256), 0, d->stream, a);
      cur = !cur;
    }
    HIP_TRY(hipGetLastError());
    int changed = 0;
    HIP_TRY(hipMemcpyAsync(&changed, d->d_changed, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    if (!changed) break;
  }
  *passes_out = passes;
  hipLaunchKernelGGL(mij::k_il_scan, dim3(nf), dim3(256), 0, d->stream, d->f_frames, d->d_nblk + c0, d->d_base + c0);
  hipLaunchKernelGGL(mij::k_il_write, grid, dim3(256), 0, d->stream, a, d->d_base + c0, d->f_coef, d->f_status);
  HIP_TRY(hipGetLastError());
  std::vector<int> st(nf);
  HIP_TRY(hipMemcpyAsync(st.data(), d->f_status, nf * sizeof(int), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  for (int j = 0; j < nf; j++)
    if (st[j]) return mij_fail(MIJ_EJPEG, "stream %d: corrupt entropy data (%d)", fgn[j], st[j]);
  return MIJ_OK;
}

// Parses n streams, stages their unstuffed scans and restart intervals in
// one device blob and decodes them chunk-parallel.  Synchronous; the
// coefficients stay on the device (mij_decoder_coefs / _component).
extern "C" int mij_decoder_decode(mij_decoder *d, const uint8_t *const *jpgs, const size_t *lens, int n) {
  mij_clear_error();
  if (!d || !jpgs || !lens || n < 1 || n > d->cap) return mij_fail(MIJ_EINVAL, "decoder_decode: bad args");
  HIP_TRY(hipSetDevice(d->dev));
  d->n = 0;  // set to n only once every stream decoded cleanly
  d->rec_valid = false;  // pixels of an earlier decode are no longer served
  d->tc_valid = false;   // nor its transcoded streams
  d->parsed.assign(n, Parsed());
  d->loc.assign(n, FrameLoc());
  // host work per stream in parallel: parse (finds the scan ends), then
  // unstuff each piece into its slot (sized by the raw length, an upper bound)
  const int nth = std::max(1, std::min(n, (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()))));
  auto parallel = [&](auto &&fn) {
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (int t = 1; t < nth; t++)
      pool.emplace_back([&] { for (int f; (f = next++) < n;) fn(f); });
    for (int f; (f = next++) < n;) fn(f);
    for (auto &th : pool) th.join();
  };
  std::vector<int> prc(n, MIJ_OK);
  for (int f = 0; f < n; f++)
    if (!jpgs[f]) return mij_fail(MIJ_EINVAL, "decoder_decode: stream %d is NULL", f);
  parallel([&](int f) { prc[f] = parse(jpgs[f], lens[f], d->parsed[f], f); });
  std::vector<int> leg, fgn;  // frames of either kind
  for (int f = 0; f < n; f++) {
    if (prc[f]) return mij_fail(prc[f], "decoder_decode: %s", d->parsed[f].err);
    const Parsed &P = d->parsed[f];
    if (P.w > d->max_w || P.h > d->max_h)
      return mij_fail(MIJ_EINVAL, "stream %d: %dx%d exceeds the decoder's %dx%d", f, P.w, P.h, d->max_w, d->max_h);
    (P.legacy ? leg : fgn).push_back(f);
  }
  // pieces (a legacy scan, or one restart interval): raw length + >= 16 zero
  // bytes, 8-aligned
  struct Piece {
    size_t at, next;
    long long data, end;
    size_t len;
  };
  std::vector<Piece> pieces;
  std::vector<size_t> piece0(n + 1);
  size_t off = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    piece0[f] = pieces.size();
    auto add = [&](long long b, long long e) {
      const size_t next = (off + (size_t)(e - b) + 16 + 7) & ~(size_t)7;
      pieces.push_back({off, next, b, e, 0});
      off = next;
    };
    if (P.legacy)
      for (int k = 0; k < 3; k++) add(P.scan[k].data, P.scan[k].end);
    else
      for (const auto &iv : P.ivl) add(iv.data, iv.end);
  }
  piece0[n] = pieces.size();
  // chunk ids are ints: every piece has max(1, ceil(bits / 512)) chunks
  if (off / 64 + pieces.size() > 0x7fff0000u) return mij_fail(MIJ_EINVAL, "decoder_decode: too much entropy data");
  if (int rc = decoder_stage(d, off)) return rc;
  // the arena of the frames that are not of the legacy shape
  const long long fs = d->plane_px * 3 / 2;  // int16 per legacy frame slot
  long long units = 0, pixb = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    FrameLoc &L = d->loc[f];
    if (P.legacy) {
      const long long ny = (long long)P.w * P.h;
      L.off[0] = f * fs;
      L.off[1] = f * fs + ny;
      L.off[2] = f * fs + ny + ny / 4;
      L.pix = f * d->plane_px * 3;
    } else {
      L.foreign = true;
      for (int c = 0; c < P.ncomp; c++) {
        L.off[c] = units;
        units += 64LL * P.bw[c] * P.bh[c];
      }
      L.pix = pixb;
      pixb += P.pitch() * P.h;
    }
  }
  d->f_pix_bytes = pixb;
  if (int rc = grow(d->f_coef, d->f_coef_cap, (size_t)units)) return rc;
  std::vector<mij::DecTab> tabs(4 * (size_t)n);
  parallel([&](int f) {
    const Parsed &P = d->parsed[f];
    for (int t = 0; t < 4; t++) tabs[4 * f + t] = P.tab[t];
    for (size_t p = piece0[f]; p < piece0[f + 1]; p++) {
      Piece &pc = pieces[p];
      pc.len = unstuff(d->h_blob + pc.at, jpgs[f], (size_t)pc.data, (size_t)pc.end);
      memset(d->h_blob + pc.at + pc.len, 0, pc.next - pc.at - pc.len);
    }
  });
  auto chunks_of = [](long long nbits) { return std::max(1, (int)((nbits + mij::CHUNK - 1) / mij::CHUNK)); };
  std::vector<mij::DecJob> jobs(3 * leg.size());
  for (size_t i = 0; i < leg.size(); i++) {
    const int f = leg[i];
    const Parsed &P = d->parsed[f];
    const long long ny = (long long)P.w * P.h;
    for (int k = 0; k < 3; k++) {
      const auto &sc = P.scan[k];
      const Piece &pc = pieces[piece0[f] + k];
      mij::DecJob &j = jobs[3 * i + k];
      j.data = (long long)pc.at;
      j.nbits = 8LL * (long long)pc.len;
      j.out = d->loc[f].off[sc.comp];
      j.nblocks = (int)(sc.comp ? ny / 256 : ny / 64);
      j.dc = 4 * f + 2 * sc.td;
      j.ac = 4 * f + 2 * sc.ta + 1;
      j.nchunks = chunks_of(j.nbits);
    }
  }
  std::vector<mij::IlFrame> iframes(fgn.size());
  std::vector<mij::IlJob> ijobs;
  for (size_t i = 0; i < fgn.size(); i++) {
    const int f = fgn[i];
    const Parsed &P = d->parsed[f];
    mij::IlFrame &F = iframes[i];
    memset(&F, 0, sizeof F);
    F.ncomp = P.ncomp;
    F.mcus_x = P.mcus_x;
    F.nmcus = P.mcus_x * P.mcus_y;
    for (int c = 0; c < P.ncomp; c++) {
      F.off[c] = d->loc[f].off[c];
      F.hs[c] = P.hs[c];
      F.vs[c] = P.vs[c];
      F.bw[c] = P.bw[c];
      F.dc[c] = 4 * f + 2 * P.td[c];
      F.ac[c] = 4 * f + 2 * P.ta[c] + 1;
      for (int y = 0; y < P.vs[c]; y++)
        for (int x = 0; x < P.hs[c]; x++) {  // at most 2 * 2 + 1 + 1 = 6: parse() admits no other sampling
          F.slot_comp[F.bpm] = c;
          F.slot_x[F.bpm] = x;
          F.slot_y[F.bpm] = y;
          F.bpm++;
        }
    }
    const int ri = P.ri ? P.ri : F.nmcus;
    for (size_t k = 0; k < P.ivl.size(); k++) {
      const Piece &pc = pieces[piece0[f] + k];
      mij::IlJob j;
      j.data = (long long)pc.at;
      j.nbits = 8LL * (long long)pc.len;
      j.frame = (int)i;
      // parse() made the interval count ceil(nmcus / ri), so mcu0 < nmcus and
      // mcu0 + nmcus_i <= nmcus: what bounds k_il_write's stores
      j.mcu0 = (int)((long long)k * ri);
      j.nmcus = std::min(ri, F.nmcus - j.mcu0);
      j.chunk0 = 0;
      j.nchunks = chunks_of(j.nbits);
      j.pad = 0;
      if (j.mcu0 >= F.nmcus || j.nmcus < 1) return mij_fail(MIJ_EJPEG, "stream %d: restart interval %zu has no MCUs", f, k);
      ijobs.push_back(j);
    }
  }
  long long nch_leg = 0, nch_il = 0;
  for (auto &j : jobs) nch_leg += j.nchunks;
  for (auto &j : ijobs) nch_il += j.nchunks;
  if (int rc = decoder_buffers(d, (int)(nch_leg + nch_il), 0)) return rc;
  HIP_TRY(hipMemcpyAsync(d->d_blob, d->h_blob, off, hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->d_tabs, tabs.data(), tabs.size() * sizeof(mij::DecTab), hipMemcpyHostToDevice,
                         d->stream));
  int p1 = 0, p2 = 0;
  if (!leg.empty())
    if (int rc = decode_legacy(d, jobs, leg, &p1)) return rc;
  if (!fgn.empty())
    if (int rc = decode_interleaved(d, ijobs, iframes, fgn, (int)nch_leg, &p2)) return rc;
  d->last_passes = std::max(p1, p2);
  d->n = n;
  return MIJ_OK;
}

extern "C" int mij_decoder_passes(mij_decoder *d) { return d ? d->last_passes : -1; }

extern "C" int mij_decoder_info(mij_decoder *d, int frame, int *w, int *h, uint8_t dqt[128]) {
  mij_clear_error();
  if (!d || frame < 0 || frame >= d->n) return mij_fail(MIJ_EINVAL, "decoder_info: bad frame");
  const Parsed &P = d->parsed[frame];
  if (w) *w = P.w;
  if (h) *h = P.h;
  if (dqt) {  // the tables of components 0 and 1 (greyscale: component 0 twice)
    memcpy(dqt, P.dqt[P.tq[0]], 64);
    memcpy(dqt + 64, P.dqt[P.tq[P.ncomp > 1 ? 1 : 0]], 64);
  }
  return MIJ_OK;
}

extern "C" int mij_decoder_layout(mij_decoder *d, int frame, int *out, int n) {
  mij_clear_error();
  if (!d || frame < 0 || frame >= d->n || !out) return mij_fail(MIJ_EINVAL, "decoder_layout: bad args");
  const Parsed &P = d->parsed[frame];
  const int need = 9 + 5 * P.ncomp;
  if (n < need) return mij_fail(MIJ_ENOSPC, "decoder_layout: need %d ints", need);
  const int head[9] = {P.w, P.h, P.ncomp, P.hmax, P.vmax, P.mcus_x, P.mcus_y, P.ri, P.interleaved ? 1 : 0};
  memcpy(out, head, sizeof head);
  for (int c = 0; c < P.ncomp; c++) {
    const int e[5] = {P.hs[c], P.vs[c], P.tq[c], P.bw[c], P.bh[c]};
    memcpy(out + 9 + 5 * c, e, sizeof e);
  }
  return MIJ_OK;
}

extern "C" int mij_decoder_coefs(mij_decoder *d, int frame, int16_t *Y, int16_t *Cb, int16_t *Cr) {
  mij_clear_error();
  if (!d || frame < 0 || frame >= d->n || !Y || !Cb || !Cr) return mij_fail(MIJ_EINVAL, "decoder_coefs: bad args");
  if (d->loc[frame].foreign)
    return mij_fail(MIJ_EINVAL, "decoder_coefs: frame %d is not of the encoder's layout; use mij_decoder_layout and "
                    "mij_decoder_component", frame);
  HIP_TRY(hipSetDevice(d->dev));
  const Parsed &P = d->parsed[frame];
  const long long ny = (long long)P.w * P.h;
  const int16_t *src = d->d_coef + frame * (d->plane_px * 3 / 2);
  HIP_TRY(hipMemcpyAsync(Y, src, ny * 2, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(Cb, src + ny, ny / 2, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(Cr, src + ny + ny / 4, ny / 2, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return MIJ_OK;
}

// A component's padded plane as jpeg_read_coefficients shows it: the device
// holds the coded DC differences (the IDCT takes its absolute DCs from the
// prefix sums of reconstruct), so the prediction is undone here on the host,
// in scan order and from 0 at every restart interval.
extern "C" int mij_decoder_component(mij_decoder *d, int frame, int comp, int16_t *dst, size_t cap) {
  mij_clear_error();
  if (!d || frame < 0 || frame >= d->n || !dst) return mij_fail(MIJ_EINVAL, "decoder_component: bad args");
  const Parsed &P = d->parsed[frame];
  if (comp < 0 || comp >= P.ncomp) return mij_fail(MIJ_EINVAL, "decoder_component: component %d of %d", comp, P.ncomp);
  const long long nb = (long long)P.bw[comp] * P.bh[comp];
  if (cap < (size_t)(64 * nb)) return mij_fail(MIJ_ENOSPC, "decoder_component: need %lld coefficients", 64 * nb);
  HIP_TRY(hipSetDevice(d->dev));
  const FrameLoc &L = d->loc[frame];
  const int16_t *src = (L.foreign ? d->f_coef : d->d_coef) + L.off[comp];
  HIP_TRY(hipMemcpyAsync(dst, src, (size_t)(128 * nb), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  // legacy: a one-component scan predicts in raster order, never resets
  const int hs = L.foreign ? P.hs[comp] : 1, vs = L.foreign ? P.vs[comp] : 1;
  const int mx_n = P.bw[comp] / hs;
  const long long seg = L.foreign && P.ri ? (long long)P.ri * hs * vs : nb;
  uint32_t run = 0;
  for (long long s = 0; s < nb; s++) {
    const long long m = s / (hs * vs), i = s % (hs * vs);
    const long long my = m / mx_n, mx = m % mx_n;
    const long long r = (my * vs + i / hs) * P.bw[comp] + mx * hs + i % hs;
    if (s % seg == 0) run = 0;
    run += (uint32_t)(int32_t)dst[64 * r];
    dst[64 * r] = (int16_t)run;
  }
  return MIJ_OK;
}

extern "C" void *mij_decoder_device_coefs(mij_decoder *d, int frame) {
  if (!d || frame < 0 || frame >= d->n) return nullptr;
  const FrameLoc &L = d->loc[frame];
  return (L.foreign ? d->f_coef : d->d_coef) + L.off[0];
}

// ---------------------------------------------------------------------------
// pixels: host side
// ---------------------------------------------------------------------------
static int decoder_rec_buffers(mij_decoder *d, bool legacy) {
  for (hipEvent_t &e : d->rec_ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  if (d->rec_ready || !legacy) return MIJ_OK;
  const size_t fs = (size_t)d->plane_px * 3 / 2, cap = (size_t)d->cap;
  auto alloc = [&]() -> int {
    HIP_TRY(hipMalloc((void **)&d->d_planes, cap * fs));
    HIP_TRY(hipMalloc((void **)&d->d_pix, cap * (size_t)d->plane_px * 3));
    HIP_TRY(hipMalloc((void **)&d->d_dc, cap * (fs / 64) * sizeof(int32_t)));
    HIP_TRY(hipMalloc((void **)&d->d_recq, cap * 128 * sizeof(int32_t)));
    // tiles: a plane of b blocks has at most b / DC_TILE + 1
    HIP_TRY(hipMalloc((void **)&d->d_tile, cap * (fs / 64 / mij::DC_TILE + 3) * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&d->d_rjobs, cap * 3 * sizeof(mij::RecJob)));
    HIP_TRY(hipMalloc((void **)&d->d_rframes, cap * sizeof(mij::RecFrame)));
    return MIJ_OK;
  };
  if (int rc = alloc()) {  // all or nothing: the next call starts over
    for (void **p : {(void **)&d->d_planes, (void **)&d->d_pix, (void **)&d->d_dc, (void **)&d->d_recq,
                     (void **)&d->d_tile, (void **)&d->d_rjobs, (void **)&d->d_rframes}) {
      hipFree(*p);
      *p = nullptr;
    }
    return rc;
  }
  d->rec_ready = true;
  return MIJ_OK;
}

static int pix_mode(const Parsed &P) {
  if (P.ncomp == 1) return mij::PIX_GREY;
  if (P.hmax == 1) return mij::PIX_444;
  const bool rep = (P.w + 1) / 2 <= 2;  // libjpeg: fancy only for downsampled_width > 2
  if (P.vmax == 1) return rep ? mij::PIX_H2V1_REP : mij::PIX_H2V1;
  return rep ? mij::PIX_H2V2_REP : mij::PIX_H2V2;
}

static int reconstruct_scaled_launch(mij_decoder *d, int order, int denom);

// denom 1: full size; 2, 4, 8: DESIGN.md §4j
static int reconstruct_any(mij_decoder *d, int order, int denom) {
  mij_clear_error();
  if (!d) return mij_fail(MIJ_EINVAL, "decoder_reconstruct: no decoder");
  if (order != MIJ_PIX_BGR && order != MIJ_PIX_RGB)
    return mij_fail(MIJ_EINVAL, "decoder_reconstruct: pixel order %d", order);
  if (denom != 1 && denom != 2 && denom != 4 && denom != 8)
    return mij_fail(MIJ_EINVAL, "decoder_reconstruct_scaled: scale 1/%d: 1/1, 1/2, 1/4 or 1/8", denom);
  if (d->n < 1) return mij_fail(MIJ_EINVAL, "decoder_reconstruct: no decoded frames");
  HIP_TRY(hipSetDevice(d->dev));
  const int n = d->n;
  int nl = 0, nf = 0;
  for (int f = 0; f < n; f++) (d->loc[f].foreign ? nf : nl)++;
  if (int rc = decoder_rec_buffers(d, nl > 0)) return rc;
  // the previous call's uploads read these vectors: let them finish first
  HIP_TRY(hipStreamSynchronize(d->stream));
  d->rec_valid = false;
  d->h_rjobs.resize(3 * (size_t)nl);
  d->h_rframes.resize(nl);
  d->h_recq.resize(128 * (size_t)n);
  long long idct_wgs = 0, col_wgs = 0, tiles = 0;
  int li = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    if (d->loc[f].foreign) continue;
    if (!P.have_dqt[P.tq[0]] || !P.have_dqt[P.tq[1]]) return mij_fail(MIJ_EJPEG, "stream %d: DQT missing", f);
    for (int t = 0; t < 2; t++)
      for (int z = 0; z < 64; z++) d->h_recq[128 * f + 64 * t + z] = P.dqt[P.tq[t]][z];
    const long long ny = (long long)P.w * P.h;
    for (int c = 0; c < 3; c++) {
      mij::RecJob &j = d->h_rjobs[3 * li + c];
      j.off = d->loc[f].off[c];
      j.nblocks = (int)(c ? ny / 256 : ny / 64);
      j.bw = c ? P.w / 16 : P.w / 8;
      j.wg0 = (int)idct_wgs;
      j.qt = 2 * f + (c != 0);
      j.tile0 = (int)tiles;
      j.pad = 0;
      idct_wgs += (j.nblocks + 255) / 256;
      tiles += (j.nblocks + mij::DC_TILE - 1) / mij::DC_TILE;
    }
    mij::RecFrame &fr = d->h_rframes[li++];
    fr.planes = d->loc[f].off[0];
    fr.pix = d->loc[f].pix;
    fr.w = P.w;
    fr.h = P.h;
    fr.wg0 = (int)col_wgs;
    fr.pad = 0;
    col_wgs += ((long long)(P.h / 2) * (P.w / 16) + 255) / 256;
  }
  // the frames in the arena: one IlRec per component, one IlPix per frame
  d->h_irec.clear();
  d->h_ipix.clear();
  d->h_irecq.clear();
  long long i_wgs = 0, i_col = 0, i_tiles = 0, units = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    const FrameLoc &L = d->loc[f];
    if (!L.foreign) continue;
    for (int c = 0; c < P.ncomp; c++) {
      mij::IlRec j;
      j.off = L.off[c];
      j.nblocks = P.bw[c] * P.bh[c];
      j.bw = P.bw[c];
      j.wg0 = (int)i_wgs;
      j.qt = (int)(d->h_irecq.size() / 64);
      j.tile0 = (int)i_tiles;
      j.hs = P.hs[c];
      j.vs = P.vs[c];
      j.mcus_x = P.mcus_x;
      j.seg = P.ri ? (int)std::min<long long>((long long)P.ri * P.hs[c] * P.vs[c], j.nblocks) : j.nblocks;
      j.pad = 0;
      for (int z = 0; z < 64; z++) d->h_irecq.push_back(P.dqt[P.tq[c]][z]);
      i_wgs += (j.nblocks + 255) / 256;
      i_tiles += (j.nblocks + mij::DC_TILE - 1) / mij::DC_TILE;
      units = std::max(units, j.off + 64LL * j.nblocks);
      d->h_irec.push_back(j);
    }
    mij::IlPix px;
    memset(&px, 0, sizeof px);
    px.y = L.off[0];
    px.cb = L.off[P.ncomp > 1 ? 1 : 0];
    px.cr = L.off[P.ncomp > 1 ? 2 : 0];
    px.pix = L.pix;
    px.G.w = P.w;
    px.G.h = P.h;
    px.G.mode = pix_mode(P);
    px.G.yp = 8 * P.bw[0];
    px.G.cp = P.ncomp > 1 ? 8 * P.bw[1] : 8 * P.bw[0];
    px.G.cw = (P.w + P.hmax - 1) / P.hmax;
    px.G.ch = (P.h + P.vmax - 1) / P.vmax;
    px.G.pitch = P.pitch();
    px.groups = (P.w + 15) / 16;
    const int rows = mij::pix_rows_per_lane(px.G.mode);
    px.units = (P.h + rows - 1) / rows;
    px.wg0 = (int)i_col;
    i_col += ((long long)px.units * px.groups + 255) / 256;
    d->h_ipix.push_back(px);
  }
  if (idct_wgs > 0x7fffffff || col_wgs > 0x7fffffff || i_wgs > 0x7fffffff || i_col > 0x7fffffff)
    return mij_fail(MIJ_EINVAL, "decoder_reconstruct: too many blocks");
  if (nf) {
    if (int rc = grow(d->f_planes, d->f_planes_cap, (size_t)units)) return rc;
    if (int rc = grow(d->f_dc, d->f_dc_cap, (size_t)(units / 64))) return rc;
    if (int rc = grow(d->f_tile, d->f_tile_cap, (size_t)i_tiles)) return rc;
    if (int rc = grow(d->f_pix, d->f_pix_cap, (size_t)d->f_pix_bytes)) return rc;
    if (int rc = grow(d->f_recq, d->f_recq_cap, d->h_irecq.size())) return rc;
    if (int rc = grow(d->f_rjobs, d->f_rjobs_cap, d->h_irec.size())) return rc;
    if (int rc = grow(d->f_rpix, d->f_rpix_cap, d->h_ipix.size())) return rc;
    HIP_TRY(hipMemcpyAsync(d->f_rjobs, d->h_irec.data(), d->h_irec.size() * sizeof(mij::IlRec), hipMemcpyHostToDevice,
                           d->stream));
    HIP_TRY(hipMemcpyAsync(d->f_rpix, d->h_ipix.data(), d->h_ipix.size() * sizeof(mij::IlPix), hipMemcpyHostToDevice,
                           d->stream));
    HIP_TRY(hipMemcpyAsync(d->f_recq, d->h_irecq.data(), d->h_irecq.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                           d->stream));
  }
  if (nl) {
    HIP_TRY(hipMemcpyAsync(d->d_rjobs, d->h_rjobs.data(), d->h_rjobs.size() * sizeof(mij::RecJob),
                           hipMemcpyHostToDevice, d->stream));
    HIP_TRY(hipMemcpyAsync(d->d_rframes, d->h_rframes.data(), d->h_rframes.size() * sizeof(mij::RecFrame),
                           hipMemcpyHostToDevice, d->stream));
    HIP_TRY(hipMemcpyAsync(d->d_recq, d->h_recq.data(), d->h_recq.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                           d->stream));
  }
  const int nir = (int)d->h_irec.size();
  if (denom > 1) {  // the same DC kernels, then the scaled IDCTs and the colour stage on the scaled geometry
    if (int rc = reconstruct_scaled_launch(d, order, denom)) return rc;
    d->rec_denom = denom;
    d->rec_valid = true;
    return MIJ_OK;
  }
  HIP_TRY(hipEventRecord(d->rec_ev[0], d->stream));
  if (nl) {
    hipLaunchKernelGGL(mij::k_dec_dc, dim3((unsigned)tiles), dim3(mij::DC_T), 0, d->stream, d->d_rjobs, 3 * nl,
                       d->d_coef, d->d_dc, d->d_tile);
    hipLaunchKernelGGL(mij::k_dec_dcbase<mij::RecJob>, dim3((3 * nl + 63) / 64), dim3(64), 0, d->stream, d->d_rjobs,
                       3 * nl, d->d_tile);
    hipLaunchKernelGGL(mij::k_dec_idct, dim3((unsigned)idct_wgs), dim3(256), 0, d->stream, d->d_rjobs, 3 * nl,
                       d->d_coef, d->d_dc, d->d_tile, d->d_recq, d->d_planes);
  }
  if (nf) {
    hipLaunchKernelGGL(mij::k_il_dc, dim3((unsigned)i_tiles), dim3(mij::DC_T), 0, d->stream, d->f_rjobs, nir,
                       d->f_coef, d->f_dc, d->f_tile);
    hipLaunchKernelGGL(mij::k_dec_dcbase<mij::IlRec>, dim3((nir + 63) / 64), dim3(64), 0, d->stream, d->f_rjobs, nir,
                       d->f_tile);
    hipLaunchKernelGGL(mij::k_il_idct, dim3((unsigned)i_wgs), dim3(256), 0, d->stream, d->f_rjobs, nir, d->f_coef,
                       d->f_dc, d->f_tile, d->f_recq, d->f_planes);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(d->rec_ev[1], d->stream));
  if (nl)
    hipLaunchKernelGGL(mij::k_dec_colour, dim3((unsigned)col_wgs), dim3(256), 0, d->stream, d->d_rframes, nl,
                       d->d_planes, d->d_pix, order == MIJ_PIX_RGB);
  if (nf)
    hipLaunchKernelGGL(mij::k_il_colour, dim3((unsigned)i_col), dim3(256), 0, d->stream, d->f_rpix, nf, d->f_planes,
                       d->f_pix, order == MIJ_PIX_RGB);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(d->rec_ev[2], d->stream));
  d->rec_denom = 1;
  d->rec_valid = true;
  return MIJ_OK;
}

static void scaled_geom(const Parsed &P, int denom, mij::ScaledGeom &G) {
  mij::scaled_geometry(P.w, P.h, P.ncomp, P.hs, P.vs, P.bw, P.bh, denom, G);
}

// reconstruct_any's second half at 1/2, 1/4, 1/8: d->h_rjobs / h_irec are
// built and on their way to the device, the buffers exist
static int reconstruct_scaled_launch(mij_decoder *d, int order, int denom) {
  const int n = d->n;
  d->sgeom.resize(n);
  // ScJobs in eight runs: legacy frames' then the arena's, each by IDCT size 8, 4, 2, 1
  std::vector<mij::ScJob> run[2][4];
  long long wgs[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, col[2] = {0, 0};
  std::vector<mij::IlPix> pix[2];
  int li = 0, ir = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    const FrameLoc &L = d->loc[f];
    mij::ScaledGeom &G = d->sgeom[f];
    scaled_geom(P, denom, G);
    const int set = L.foreign ? 1 : 0;
    for (int c = 0; c < P.ncomp; c++) {
      mij::ScJob j;
      memset(&j, 0, sizeof j);
      j.off = L.off[c];
      j.bw = P.bw[c];
      j.bh = P.bh[c];
      j.nblocks = P.bw[c] * P.bh[c];
      if (L.foreign) {
        const mij::IlRec &r = d->h_irec[ir++];
        j.qt = r.qt;
        j.tile0 = r.tile0;
        j.hs = r.hs;
        j.vs = r.vs;
        j.mcus_x = r.mcus_x;
        j.seg = r.seg;
        j.il = 1;
      } else {
        const mij::RecJob &r = d->h_rjobs[3 * li + c];
        j.qt = r.qt;
        j.tile0 = r.tile0;
        j.hs = j.vs = j.mcus_x = j.seg = 1;
      }
      const int S = G.c[c].S, k = S == 8 ? 0 : S == 4 ? 1 : S == 2 ? 2 : 3;
      j.pitch = G.c[c].pitch;
      j.spr = G.c[c].pitch / 8;
      j.wg0 = (int)wgs[set][k];
      wgs[set][k] += ((long long)j.bh * j.spr + 32 * S - 1) / (32 * S);  // 256 * S / 8 strips per workgroup
      run[set][k].push_back(j);
    }
    if (!L.foreign) li++;
    mij::IlPix px;
    memset(&px, 0, sizeof px);
    px.y = L.off[0];
    px.cb = L.off[P.ncomp > 1 ? 1 : 0];
    px.cr = L.off[P.ncomp > 1 ? 2 : 0];
    px.pix = L.pix;
    px.G.w = G.ow;
    px.G.h = G.oh;
    px.G.mode = G.mode;
    px.G.yp = G.c[0].pitch;
    px.G.cp = G.c[1].pitch;
    px.G.cw = G.c[1].cw;
    px.G.ch = G.c[1].ch;
    px.G.pitch = (3LL * G.ow + 15) / 16 * 16;
    px.groups = (G.ow + 15) / 16;
    const int rows = mij::pix_rows_per_lane(G.mode);
    px.units = (G.oh + rows - 1) / rows;
    px.wg0 = (int)col[set];
    col[set] += ((long long)px.units * px.groups + 255) / 256;
    pix[set].push_back(px);
  }
  d->h_sjobs.clear();
  d->h_spix.clear();
  size_t first[2][4], pfirst[2];
  for (int set = 0; set < 2; set++) {
    for (int k = 0; k < 4; k++) {
      if (wgs[set][k] > 0x7fffffff) return mij_fail(MIJ_EINVAL, "decoder_reconstruct_scaled: too many blocks");
      first[set][k] = d->h_sjobs.size();
      d->h_sjobs.insert(d->h_sjobs.end(), run[set][k].begin(), run[set][k].end());
    }
    if (col[set] > 0x7fffffff) return mij_fail(MIJ_EINVAL, "decoder_reconstruct_scaled: too many blocks");
    pfirst[set] = d->h_spix.size();
    d->h_spix.insert(d->h_spix.end(), pix[set].begin(), pix[set].end());
  }
  if (int rc = grow(d->s_jobs, d->s_jobs_cap, d->h_sjobs.size())) return rc;
  if (int rc = grow(d->s_pix, d->s_pix_cap, d->h_spix.size())) return rc;
  HIP_TRY(hipMemcpyAsync(d->s_jobs, d->h_sjobs.data(), d->h_sjobs.size() * sizeof(mij::ScJob), hipMemcpyHostToDevice,
                         d->stream));
  HIP_TRY(hipMemcpyAsync(d->s_pix, d->h_spix.data(), d->h_spix.size() * sizeof(mij::IlPix), hipMemcpyHostToDevice,
                         d->stream));
  HIP_TRY(hipEventRecord(d->rec_ev[0], d->stream));
  const int nl = (int)pix[0].size(), nf = (int)pix[1].size(), nir = (int)d->h_irec.size();
  if (nl) {
    const mij::RecJob &last = d->h_rjobs.back();
    const int tiles = last.tile0 + (last.nblocks + mij::DC_TILE - 1) / mij::DC_TILE;
    hipLaunchKernelGGL(mij::k_dec_dc, dim3((unsigned)tiles), dim3(mij::DC_T), 0, d->stream, d->d_rjobs, 3 * nl,
                       d->d_coef, d->d_dc, d->d_tile);
    hipLaunchKernelGGL(mij::k_dec_dcbase<mij::RecJob>, dim3((3 * nl + 63) / 64), dim3(64), 0, d->stream, d->d_rjobs,
                       3 * nl, d->d_tile);
  }
  if (nf) {
    const mij::IlRec &last = d->h_irec.back();
    const int tiles = last.tile0 + (last.nblocks + mij::DC_TILE - 1) / mij::DC_TILE;
    hipLaunchKernelGGL(mij::k_il_dc, dim3((unsigned)tiles), dim3(mij::DC_T), 0, d->stream, d->f_rjobs, nir, d->f_coef,
                       d->f_dc, d->f_tile);
    hipLaunchKernelGGL(mij::k_dec_dcbase<mij::IlRec>, dim3((nir + 63) / 64), dim3(64), 0, d->stream, d->f_rjobs, nir,
                       d->f_tile);
  }
  for (int set = 0; set < 2; set++) {
    const int16_t *coefs = set ? d->f_coef : d->d_coef;
    const int32_t *dc = set ? d->f_dc : d->d_dc, *q = set ? d->f_recq : d->d_recq;
    const uint32_t *tile = set ? d->f_tile : d->d_tile;
    uint8_t *planes = set ? d->f_planes : d->d_planes;
#define SC_LAUNCH(S, k)                                                                                           \
  if (wgs[set][k])                                                                                                \
    hipLaunchKernelGGL(mij::k_sc_idct<S>, dim3((unsigned)wgs[set][k]), dim3(256), 0, d->stream,                   \
                       d->s_jobs + first[set][k], (int)run[set][k].size(), coefs, dc, tile, q, planes)
    SC_LAUNCH(8, 0);
    SC_LAUNCH(4, 1);
    SC_LAUNCH(2, 2);
    SC_LAUNCH(1, 3);
#undef SC_LAUNCH
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(d->rec_ev[1], d->stream));
  for (int set = 0; set < 2; set++)
    if (col[set])
      hipLaunchKernelGGL(mij::k_il_colour, dim3((unsigned)col[set]), dim3(256), 0, d->stream, d->s_pix + pfirst[set],
                         (int)pix[set].size(), set ? d->f_planes : d->d_planes, set ? d->f_pix : d->d_pix,
                         order == MIJ_PIX_RGB);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(d->rec_ev[2], d->stream));
  return MIJ_OK;
}

extern "C" int mij_decoder_reconstruct(mij_decoder *d, int order) { return reconstruct_any(d, order, 1); }

extern "C" int mij_decoder_reconstruct_scaled(mij_decoder *d, int order, int denom) {
  return reconstruct_any(d, order, denom);
}

extern "C" int mij_decoder_scaled_layout(mij_decoder *d, int frame, int denom, int *out, int n) {
  mij_clear_error();
  if (!d || frame < 0 || frame >= d->n || !out) return mij_fail(MIJ_EINVAL, "decoder_scaled_layout: bad args");
  if (denom != 1 && denom != 2 && denom != 4 && denom != 8)
    return mij_fail(MIJ_EINVAL, "decoder_scaled_layout: scale 1/%d: 1/1, 1/2, 1/4 or 1/8", denom);
  const Parsed &P = d->parsed[frame];
  const int need = 3 + 5 * P.ncomp;
  if (n < need) return mij_fail(MIJ_ENOSPC, "decoder_scaled_layout: need %d ints", need);
  mij::ScaledGeom G;
  scaled_geom(P, denom, G);
  out[0] = G.ow;
  out[1] = G.oh;
  out[2] = P.ncomp;
  for (int c = 0; c < P.ncomp; c++) {
    const int e[5] = {G.c[c].S, G.c[c].cw, G.c[c].ch, G.c[c].pitch, G.c[c].rows};
    memcpy(out + 3 + 5 * c, e, sizeof e);
  }
  return MIJ_OK;
}

// the frame's geometry once pixels of the last decode exist
static int rec_frame(mij_decoder *d, int frame, const char *what, const Parsed **P) {
  if (!d) return mij_fail(MIJ_EINVAL, "%s: no decoder", what);
  if (!d->rec_valid) return mij_fail(MIJ_EINVAL, "%s: no mij_decoder_reconstruct since the last decode", what);
  if (frame < 0 || frame >= d->n) return mij_fail(MIJ_EINVAL, "%s: frame %d of %d", what, frame, d->n);
  *P = &d->parsed[frame];
  return MIJ_OK;
}

// size and device pitch of the frame's pixels as the last reconstruct left them
static void rec_size(const mij_decoder *d, int frame, int *w, int *h, long long *pitch) {
  const Parsed &P = d->parsed[frame];
  if (d->rec_denom > 1) {
    *w = d->sgeom[frame].ow;
    *h = d->sgeom[frame].oh;
    *pitch = (3LL * *w + 15) / 16 * 16;
  } else {
    *w = P.w;
    *h = P.h;
    *pitch = d->loc[frame].foreign ? P.pitch() : 3LL * P.w;  // legacy widths: 3 * w is a multiple of 16 already
  }
}

extern "C" int mij_decoder_pixels(mij_decoder *d, int frame, uint8_t *dst, size_t cap, long long pitch) {
  mij_clear_error();
  const Parsed *P;
  if (int rc = rec_frame(d, frame, "decoder_pixels", &P)) return rc;
  if (!dst) return mij_fail(MIJ_EINVAL, "decoder_pixels: dst is NULL");
  int w, h;
  long long dpitch;
  rec_size(d, frame, &w, &h, &dpitch);
  const long long row = 3LL * w;
  if (pitch == 0) pitch = row;
  if (pitch < row) return mij_fail(MIJ_EINVAL, "decoder_pixels: pitch %lld < %lld", pitch, row);
  const unsigned long long need = (unsigned long long)(h - 1) * pitch + row;
  if (cap < need) return mij_fail(MIJ_ENOSPC, "decoder_pixels: need %llu bytes", need);
  HIP_TRY(hipSetDevice(d->dev));
  const FrameLoc &L = d->loc[frame];
  const uint8_t *src = (L.foreign ? d->f_pix : d->d_pix) + L.pix;
  HIP_TRY(hipMemcpy2DAsync(dst, (size_t)pitch, src, (size_t)dpitch, (size_t)row, h, hipMemcpyDeviceToHost,
                           d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return MIJ_OK;
}

extern "C" int mij_decoder_planes(mij_decoder *d, int frame, uint8_t *Y, uint8_t *Cb, uint8_t *Cr) {
  mij_clear_error();
  const Parsed *P;
  if (int rc = rec_frame(d, frame, "decoder_planes", &P)) return rc;
  if (!Y || !Cb || !Cr) return mij_fail(MIJ_EINVAL, "decoder_planes: NULL plane");
  if (d->rec_denom > 1)
    return mij_fail(MIJ_EINVAL, "decoder_planes: the last reconstruct was at 1/%d scale; use mij_decoder_scaled_layout "
                    "and mij_decoder_plane", d->rec_denom);
  if (d->loc[frame].foreign)
    return mij_fail(MIJ_EINVAL, "decoder_planes: frame %d is not of the encoder's layout; use mij_decoder_layout and "
                    "mij_decoder_plane", frame);
  HIP_TRY(hipSetDevice(d->dev));
  const long long ny = (long long)P->w * P->h;
  const uint8_t *src = d->d_planes + frame * (d->plane_px * 3 / 2);
  HIP_TRY(hipMemcpyAsync(Y, src, ny, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(Cb, src + ny, ny / 4, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(Cr, src + ny + ny / 4, ny / 4, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return MIJ_OK;
}

extern "C" int mij_decoder_plane(mij_decoder *d, int frame, int comp, uint8_t *dst, size_t cap) {
  mij_clear_error();
  const Parsed *P;
  if (int rc = rec_frame(d, frame, "decoder_plane", &P)) return rc;
  if (!dst) return mij_fail(MIJ_EINVAL, "decoder_plane: dst is NULL");
  if (comp < 0 || comp >= P->ncomp) return mij_fail(MIJ_EINVAL, "decoder_plane: component %d of %d", comp, P->ncomp);
  size_t nbytes = (size_t)64 * P->bw[comp] * P->bh[comp];
  if (d->rec_denom > 1) nbytes = (size_t)d->sgeom[frame].c[comp].pitch * d->sgeom[frame].c[comp].rows;
  if (cap < nbytes) return mij_fail(MIJ_ENOSPC, "decoder_plane: need %zu bytes", nbytes);
  HIP_TRY(hipSetDevice(d->dev));
  const FrameLoc &L = d->loc[frame];
  HIP_TRY(hipMemcpyAsync(dst, (L.foreign ? d->f_planes : d->d_planes) + L.off[comp], nbytes, hipMemcpyDeviceToHost,
                         d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return MIJ_OK;
}

extern "C" void *mij_decoder_device_pixels(mij_decoder *d, int frame, long long *pitch) {
  mij_clear_error();
  const Parsed *P;
  if (rec_frame(d, frame, "decoder_device_pixels", &P)) return nullptr;
  const FrameLoc &L = d->loc[frame];
  int w, h;
  long long dpitch;
  rec_size(d, frame, &w, &h, &dpitch);
  if (pitch) *pitch = dpitch;
  return (L.foreign ? d->f_pix : d->d_pix) + L.pix;
}

extern "C" int mij_decoder_reconstruct_ms(mij_decoder *d, float ms[2]) {
  mij_clear_error();
  if (!d || !ms) return mij_fail(MIJ_EINVAL, "decoder_reconstruct_ms: bad args");
  if (!d->rec_valid) return mij_fail(MIJ_EINVAL, "decoder_reconstruct_ms: no mij_decoder_reconstruct since the last decode");
  HIP_TRY(hipSetDevice(d->dev));
  HIP_TRY(hipEventSynchronize(d->rec_ev[2]));
  HIP_TRY(hipEventElapsedTime(&ms[0], d->rec_ev[0], d->rec_ev[1]));
  HIP_TRY(hipEventElapsedTime(&ms[1], d->rec_ev[1], d->rec_ev[2]));
  return MIJ_OK;
}

// ---------------------------------------------------------------------------
// lossless transcoding: host side
// ---------------------------------------------------------------------------
static long long round_to(long long v, long long m) { return (v + m - 1) / m * m; }

// One frame's output geometry: the source's own for a plain transcode, the
// transformed image's for mij_decoder_transform.
struct XfPlan {
  int bits = 0;                // mij::XF_T | XF_FH | XF_FV
  int w = 0, h = 0;            // SOF0's size
  int mcus_x = 0, mcus_y = 0;
  int hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1};
  int bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};  // the planes, in blocks
  int ox[3] = {0, 0, 0}, oy[3] = {0, 0, 0};  // the crop's offset in the source planes, in blocks
  uint8_t hv[3] = {0x11, 0x11, 0x11};        // SOF0's H/V bytes
};

// crop, then the edge rule, then the operation: decided from the markers
// alone, before any device work.  MIJ_EINVAL names the frame and the reason.
static int xf_plan(const Parsed &P, int op, int flags, const area_t *crop, int restart_rows, const char *who,
                   int frame, XfPlan &X) {
  static const char *const names[mij::XF_OPS] = {"NONE",       "FLIP_H", "FLIP_V", "TRANSPOSE",
                                                 "TRANSVERSE", "ROT90",  "ROT180", "ROT270"};
  if (op < 0 || op >= mij::XF_OPS) return mij_fail(MIJ_EINVAL, "%s: frame %d: unknown operation %d", who, frame, op);
  if (flags & ~MIJ_XF_TRIM) return mij_fail(MIJ_EINVAL, "%s: frame %d: unknown flag bits 0x%x", who, frame, flags);
  const int Mw = 8 * P.hmax, Mh = 8 * P.vmax;
  int x = 0, y = 0, w = P.w, h = P.h;
  if (crop) {
    x = crop->x, y = crop->y, w = crop->w, h = crop->h;
    if (w < 1 || h < 1) return mij_fail(MIJ_EINVAL, "%s: frame %d: empty crop %dx%d", who, frame, w, h);
    if (x < 0 || y < 0 || (long long)x + w > P.w || (long long)y + h > P.h)
      return mij_fail(MIJ_EINVAL, "%s: frame %d: crop %dx%d+%d+%d lies outside the %dx%d frame", who, frame, w, h, x,
                      y, P.w, P.h);
    if (x % Mw || y % Mh)
      return mij_fail(MIJ_EINVAL, "%s: frame %d: crop offset +%d+%d is not aligned to the %dx%d MCU", who, frame, x,
                      y, Mw, Mh);
  }
  X.bits = mij::xf_op_bits(op);
  const bool T = X.bits & mij::XF_T;
  if (T)
    for (int c = 0; c < P.ncomp; c++)
      if (P.hs[c] != P.vs[c])
        return mij_fail(MIJ_EINVAL, "%s: frame %d: %s of a component with sampling %dx%d: the transposed %dx%d is "
                        "not decodable here", who, frame, names[op], P.hs[c], P.vs[c], P.vs[c], P.hs[c]);
  // mirrors of the SOURCE: the output's top-bottom flip after a transpose is the source's left-right one
  const bool mir_h = X.bits & (T ? mij::XF_FV : mij::XF_FH), mir_v = X.bits & (T ? mij::XF_FH : mij::XF_FV);
  if (mir_h && w % Mw) {
    if (!(flags & MIJ_XF_TRIM))
      return mij_fail(MIJ_EINVAL, "%s: frame %d: %s mirrors the width %d, which is not whole MCUs of %d "
                      "(MIJ_XF_TRIM cuts it down)", who, frame, names[op], w, Mw);
    if (w < Mw)
      return mij_fail(MIJ_EINVAL, "%s: frame %d: %s with MIJ_XF_TRIM: nothing left of the width %d (MCUs of %d)",
                      who, frame, names[op], w, Mw);
    w = w / Mw * Mw;
  }
  if (mir_v && h % Mh) {
    if (!(flags & MIJ_XF_TRIM))
      return mij_fail(MIJ_EINVAL, "%s: frame %d: %s mirrors the height %d, which is not whole MCUs of %d "
                      "(MIJ_XF_TRIM cuts it down)", who, frame, names[op], h, Mh);
    if (h < Mh)
      return mij_fail(MIJ_EINVAL, "%s: frame %d: %s with MIJ_XF_TRIM: nothing left of the height %d (MCUs of %d)",
                      who, frame, names[op], h, Mh);
    h = h / Mh * Mh;
  }
  const int smx = (w + Mw - 1) / Mw, smy = (h + Mh - 1) / Mh;  // the kept MCUs, in the source's orientation
  X.w = T ? h : w;
  X.h = T ? w : h;
  X.mcus_x = T ? smy : smx;
  X.mcus_y = T ? smx : smy;
  for (int c = 0; c < P.ncomp; c++) {
    X.hs[c] = T ? P.vs[c] : P.hs[c];
    X.vs[c] = T ? P.hs[c] : P.vs[c];
    X.bw[c] = X.mcus_x * X.hs[c];
    X.bh[c] = X.mcus_y * X.vs[c];
    X.ox[c] = x / Mw * P.hs[c];  // ox + kept blocks across <= P.bw: x + w <= P.w <= mcus_x * Mw
    X.oy[c] = y / Mh * P.vs[c];
    X.hv[c] = T ? (uint8_t)((P.decl_hv[c] << 4) | (P.decl_hv[c] >> 4)) : P.decl_hv[c];
  }
  const long long ri = (long long)restart_rows * X.mcus_x;
  if (restart_rows < 0 || ri > 65535)
    return mij_fail(MIJ_EINVAL, "%s: frame %d: restart interval of %d rows x %d MCUs = %lld MCUs (0..65535)", who,
                    frame, restart_rows, X.mcus_x, ri);
  return MIJ_OK;
}

// Every frame of the last decode -> one interleaved baseline stream with the
// same coefficients, sampling and DQTs, tables optimised for it and restart
// intervals of restart_rows MCU rows.  Waits for the device twice: once for
// the frames' bits (they size the scan words and the output), once at the
// end for the lengths.
//
// The shared worker of mij_decoder_transcode and mij_decoder_transform (§4i):
// plans[f] is frame f's output geometry; with xform the stage k_xf_blocks
// writes transformed planes and absolute DCs between k_tc_abs and k_tc_hist
// and the TcFrames point at those, without it they point at the decoded
// planes and the plans are the source's own geometry.
static int tc_run(mij_decoder *d, int restart_rows, const XfPlan *plans, bool xform, const char *who) {
  const int n = d->n;
  HIP_TRY(hipSetDevice(d->dev));
  for (hipEvent_t &e : d->tc_ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  // the previous call's uploads read the vectors below: let them finish first
  HIP_TRY(hipStreamSynchronize(d->stream));
  d->tc_valid = false;
  // sizes of the per-call arrays
  // (src_nblk: the decoded planes' blocks; nblk, nmcu, nrows: the output's,
  // never more than the source's)
  long long src_nblk = 0, nblk = 0, nmcu = 0, nrows = 0, dcl = 0, dcf = 0, tiles_l = 0, tiles_f = 0;
  int ncl = 0, ncf = 0, max_nblk = 0, max_rows = 0, max_comp = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    const FrameLoc &L = d->loc[f];
    const XfPlan &X = plans[f];
    long long fb = 0;
    for (int c = 0; c < P.ncomp; c++) {
      const long long nb = (long long)P.bw[c] * P.bh[c];
      src_nblk += nb;
      fb += (long long)X.bw[c] * X.bh[c];
      (L.foreign ? dcf : dcl) = std::max(L.foreign ? dcf : dcl, L.off[c] / 64 + nb);
      (L.foreign ? tiles_f : tiles_l) += (nb + mij::DC_TILE - 1) / mij::DC_TILE;
      (L.foreign ? ncf : ncl)++;
      max_comp = (int)std::max<long long>(max_comp, nb);
    }
    nblk += fb;
    nmcu += (long long)X.mcus_x * X.mcus_y;
    nrows += X.mcus_y;
    max_nblk = (int)std::max<long long>(max_nblk, fb);
    max_rows = std::max(max_rows, X.mcus_y);
  }
  if (src_nblk > 0x7fff0000LL) return mij_fail(MIJ_EINVAL, "%s: too many blocks", who);
  const int ncomp = ncl + ncf;
#define TC_GROW(p, cnt)                                            \
  if (int rc = grow(d->p, d->p##_cap, (size_t)(cnt))) return rc
  TC_GROW(t_dcl, dcl);
  TC_GROW(t_dcf, dcf);
  TC_GROW(t_tile, tiles_l + tiles_f);
  TC_GROW(t_rec, ncomp);
  TC_GROW(t_dcjobs, ncomp);
  TC_GROW(t_abs, src_nblk);
  if (xform) {
    TC_GROW(x_plane, (size_t)nblk * 64);
    TC_GROW(x_abs, nblk);
    TC_GROW(x_frames, n);
    d->h_xframes.assign(n, mij::XfFrame());
  }
  TC_GROW(t_frames, n);
  TC_GROW(t_outs, n);
  TC_GROW(t_hist, (size_t)n * 4 * 257);
  TC_GROW(t_ehuf, (size_t)n * 1024);
  TC_GROW(t_hc, (size_t)n * 4);
  TC_GROW(t_blk_bits, nblk);
  TC_GROW(t_mcu_off, nmcu);
  TC_GROW(t_row_bits, nrows);
  TC_GROW(t_row_pre, nrows + n);
  TC_GROW(t_ival, nrows + n);
  TC_GROW(t_row_off, nrows + n);
  TC_GROW(t_bits, n);
  TC_GROW(t_hdr, n);
  TC_GROW(t_err, n);
  TC_GROW(t_len, n);
  // descriptors: the legacy frames' components first (k_il_dc runs once over
  // each of the two coefficient buffers), a legacy plane as a 1x1 scan of
  // MCUs one block wide that never resets
  d->h_trec.assign(ncomp, mij::IlRec());
  d->h_tdc.assign(ncomp, mij::TcDc());
  d->h_tframes.assign(n, mij::TcFrame());
  int il = 0, ifg = ncl;
  long long tl = 0, tf = 0, ab = 0, xb = 0, b0 = 0, m0 = 0, r0 = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    const FrameLoc &L = d->loc[f];
    const XfPlan &X = plans[f];
    mij::TcFrame &F = d->h_tframes[f];
    memset(&F, 0, sizeof F);
    F.ncomp = P.ncomp;
    F.mcus_x = X.mcus_x;
    F.mcus_y = X.mcus_y;
    F.R = restart_rows > 0 && restart_rows < X.mcus_y ? restart_rows : X.mcus_y;
    F.nint = (X.mcus_y + F.R - 1) / F.R;
    F.ri = restart_rows * X.mcus_x;
    F.blk0 = b0;
    F.mcu0 = (int)m0;
    F.row0 = (int)r0;
    F.rowp0 = (int)r0 + f;
    F.w = X.w;
    F.h = X.h;
    if (xform) {
      memset(&d->h_xframes[f], 0, sizeof(mij::XfFrame));
      d->h_xframes[f].ncomp = P.ncomp;
    }
    bool used[4] = {false, false, false, false};
    for (int c = 0; c < P.ncomp; c++) {
      const int nb = P.bw[c] * P.bh[c];
      const int k = L.foreign ? ifg++ : il++;
      long long &t0 = L.foreign ? tf : tl;
      mij::IlRec &j = d->h_trec[k];
      memset(&j, 0, sizeof j);
      j.off = L.off[c];
      j.nblocks = nb;
      j.bw = P.bw[c];
      j.tile0 = (int)t0;
      j.hs = L.foreign ? P.hs[c] : 1;
      j.vs = L.foreign ? P.vs[c] : 1;
      j.mcus_x = L.foreign ? P.mcus_x : P.bw[c];
      j.seg = L.foreign && P.ri ? (int)std::min<long long>((long long)P.ri * P.hs[c] * P.vs[c], nb) : nb;
      mij::TcDc &q = d->h_tdc[k];
      q.pre = (L.foreign ? d->t_dcf : d->t_dcl) + L.off[c] / 64;
      q.tile = d->t_tile + (L.foreign ? tiles_l : 0) + t0;
      q.abs = d->t_abs + ab;
      q.nblocks = nb;
      q.seg = j.seg;
      q.hs = j.hs;
      q.vs = j.vs;
      q.mcus_x = j.mcus_x;
      q.bw = j.bw;
      q.dc_tile = mij::DC_TILE;
      q.pad = 0;
      t0 += (nb + mij::DC_TILE - 1) / mij::DC_TILE;
      mij::TcComp &C = F.c[c];
      C.plane = (L.foreign ? d->f_coef : d->d_coef) + L.off[c];
      C.abs = q.abs;
      C.hs = X.hs[c];
      C.vs = X.vs[c];
      C.bw = X.bw[c];
      ab += nb;
      if (xform) {  // the stages after k_xf_blocks see its output
        mij::XfFrame &XF = d->h_xframes[f];
        mij::XfComp &K = XF.c[c];
        K.src = C.plane;
        K.src_abs = q.abs;
        K.dst = d->x_plane + 64 * xb;
        K.dst_abs = d->x_abs + xb;
        K.g.sbw = P.bw[c];
        K.g.dbw = X.bw[c];
        K.g.dbh = X.bh[c];
        K.g.ox = X.ox[c];
        K.g.oy = X.oy[c];
        K.g.bits = X.bits;
        K.blk0 = XF.nblk;
        XF.nblk += X.bw[c] * X.bh[c];
        C.plane = K.dst;
        C.abs = K.dst_abs;
        xb += (long long)X.bw[c] * X.bh[c];
      }
      F.bpm += X.hs[c] * X.vs[c];
      // SOF0's entry verbatim: a lone component keeps the sampling it declared,
      // which parse() replaced by 1x1 (P.decl_hv); X.hv is that byte, its
      // nibbles swapped by a transposing operation
      F.sof[c][0] = (uint8_t)P.cid[c];
      F.sof[c][1] = X.hv[c];
      F.sof[c][2] = (uint8_t)P.tq[c];
      if (!P.have_dqt[P.tq[c]]) return mij_fail(MIJ_EJPEG, "stream %d: DQT %d of component %d missing", f, P.tq[c], c);
      used[P.tq[c]] = true;
    }
    for (int t = 0; t < 4; t++)
      if (used[t]) {  // at most three components: at most three ids
        F.dqt_id[F.ndqt] = (uint8_t)t;
        // (transposed with the blocks)
        for (int z = 0; z < 64; z++) F.dqt[F.ndqt][z] = P.dqt[t][mij::xf_src_pos(X.bits, z)];
        F.ndqt++;
      }
    F.nblk = X.mcus_x * X.mcus_y * F.bpm;
    b0 += F.nblk;
    m0 += (long long)X.mcus_x * X.mcus_y;
    r0 += X.mcus_y;
  }
  if (xform)
    HIP_TRY(hipMemcpyAsync(d->x_frames, d->h_xframes.data(), n * sizeof(mij::XfFrame), hipMemcpyHostToDevice,
                           d->stream));
  HIP_TRY(hipMemcpyAsync(d->t_rec, d->h_trec.data(), ncomp * sizeof(mij::IlRec), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->t_dcjobs, d->h_tdc.data(), ncomp * sizeof(mij::TcDc), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->t_frames, d->h_tframes.data(), n * sizeof(mij::TcFrame), hipMemcpyHostToDevice,
                         d->stream));
  HIP_TRY(hipMemsetAsync(d->t_hist, 0, sizeof(uint32_t) * n * 4 * 257, d->stream));
  HIP_TRY(hipMemsetAsync(d->t_err, 0, sizeof(int) * n, d->stream));
  HIP_TRY(hipEventRecord(d->tc_ev[0], d->stream));
  // absolute DCs: the decoder's prefix sums over the source's scan order
  if (ncl) {
    hipLaunchKernelGGL(mij::k_il_dc, dim3((unsigned)tiles_l), dim3(mij::DC_T), 0, d->stream, d->t_rec, ncl, d->d_coef,
                       d->t_dcl, d->t_tile);
    hipLaunchKernelGGL(mij::k_dec_dcbase<mij::IlRec>, dim3((ncl + 63) / 64), dim3(64), 0, d->stream, d->t_rec, ncl,
                       d->t_tile);
  }
  if (ncf) {
    hipLaunchKernelGGL(mij::k_il_dc, dim3((unsigned)tiles_f), dim3(mij::DC_T), 0, d->stream, d->t_rec + ncl, ncf,
                       d->f_coef, d->t_dcf, d->t_tile + tiles_l);
    hipLaunchKernelGGL(mij::k_dec_dcbase<mij::IlRec>, dim3((ncf + 63) / 64), dim3(64), 0, d->stream, d->t_rec + ncl,
                       ncf, d->t_tile + tiles_l);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(mij::launch_tc_abs(d->t_dcjobs, ncomp, max_comp, d->stream));
  if (xform) HIP_TRY(mij::launch_xf_blocks(d->x_frames, n, max_nblk, d->stream));
  mij::TcArgs a;
  memset(&a, 0, sizeof a);
  a.fr = d->t_frames;
  a.o = d->t_outs;
  a.nframes = n;
  a.max_nblk = max_nblk;
  a.max_rows = max_rows;
  a.hist = d->t_hist;
  a.ehuf = d->t_ehuf;
  a.hc = d->t_hc;
  a.blk_bits = d->t_blk_bits;
  a.mcu_off = d->t_mcu_off;
  a.row_bits = d->t_row_bits;
  a.row_pre = d->t_row_pre;
  a.ival_off = d->t_ival;
  a.row_off = d->t_row_off;
  a.bits = d->t_bits;
  a.hdr = d->t_hdr;
  a.out_len = d->t_len;
  a.err = d->t_err;
  HIP_TRY(mij::launch_tc_hist(a, d->stream));
  mij::EntArgs e;  // k_tables_1w: one wave per table, all four of every frame
  memset(&e, 0, sizeof e);
  e.nframes = n;
  e.hist = d->t_hist;
  e.ehuf = d->t_ehuf;
  e.hc = d->t_hc;
  e.err = d->t_err;
  HIP_TRY(mij::launch_tables(e, d->stream));
  HIP_TRY(mij::launch_tc_sizes(a, d->stream));
  // the frames' bits size the scan words, the chunks and the output:
  // headers + entropy bytes, every one of them stuffed + markers + EOI
  std::vector<unsigned long long> bits(n);
  HIP_TRY(hipMemcpyAsync(bits.data(), d->t_bits, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  d->h_touts.assign(n, mij::TcOut());
  long long raw = 0, out = 0, chunks = 0, max_chunks = 0;
  for (int f = 0; f < n; f++) {
    mij::TcOut &O = d->h_touts[f];
    const long long nbytes = (long long)(bits[f] >> 3), nch = (nbytes + mij::TC_CH - 1) / mij::TC_CH;
    O.raw0 = raw;
    O.raw_words = round_to((long long)(bits[f] / 128 + 1) * 4, 64);
    O.out0 = out;
    O.out_cap = round_to(mij::TC_HDR_MAX + 2 * nbytes + 2LL * d->h_tframes[f].nint + 2, 256);
    O.chunk0 = chunks;
    raw += O.raw_words;
    out += O.out_cap;
    chunks += nch;
    max_chunks = std::max(max_chunks, nch);
  }
  TC_GROW(t_raw, raw);
  TC_GROW(t_out, out);
  TC_GROW(t_ffc, chunks + 1);
#undef TC_GROW
  HIP_TRY(hipMemcpyAsync(d->t_outs, d->h_touts.data(), n * sizeof(mij::TcOut), hipMemcpyHostToDevice, d->stream));
  a.max_chunks = (int)std::min<long long>(max_chunks, 1 << 20);
  a.raw = d->t_raw;
  a.ffc = d->t_ffc;
  a.out = d->t_out;
  HIP_TRY(mij::launch_tc_write(a, d->stream));
  HIP_TRY(hipEventRecord(d->tc_ev[1], d->stream));
  d->tc_len.assign(n, 0);
  d->tc_err.assign(n, 0);
  HIP_TRY(hipMemcpyAsync(d->tc_len.data(), d->t_len, n * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(d->tc_err.data(), d->t_err, n * sizeof(int), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  d->tc_valid = true;
  return MIJ_OK;
}

extern "C" int mij_decoder_transcode(mij_decoder *d, int restart_rows) {
  mij_clear_error();
  if (!d) return mij_fail(MIJ_EINVAL, "decoder_transcode: no decoder");
  if (d->n < 1) return mij_fail(MIJ_EINVAL, "decoder_transcode: no decoded frames");
  const int n = d->n;
  for (int f = 0; f < n; f++) {
    const long long ri = (long long)restart_rows * d->parsed[f].mcus_x;
    if (restart_rows < 0 || ri > 65535)
      return mij_fail(MIJ_EINVAL, "decoder_transcode: frame %d: restart interval of %d rows x %d MCUs = %lld MCUs "
                      "(0..65535)", f, restart_rows, d->parsed[f].mcus_x, ri);
  }
  std::vector<XfPlan> plans(n);
  for (int f = 0; f < n; f++)
    if (int rc = xf_plan(d->parsed[f], MIJ_XF_NONE, 0, nullptr, restart_rows, "decoder_transcode", f, plans[f]))
      return rc;
  return tc_run(d, restart_rows, plans.data(), false, "decoder_transcode");
}

// mij_decoder_transcode with a transform in front: the same
// operation, flags and crop for every frame of the last decode; one refused
// frame refuses the call before any device work.  MIJ_XF_NONE without a crop
// is the plain transcode.
extern "C" int mij_decoder_transform(mij_decoder *d, int op, int flags, const area_t *crop, int restart_rows) {
  mij_clear_error();
  if (!d) return mij_fail(MIJ_EINVAL, "decoder_transform: no decoder");
  if (d->n < 1) return mij_fail(MIJ_EINVAL, "decoder_transform: no decoded frames");
  const int n = d->n;
  std::vector<XfPlan> plans(n);
  for (int f = 0; f < n; f++)
    if (int rc = xf_plan(d->parsed[f], op, flags, crop, restart_rows, "decoder_transform", f, plans[f])) return rc;
  return tc_run(d, restart_rows, plans.data(), op != MIJ_XF_NONE || crop, "decoder_transform");
}

// the frame's stream once the last decode has been transcoded
static int tc_frame(mij_decoder *d, int frame, const char *what) {
  if (!d) return mij_fail(MIJ_EINVAL, "%s: no decoder", what);
  if (!d->tc_valid)
    return mij_fail(MIJ_EINVAL, "%s: no mij_decoder_transcode or mij_decoder_transform since the last decode", what);
  if (frame < 0 || frame >= d->n) return mij_fail(MIJ_EINVAL, "%s: frame %d of %d", what, frame, d->n);
  if (d->tc_err[frame]) return mij_frame_fail(d->tc_err[frame], what, frame);
  return MIJ_OK;
}

extern "C" int mij_decoder_transcoded(mij_decoder *d, int frame, uint8_t *dst, size_t cap, size_t *len) {
  mij_clear_error();
  if (len) *len = 0;
  if (int rc = tc_frame(d, frame, "decoder_transcoded")) return rc;
  const size_t nbytes = (size_t)d->tc_len[frame];
  if (len) *len = nbytes;
  if (cap < nbytes) return mij_fail(MIJ_ENOSPC, "decoder_transcoded: need %zu bytes", nbytes);
  if (!dst) return mij_fail(MIJ_EINVAL, "decoder_transcoded: dst is NULL");
  HIP_TRY(hipSetDevice(d->dev));
  HIP_TRY(hipMemcpyAsync(dst, d->t_out + d->h_touts[frame].out0, nbytes, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return MIJ_OK;
}

extern "C" void *mij_decoder_device_transcoded(mij_decoder *d, int frame, size_t *len) {
  mij_clear_error();
  if (len) *len = 0;
  if (tc_frame(d, frame, "decoder_device_transcoded")) return nullptr;
  if (len) *len = (size_t)d->tc_len[frame];
  return d->t_out + d->h_touts[frame].out0;
}

extern "C" int mij_decoder_transcode_ms(mij_decoder *d, float *ms) {
  mij_clear_error();
  if (!d || !ms) return mij_fail(MIJ_EINVAL, "decoder_transcode_ms: bad args");
  if (!d->tc_valid)
    return mij_fail(MIJ_EINVAL, "decoder_transcode_ms: no mij_decoder_transcode or mij_decoder_transform since the "
                    "last decode");
  HIP_TRY(hipSetDevice(d->dev));
  HIP_TRY(hipEventSynchronize(d->tc_ev[1]));
  HIP_TRY(hipEventElapsedTime(ms, d->tc_ev[0], d->tc_ev[1]));
  return MIJ_OK;
}

extern "C" void *mij_decoder_stream(mij_decoder *d) { return d ? (void *)d->stream : nullptr; }

extern "C" int mij_decode(const uint8_t *jpg, size_t len, int order, uint8_t *out, size_t cap, int *w, int *h) {
  mij_clear_error();
  if (!jpg || !out) return mij_fail(MIJ_EINVAL, "mij_decode: NULL buffer");
  if (order != MIJ_PIX_BGR && order != MIJ_PIX_RGB) return mij_fail(MIJ_EINVAL, "mij_decode: pixel order %d", order);
  Parsed P;  // the size first: the decoder is made for it
  if (int rc = parse(jpg, len, P, 0)) return mij_fail(rc, "mij_decode: %s", P.err);
  if (w) *w = P.w;
  if (h) *h = P.h;
  const unsigned long long need = 3ULL * P.w * P.h;
  if (cap < need) return mij_fail(MIJ_ENOSPC, "mij_decode: need %llu bytes", need);
  mij_decoder *d = mij_decoder_create(mij_drop_device(), (P.w + 15) / 16 * 16, (P.h + 15) / 16 * 16, 1);
  if (!d) return mij_last_error();
  int rc = mij_decoder_decode(d, &jpg, &len, 1);
  if (!rc) rc = mij_decoder_reconstruct(d, order);
  if (!rc) rc = mij_decoder_pixels(d, 0, out, cap, 0);
  decoder_free(d);  // (leaves the failure's message in place)
  return rc;
}

extern "C" int mij_decode_scaled(const uint8_t *jpg, size_t len, int order, int denom, uint8_t *out, size_t cap,
                                 int *w, int *h) {
  if (denom == 1) return mij_decode(jpg, len, order, out, cap, w, h);
  mij_clear_error();
  if (!jpg || !out) return mij_fail(MIJ_EINVAL, "mij_decode_scaled: NULL buffer");
  if (order != MIJ_PIX_BGR && order != MIJ_PIX_RGB)
    return mij_fail(MIJ_EINVAL, "mij_decode_scaled: pixel order %d", order);
  if (denom != 2 && denom != 4 && denom != 8)
    return mij_fail(MIJ_EINVAL, "mij_decode_scaled: scale 1/%d: 1/1, 1/2, 1/4 or 1/8", denom);
  Parsed P;
  if (int rc = parse(jpg, len, P, 0)) return mij_fail(rc, "mij_decode_scaled: %s", P.err);
  mij::ScaledGeom G;
  scaled_geom(P, denom, G);
  if (w) *w = G.ow;
  if (h) *h = G.oh;
  const unsigned long long need = 3ULL * G.ow * G.oh;
  if (cap < need) return mij_fail(MIJ_ENOSPC, "mij_decode_scaled: need %llu bytes", need);
  mij_decoder *d = mij_decoder_create(mij_drop_device(), (P.w + 15) / 16 * 16, (P.h + 15) / 16 * 16, 1);
  if (!d) return mij_last_error();
  int rc = mij_decoder_decode(d, &jpg, &len, 1);
  if (!rc) rc = mij_decoder_reconstruct_scaled(d, order, denom);
  if (!rc) rc = mij_decoder_pixels(d, 0, out, cap, 0);
  decoder_free(d);  // (leaves the failure's message in place)
  return rc;
}

extern "C" int mij_transcode(const uint8_t *jpg, size_t len, int restart_rows, uint8_t *out, size_t cap,
                             size_t *out_len) {
  mij_clear_error();
  if (out_len) *out_len = 0;
  if (!jpg || (!out && cap)) return mij_fail(MIJ_EINVAL, "mij_transcode: NULL buffer");
  Parsed P;  // the size first: the decoder is made for it
  if (int rc = parse(jpg, len, P, 0)) return mij_fail(rc, "mij_transcode: %s", P.err);
  if (restart_rows < 0 || (long long)restart_rows * P.mcus_x > 65535)
    return mij_fail(MIJ_EINVAL, "mij_transcode: frame 0: restart interval of %d rows x %d MCUs (0..65535 MCUs)",
                    restart_rows, P.mcus_x);
  mij_decoder *d = mij_decoder_create(mij_drop_device(), (P.w + 15) / 16 * 16, (P.h + 15) / 16 * 16, 1);
  if (!d) return mij_last_error();
  int rc = mij_decoder_decode(d, &jpg, &len, 1);
  if (!rc) rc = mij_decoder_transcode(d, restart_rows);
  if (!rc) rc = mij_decoder_transcoded(d, 0, out, cap, out_len);
  decoder_free(d);  // (leaves the failure's message in place)
  return rc;
}

extern "C" int mij_transform(const uint8_t *jpg, size_t len, int op, int flags, const area_t *crop, int restart_rows,
                             uint8_t *out, size_t cap, size_t *out_len) {
  mij_clear_error();
  if (out_len) *out_len = 0;
  if (!jpg || (!out && cap)) return mij_fail(MIJ_EINVAL, "mij_transform: NULL buffer");
  Parsed P;  // the size first: the decoder is made for it; and every refusal, before any device work
  if (int rc = parse(jpg, len, P, 0)) return mij_fail(rc, "mij_transform: %s", P.err);
  XfPlan X;
  if (int rc = xf_plan(P, op, flags, crop, restart_rows, "mij_transform", 0, X)) return rc;
  mij_decoder *d = mij_decoder_create(mij_drop_device(), (P.w + 15) / 16 * 16, (P.h + 15) / 16 * 16, 1);
  if (!d) return mij_last_error();
  int rc = mij_decoder_decode(d, &jpg, &len, 1);
  if (!rc) rc = mij_decoder_transform(d, op, flags, crop, restart_rows);
  if (!rc) rc = mij_decoder_transcoded(d, 0, out, cap, out_len);
  decoder_free(d);  // (leaves the failure's message in place)
  return rc;
}

// ---------------------------------------------------------------------------
// EXIF orientation (host only)
// ---------------------------------------------------------------------------
// The segments before SOS: the APP1 that begins "Exif\0\0", its TIFF header
// (II or MM), IFD0's tag 0x0112 (SHORT).  Every offset is checked against the
// segment; anything malformed or absent gives 1.
extern "C" int mij_exif_orientation(const uint8_t *jpg, size_t len) {
  if (!jpg || len < 4 || jpg[0] != 0xFF || jpg[1] != 0xD8) return 1;
  size_t i = 2;
  while (i + 4 <= len) {
    if (jpg[i] != 0xFF) return 1;
    const int m = jpg[i + 1];
    if (m == 0xFF) {  // fill byte
      i++;
      continue;
    }
    if (m == 0xDA || m == 0xD9) return 1;
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {  // no length
      i += 2;
      continue;
    }
    const size_t n = (size_t)be16(jpg + i + 2);
    if (n < 2 || i + 2 + n > len) return 1;
    const uint8_t *seg = jpg + i + 4;  // n - 2 bytes
    i += 2 + n;
    if (m != 0xE1 || n < 2 + 6 || memcmp(seg, "Exif\0\0", 6)) continue;
    const uint8_t *t = seg + 6;   // the TIFF header, where offsets count from
    const size_t tn = n - 2 - 6;  // its bytes inside the segment
    if (tn < 8) return 1;
    const bool le = t[0] == 'I' && t[1] == 'I';
    if (!le && !(t[0] == 'M' && t[1] == 'M')) return 1;
    auto u16 = [&](size_t o) { return le ? (unsigned)(t[o] | (t[o + 1] << 8)) : (unsigned)((t[o] << 8) | t[o + 1]); };
    auto u32 = [&](size_t o) { return le ? u16(o) | (u16(o + 2) << 16) : (u16(o) << 16) | u16(o + 2); };
    if (u16(2) != 42) return 1;
    const size_t ifd = u32(4);
    if (ifd > tn || tn - ifd < 2) return 1;
    const size_t cnt = u16(ifd);
    for (size_t k = 0; k < cnt; k++) {
      const size_t e = ifd + 2 + 12 * k;
      if (e > tn || tn - e < 12) return 1;
      if (u16(e) != 0x0112) continue;
      if (u16(e + 2) != 3 || u32(e + 4) != 1) return 1;  // one SHORT, held in the entry
      const unsigned v = u16(e + 8);
      return v >= 1 && v <= 8 ? (int)v : 1;
    }
    return 1;
  }
  return 1;
}

extern "C" int mij_orientation_op(int orientation) {
  static const int ops[9] = {MIJ_XF_NONE,      MIJ_XF_NONE,  MIJ_XF_FLIP_H,     MIJ_XF_ROT180, MIJ_XF_FLIP_V,
                             MIJ_XF_TRANSPOSE, MIJ_XF_ROT90, MIJ_XF_TRANSVERSE, MIJ_XF_ROT270};
  return orientation >= 1 && orientation <= 8 ? ops[orientation] : MIJ_XF_NONE;
}
