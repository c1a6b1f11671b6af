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
// padded to whole MCUs.  Both shapes go through the same kernels and share
// one arena: a one-component scan is an interleaved scan whose MCU is one
// block (DESIGN.md "Decoding ordinary baseline files").  Refused with MIJ_EJPEG and
// the reason: SOF1..15, 12-bit samples, 16-bit DQT, 2 or 4 components, Adobe
// RGB / YCCK, other sampling, further scans, Ss/Se/AhAl other than 0/63/0,
// missing tables, restart markers missing or out of order.  (c) Opt-in
// (mij_decoder_accept): progressive streams, parsed by mij_progressive.h and
// decoded by mij_progressive.hip into the same arena; this
// file stages their scans and describes the result as a frame of shape (b);
// and luma 1x2 (4:4:0, MIJ_ACCEPT_440), with which a
// transposing transform of a frame with H != V swaps them.
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
#include <memory>
#include <thread>
#include <vector>

#include "mij_host.h"
#include "mij_huff.h"
#include "mij_pixels.h"
#include "mij_progressive.h"
#include "mij_transcode.h"
#include "mij_progwrite.h"
#include "mij_transform.h"

#define HIP_TRY(x)                                                                 \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess)                                                          \
      return mij_fail(MIJ_EHIP, "%s failed: %s", #x, hipGetErrorString(e_));       \
  } while (0)

namespace mij {

// chunk c of a scan covers bits [c*CHUNK, (c+1)*CHUNK): a symbol belongs to
// the chunk its first bit lies in.  512: measured against 1024 / 2048 / 4096
// on 256 config-3 streams, 16.3 / 17.7 / 21.1 / 23.9 ms per decode call.
constexpr int CHUNK = 512;

// the last entry of a table sorted by KEY whose KEY is <= v (entry 0 if none is)
template <auto KEY, class T>
__device__ __forceinline__ int last_le(const T *tab, int n, int v) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].*KEY <= v) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ---------------------------------------------------------------------------
// Entropy decoding (DESIGN.md "Decoding ordinary baseline files").  A scan
// holds MCUs of up to 6 blocks, cut into restart intervals; a one-component
// scan (the encoder's streams hold three) is a scan whose MCU is one block:
// bpm == 1, hs == vs == 1, mcus_x == bw, never reset.  An interval has its
// own zero-padded slot of the blob, its own chunks and an exact entry (first
// bit, k 0, slot 0) for its first chunk.  A chunk's state is (bit position,
// coefficient index k, block slot within the MCU); the Huffman tables follow
// the slot.
//
// Bounds, whatever the bits say.  Reads: a window is taken only at pos <
// stop <= nbits and covers words pos/64 and pos/64 + 1, i.e. at most 15
// bytes past the interval's last byte; every slot ends in >= 16 zero bytes.
// States: k leaves a span in 0..63 (a run past 63 is "bad", ZRL / EOB end
// the block), slot in 0..bpm-1 (only ever stepped modulo bpm), and a state
// is only ever produced by these kernels.  Stores: k_dec_write stores block
// b of interval i only while b < nmcus_i * bpm, to MCU mcu0_i + b / bpm <
// the scan's MCU count (the host checks mcu0_i + nmcus_i <= mcus_x *
// mcus_y before any launch), at a position inside that MCU (slot_x < h_c,
// slot_y < v_c), hence inside the component's padded plane; b itself comes
// from the prefix sum and is checked >= 0 and congruent to the entry slot
// first.  A one-component scan is the case bpm == 1: the slot is always 0,
// block b < nmcus is MCU b, and it is stored at raster block b of a plane of
// bw * bh == nmcus blocks.  A stream that breaks any of this ends in a
// status code.
// ---------------------------------------------------------------------------
struct DecScan {
  long long off[3];  // first int16 of each of its components' padded planes
  int ncomp, bpm;    // blocks per MCU; bpm == 1 implies hs == vs == 1 and bw == mcus_x
  int mcus_x, nmcus;
  int chunk0, nchunks;  // all chunks of the scan's intervals, contiguous
  int hs[3], vs[3], bw[3];
  int dc[3], ac[3];  // table indices per component
  int slot_comp[6], slot_x[6], slot_y[6];
};

struct DecIvl {         // one restart interval (a whole scan without DRI)
  long long data;       // byte offset of the UNSTUFFED interval in the blob (8-aligned)
  long long nbits;      // its length in bits (the pad bits included)
  int scan;             // index into the DecScan table
  int mcu0, nmcus;
  int chunk0, nchunks;  // global ids of the interval's chunks
  int pad;
};

struct DecArgs {
  const uint8_t *blob;
  const DecIvl *jobs;
  const DecScan *scans;
  int njobs;
  int chunk0, chunk1;  // the chunks this launch covers
  const DecTab *tabs;
  long long *entry_pos, *exit_in, *exit_out;  // (pos * 8 + slot) * 64 + k
  int *nblk;
  int *changed;
  int first;
};

__device__ __forceinline__ long long pack_state(long long pos, int slot, int k) { return (pos * 8 + slot) * 64 + k; }

// Self-synchronising pass (Weissenberger & Schmidt, ICPP 2018): chunk c
// decodes from its entry state to its end.  First pass: every chunk starts
// at its first bit as if an MCU began there (exact for chunk 0 of an
// interval).  Later passes: the entry of chunk c is the exit of chunk c-1
// from the previous pass; a chunk whose entry, slot included, did not change
// keeps its result.  Huffman streams resynchronise within a few symbols, so
// 2-3 passes settle.
//
// ONE (this kernel and k_dec_write): every chunk of the launch belongs to a
// scan of one-block MCUs.  The host puts those scans' chunks first and
// launches them apart, so that slot 0, bpm 1 and the scan's one pair of
// tables are compile-time facts there: the same source measured 6 % (this
// kernel) and 10 % (k_dec_write) slower on the encoder's streams with them
// read per block.
template <bool ONE>
__global__ __launch_bounds__(256) void k_dec_sync(DecArgs a) {
  const int c = a.chunk0 + blockIdx.x * 256 + threadIdx.x;
  if (c >= a.chunk1) return;
  const DecIvl &job = a.jobs[last_le<&DecIvl::chunk0>(a.jobs, a.njobs, c)];
  const int lc = c - job.chunk0;
  long long entry;
  if (a.first || lc == 0) {
    entry = pack_state((long long)lc * CHUNK, 0, 0);
    if (!a.first) {
      a.exit_out[c] = a.exit_in[c];
      return;
    }
  } else {
    entry = a.exit_in[c - 1];
    if (entry < 0) entry = pack_state((long long)lc * CHUNK, 0, 0);  // predecessor met a bad code
    if (entry == a.entry_pos[c]) {
      a.exit_out[c] = a.exit_in[c];
      return;
    }
    *a.changed = 1;
  }
  a.entry_pos[c] = entry;
  const DecScan &S = a.scans[job.scan];
  const int bpm = ONE ? 1 : S.bpm;
  Bits br{(const unsigned long long *)(a.blob + job.data)};
  long long pos = entry >> 9;
  int slot = ONE ? 0 : (int)(entry >> 6) & 7, k = (int)(entry & 63);
  const long long stop = min((long long)(lc + 1) * CHUNK, job.nbits);
  long long blocks_left = (long long)job.nmcus * bpm;
  int comp = ONE ? 0 : S.slot_comp[slot];
  const DecTab *dc = a.tabs + S.dc[comp], *ac = a.tabs + S.ac[comp];
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
      if (!ONE) {
        slot = slot + 1 == bpm ? 0 : slot + 1;
        comp = S.slot_comp[slot];
        dc = a.tabs + S.dc[comp];
        ac = a.tabs + S.ac[comp];
      }
    }
  }
  a.nblk[c] = started;
  a.exit_out[c] = bad ? -1 : pack_state(pos, slot, k);
}

// per scan (not per interval: a file may hold thousands of one-MCU
// intervals; one workgroup each, sequential over 256-chunk tiles): exclusive
// scan of its chunks' block counts across all its intervals.  k_dec_write
// takes differences against its interval's first chunk.
__global__ __launch_bounds__(256) void k_dec_scan(const DecScan *scans, const int *nblk, long long *base) {
  __shared__ long long part[256];
  const int chunk0 = scans[blockIdx.x].chunk0, nchunks = scans[blockIdx.x].nchunks;
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

// Scan-order block `slot` of MCU `mcu` lies in that component's padded plane
// at block row my * v_c + slot_y, block column mx * h_c + slot_x; for a
// one-block MCU (h_c == v_c == 1, bw == mcus_x) that is raster block `mcu`.
template <bool ONE>
__device__ __forceinline__ int16_t *scan_block(const DecScan &S, int16_t *coefs, int mcu, int slot, int comp) {
  if (ONE) return coefs + S.off[0] + 64LL * mcu;
  const int my = mcu / S.mcus_x, mx = mcu - my * S.mcus_x;
  return coefs + S.off[comp] +
         64 * ((long long)(my * S.vs[comp] + S.slot_y[slot]) * S.bw[comp] + mx * S.hs[comp] + S.slot_x[slot]);
}

// final pass: every chunk decodes from its settled entry and writes.  A
// lane assembles each block in its own LDS slot (128 B) and stores it whole
// (8 x 16 B, zeros included: no memset of the planes).  A block split
// between two chunks is stored in halves with 2-byte stores: the lane that
// started it writes positions [first, k_exit), the next lane [k_entry, 64)
// -- the settled states make k_exit == k_entry.  Scan-order block b of the
// interval lies in MCU mcu0 + b / bpm at slot b % bpm (scan_block).  A
// chunk that decodes the last block may go on through the pad bits; fewer
// blocks than the interval's MCUs need is a truncated stream.  status: one
// int per scan; 5 = an interval holds fewer blocks than its MCUs need, 6 =
// invalid code, 7 = the prefix sum and the settled slot disagree.
template <bool ONE>
__global__ __launch_bounds__(256) void k_dec_write(DecArgs a, const long long *base, int16_t *coefs, int *status) {
  __shared__ int4 slotbuf[256][8];
  const int c = a.chunk0 + blockIdx.x * 256 + threadIdx.x;
  if (c >= a.chunk1) return;
  const DecIvl &job = a.jobs[last_le<&DecIvl::chunk0>(a.jobs, a.njobs, c)];
  const DecScan &S = a.scans[job.scan];
  const int bpm = ONE ? 1 : S.bpm;
  const DecTab &dc1 = a.tabs[S.dc[0]], &ac1 = a.tabs[S.ac[0]];  // ONE: the scan's only tables
  const int lc = c - job.chunk0;
  const long long nblocks = (long long)job.nmcus * bpm;
  const long long lb = base[c] - base[job.chunk0];  // blocks the interval's earlier chunks started
  if (lc == job.nchunks - 1 && lb + a.nblk[c] < nblocks) atomicMax(&status[job.scan], 5);
  const long long entry = a.entry_pos[c];
  long long pos = entry >> 9;
  int slot = ONE ? 0 : (int)(entry >> 6) & 7, k = (int)(entry & 63);
  // the block in progress at the entry was started by an earlier chunk
  long long blk = lb - (k ? 1 : 0);
  if (blk >= nblocks) return;  // pad bits after the last block
  if (blk < 0 || (int)(blk % bpm) != slot) {
    atomicMax(&status[job.scan], 7);
    return;
  }
  int mcu = job.mcu0 + (int)(blk / bpm);
  Bits br{(const unsigned long long *)(a.blob + job.data)};
  const long long stop = min((long long)(lc + 1) * CHUNK, job.nbits);
  int4 *sl = slotbuf[threadIdx.x];
  int16_t *b16 = (int16_t *)sl;
#pragma unroll
  for (int q = 0; q < 8; q++) sl[q] = int4{0, 0, 0, 0};
  int first = k;
  bool bad = false;
  while (pos < stop && blk < nblocks) {
    const int comp = ONE ? 0 : S.slot_comp[slot];
    int sym, val;
    const int n = decode_one(br, pos, ONE ? (k ? ac1 : dc1) : a.tabs[k ? S.ac[comp] : S.dc[comp]], sym, val);
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
      int16_t *o = scan_block<ONE>(S, coefs, mcu, slot, comp);
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
      if (++slot == bpm) {
        slot = 0;
        mcu++;
      }
    }
  }
  if (!bad && k && blk < nblocks) {  // block continues in the next chunk
    int16_t *o = scan_block<ONE>(S, coefs, mcu, slot, ONE ? 0 : S.slot_comp[slot]);
    for (int t = first; t < k; t++) o[t] = b16[t];
  }
  if (bad) atomicMax(&status[job.scan], 6);
}

// ---------------------------------------------------------------------------
// Pixels (DESIGN.md "Decode to pixels", §4j for the reduced sizes): libjpeg's
// "islow" IDCT and its reduced IDCTs, "fancy" upsampling and fixed-point
// colour conversion, integer only, in two passes through uint8 planes:
// k_dec_dc + k_dec_dcbase (absolute DCs), k_dec_idct<S> (coefficients -> Y /
// Cb / Cr samples, S x S per block), k_dec_colour (samples -> packed 3-byte
// pixels).  The arithmetic itself is mij_pixels.h.
// The IDCT's sums run in uint32_t: streams no 8-bit image produces wrap
// instead of overflowing a signed type; encoder-made streams never wrap.
// ---------------------------------------------------------------------------
struct RecJob {      // one component of one frame
  long long off;     // first int16 of its coefficient plane == first byte of its sample plane
  int nblocks, bw, bh;  // padded plane: 8x8 blocks, blocks per row (mcus_x * h_c), block rows
  int wg0;           // its first workgroup in k_dec_idct's grid
  int qt;            // its quantiser: 64 ints (zigzag order) at q + 64 * qt
  int tile0;         // its first workgroup in k_dec_dc's grid == its first entry of the tile bases
  int hs, vs, mcus_x;  // its scan's order: blocks per MCU across and down, MCUs across
  int seg;           // blocks between DC resets: Ri * h_c * v_c, nblocks without DRI
  int pitch;         // bytes between the sample plane's rows
  int spr;           // strips of 8 samples per block row: ceil(bw * S / 8)
};

// Absolute DCs in two levels.  DC prediction runs per component in scan order
// (inside an MCU left-right, top-bottom, then the next MCU; raster order for a
// one-component scan) and starts again at 0 every restart interval, i.e.
// every `seg` blocks of the component.  A component's blocks are cut, in scan
// order, into tiles of DC_TILE; k_dec_dc, one 1024-lane workgroup per tile (so
// luma and chroma planes load the chip alike), writes the sum of differences
// 0..s relative to the tile (each lane DC_PER consecutive blocks, a shuffle
// scan per wave, the waves' totals through LDS) to dc[off / 64 + s] and the
// tile's total to tile[blockIdx.x]; k_dec_dcbase, one lane per plane, turns
// the totals into each tile's base.  With P(s) = dc + tile base, block s has
// absolute DC P(s) - P(first block of its segment - 1): two loads in
// k_dec_idct, no segmented scan.  All sums modulo 2^32.
constexpr int DC_T = 1024, DC_PER = 8, DC_TILE = DC_T * DC_PER;

// scan-order index -> raster index in the padded plane
__device__ __forceinline__ int scan_to_raster(const RecJob &j, int s) {
  const int hv = j.hs * j.vs, m = s / hv, i = s - m * hv;
  const int my = m / j.mcus_x, mx = m - my * j.mcus_x, iy = i / j.hs, ix = i - iy * j.hs;
  return (my * j.vs + iy) * j.bw + mx * j.hs + ix;
}

__global__ __launch_bounds__(DC_T) void k_dec_dc(const RecJob *jobs, int njobs, const int16_t *coefs, int32_t *dc,
                                                 uint32_t *tile) {
  __shared__ uint32_t wsum[DC_T / 64];
  const RecJob job = jobs[last_le<&RecJob::tile0>(jobs, njobs, blockIdx.x)];
  const int16_t *src = coefs + job.off;
  int32_t *dst = dc + job.off / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b0 = ((int)blockIdx.x - job.tile0) * DC_TILE + (int)threadIdx.x * DC_PER;
  uint32_t v[DC_PER], s = 0;
#pragma unroll
  for (int i = 0; i < DC_PER; i++) {
    if (b0 + i < job.nblocks) s += (uint32_t)(int32_t)src[64LL * scan_to_raster(job, b0 + i)];
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
__global__ __launch_bounds__(64) void k_dec_dcbase(const RecJob *jobs, int njobs, uint32_t *tile) {
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

// the absolute DC of raster block blk.  A 1x1 component's scan order is the
// raster order (bw == mcus_x); without DC resets the segment begins at 0.
// RASTER: the host found both true of every job of the launch (hs * vs == 1,
// seg >= nblocks), so the rule is one prefix sum at blk < nblocks.
//
// DC range: the absolute DC is the sum of the coded
// differences modulo 2^16, as int16 -- the value mij_decoder_component
// reports and the transcoder codes (k_tc_abs) -- so the pixels are those of
// the planes also where a stream's sums leave int16, which no 8-bit image's
// do.  dc16 sign-extends the low half of the 32-bit sum.
__device__ __forceinline__ uint32_t dc16(uint32_t v) { return (uint32_t)(int32_t)(int16_t)v; }

template <bool RASTER>
__device__ __forceinline__ uint32_t rec_dc(const RecJob &j, const int32_t *pd, const uint32_t *tile, int blk) {
  if (RASTER) return dc16((uint32_t)pd[blk] + tile[j.tile0 + blk / DC_TILE]);
  int s = blk;
  if (j.hs * j.vs > 1) {
    const int by = blk / j.bw, bx = blk - by * j.bw;
    const int my = by / j.vs, iy = by - my * j.vs, mx = bx / j.hs, ix = bx - mx * j.hs;
    s = (my * j.mcus_x + mx) * (j.hs * j.vs) + iy * j.hs + ix;
  }
  const int s0 = j.seg >= j.nblocks ? 0 : s / j.seg * j.seg;
  uint32_t v = (uint32_t)pd[s] + tile[j.tile0 + s / DC_TILE];
  if (s0 > 0) v -= (uint32_t)pd[s0 - 1] + tile[j.tile0 + (s0 - 1) / DC_TILE];
  return dc16(v);
}

// A component whose blocks become S x S samples (8 at full size; at 1/2, 1/4
// and 1/8 scale mij_pixels.h scaled_geometry says which) goes into a plane
// whose rows are S * bw rounded up to 8 bytes apart, at the place its
// full-size plane takes.
//
// One lane stores a strip: the 8 / S horizontally adjacent blocks of one
// block row that make 8 output samples, so every row leaves as one aligned
// 8-byte store.  A workgroup takes 256 * S / 8 consecutive strips, i.e. at
// most 256 blocks, consecutive in raster order also where a block row ends
// in a partial strip.  Its up to 32 KiB of coefficients come in with
// coalesced 16-byte loads and are staged in LDS, a block's 8 int4 in a slot
// of 9 (a lane's 16-byte reads then fall on distinct bank groups).  S == 8:
// strip == block (spr == bw); the lane dequantises into natural order (all
// indices compile-time: registers), runs the column pass (descale 11) and
// the row pass (descale 18).  S == 4 and 2: every lane runs the IDCT of one
// block (so none idles), leaves its S rows in LDS, in the staging area once
// every lane has read its coefficients, and the strip lanes gather them.
// S == 1 reads the DC buffers alone, 8 blocks per lane.
//
// Bounds.  A lane owns strip t < bh * spr of its component: block row by =
// t / spr, blocks bx0 = (8 / S) * sx .. of which only those < bw are read.
// Its S stores of 8 bytes go to rows S * by .. S * by + S - 1 < S * bh at
// byte 8 * sx, and 8 * sx + 8 <= 8 * spr == pitch, so each stays inside its
// row of the plane, which is pitch * S * bh <= 64 * bw * bh bytes: inside the
// slot of the full-size plane.  In LDS a workgroup's block b < nb <= 256
// has its staging slot at 9 * b int4 and its rows at words 256 * r + b,
// r < S <= 4: both inside the 256 * 9 int4.  Nothing is addressed from data.
// A one-component scan's plane is the case hs == vs == 1, mcus_x == bw, seg
// == nblocks: rec_dc reads entry blk < nblocks of its DC sums and no other.
//
// RASTER is launched at S == 8 only, over the planes that are coded in raster
// order and never reset their DCs (every plane of the encoder's streams, the
// 1x1 components of files without DRI).  With the rule decided per block at
// run time this kernel took 0.58 .. 0.62 ms on 64 three-scan 3840x2160
// frames, with it 0.54 .. 0.58.
template <int S, bool RASTER>
__global__ __launch_bounds__(256) void k_dec_idct(const RecJob *jobs, int njobs, const int16_t *coefs,
                                                  const int32_t *dc, const uint32_t *tile, const int32_t *q,
                                                  uint8_t *planes) {
  constexpr int PER = 8 / S, LANES = 256 / PER;
  __shared__ int4 stage[S > 1 ? 256 * 9 : 1];
  const RecJob job = jobs[last_le<&RecJob::wg0>(jobs, njobs, blockIdx.x)];
  const int spr = S == 8 ? job.bw : job.spr;  // S == 8: strip t is block t
  const int nstrips = job.bh * spr;
  const int t0 = ((int)blockIdx.x - job.wg0) * LANES, t1 = min(t0 + LANES, nstrips);
  const int by0 = S == 8 ? 0 : t0 / spr, first = S == 8 ? t0 : by0 * job.bw + (t0 - by0 * spr) * PER;
  const int32_t *pd = dc + job.off / 64;
  const int32_t *qz = q + 64 * job.qt;
  int nb = 0;  // the workgroup's blocks: <= 256
  if (S > 1) {
    const int by1 = S == 8 ? 0 : t1 / spr;
    const int last = S == 8 ? t1 : t1 == nstrips ? job.nblocks : by1 * job.bw + (t1 - by1 * spr) * PER;
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
      const uint32_t dc_abs = rec_dc<RASTER>(job, pd, tile, first + (int)threadIdx.x);
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
  const int by = t / spr, sx = t - by * spr;
  const int blk0 = S == 8 ? t : by * job.bw + sx * PER, nbl = S == 8 ? 1 : min(PER, job.bw - sx * PER);
  uint32_t out[S][2];
#pragma unroll
  for (int r = 0; r < S; r++) out[r][0] = out[r][1] = 0;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    if (k >= nbl) break;
    const int blk = blk0 + k;
    if constexpr (S == 1) {
      out[0][k >> 2] |= idct1_block(rec_dc<RASTER>(job, pd, tile, blk), qz[0]) << (8 * (k & 3));
    } else if constexpr (S == 8) {
      union {
        int4 v[8];
        int16_t c[64];
      } in;
#pragma unroll
      for (int j = 0; j < 8; j++) in.v[j] = stage[(blk - first) * 9 + j];
      idct_block(in.c, rec_dc<RASTER>(job, pd, tile, blk), qz, out);
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

struct RecPix {         // one frame
  long long y, cb, cr;  // first byte of each padded sample plane
  long long pix;        // first byte of the pixels, rows G.pitch apart
  PixGeom G;
  int groups, units;    // 16-pixel groups per row; rows or row pairs (colour_tile_any)
  int wg0, pad;         // its first workgroup in k_dec_colour's grid
};

// One lane per 16 x 1 or 16 x 2 output pixels (colour_tile_any, mij_pixels.h),
// a frame's tiles in raster order, 256 per workgroup; no workgroup spans two
// frames.
__global__ __launch_bounds__(256) void k_dec_colour(const RecPix *frames, int nframes, const uint8_t *planes,
                                                    uint8_t *pix, int rgb) {
  const RecPix fr = frames[last_le<&RecPix::wg0>(frames, nframes, blockIdx.x)];
  // (units * groups < 2^28: a frame is at most 65535 x 65535)
  const int idx = ((int)blockIdx.x - fr.wg0) * 256 + (int)threadIdx.x;
  if (idx >= fr.units * fr.groups) return;
  const int u = idx / fr.groups, g = idx - u * fr.groups;
  colour_tile_any(planes + fr.y, planes + fr.cb, planes + fr.cr, fr.G, u, g, rgb, pix + fr.pix);
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
  std::shared_ptr<mij::ProgFrame> prog;  // a progressive frame's scans (MIJ_ACCEPT_PROGRESSIVE); else null
  char err[200] = "";
  long long units() const {  // int16 coefficients == sample bytes of all padded planes
    long long u = 0;
    for (int c = 0; c < ncomp; c++) u += 64LL * bw[c] * bh[c];
    return u;
  }
  long long pitch() const { return (3LL * w + 15) / 16 * 16; }
};

int be16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

using mij::build_table;  // mij_huff.h

int parse_progressive(const uint8_t *s, size_t n, Parsed &P, int frame, unsigned accept);

// The stream's frame header, found by walking the segments in front of the
// first SOS (no rule of either stream kind is applied on the way): the SOFn
// marker's second byte and, if the segment is long enough, width and height;
// 0 if there is none.
int frame_header(const uint8_t *s, size_t n, int *w, int *h) {
  if (n < 4 || s[0] != 0xFF || s[1] != 0xD8) return 0;
  size_t i = 2;
  while (i + 4 <= n && s[i] == 0xFF) {
    const int m = s[i + 1];
    if (m == 0xFF) {
      i++;
      continue;
    }
    if (m == 0xD9 || m == 0xDA || (m >= 0xD0 && m <= 0xD7)) break;
    const size_t len = (size_t)((s[i + 2] << 8) | s[i + 3]);
    if (len < 2 || i + 2 + len > n) break;
    if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      if (len >= 7) {
        if (h) *h = (s[i + 5] << 8) | s[i + 6];
        if (w) *w = (s[i + 7] << 8) | s[i + 8];
      }
      return m;
    }
    i += 2 + len;
  }
  return 0;
}

// Host only (no device use): the message goes to P.err, since streams are
// parsed on worker threads; the caller reports it.  accept: MIJ_ACCEPT_*;
// with 0 (the one-shot calls, a decoder by default) SOF2 is refused below,
// and luma 1x2 (4:4:0, MIJ_ACCEPT_440) by both parsers.
// With MIJ_ACCEPT_PROGRESSIVE the frame type is found first, so that the
// segments in front of an SOF2 (a DHT with Th 2 or 3, say) are judged by the
// progressive rules from the start, never by the baseline ones.
int parse(const uint8_t *s, size_t n, Parsed &P, int frame, unsigned accept = 0) {
  if ((accept & MIJ_ACCEPT_PROGRESSIVE) && frame_header(s, n, nullptr, nullptr) == 0xC2)
    return parse_progressive(s, n, P, frame, accept);
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
        if (!(P.hs[0] <= 2 && P.vs[0] <= P.hs[0]) && !((accept & MIJ_ACCEPT_440) && P.hs[0] == 1 && P.vs[0] == 2)) {
          if (accept & MIJ_ACCEPT_440)
            BAD("stream %d: luma sampling %dx%d (only 1x1, 2x1, 2x2, 1x2)", frame, P.hs[0], P.vs[0]);
          BAD("stream %d: luma sampling %dx%d (only 1x1, 2x1, 2x2)", frame, P.hs[0], P.vs[0]);
        }
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

// A progressive stream (mij_progressive.h parses it and checks its scan
// script): afterwards P describes the frame as everything downstream of the
// entropy decoder expects an interleaved baseline frame without restart
// intervals, which is what the progressive kernels leave in the arena.
int parse_progressive(const uint8_t *s, size_t n, Parsed &P, int frame, unsigned accept) {
  P = Parsed();
  auto F = std::make_shared<mij::ProgFrame>();
  if (int rc = mij::prog_parse(s, n, *F, frame, (accept & MIJ_ACCEPT_440) != 0)) {
    memcpy(P.err, F->err, sizeof P.err);
    return rc;
  }
  P.w = F->w, P.h = F->h, P.ncomp = F->ncomp;
  P.hmax = F->hmax, P.vmax = F->vmax, P.mcus_x = F->mcus_x, P.mcus_y = F->mcus_y;
  for (int c = 0; c < 3; c++) {
    P.cid[c] = F->cid[c], P.hs[c] = F->hs[c], P.vs[c] = F->vs[c], P.tq[c] = F->tq[c];
    P.decl_hv[c] = F->decl_hv[c], P.bw[c] = F->bw[c], P.bh[c] = F->bh[c];
  }
  P.adobe = F->adobe;
  memcpy(P.dqt, F->dqt, sizeof P.dqt);
  memcpy(P.have_dqt, F->have_dqt, sizeof P.have_dqt);
  P.interleaved = true;
  P.ri = 0;
  P.prog = F;
  return MIJ_OK;
}

// where a frame of the last decode lives
struct FrameLoc {
  long long off[3] = {0, 0, 0};  // first int16 / sample byte of each component's plane
  long long pix = 0;             // first byte of its pixels
};

// The order a component's blocks were coded in, hence its DC prediction:
// inside an MCU of hs x vs blocks left-right, top-bottom, MCUs in raster
// order, the prediction starting again every seg blocks.  A one-component
// scan is a 1x1 scan of MCUs one block wide that never resets.
struct ScanGeom {
  int hs, vs, mcus_x, seg;
};

ScanGeom scan_geom(const Parsed &P, int c) {
  const int nb = P.bw[c] * P.bh[c];
  if (!P.interleaved) return {1, 1, P.bw[c], nb};
  const long long seg = P.ri ? std::min<long long>((long long)P.ri * P.hs[c] * P.vs[c], nb) : nb;
  return {P.hs[c], P.vs[c], P.mcus_x, (int)seg};
}

// at least `need` elements, and `floor` of them at the first allocation
template <class T>
int grow(T *&p, size_t &cap, size_t need, size_t floor = 0) {
  if (need <= cap) return MIJ_OK;
  hipFree(p);  // waits for the device
  p = nullptr;
  cap = 0;
  need = std::max(need, floor);
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
  mij::DecTab *d_tabs = nullptr;
  int *d_changed = nullptr;
  long long *d_entry = nullptr, *d_exit[2] = {nullptr, nullptr}, *d_base = nullptr;
  int *d_nblk = nullptr;
  int chunk_cap = 0, last_passes = 0;
  unsigned accept = 0;        // MIJ_ACCEPT_* (mij_decoder_accept)
  mij::ProgBuffers prog;      // the progressive path's buffers, allocated at its first use
  int prog_mapping = mij::PROG_MAP_WAVE;  // the faster of the two as measured
  std::vector<Parsed> parsed;
  std::vector<FrameLoc> loc;
  int n = 0;
  // One arena for every frame: planes padded to whole MCUs (the encoder's
  // shape has no padding), packed frame after frame in the order of the call.
  // A buffer's first allocation takes what max_frames frames of max_w x max_h
  // of the encoder's shape need (the coefficients' at create, the others' at
  // first use); it grows (is freed and allocated again) only when a call's
  // padded planes need more, so a decoder that only sees the encoder's
  // streams never reallocates.
  int16_t *d_coef = nullptr;
  uint8_t *d_planes = nullptr, *d_pix = nullptr;
  int32_t *d_dc = nullptr, *d_recq = nullptr;
  uint32_t *d_tile = nullptr;
  mij::DecIvl *d_jobs = nullptr;
  mij::DecScan *d_scans = nullptr;
  int *d_status = nullptr;
  mij::RecJob *d_rjobs = nullptr;
  mij::RecPix *d_rpix = nullptr;
  size_t d_coef_cap = 0, d_planes_cap = 0, d_pix_cap = 0, d_dc_cap = 0, d_recq_cap = 0, d_tile_cap = 0,
         d_jobs_cap = 0, d_scans_cap = 0, d_status_cap = 0, d_rjobs_cap = 0, d_rpix_cap = 0;
  long long pix_bytes = 0;  // of the last decode's frames
  // pixels (mij_decoder_reconstruct / _scaled)
  bool rec_valid = false;  // the planes and pixels are the last decode's
  int rec_denom = 1;       // of the last reconstruct
  std::vector<mij::ScaledGeom> sgeom;  // per frame, of the last reconstruct
  std::vector<mij::RecJob> h_rjobs;    // kept: the uploads are asynchronous
  std::vector<mij::RecPix> h_rpix;
  std::vector<int32_t> h_recq;
  hipEvent_t rec_ev[3] = {nullptr, nullptr, nullptr};
  // lossless transcoding (mij_decoder_transcode): everything allocated at its
  // first call and grown like the arena.  It keeps its own DC prefix sums, so
  // that it and reconstruct may run in either order, or alone.
  bool tc_valid = false;  // the streams below are the last decode's
  hipEvent_t tc_ev[2] = {nullptr, nullptr};
  int32_t *t_dc = nullptr;  // prefix sums of the arena's DCs
  uint32_t *t_tile = nullptr;
  mij::RecJob *t_rec = nullptr;
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
  size_t t_dc_cap = 0, t_tile_cap = 0, t_rec_cap = 0, t_dcjobs_cap = 0, t_abs_cap = 0, t_frames_cap = 0,
         t_outs_cap = 0, t_hist_cap = 0, t_ehuf_cap = 0, t_hc_cap = 0, t_blk_bits_cap = 0, t_mcu_off_cap = 0,
         t_row_bits_cap = 0, t_row_pre_cap = 0, t_ival_cap = 0, t_row_off_cap = 0, t_bits_cap = 0, t_raw_cap = 0,
         t_ffc_cap = 0, t_hdr_cap = 0, t_err_cap = 0, t_out_cap = 0, t_len_cap = 0;
  std::vector<mij::RecJob> h_trec;  // kept: the uploads are asynchronous
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
  // progressive output (mij_decoder_output): one entry per scan
  // of every frame; the other per-scan arrays are the transcoder's, grown
  int out_fmt = MIJ_OUT_BASELINE;
  mij::TcFrame *p_segs = nullptr;
  mij::PwScan *p_sc = nullptr;
  mij::PwFrame *p_pf = nullptr;
  mij::TcOut *p_souts = nullptr;
  uint8_t *p_info = nullptr;
  uint16_t *p_runlen = nullptr;
  int *p_perr = nullptr, *p_serr = nullptr;
  uint64_t *p_slen = nullptr;
  size_t p_segs_cap = 0, p_sc_cap = 0, p_pf_cap = 0, p_souts_cap = 0, p_info_cap = 0, p_runlen_cap = 0, p_perr_cap = 0,
         p_serr_cap = 0, p_slen_cap = 0;
  std::vector<mij::TcFrame> h_psegs;  // kept: the uploads are asynchronous
  std::vector<mij::PwScan> h_psc;
  std::vector<mij::PwFrame> h_ppf;
  std::vector<mij::TcOut> h_psouts;
  // what max_frames frames of max_w x max_h of the encoder's shape take: int16
  // coefficients == sample bytes, and components == scans
  size_t floor_units() const { return (size_t)cap * max_w * max_h * 3 / 2; }
  size_t floor_comps() const { return (size_t)cap * 3; }
};

static void decoder_free(mij_decoder *d) {
  if (!d) return;
  hipSetDevice(d->dev);
  if (d->stream) hipStreamSynchronize(d->stream);
  for (void *p : {(void *)d->d_blob, (void *)d->d_tabs, (void *)d->d_changed, (void *)d->d_entry, (void *)d->d_exit[0],
                  (void *)d->d_exit[1], (void *)d->d_nblk, (void *)d->d_base, (void *)d->d_coef, (void *)d->d_planes,
                  (void *)d->d_pix, (void *)d->d_dc, (void *)d->d_recq, (void *)d->d_tile, (void *)d->d_jobs,
                  (void *)d->d_scans, (void *)d->d_status, (void *)d->d_rjobs, (void *)d->d_rpix, (void *)d->t_dc,
                  (void *)d->t_tile, (void *)d->t_rec, (void *)d->t_dcjobs, (void *)d->t_abs, (void *)d->t_frames,
                  (void *)d->t_outs, (void *)d->t_hist, (void *)d->t_ehuf, (void *)d->t_hc, (void *)d->t_blk_bits,
                  (void *)d->t_mcu_off, (void *)d->t_row_bits, (void *)d->t_row_pre, (void *)d->t_ival,
                  (void *)d->t_row_off, (void *)d->t_bits, (void *)d->t_raw, (void *)d->t_ffc, (void *)d->t_hdr,
                  (void *)d->t_err, (void *)d->t_out, (void *)d->t_len, (void *)d->x_plane, (void *)d->x_abs,
                  (void *)d->x_frames, (void *)d->p_segs, (void *)d->p_sc, (void *)d->p_pf, (void *)d->p_souts,
                  (void *)d->p_info, (void *)d->p_runlen, (void *)d->p_perr, (void *)d->p_serr, (void *)d->p_slen})
    hipFree(p);
  mij::prog_free(d->prog);
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
  auto init = [&]() -> int {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    if (int rc = grow(d->d_coef, d->d_coef_cap, 1, d->floor_units())) return rc;
    HIP_TRY(hipMalloc((void **)&d->d_tabs, (size_t)max_frames * 4 * sizeof(mij::DecTab)));
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

static int decoder_buffers(mij_decoder *d, int nchunks) {
  if (nchunks <= d->chunk_cap) return MIJ_OK;
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

// which stream a scan belongs to, for the error text
struct ScanId {
  int stream;
  int scan;  // of a stream of one-component scans; -1: the stream's interleaved scan
};

// Every scan of the call: assigns the chunks, uploads the intervals and the
// scans, runs the passes until the chunk states settle, then the prefix sums
// and the writing pass.
static int decode_scans(mij_decoder *d, std::vector<mij::DecIvl> &jobs, std::vector<mij::DecScan> &scans,
                        const std::vector<ScanId> &ids) {
  const int nj = (int)jobs.size(), ns = (int)scans.size();
  // chunks [0, n1): the scans of one-block MCUs (k_dec_sync / k_dec_write <true>), then the others
  std::stable_partition(jobs.begin(), jobs.end(), [&](const mij::DecIvl &j) { return scans[j.scan].bpm == 1; });
  int nchunks = 0, n1 = 0, max_chunks = 1;
  for (auto &j : jobs) {
    mij::DecScan &S = scans[j.scan];
    if (S.nchunks == 0) S.chunk0 = nchunks;
    j.chunk0 = nchunks;
    nchunks += j.nchunks;
    S.nchunks += j.nchunks;
    max_chunks = std::max(max_chunks, j.nchunks);
    if (S.bpm == 1) n1 = nchunks;
  }
  bool any_il = false;  // an interleaved scan (a greyscale file's included) sets the passes' policy below
  for (const ScanId &id : ids) any_il |= id.scan < 0;
  if (int rc = decoder_buffers(d, nchunks)) return rc;
  if (int rc = grow(d->d_jobs, d->d_jobs_cap, (size_t)nj, d->floor_comps())) return rc;
  if (int rc = grow(d->d_scans, d->d_scans_cap, (size_t)ns, d->floor_comps())) return rc;
  if (int rc = grow(d->d_status, d->d_status_cap, (size_t)ns, d->floor_comps())) return rc;
  HIP_TRY(hipMemcpyAsync(d->d_jobs, jobs.data(), nj * sizeof(mij::DecIvl), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->d_scans, scans.data(), ns * sizeof(mij::DecScan), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemsetAsync(d->d_status, 0, ns * sizeof(int), d->stream));
  mij::DecArgs a{d->d_blob, d->d_jobs, d->d_scans, nj, 0, 0, d->d_tabs, d->d_entry, d->d_exit[1], d->d_exit[0],
                 d->d_nblk, d->d_changed, 1};
  // one launch per kind of chunk that the call holds
  auto both = [&](auto one, auto others, auto... more) {
    if (n1) {
      a.chunk0 = 0, a.chunk1 = n1;
      hipLaunchKernelGGL(one, dim3((n1 + 255) / 256), dim3(256), 0, d->stream, a, more...);
    }
    if (n1 < nchunks) {
      a.chunk0 = n1, a.chunk1 = nchunks;
      hipLaunchKernelGGL(others, dim3((nchunks - n1 + 255) / 256), dim3(256), 0, d->stream, a, more...);
    }
  };
  both(mij::k_dec_sync<true>, mij::k_dec_sync<false>);
  HIP_TRY(hipGetLastError());
  int cur = 0, passes = 1;
  for (;;) {
    // Every pass settles at least one more chunk of each interval, so the
    // bound below is never reached by a valid stream (badly synchronising
    // content, e.g. Q=100 noise with blocks longer than a chunk, only costs
    // more passes).  One-component scans settle in 2-3 passes and the host
    // looks after each.  The slot makes interleaved scans settle later (a
    // chunk may find the right bit and the wrong luma slot, which only the
    // next chroma block exposes), and a pass in which nothing changes costs
    // little, so with such a scan in the call the host looks only every
    // fourth pass after the first two.
    const int group = any_il && passes >= 3 ? 4 : 1;
    if (passes > max_chunks + 1 + (any_il ? group : 0))
      return mij_fail(MIJ_EJPEG, "decoder: chunk states did not settle");
    HIP_TRY(hipMemsetAsync(d->d_changed, 0, sizeof(int), d->stream));
    a.first = 0;
    for (int g = 0; g < group; g++, passes++) {
      a.exit_in = d->d_exit[cur];
      a.exit_out = d->d_exit[!cur];
      both(mij::k_dec_sync<true>, mij::k_dec_sync<false>);
      cur = !cur;
    }
    HIP_TRY(hipGetLastError());
    int changed = 0;
    HIP_TRY(hipMemcpyAsync(&changed, d->d_changed, sizeof(int), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    if (!changed) break;
  }
  // (a call of one-component scans alone has always reported its passes
  // without the last, which only confirms)
  d->last_passes = any_il ? passes : passes - 1;
  hipLaunchKernelGGL(mij::k_dec_scan, dim3(ns), dim3(256), 0, d->stream, d->d_scans, d->d_nblk, d->d_base);
  both(mij::k_dec_write<true>, mij::k_dec_write<false>, d->d_base, d->d_coef, d->d_status);
  HIP_TRY(hipGetLastError());
  std::vector<int> st(ns);
  HIP_TRY(hipMemcpyAsync(st.data(), d->d_status, ns * sizeof(int), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  for (int s = 0; s < ns; s++) {
    if (!st[s]) continue;
    if (ids[s].scan < 0) return mij_fail(MIJ_EJPEG, "stream %d: corrupt entropy data (%d)", ids[s].stream, st[s]);
    return mij_fail(MIJ_EJPEG, "stream %d scan %d: corrupt entropy data (%d)", ids[s].stream, ids[s].scan, st[s]);
  }
  return MIJ_OK;
}

// The progressive frames of the call: their planes zeroed,
// their units sorted by level and, inside a level, by scan, frame and
// interval, one launch per level (mij_progressive.hip), then the hand-over.
// piece0[f]: the first piece of frame f; at_len: every piece's blob offset
// and unstuffed length; a frame's pieces are its scans' intervals in order.
static int decode_progressive(mij_decoder *d, const std::vector<size_t> &piece0,
                              const std::vector<std::pair<long long, long long>> &at_len, long long arena_units) {
  const int n = (int)d->parsed.size();
  std::vector<mij::DecTab> tabs;
  std::vector<mij::ProgScanDev> scans;
  std::vector<mij::ProgUnit> units;
  std::vector<mij::ProgDcJob> dcjobs;
  struct Key {
    int level, ordinal, frame, ivl;
  };
  std::vector<Key> keys;
  std::vector<ScanId> ids;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    if (!P.prog) continue;
    const mij::ProgFrame &F = *P.prog;
    const FrameLoc &L = d->loc[f];
    HIP_TRY(hipMemsetAsync(d->d_coef + L.off[0], 0, (size_t)P.units() * sizeof(int16_t), d->stream));
    std::vector<size_t> first(F.scans.size() + 1, 0);  // of each scan's pieces, relative to the frame's
    for (size_t k = 0; k < F.scans.size(); k++) first[k + 1] = first[k] + F.scans[k].ivl.size();
    const size_t s0 = scans.size(), u0 = units.size();
    const int tab0 = (int)tabs.size();
    tabs.insert(tabs.end(), F.tabs.begin(), F.tabs.end());
    auto piece = [&](int k, int i, long long &at, long long &len) {
      const auto &pl = at_len[piece0[f] + first[k] + i];
      at = pl.first, len = pl.second;
    };
    if (mij::prog_tables(F, L.off, tab0, piece, scans, units))
      return mij_fail(MIJ_EJPEG, "stream %d: a restart interval has no MCUs", f);
    for (size_t k = 0; k < F.scans.size(); k++) ids.push_back({f, (int)k});
    for (size_t u = u0; u < units.size(); u++) {
      const int k = units[u].scan - (int)s0;
      keys.push_back({F.scans[k].level, k, f, (int)(u - u0 - first[k])});
    }
    for (int c = 0; c < P.ncomp; c++)
      dcjobs.push_back({L.off[c], P.bw[c] * P.bh[c], P.bw[c], P.hs[c], P.vs[c], P.mcus_x, 0});
  }
  if (units.empty()) return MIJ_OK;
  std::vector<int> order(units.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
  std::sort(order.begin(), order.end(), [&](int a, int b) {
    const Key &x = keys[a], &y = keys[b];
    if (x.level != y.level) return x.level < y.level;
    if (x.ordinal != y.ordinal) return x.ordinal < y.ordinal;
    if (x.frame != y.frame) return x.frame < y.frame;
    return x.ivl < y.ivl;
  });
  std::vector<mij::ProgUnit> sorted(units.size());
  std::vector<int> level_end;
  for (size_t i = 0; i < order.size(); i++) {
    sorted[i] = units[order[i]];
    const int lv = keys[order[i]].level;
    if ((int)level_end.size() < lv) level_end.resize(lv, (int)i);
    level_end[lv - 1] = (int)i + 1;
  }
  std::vector<int> st;
  if (int rc = mij::prog_run(d->stream, d->prog, d->d_blob, d->d_coef, arena_units / 64, tabs, scans, sorted, level_end,
                             dcjobs, d->prog_mapping, st))
    return rc;
  for (size_t s = 0; s < st.size(); s++)
    if (st[s])
      return mij_fail(MIJ_EJPEG, "stream %d scan %d: corrupt entropy data (%d)", ids[s].stream, ids[s].scan, st[s]);
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
  const unsigned accept = d->accept;
  parallel([&](int f) { prc[f] = parse(jpgs[f], lens[f], d->parsed[f], f, accept); });
  for (int f = 0; f < n; f++) {
    if (prc[f]) return mij_fail(prc[f], "decoder_decode: %s", d->parsed[f].err);
    const Parsed &P = d->parsed[f];
    if (P.w > d->max_w || P.h > d->max_h)
      return mij_fail(MIJ_EINVAL, "stream %d: %dx%d exceeds the decoder's %dx%d", f, P.w, P.h, d->max_w, d->max_h);
  }
  // pieces (a one-component scan, or one restart interval): raw length + >= 16 zero
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
    if (P.prog)
      for (const auto &sc : P.prog->scans)
        for (const auto &iv : sc.ivl) add(iv.data, iv.end);
    else if (P.interleaved)
      for (const auto &iv : P.ivl) add(iv.data, iv.end);
    else
      for (int k = 0; k < 3; k++) add(P.scan[k].data, P.scan[k].end);
  }
  piece0[n] = pieces.size();
  // chunk ids are ints: every piece has max(1, ceil(bits / 512)) chunks
  if (off / 64 + pieces.size() > 0x7fff0000u) return mij_fail(MIJ_EINVAL, "decoder_decode: too much entropy data");
  if (int rc = decoder_stage(d, off)) return rc;
  // the arena: every frame's padded planes and pixels, back to back
  long long units = 0, pixb = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    FrameLoc &L = d->loc[f];
    for (int c = 0; c < P.ncomp; c++) {
      L.off[c] = units;
      units += 64LL * P.bw[c] * P.bh[c];
    }
    L.pix = pixb;
    pixb += P.pitch() * P.h;
  }
  d->pix_bytes = pixb;
  if (int rc = grow(d->d_coef, d->d_coef_cap, (size_t)units, d->floor_units())) return rc;
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
  // one scan per stream, or its three one-component scans; one interval per piece
  std::vector<mij::DecScan> scans;
  std::vector<mij::DecIvl> jobs;
  std::vector<ScanId> ids;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    if (P.prog) continue;  // decode_progressive below
    const int nscans = P.interleaved ? 1 : 3;
    for (int k = 0; k < nscans; k++) {
      mij::DecScan S;
      memset(&S, 0, sizeof S);
      const int c0 = P.interleaved ? 0 : P.scan[k].comp;  // the scan's first component
      S.ncomp = P.interleaved ? P.ncomp : 1;
      for (int i = 0; i < S.ncomp; i++) {
        const int c = c0 + i;
        const ScanGeom g = scan_geom(P, c);
        S.off[i] = d->loc[f].off[c];
        S.hs[i] = g.hs;
        S.vs[i] = g.vs;
        S.bw[i] = P.bw[c];
        S.mcus_x = g.mcus_x;
        S.nmcus = P.bw[c] * P.bh[c] / (g.hs * g.vs);
        S.dc[i] = 4 * f + 2 * (P.interleaved ? P.td[c] : P.scan[k].td);
        S.ac[i] = 4 * f + 2 * (P.interleaved ? P.ta[c] : P.scan[k].ta) + 1;
        for (int y = 0; y < g.vs; y++)
          for (int x = 0; x < g.hs; x++) {  // at most 2 * 2 + 1 + 1 = 6: parse() admits no larger sampling
            S.slot_comp[S.bpm] = i;
            S.slot_x[S.bpm] = x;
            S.slot_y[S.bpm] = y;
            S.bpm++;
          }
      }
      const int ri = P.ri ? P.ri : S.nmcus;  // (parse() admits no DRI before one-component scans)
      const size_t p0 = piece0[f] + (P.interleaved ? 0 : k), np = P.interleaved ? P.ivl.size() : 1;
      for (size_t i = 0; i < np; i++) {
        const Piece &pc = pieces[p0 + i];
        mij::DecIvl j;
        j.data = (long long)pc.at;
        j.nbits = 8LL * (long long)pc.len;
        j.scan = (int)scans.size();
        // parse() made the interval count ceil(nmcus / ri), so mcu0 < nmcus and
        // mcu0 + nmcus_i <= nmcus: what bounds k_dec_write's stores
        j.mcu0 = (int)((long long)i * ri);
        j.nmcus = std::min(ri, S.nmcus - j.mcu0);
        j.chunk0 = 0;
        j.nchunks = chunks_of(j.nbits);
        j.pad = 0;
        if (j.mcu0 >= S.nmcus || j.nmcus < 1) return mij_fail(MIJ_EJPEG, "stream %d: restart interval %zu has no MCUs", f, i);
        jobs.push_back(j);
      }
      scans.push_back(S);
      ids.push_back({f, P.interleaved ? -1 : k});
    }
  }
  HIP_TRY(hipMemcpyAsync(d->d_blob, d->h_blob, off, hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->d_tabs, tabs.data(), tabs.size() * sizeof(mij::DecTab), hipMemcpyHostToDevice,
                         d->stream));
  d->last_passes = 0;  // counts self-synchronising passes only
  if (!scans.empty())
    if (int rc = decode_scans(d, jobs, scans, ids)) return rc;
  std::vector<std::pair<long long, long long>> at_len(pieces.size());
  for (size_t p = 0; p < pieces.size(); p++) at_len[p] = {(long long)pieces[p].at, (long long)pieces[p].len};
  if (int rc = decode_progressive(d, piece0, at_len, units)) return rc;
  d->n = n;
  return MIJ_OK;
}

extern "C" int mij_decoder_passes(mij_decoder *d) { return d ? d->last_passes : -1; }

extern "C" int mij_decoder_accept(mij_decoder *d, unsigned mask) {
  mij_clear_error();
  if (!d) return mij_fail(MIJ_EINVAL, "decoder_accept: null decoder");
  if (mask & ~(unsigned)(MIJ_ACCEPT_PROGRESSIVE | MIJ_ACCEPT_440)) return mij_fail(MIJ_EINVAL, "decoder_accept: unknown bits in mask 0x%X", mask);
  d->accept = mask;
  return MIJ_OK;
}

unsigned mij_decoder_accepted(mij_decoder *d) { return d ? d->accept : 0; }

extern "C" int mij_decoder_scan_info(mij_decoder *d, int frame, int *progressive, int *nscans, int *levels) {
  mij_clear_error();
  if (!d || frame < 0 || frame >= d->n) return mij_fail(MIJ_EINVAL, "decoder_scan_info: bad frame");
  const Parsed &P = d->parsed[frame];
  if (progressive) *progressive = P.prog ? 1 : 0;
  if (nscans) *nscans = P.prog ? (int)P.prog->scans.size() : P.interleaved ? 1 : 3;
  if (levels) *levels = P.prog ? P.prog->levels : 1;
  return MIJ_OK;
}

// test-only (mij_testing.h): the lane mapping of k_prog_scan, MIJ_PROG_MAP_*; returns the previous one
extern "C" int mij_test_prog_mapping(mij_decoder *d, int mapping) {
  if (!d || (mapping != mij::PROG_MAP_LANE && mapping != mij::PROG_MAP_WAVE)) return -2;
  const int was = d->prog_mapping;
  d->prog_mapping = mapping;
  return was;
}

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
  const Parsed &P = d->parsed[frame];
  if (!P.legacy)
    return mij_fail(MIJ_EINVAL, "decoder_coefs: frame %d is not of the encoder's layout; use mij_decoder_layout and "
                    "mij_decoder_component", frame);
  HIP_TRY(hipSetDevice(d->dev));
  const long long ny = (long long)P.w * P.h;
  const long long *off = d->loc[frame].off;
  HIP_TRY(hipMemcpyAsync(Y, d->d_coef + off[0], ny * 2, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(Cb, d->d_coef + off[1], ny / 2, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(Cr, d->d_coef + off[2], ny / 2, hipMemcpyDeviceToHost, d->stream));
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
  HIP_TRY(hipMemcpyAsync(dst, d->d_coef + d->loc[frame].off[comp], (size_t)(128 * nb), hipMemcpyDeviceToHost,
                         d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  const ScanGeom g = scan_geom(P, comp);
  const int hs = g.hs, vs = g.vs, mx_n = g.mcus_x, seg = g.seg;
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
  return d->d_coef + d->loc[frame].off[0];
}

// ---------------------------------------------------------------------------
// pixels: host side
// ---------------------------------------------------------------------------
static void scaled_geom(const Parsed &P, int denom, mij::ScaledGeom &G) {
  mij::scaled_geometry(P.w, P.h, P.ncomp, P.hs, P.vs, P.bw, P.bh, denom, G);
}

// denom 1: full size; 2, 4, 8: DESIGN.md §4j.  The absolute DCs, then every
// component through the IDCT of the size scaled_geometry gives it, then the
// colour stage on that geometry.
static int reconstruct(mij_decoder *d, int order, int denom) {
  mij_clear_error();
  if (!d) return mij_fail(MIJ_EINVAL, "decoder_reconstruct: no decoder");
  if (order != MIJ_PIX_BGR && order != MIJ_PIX_RGB)
    return mij_fail(MIJ_EINVAL, "decoder_reconstruct: pixel order %d", order);
  if (denom != 1 && denom != 2 && denom != 4 && denom != 8)
    return mij_fail(MIJ_EINVAL, "decoder_reconstruct_scaled: scale 1/%d: 1/1, 1/2, 1/4 or 1/8", denom);
  if (d->n < 1) return mij_fail(MIJ_EINVAL, "decoder_reconstruct: no decoded frames");
  HIP_TRY(hipSetDevice(d->dev));
  for (hipEvent_t &e : d->rec_ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  // the previous call's uploads read the vectors below: let them finish first
  HIP_TRY(hipStreamSynchronize(d->stream));
  d->rec_valid = false;
  const int n = d->n;
  d->sgeom.resize(n);
  d->h_recq.clear();
  d->h_rpix.clear();
  // the components' jobs in five runs: IDCT size 8 with the raster DC rule, then sizes 8, 4, 2, 1
  std::vector<mij::RecJob> run[5];
  long long wgs[5] = {0, 0, 0, 0, 0}, col = 0, units = 0, tiles = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    const FrameLoc &L = d->loc[f];
    mij::ScaledGeom &G = d->sgeom[f];
    scaled_geom(P, denom, G);
    for (int c = 0; c < P.ncomp; c++) {
      if (!P.have_dqt[P.tq[c]]) return mij_fail(MIJ_EJPEG, "stream %d: DQT missing", f);
      const ScanGeom g = scan_geom(P, c);
      mij::RecJob j;
      memset(&j, 0, sizeof j);
      j.off = L.off[c];
      j.bw = P.bw[c];
      j.bh = P.bh[c];
      j.nblocks = P.bw[c] * P.bh[c];
      j.qt = (int)(d->h_recq.size() / 64);
      for (int z = 0; z < 64; z++) d->h_recq.push_back(P.dqt[P.tq[c]][z]);
      j.hs = g.hs;
      j.vs = g.vs;
      j.mcus_x = g.mcus_x;
      j.seg = g.seg;
      // raster: the scan order is the plane's raster order and the DCs never reset
      const bool raster = g.hs * g.vs == 1 && g.seg >= j.nblocks;
      const int S = G.c[c].S, k = S == 8 ? (raster ? 0 : 1) : S == 4 ? 2 : S == 2 ? 3 : 4;
      j.pitch = G.c[c].pitch;
      j.spr = G.c[c].pitch / 8;
      j.wg0 = (int)wgs[k];
      wgs[k] += ((long long)j.bh * j.spr + 32 * S - 1) / (32 * S);  // 256 * S / 8 strips per workgroup
      units = std::max(units, j.off + 64LL * j.nblocks);
      run[k].push_back(j);
    }
    mij::RecPix px;
    memset(&px, 0, sizeof px);
    px.y = L.off[0];
    px.cb = L.off[P.ncomp > 1 ? 1 : 0];
    px.cr = L.off[P.ncomp > 1 ? 2 : 0];
    px.pix = L.pix;
    px.G = mij::pix_geometry(G);
    px.groups = (G.ow + 15) / 16;
    const int rows = mij::pix_rows_per_lane(G.mode);
    px.units = (G.oh + rows - 1) / rows;
    px.wg0 = (int)col;
    col += ((long long)px.units * px.groups + 255) / 256;
    d->h_rpix.push_back(px);
  }
  // one table: k_dec_dc walks all of it, so the tiles are numbered along it
  d->h_rjobs.clear();
  size_t first[5];
  for (int k = 0; k < 5; k++) {
    first[k] = d->h_rjobs.size();
    for (mij::RecJob &j : run[k]) {
      j.tile0 = (int)tiles;
      tiles += (j.nblocks + mij::DC_TILE - 1) / mij::DC_TILE;
      d->h_rjobs.push_back(j);
    }
    if (wgs[k] > 0x7fffffff) return mij_fail(MIJ_EINVAL, "decoder_reconstruct: too many blocks");
  }
  if (col > 0x7fffffff || tiles > 0x7fffffff) return mij_fail(MIJ_EINVAL, "decoder_reconstruct: too many blocks");
  const int nj = (int)d->h_rjobs.size();
  const size_t fu = d->floor_units(), fc = d->floor_comps();
  if (int rc = grow(d->d_planes, d->d_planes_cap, (size_t)units, fu)) return rc;
  if (int rc = grow(d->d_dc, d->d_dc_cap, (size_t)(units / 64), fu / 64)) return rc;
  // tiles: a plane of b blocks has at most b / DC_TILE + 1
  if (int rc = grow(d->d_tile, d->d_tile_cap, (size_t)tiles, fu / 64 / mij::DC_TILE + fc)) return rc;
  if (int rc = grow(d->d_pix, d->d_pix_cap, (size_t)d->pix_bytes, 2 * fu)) return rc;
  if (int rc = grow(d->d_recq, d->d_recq_cap, d->h_recq.size(), 64 * fc)) return rc;
  if (int rc = grow(d->d_rjobs, d->d_rjobs_cap, (size_t)nj, fc)) return rc;
  if (int rc = grow(d->d_rpix, d->d_rpix_cap, (size_t)n, (size_t)d->cap)) return rc;
  HIP_TRY(hipMemcpyAsync(d->d_rjobs, d->h_rjobs.data(), nj * sizeof(mij::RecJob), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->d_rpix, d->h_rpix.data(), n * sizeof(mij::RecPix), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->d_recq, d->h_recq.data(), d->h_recq.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                         d->stream));
  HIP_TRY(hipEventRecord(d->rec_ev[0], d->stream));
  hipLaunchKernelGGL(mij::k_dec_dc, dim3((unsigned)tiles), dim3(mij::DC_T), 0, d->stream, d->d_rjobs, nj, d->d_coef,
                     d->d_dc, d->d_tile);
  hipLaunchKernelGGL(mij::k_dec_dcbase, dim3((nj + 63) / 64), dim3(64), 0, d->stream, d->d_rjobs, nj, d->d_tile);
#define IDCT_LAUNCH(S, R, k)                                                                                \
  if (wgs[k])                                                                                               \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(mij::k_dec_idct<S, R>), dim3((unsigned)wgs[k]), dim3(256), 0, d->stream, \
                       d->d_rjobs + first[k], (int)run[k].size(), d->d_coef, d->d_dc, d->d_tile, d->d_recq,  \
                       d->d_planes)
  IDCT_LAUNCH(8, true, 0);
  IDCT_LAUNCH(8, false, 1);
  IDCT_LAUNCH(4, false, 2);
  IDCT_LAUNCH(2, false, 3);
  IDCT_LAUNCH(1, false, 4);
#undef IDCT_LAUNCH
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(d->rec_ev[1], d->stream));
  hipLaunchKernelGGL(mij::k_dec_colour, dim3((unsigned)col), dim3(256), 0, d->stream, d->d_rpix, n, d->d_planes,
                     d->d_pix, order == MIJ_PIX_RGB);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(d->rec_ev[2], d->stream));
  d->rec_denom = denom;
  d->rec_valid = true;
  return MIJ_OK;
}

extern "C" int mij_decoder_reconstruct(mij_decoder *d, int order) { return reconstruct(d, order, 1); }

extern "C" int mij_decoder_reconstruct_scaled(mij_decoder *d, int order, int denom) {
  return reconstruct(d, order, denom);
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
  *w = d->sgeom[frame].ow;
  *h = d->sgeom[frame].oh;
  *pitch = mij::pix_geometry(d->sgeom[frame]).pitch;
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
  HIP_TRY(hipMemcpy2DAsync(dst, (size_t)pitch, d->d_pix + d->loc[frame].pix, (size_t)dpitch, (size_t)row, h,
                           hipMemcpyDeviceToHost, d->stream));
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
  if (!P->legacy)
    return mij_fail(MIJ_EINVAL, "decoder_planes: frame %d is not of the encoder's layout; use mij_decoder_layout and "
                    "mij_decoder_plane", frame);
  HIP_TRY(hipSetDevice(d->dev));
  const long long ny = (long long)P->w * P->h;
  const long long *off = d->loc[frame].off;
  HIP_TRY(hipMemcpyAsync(Y, d->d_planes + off[0], ny, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(Cb, d->d_planes + off[1], ny / 4, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(Cr, d->d_planes + off[2], ny / 4, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return MIJ_OK;
}

extern "C" int mij_decoder_plane(mij_decoder *d, int frame, int comp, uint8_t *dst, size_t cap) {
  mij_clear_error();
  const Parsed *P;
  if (int rc = rec_frame(d, frame, "decoder_plane", &P)) return rc;
  if (!dst) return mij_fail(MIJ_EINVAL, "decoder_plane: dst is NULL");
  if (comp < 0 || comp >= P->ncomp) return mij_fail(MIJ_EINVAL, "decoder_plane: component %d of %d", comp, P->ncomp);
  const size_t nbytes = (size_t)d->sgeom[frame].c[comp].pitch * d->sgeom[frame].c[comp].rows;
  if (cap < nbytes) return mij_fail(MIJ_ENOSPC, "decoder_plane: need %zu bytes", nbytes);
  HIP_TRY(hipSetDevice(d->dev));
  HIP_TRY(hipMemcpyAsync(dst, d->d_planes + d->loc[frame].off[comp], nbytes, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return MIJ_OK;
}

extern "C" void *mij_decoder_device_pixels(mij_decoder *d, int frame, long long *pitch) {
  mij_clear_error();
  const Parsed *P;
  if (rec_frame(d, frame, "decoder_device_pixels", &P)) return nullptr;
  int w, h;
  long long dpitch;
  rec_size(d, frame, &w, &h, &dpitch);
  if (pitch) *pitch = dpitch;
  return d->d_pix + d->loc[frame].pix;
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
// accept: the decoder's MIJ_ACCEPT_* mask; with MIJ_ACCEPT_440 a transposing
// operation on a frame with H != V swaps every component's H and V (4:2:2 <->
// 4:4:0), which the decoder can then read back; without it
// the operation is refused.  The crop, trim and whole-MCU rules below use the
// source's MCU (Mw x Mh); the output's MCU is Mh x Mw after a transposition,
// so X.mcus_x / _y, hence restart_rows, count the output's grid.
static int xf_plan(const Parsed &P, int op, int flags, const area_t *crop, int restart_rows, const char *who,
                   int frame, XfPlan &X, unsigned accept = 0) {
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
  if (T && !(accept & MIJ_ACCEPT_440))
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

// ---------------------------------------------------------------------------
// progressive output: host side
// ---------------------------------------------------------------------------
// the scan's own MCU grid: the frame's for an interleaved scan, the blocks
// that cover component c's own samples otherwise
static void pw_grid(const Parsed &P, const XfPlan &X, int comps, int &ux, int &uy) {
  if (P.ncomp == 1) comps = 1;  // (its DC scans too are scans of component 0 alone)
  if (comps == 7) {
    ux = X.mcus_x;
    uy = X.mcus_y;
    return;
  }
  const int c = comps == 1 ? 0 : comps == 2 ? 1 : 2;
  int hmax = 1, vmax = 1;
  for (int k = 0; k < P.ncomp; k++) {
    hmax = std::max(hmax, X.hs[k]);
    vmax = std::max(vmax, X.vs[k]);
  }
  const int wc = (int)(((long long)X.w * X.hs[c] + hmax - 1) / hmax), hc = (int)(((long long)X.h * X.vs[c] + vmax - 1) / vmax);
  ux = (wc + 7) / 8;  // <= mcus_x * hs
  uy = (hc + 7) / 8;
}

// restart_rows rows of every scan's own MCUs must fit a DRI: before any device work
static int pw_check(const Parsed &P, const XfPlan &X, int restart_rows, const char *who, int frame) {
  for (const mij::PwScript &K : mij::PW_SCRIPT) {
    if (P.ncomp == 1 && !(K.comps & 1)) continue;
    int ux, uy;
    pw_grid(P, X, K.comps, ux, uy);
    const long long ri = (long long)restart_rows * ux;
    if (restart_rows < 0 || ri > 65535)
      return mij_fail(MIJ_EINVAL, "%s: frame %d: restart interval of %d rows x %d MCUs = %lld MCUs in the scan Ss %d Se %d "
                      "Ah %d Al %d (0..65535)", who, frame, restart_rows, ux, ri, K.ss, K.se, K.ah, K.al);
  }
  return MIJ_OK;
}

// tc_run's second half when the decoder writes progressive files: the planes
// and absolute DCs the frames' TcFrames point at (d->h_tframes, uploaded to
// d->t_frames) become the scans of mij::PW_SCRIPT.  Waits for the device
// twice, as tc_run does.
static int pw_run(mij_decoder *d, int restart_rows, const XfPlan *plans, const char *who) {
  const int n = d->n;
  d->h_psegs.clear();
  d->h_psc.clear();
  d->h_ppf.assign(n, mij::PwFrame());
  long long b0 = 0, m0 = 0, r0 = 0;
  int npf = 0, max_nblk = 0, max_rows = 0, max_nint = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    const XfPlan &X = plans[f];
    const mij::TcFrame &F = d->h_tframes[f];
    mij::PwFrame &Q = d->h_ppf[f];
    memset(&Q, 0, sizeof Q);
    Q.seg0 = (int)d->h_psegs.size();
    Q.pf0 = npf;
    int ntab = 0;
    for (const mij::PwScript &K : mij::PW_SCRIPT) {
      if (P.ncomp == 1 && !(K.comps & 1)) continue;
      const bool il = P.ncomp > 1 && K.comps == 7;
      mij::TcFrame G;
      memset(&G, 0, sizeof G);
      mij::PwScan S;
      memset(&S, 0, sizeof S);
      pw_grid(P, X, K.comps, G.mcus_x, G.mcus_y);
      if (il) {
        for (int c = 0; c < 3; c++) G.c[c] = F.c[c];
        G.ncomp = F.ncomp;
        G.bpm = F.bpm;
      } else {
        S.comp = P.ncomp == 1 || K.comps == 1 ? 0 : K.comps == 2 ? 1 : 2;
        G.c[0] = F.c[S.comp];
        G.c[0].hs = G.c[0].vs = 1;  // (bw stays the padded plane's stride)
        G.ncomp = 1;
        G.bpm = 1;
      }
      G.R = restart_rows > 0 && restart_rows < G.mcus_y ? restart_rows : G.mcus_y;
      G.nint = (G.mcus_y + G.R - 1) / G.R;
      G.ri = restart_rows * G.mcus_x;
      G.nblk = G.mcus_x * G.mcus_y * G.bpm;
      G.blk0 = b0;
      G.mcu0 = (int)m0;
      G.row0 = (int)r0;
      G.rowp0 = (int)r0 + (int)d->h_psegs.size();
      S.frame = f;
      S.ss = K.ss;
      S.se = K.se;
      S.ah = K.ah;
      S.al = K.al;
      S.ncomp = il ? P.ncomp : 1;
      S.ntab = K.ss == 0 ? (K.ah ? 0 : il ? 2 : 1) : 1;
      for (int t = 0; t < S.ntab; t++) S.tab[t] = 4 * Q.pf0 + ntab++;
      S.first = Q.nseg == 0;
      b0 += G.nblk;
      m0 += (long long)G.mcus_x * G.mcus_y;
      r0 += G.mcus_y;
      max_nblk = std::max(max_nblk, G.nblk);
      max_rows = std::max(max_rows, G.mcus_y);
      max_nint = std::max(max_nint, G.nint);
      d->h_psegs.push_back(G);
      d->h_psc.push_back(S);
      Q.nseg++;
    }
    Q.ntab = ntab;
    Q.npf = (ntab + 3) / 4;
    npf += Q.npf;
  }
  const int nseg = (int)d->h_psegs.size();
  if (b0 > 0x7fff0000LL || m0 + nseg > 0x7fff0000LL) return mij_fail(MIJ_EINVAL, "%s: too many blocks", who);
#define PW_GROW(p, cnt)                                            \
  if (int rc = grow(d->p, d->p##_cap, (size_t)(cnt))) return rc
  PW_GROW(p_segs, nseg);
  PW_GROW(p_sc, nseg);
  PW_GROW(p_pf, n);
  PW_GROW(p_souts, nseg);
  PW_GROW(p_info, b0);
  PW_GROW(p_runlen, b0);
  PW_GROW(p_perr, npf);
  PW_GROW(p_serr, nseg);
  PW_GROW(p_slen, nseg);
  PW_GROW(t_hist, (size_t)npf * 4 * 257);
  PW_GROW(t_ehuf, (size_t)npf * 1024);
  PW_GROW(t_hc, (size_t)npf * 4);
  PW_GROW(t_blk_bits, b0);
  PW_GROW(t_mcu_off, m0);
  PW_GROW(t_row_bits, r0);
  PW_GROW(t_row_pre, r0 + nseg);
  PW_GROW(t_ival, r0 + nseg);
  PW_GROW(t_row_off, r0 + nseg);
  PW_GROW(t_bits, nseg);
  PW_GROW(t_hdr, nseg);
  HIP_TRY(hipMemcpyAsync(d->p_segs, d->h_psegs.data(), nseg * sizeof(mij::TcFrame), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->p_sc, d->h_psc.data(), nseg * sizeof(mij::PwScan), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->p_pf, d->h_ppf.data(), n * sizeof(mij::PwFrame), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemsetAsync(d->t_hist, 0, sizeof(uint32_t) * npf * 4 * 257, d->stream));
  HIP_TRY(hipMemsetAsync(d->p_perr, 0, sizeof(int) * npf, d->stream));
  HIP_TRY(hipMemsetAsync(d->p_serr, 0, sizeof(int) * nseg, d->stream));
  mij::PwArgs a;
  memset(&a, 0, sizeof a);
  a.seg.fr = d->p_segs;
  a.seg.o = d->p_souts;
  a.seg.nframes = nseg;
  a.seg.max_nblk = max_nblk;
  a.seg.max_rows = max_rows;
  a.seg.hist = d->t_hist;
  a.seg.ehuf = d->t_ehuf;
  a.seg.hc = d->t_hc;
  a.seg.blk_bits = d->t_blk_bits;
  a.seg.mcu_off = d->t_mcu_off;
  a.seg.row_bits = d->t_row_bits;
  a.seg.row_pre = d->t_row_pre;
  a.seg.ival_off = d->t_ival;
  a.seg.row_off = d->t_row_off;
  a.seg.bits = d->t_bits;
  a.seg.hdr = d->t_hdr;
  a.seg.out_len = d->p_slen;
  a.seg.err = d->p_serr;
  a.sc = d->p_sc;
  a.pf = d->p_pf;
  a.fr = d->t_frames;
  a.nframes = n;
  a.max_nint = max_nint;
  a.info = d->p_info;
  a.runlen = d->p_runlen;
  a.perr = d->p_perr;
  a.ferr = d->t_err;
  a.flen = d->t_len;
  HIP_TRY(mij::launch_pw_count(a, d->stream));
  mij::EntArgs e;  // k_tables_1w: one wave per table, four per pseudo-frame
  memset(&e, 0, sizeof e);
  e.nframes = npf;
  e.hist = d->t_hist;
  e.ehuf = d->t_ehuf;
  e.hc = d->t_hc;
  e.err = d->p_perr;
  HIP_TRY(mij::launch_tables(e, d->stream));
  HIP_TRY(mij::launch_pw_sizes(a, d->stream));
  // the scans' bits size their words and chunks, and their sum the frame's
  // output: the header bound + every entropy byte stuffed + markers + EOI
  std::vector<unsigned long long> bits(nseg);
  HIP_TRY(hipMemcpyAsync(bits.data(), d->t_bits, nseg * sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  d->h_psouts.assign(nseg, mij::TcOut());
  d->h_touts.assign(n, mij::TcOut());
  long long raw = 0, out = 0, chunks = 0, max_chunks = 0;
  for (int f = 0; f < n; f++) {
    mij::PwFrame &Q = d->h_ppf[f];
    long long cap = mij::PW_HDR_MAX + 2;
    for (int s = Q.seg0; s < Q.seg0 + Q.nseg; s++) {
      mij::TcOut &O = d->h_psouts[s];
      const long long nbytes = (long long)(bits[s] >> 3), nch = (nbytes + mij::TC_CH - 1) / mij::TC_CH;
      O.raw0 = raw;
      O.raw_words = round_to((long long)(bits[s] / 128 + 1) * 4, 64);
      O.out0 = out;  // the frame's: k_pw_head gives each scan its offset (TcArgs::hdr)
      O.chunk0 = chunks;
      raw += O.raw_words;
      chunks += nch;
      max_chunks = std::max(max_chunks, nch);
      cap += 2 * nbytes + 2LL * d->h_psegs[s].nint;
    }
    cap = round_to(cap, 256);
    if (cap > 0x7fff0000LL) return mij_fail(MIJ_ENOSPC, "%s: frame %d: a stream of up to %lld bytes", who, f, cap);
    for (int s = Q.seg0; s < Q.seg0 + Q.nseg; s++) d->h_psouts[s].out_cap = cap;
    Q.out0 = out;
    Q.out_cap = cap;
    d->h_touts[f].out0 = out;
    d->h_touts[f].out_cap = cap;
    out += cap;
  }
  PW_GROW(t_raw, raw);
  PW_GROW(t_out, out);
  PW_GROW(t_ffc, chunks + 1);
#undef PW_GROW
  HIP_TRY(hipMemcpyAsync(d->p_souts, d->h_psouts.data(), nseg * sizeof(mij::TcOut), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->p_pf, d->h_ppf.data(), n * sizeof(mij::PwFrame), hipMemcpyHostToDevice, d->stream));
  a.seg.max_chunks = (int)std::min<long long>(max_chunks, 1 << 20);
  a.seg.raw = d->t_raw;
  a.seg.ffc = d->t_ffc;
  a.seg.out = d->t_out;
  HIP_TRY(mij::launch_pw_write(a, d->stream));
  HIP_TRY(hipEventRecord(d->tc_ev[1], d->stream));
  d->tc_len.assign(n, 0);
  d->tc_err.assign(n, 0);
  HIP_TRY(hipMemcpyAsync(d->tc_len.data(), d->t_len, n * sizeof(uint64_t), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(d->tc_err.data(), d->t_err, n * sizeof(int), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  d->tc_valid = true;
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
  long long src_nblk = 0, nblk = 0, nmcu = 0, nrows = 0, ndc = 0, tiles = 0;
  int ncomp = 0, max_nblk = 0, max_rows = 0, max_comp = 0;
  for (int f = 0; f < n; f++) {
    const Parsed &P = d->parsed[f];
    const FrameLoc &L = d->loc[f];
    const XfPlan &X = plans[f];
    long long fb = 0;
    for (int c = 0; c < P.ncomp; c++) {
      const long long nb = (long long)P.bw[c] * P.bh[c];
      src_nblk += nb;
      fb += (long long)X.bw[c] * X.bh[c];
      ndc = std::max(ndc, L.off[c] / 64 + nb);
      tiles += (nb + mij::DC_TILE - 1) / mij::DC_TILE;
      ncomp++;
      max_comp = (int)std::max<long long>(max_comp, nb);
    }
    nblk += fb;
    nmcu += (long long)X.mcus_x * X.mcus_y;
    nrows += X.mcus_y;
    max_nblk = (int)std::max<long long>(max_nblk, fb);
    max_rows = std::max(max_rows, X.mcus_y);
  }
  if (src_nblk > 0x7fff0000LL) return mij_fail(MIJ_EINVAL, "%s: too many blocks", who);
#define TC_GROW(p, cnt)                                            \
  if (int rc = grow(d->p, d->p##_cap, (size_t)(cnt))) return rc
  TC_GROW(t_dc, ndc);
  TC_GROW(t_tile, tiles);
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
  // descriptors: of a RecJob only what k_dec_dc and k_dec_dcbase read
  d->h_trec.assign(ncomp, mij::RecJob());
  d->h_tdc.assign(ncomp, mij::TcDc());
  d->h_tframes.assign(n, mij::TcFrame());
  int k = 0;
  long long t0 = 0, ab = 0, xb = 0, b0 = 0, m0 = 0, r0 = 0;
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
    for (int c = 0; c < P.ncomp; c++, k++) {
      const int nb = P.bw[c] * P.bh[c];
      const ScanGeom g = scan_geom(P, c);
      mij::RecJob &j = d->h_trec[k];
      memset(&j, 0, sizeof j);
      j.off = L.off[c];
      j.nblocks = nb;
      j.bw = P.bw[c];
      j.tile0 = (int)t0;
      j.hs = g.hs;
      j.vs = g.vs;
      j.mcus_x = g.mcus_x;
      j.seg = g.seg;
      mij::TcDc &q = d->h_tdc[k];
      q.pre = d->t_dc + L.off[c] / 64;
      q.tile = d->t_tile + t0;
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
      C.plane = d->d_coef + L.off[c];
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
  HIP_TRY(hipMemcpyAsync(d->t_rec, d->h_trec.data(), ncomp * sizeof(mij::RecJob), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->t_dcjobs, d->h_tdc.data(), ncomp * sizeof(mij::TcDc), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(d->t_frames, d->h_tframes.data(), n * sizeof(mij::TcFrame), hipMemcpyHostToDevice,
                         d->stream));
  HIP_TRY(hipMemsetAsync(d->t_hist, 0, sizeof(uint32_t) * n * 4 * 257, d->stream));
  HIP_TRY(hipMemsetAsync(d->t_err, 0, sizeof(int) * n, d->stream));
  HIP_TRY(hipEventRecord(d->tc_ev[0], d->stream));
  // absolute DCs: the decoder's prefix sums over the source's scan order
  hipLaunchKernelGGL(mij::k_dec_dc, dim3((unsigned)tiles), dim3(mij::DC_T), 0, d->stream, d->t_rec, ncomp, d->d_coef,
                     d->t_dc, d->t_tile);
  hipLaunchKernelGGL(mij::k_dec_dcbase, dim3((ncomp + 63) / 64), dim3(64), 0, d->stream, d->t_rec, ncomp, d->t_tile);
  HIP_TRY(hipGetLastError());
  HIP_TRY(mij::launch_tc_abs(d->t_dcjobs, ncomp, max_comp, d->stream));
  if (xform) HIP_TRY(mij::launch_xf_blocks(d->x_frames, n, max_nblk, d->stream));
  if (d->out_fmt == MIJ_OUT_PROGRESSIVE) return pw_run(d, restart_rows, plans, who);
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
    if (int rc = xf_plan(d->parsed[f], MIJ_XF_NONE, 0, nullptr, restart_rows, "decoder_transcode", f, plans[f], d->accept))
      return rc;
  if (d->out_fmt == MIJ_OUT_PROGRESSIVE)
    for (int f = 0; f < n; f++)
      if (int rc = pw_check(d->parsed[f], plans[f], restart_rows, "decoder_transcode", f)) return rc;
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
    if (int rc = xf_plan(d->parsed[f], op, flags, crop, restart_rows, "decoder_transform", f, plans[f], d->accept))
      return rc;
  if (d->out_fmt == MIJ_OUT_PROGRESSIVE)
    for (int f = 0; f < n; f++)
      if (int rc = pw_check(d->parsed[f], plans[f], restart_rows, "decoder_transform", f)) return rc;
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

// for the other host translation units (mij_host.h): the headers alone
int mij_parse_size(const char *what, const uint8_t *jpg, size_t len, int frame, int *w, int *h) {
  return mij_parse_size_accept(what, jpg, len, frame, 0, w, h);
}

extern "C" int mij_jpeg_size(const uint8_t *jpg, size_t len, int *w, int *h) {
  int fw = 0, fh = 0;
  if (!jpg || !frame_header(jpg, len, &fw, &fh)) return 0;
  if (w) *w = fw;
  if (h) *h = fh;
  return 1;
}

int mij_parse_size_accept(const char *what, const uint8_t *jpg, size_t len, int frame, unsigned accept, int *w, int *h) {
  Parsed P;
  if (int rc = parse(jpg, len, P, frame, accept)) return mij_fail(rc, "%s: %s", what, P.err);
  *w = P.w;
  *h = P.h;
  return MIJ_OK;
}

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

// what mij_decoder_transcode and mij_decoder_transform write from now on
extern "C" int mij_decoder_output(mij_decoder *d, int format) {
  mij_clear_error();
  if (!d) return mij_fail(MIJ_EINVAL, "decoder_output: null decoder");
  if (format != MIJ_OUT_BASELINE && format != MIJ_OUT_PROGRESSIVE)
    return mij_fail(MIJ_EINVAL, "decoder_output: unknown format %d", format);
  d->out_fmt = format;
  return MIJ_OK;
}

extern "C" int mij_transcode_progressive(const uint8_t *jpg, size_t len, int restart_rows, uint8_t *out, size_t cap,
                                         size_t *out_len) {
  mij_clear_error();
  if (out_len) *out_len = 0;
  if (!jpg || (!out && cap)) return mij_fail(MIJ_EINVAL, "mij_transcode_progressive: NULL buffer");
  Parsed P;  // the size first: the decoder is made for it; and every refusal, before any device work
  if (int rc = parse(jpg, len, P, 0, MIJ_ACCEPT_PROGRESSIVE)) return mij_fail(rc, "mij_transcode_progressive: %s", P.err);
  XfPlan X;
  if (int rc = xf_plan(P, MIJ_XF_NONE, 0, nullptr, restart_rows, "mij_transcode_progressive", 0, X)) return rc;
  if (int rc = pw_check(P, X, restart_rows, "mij_transcode_progressive", 0)) return rc;
  mij_decoder *d = mij_decoder_create(mij_drop_device(), (P.w + 15) / 16 * 16, (P.h + 15) / 16 * 16, 1);
  if (!d) return mij_last_error();
  d->accept = MIJ_ACCEPT_PROGRESSIVE;
  d->out_fmt = MIJ_OUT_PROGRESSIVE;
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
