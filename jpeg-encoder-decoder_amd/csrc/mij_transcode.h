// mij_transcode.h -- lossless transcoding: what
// mij_transcode.hip (kernels) and mij_decode.hip (host) share.  Not public.
#pragma once
#include "mij_internal.h"

namespace mij {

// entropy bytes per stuffing chunk: 256 threads x 16 bytes (one uint4 of scan words each)
constexpr int TC_CH = 4096;
// bytes before the entropy data at most: APP0 20 + 3 DQT x 69 + 4 DHT x (21 + 256) + SOF0 19 + DRI 6 + SOS 14
constexpr int TC_HDR_MAX = 1408;

// One component's absolute DCs from the prefix sums k_dec_dc / k_dec_dcbase
// left (mij_decode.hip): with P(s) = pre[s] + tile[s / DC tile] over the
// source's scan order, block s has P(s) - P(first block of its segment - 1).
struct TcDc {
  const int32_t *pre;    // the component's prefix sums relative to their tile
  const uint32_t *tile;  // its tiles' bases
  int16_t *abs;          // out: one absolute DC per block, raster order of the padded plane
  int nblocks, seg;      // blocks; blocks between the source's DC resets
  int hs, vs, mcus_x, bw;  // the source scan's order: blocks per MCU, MCUs across, blocks across
  int dc_tile;           // blocks per tile
  int pad;
};

struct TcComp {
  const int16_t *plane;  // padded plane in the arena: raster blocks of 64 zigzag coefficients
  const int16_t *abs;    // its absolute DCs (TcDc::abs)
  int hs, vs, bw;        // blocks per MCU across and down, blocks across the plane
  int pad;
};

// A frame of the call.  Its blocks are numbered in the new scan's order: MCUs
// in raster order, inside an MCU the components in SOF order, each with its
// hs x vs blocks left to right, top to bottom.  The per-call work arrays are
// packed frame after frame: this frame's entries start at blk0 (per block),
// mcu0 (per MCU), row0 (per MCU row) and rowp0 (the prefix arrays, one entry
// more per frame).
struct TcFrame {
  TcComp c[3];
  int ncomp, bpm;        // components; blocks per MCU
  int mcus_x, mcus_y;
  int R, nint;           // MCU rows per restart interval, intervals
  int nblk;              // mcus_x * mcus_y * bpm
  int ri;                // DRI value (restart_rows * mcus_x), 0: no DRI segment
  long long blk0;
  int mcu0, row0, rowp0;
  // headers
  int w, h;              // SOF0's size
  int ndqt;              // DQT segments
  uint8_t sof[3][3];     // SOF0's component entries verbatim: id, H/V, Tq
  uint8_t dqt_id[3];     // ascending
  uint8_t pad[2];
  uint8_t dqt[3][64];    // the source's tables, as stored
};

// Where a frame's scan words and output lie: known once the frame's bits are
// (the host reads them back after k_tc_scan).
struct TcOut {
  long long raw0, raw_words;  // first word and words of the unstuffed entropy data (multiples of 64)
  long long out0, out_cap;    // first byte and bytes of the stream
  long long chunk0;           // first TC_CH chunk
};

struct TcArgs {
  const TcFrame *fr;
  const TcOut *o;
  int nframes;
  int max_nblk, max_rows, max_chunks;  // the grids: the largest frame's
  uint32_t *hist;           // per frame [4][257]: DC, AC of component 0; DC, AC of the others
  const uint32_t *ehuf;     // per frame [4][256] = len << 16 | code
  const HuffCode *hc;       // per frame [4]
  uint16_t *blk_bits;       // per block, scan order
  uint32_t *mcu_off;        // per MCU: its bit offset inside its MCU row
  uint32_t *row_bits;       // per MCU row
  unsigned long long *row_pre;   // per MCU row: bits of the rows before it, unpadded; [rows] = all
  unsigned long long *ival_off;  // per interval: its first bit in the entropy data; [nint] = all
  unsigned long long *row_off;   // per MCU row: its first bit in the entropy data; [rows] = all
  unsigned long long *bits;      // per frame: bits of the entropy data (intervals rounded to bytes)
  uint32_t *raw;            // big-endian words: the unstuffed entropy data
  uint32_t *ffc;            // per TC_CH chunk: its 0xFF bytes, then those of the frame's chunks before it
  int *hdr;                 // per frame: bytes before the entropy data
  uint8_t *out;
  uint64_t *out_len;        // per frame, 0: failed
  int *err;                 // per frame FERR_*
};

hipError_t launch_tc_abs(const TcDc *jobs, int njobs, int max_blocks, hipStream_t s);
// counts; then (after the tables) bits per block, per row, offsets, the frame's bits
hipError_t launch_tc_hist(const TcArgs &a, hipStream_t s);
hipError_t launch_tc_sizes(const TcArgs &a, hipStream_t s);
// after the read-back of TcArgs::bits: zero, pack, 0xFF counts, headers, stuffed write
hipError_t launch_tc_write(const TcArgs &a, hipStream_t s);
// the same stages one by one, for the scans of a progressive file (mij_progwrite.hip): k_tc_rows and k_tc_scan
// over blk_bits; k_tc_zero; k_tc_ffcount; k_tc_write (it needs hdr, out_len and the exclusive ffc of a head stage)
hipError_t launch_tc_layout(const TcArgs &a, hipStream_t s);
hipError_t launch_tc_zero(const TcArgs &a, hipStream_t s);
hipError_t launch_tc_ffcount(const TcArgs &a, hipStream_t s);
hipError_t launch_tc_stuffed(const TcArgs &a, hipStream_t s);
// k_tables_1w (mij_kernels.hip): reads hist, hc, ehuf, err, nframes
hipError_t launch_tables(const EntArgs &a, hipStream_t s);

}  // namespace mij
