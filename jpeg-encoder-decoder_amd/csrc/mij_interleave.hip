// mij_interleave.hip -- gfx950 kernels of the interleaved output format
// (DESIGN.md §4g): one baseline scan of Y Y Y Y Cb Cr MCUs over MCU-padded
// planes, restart intervals of whole MCU rows, the frame's true size in SOF0.
//
//   k_il_pad      frames of any size, alignment and pitch edge-extended to
//                 multiples of 16 into the batch's canvas slots
//   (K1 + k_fix_blocks run unchanged on the padded slots, coefficient mode)
//   k_il_hist     symbol counts in MCU order (DC prediction per component,
//                 back to 0 at every restart)
//   (k_tables_1w builds the four tables from the counts)
//   k_il_bits     bits per block
//   k_il_rows     bits per MCU row, MCU offsets inside their row
//   k_il_scan     row offsets in the frame, intervals rounded up to bytes
//   k_il_zero     the words the packing ORs onto
//   k_il_pack     every block's codes at its bit offset, interval pad bits
//   k_il_ffcount  0xFF bytes per chunk
//   k_il_head     headers, DRI, SOS, chunk offsets, EOI, the length
//   k_il_write    stuffed bytes and RSTn markers
//
// Block coding is the three-scan path's (encoder.c:315-358, :434-502): DC
// class + bits, AC run/size with ZRL, EOB unless coefficient 63 is nonzero.
#include "mij_headers.h"
#include "mij_ilcode.h"
#include "mij_interleave.h"

namespace mij {

namespace {

struct IlFrame {
  int mw, rows, bw, nY, nC;
  int R, nint;  // MCU rows per interval, intervals
};
__device__ __forceinline__ IlFrame il_frame(const IlArgs &a, int f) {
  const int w = __builtin_amdgcn_readfirstlane(a.pdims[f].x), h = __builtin_amdgcn_readfirstlane(a.pdims[f].y);
  IlFrame r;
  r.mw = w >> 4;
  r.rows = h >> 4;
  r.bw = w >> 3;
  r.nC = r.mw * r.rows;
  r.nY = 4 * r.nC;
  r.R = a.restart_rows > 0 && a.restart_rows < r.rows ? a.restart_rows : r.rows;
  r.nint = (r.rows + r.R - 1) / r.R;
  return r;
}

// Block k (Y00 Y01 Y10 Y11 Cb Cr) of MCU m: its index in the frame's planes
// and its DC predictor's (-1: the interval starts here, predictor 0)
__device__ __forceinline__ int il_block(const IlFrame &g, int m, int k, int &pred) {
  const int r = m / g.mw, c = m - r * g.mw;
  const bool first = c == 0 && r % g.R == 0;
  if (k >= 4) {
    const int blk = g.nY + (k == 5 ? g.nC : 0) + m;
    pred = first ? -1 : blk - 1;
    return blk;
  }
  const int blk = (2 * r + (k >> 1)) * g.bw + 2 * c + (k & 1);
  if (k == 0)  // the MCU before: its Y11
    pred = first ? -1 : (c ? (2 * r + 1) * g.bw + 2 * c - 1 : (2 * r - 1) * g.bw + g.bw - 1);
  else if (k == 2)
    pred = blk - g.bw + 1;  // Y01
  else
    pred = blk - 1;
  return blk;
}

// the thread's block of frame f: false past the frame's blocks
struct IlBlk {
  const int16_t *coef;
  int diff, chroma, m, k;
};
__device__ __forceinline__ bool il_thread_block(const IlArgs &a, const IlFrame &g, int f, int i, IlBlk &b) {
  if (i >= 6 * g.nC) return false;
  b.m = i / 6;
  b.k = i - 6 * b.m;
  int pred;
  const int blk = il_block(g, b.m, b.k, pred);
  const int16_t *dc = a.dc + (long long)f * a.g.nblk;
  b.diff = (int)dc[blk] - (pred < 0 ? 0 : (int)dc[pred]);
  b.coef = a.coef + (long long)f * a.g.coef_fs + (long long)blk * 64;
  b.chroma = b.k >= 4;
  return true;
}

}  // namespace

// ---- edge extension into the canvas slots ----------------------------------
// Thread = one 16-byte line of a padded row.  A line wholly inside the source
// row comes from five aligned dwords re-aligned with v_alignbyte (the source
// has any alignment); a line touching the right edge, and every line of a
// swapped frame, byte by byte with the column clamped.  Rows past the last
// repeat it.  Every store is a whole aligned 16-byte line.
__global__ __launch_bounds__(256) void k_il_pad(IlPadArgs a) {
  const int f = blockIdx.y;
  const int w = a.tdims[f].x, h = a.tdims[f].y;
  if (w < 1 || h < 1) return;
  const int W16 = (w + 15) & ~15, H16 = (h + 15) & ~15;
  if (W16 > a.cw || H16 > a.ch) return;  // (the host refuses these)
  const int lpr = W16 * 3 / 16;          // lines per padded row
  const long long nlines = (long long)lpr * H16;
  const uint8_t *src = a.src + (long long)f * a.src_fs;
  uint8_t *dst = a.dst + (long long)f * a.slot_bytes;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nlines; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / lpr), l = (int)(i - (long long)y * lpr);
    const uint8_t *srow = src + (long long)min(y, h - 1) * a.src_pitch;
    uint32_t o[4];
    if (!a.swap && 16 * l + 16 <= 3 * w) {
      const uint8_t *p = srow + 16 * l;
      const uint32_t sh = (uint32_t)((uintptr_t)p & 3);
      const uint32_t *pw = (const uint32_t *)(p - sh);
      // (sh != 0: the fifth dword holds bytes 16 - sh .. 15 of the line, inside the row)
      const uint32_t d0 = pw[0], d1 = pw[1], d2 = pw[2], d3 = pw[3], d4 = sh ? pw[4] : 0u;
      o[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
      o[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
      o[2] = __builtin_amdgcn_alignbyte(d3, d2, sh);
      o[3] = __builtin_amdgcn_alignbyte(d4, d3, sh);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int bi = 16 * l + 4 * k + j, x = bi / 3, c = bi - 3 * x;
          v |= (uint32_t)srow[min(x, w - 1) * 3 + (a.swap ? 2 - c : c)] << (8 * j);
        }
        o[k] = v;
      }
    }
    *(uint4 *)(dst + (long long)y * a.pitch + 16 * l) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ---- symbol counts in MCU order ---------------------------------------------
__global__ __launch_bounds__(256) void k_il_hist(IlArgs a) {
  __shared__ uint32_t h[4][256];
  const int f = blockIdx.y;
  const IlFrame g = il_frame(a, f);
  if ((long long)blockIdx.x * 256 >= 6LL * g.nC) return;
  for (int i = threadIdx.x; i < 1024; i += 256) h[i >> 8][i & 255] = 0;
  __syncthreads();
  IlBlk b;
  if (il_thread_block(a, g, f, blockIdx.x * 256 + threadIdx.x, b)) {
    const int t0 = b.chroma ? 2 : 0;
    il_walk(b.coef, b.diff, [&](int ac, int sym, int, int) { atomicAdd(&h[t0 + ac][sym & 255], 1u); });
  }
  __syncthreads();
  uint32_t *gh = a.hist + (long long)f * 4 * 257;
  for (int i = threadIdx.x; i < 1024; i += 256) {
    const uint32_t v = h[i >> 8][i & 255];
    if (v) atomicAdd(&gh[(i >> 8) * 257 + (i & 255)], v);
  }
}

// ---- bits per block -----------------------------------------------------------
__global__ __launch_bounds__(256) void k_il_bits(IlArgs a) {
  __shared__ uint32_t tab[4][256];
  const int f = blockIdx.y;
  if (a.err[f]) return;
  const IlFrame g = il_frame(a, f);
  if ((long long)blockIdx.x * 256 >= 6LL * g.nC) return;
  for (int i = threadIdx.x; i < 1024; i += 256) tab[i >> 8][i & 255] = a.ehuf[(long long)f * 1024 + i];
  __syncthreads();
  IlBlk b;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (!il_thread_block(a, g, f, i, b)) return;
  const int t0 = b.chroma ? 2 : 0;
  uint32_t bits = 0;
  il_walk(b.coef, b.diff, [&](int ac, int sym, int, int nv) { bits += (tab[t0 + ac][sym & 255] >> 16) + nv; });
  a.blk_bits[(long long)f * a.g.nblk + i] = (uint16_t)bits;  // <= 64 * (16 + 12)
}

// ---- bits per MCU row, MCU offsets inside the row -------------------------------
__global__ __launch_bounds__(256) void k_il_rows(IlArgs a) {
  __shared__ uint32_t red[4];
  const int f = blockIdx.y, r = blockIdx.x;
  if (a.err[f]) return;
  const IlFrame g = il_frame(a, f);
  if (r >= g.rows) return;
  const uint16_t *bb = a.blk_bits + (long long)f * a.g.nblk + (long long)r * g.mw * 6;
  uint32_t *mo = a.mcu_off + (long long)f * a.g.nC + (long long)r * g.mw;
  uint32_t carry = 0;
  for (int c0 = 0; c0 < g.mw; c0 += 256) {
    const int c = c0 + threadIdx.x;
    uint32_t v = 0;
    if (c < g.mw)
      for (int k = 0; k < 6; k++) v += bb[c * 6 + k];
    uint32_t tot;
    const uint32_t incl = il_scan256(v, red, tot);
    if (c < g.mw) mo[c] = carry + incl - v;
    carry += tot;
  }
  if (threadIdx.x == 0) a.row_bits[(long long)f * il_rows(a.g) + r] = carry;
}

// ---- row offsets in the frame; every interval rounded up to a byte --------------
__global__ __launch_bounds__(256) void k_il_scan(IlArgs a) {
  __shared__ unsigned long long red[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (a.err[f]) return;
  const IlFrame g = il_frame(a, f);
  const long long rs = il_rows(a.g) + 1;
  const uint32_t *rb = a.row_bits + (long long)f * il_rows(a.g);
  unsigned long long *pre = a.row_pre + f * rs, *iv = a.ival_off + f * rs, *ro = a.row_off + f * rs;
  unsigned long long carry = 0;
  for (int r0 = 0; r0 < g.rows; r0 += 256) {
    const int r = r0 + tid;
    const unsigned long long v = r < g.rows ? rb[r] : 0ull;
    unsigned long long tot;
    const unsigned long long incl = il_scan256(v, red, tot);
    if (r < g.rows) pre[r] = carry + incl - v;
    carry += tot;
  }
  if (tid == 0) pre[g.rows] = carry;
  __syncthreads();  // (pre: this workgroup's stores, read below)
  carry = 0;
  for (int i0 = 0; i0 < g.nint; i0 += 256) {
    const int i = i0 + tid;
    unsigned long long v = 0;
    if (i < g.nint) v = (pre[min((i + 1) * g.R, g.rows)] - pre[i * g.R] + 7ull) & ~7ull;
    unsigned long long tot;
    const unsigned long long incl = il_scan256(v, red, tot);
    if (i < g.nint) iv[i] = carry + incl - v;
    carry += tot;
  }
  if (tid == 0) {
    iv[g.nint] = carry;
    ro[g.rows] = carry;
    // the packing stays inside the frame's scan words
    if (carry > 32ull * (unsigned long long)a.g.raw_fs) a.err[f] = FERR_OVERFLOW;
  }
  __syncthreads();
  for (int r = tid; r < g.rows; r += 256) {
    const int i = r / g.R;
    ro[r] = iv[i] + pre[r] - pre[i * g.R];
  }
}

// ---- the scan words the packing ORs onto ------------------------------------------
__global__ __launch_bounds__(256) void k_il_zero(IlArgs a) {
  const int f = blockIdx.y;
  if (a.err[f]) return;
  const IlFrame g = il_frame(a, f);
  const unsigned long long bits = a.row_off[f * (long long)(il_rows(a.g) + 1) + g.rows];
  // whole 16-byte lines up to the word after the last bit (raw_fs is a multiple of 64 words)
  const long long n4 = min((long long)(bits / 128 + 1), (long long)(a.g.raw_fs / 4));
  uint4 *p = (uint4 *)(a.raw + (long long)f * a.g.raw_fs);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- packing: thread = block, at its bit offset ------------------------------------
// A block's first and last words are shared with its neighbours (atomic OR
// onto zeroed words); the words between are its own (plain stores).
__global__ __launch_bounds__(256) void k_il_pack(IlArgs a) {
  __shared__ uint32_t tab[4][256];
  const int f = blockIdx.y;
  if (a.err[f]) return;
  const IlFrame g = il_frame(a, f);
  if ((long long)blockIdx.x * 256 >= 6LL * g.nC) return;
  for (int i = threadIdx.x; i < 1024; i += 256) tab[i >> 8][i & 255] = a.ehuf[(long long)f * 1024 + i];
  __syncthreads();
  IlBlk b;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (!il_thread_block(a, g, f, i, b)) return;
  const int r = b.m / g.mw, c = b.m - r * g.mw;
  const uint16_t *bb = a.blk_bits + (long long)f * a.g.nblk + (long long)b.m * 6;
  unsigned long long pos = a.row_off[f * (long long)(il_rows(a.g) + 1) + r] + a.mcu_off[(long long)f * a.g.nC + b.m];
  for (int k = 0; k < b.k; k++) pos += bb[k];
  uint32_t *raw = a.raw + (long long)f * a.g.raw_fs;
  unsigned long long wi = pos >> 5, acc = 0;
  int n = (int)(pos & 31);
  bool first = true;
  const unsigned long long wmax = (unsigned long long)a.g.raw_fs;  // (k_il_scan checked the frame's bits)
  auto put = [&](uint32_t v, int len) {  // len <= 16
    if (!len) return;
    acc |= (unsigned long long)v << (64 - n - len);
    n += len;
    if (n >= 32) {
      const uint32_t w = (uint32_t)(acc >> 32);
      if (wi < wmax) {
        if (first) atomicOr(&raw[wi], w);
        else raw[wi] = w;
      }
      first = false;
      wi++;
      acc <<= 32;
      n -= 32;
    }
  };
  const int t0 = b.chroma ? 2 : 0;
  il_walk(b.coef, b.diff, [&](int ac, int sym, int v, int nv) {
    const uint32_t e = tab[t0 + ac][sym & 255];
    const int len = (int)(e >> 16);
    put(e & ((1u << len) - 1u), len);
    put(il_mag(v, nv), nv);
  });
  // the interval's last block pads it to a byte with 1-bits
  if (b.k == 5 && c == g.mw - 1 && ((r + 1) % g.R == 0 || r == g.rows - 1)) {
    const int np = (8 - (n & 7)) & 7;
    put((1u << np) - 1u, np);
  }
  if (n > 0 && wi < wmax) atomicOr(&raw[wi], (uint32_t)(acc >> 32));
}

// ---- 0xFF bytes per chunk ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_il_ffcount(IlArgs a) {
  __shared__ uint32_t red[4];
  const int f = blockIdx.y;
  if (a.err[f]) return;
  const IlFrame g = il_frame(a, f);
  const unsigned long long nbytes = a.row_off[f * (long long)(il_rows(a.g) + 1) + g.rows] >> 3;
  const long long nch = (long long)((nbytes + IL_CH - 1) / IL_CH);
  const uint32_t *raw = a.raw + (long long)f * a.g.raw_fs;
  for (long long c = blockIdx.x; c < nch; c += gridDim.x) {
    const unsigned long long b0 = (unsigned long long)c * IL_CH + 16 * threadIdx.x;
    uint32_t cnt = 0;
    if (b0 < nbytes) {
      const uint4 v = *(const uint4 *)(raw + (b0 >> 2));
      const int rem = (int)min(nbytes - b0, 16ull);
      cnt = il_ff(v.x, rem) + il_ff(v.y, rem - 4) + il_ff(v.z, rem - 8) + il_ff(v.w, rem - 12);
    }
    uint32_t tot;
    il_scan256(cnt, red, tot);
    if (threadIdx.x == 0) a.ffc[f * il_chunks(a.g) + c] = tot;
  }
}

// ---- headers, chunk offsets, EOI, length: one workgroup per frame ------------------------
__global__ __launch_bounds__(256) void k_il_head(IlArgs a) {
  __shared__ uint32_t red[4];
  __shared__ int s_n[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (a.err[f]) {
    if (tid == 0) a.out_len[f] = 0;
    return;
  }
  const IlFrame g = il_frame(a, f);
  const unsigned long long nbytes = a.row_off[f * (long long)(il_rows(a.g) + 1) + g.rows] >> 3;
  const long long nch = (long long)((nbytes + IL_CH - 1) / IL_CH);
  uint32_t *ffc = a.ffc + f * il_chunks(a.g);
  unsigned long long carry = 0;  // 0xFF bytes of the chunks before
  for (long long c0 = 0; c0 < nch; c0 += 256) {
    const long long c = c0 + tid;
    const uint32_t v = c < nch ? ffc[c] : 0u;
    uint32_t tot;
    const uint32_t incl = il_scan256(v, red, tot);
    if (c < nch) ffc[c] = (uint32_t)carry + incl - v;
    carry += tot;
  }
  // headers <= 20 + 138 + 4 * 277 + 19, DRI 6, SOS 14, EOI 2
  const unsigned long long need = 1320ull + nbytes + carry + 2ull * (unsigned long long)g.nint;
  if (need > (unsigned long long)a.g.out_cap) {
    if (tid == 0) {
      a.err[f] = FERR_OVERFLOW;
      a.out_len[f] = 0;
    }
    return;
  }
  uint8_t *out = a.out + (long long)f * a.g.out_cap;
  EntArgs e;  // emit_headers reads the tables and the frame's size: the true one here
  e.g = a.g;
  e.hc = a.hc;
  e.tab = a.tab;
  e.fdims = a.tdims;
  int pos = emit_headers(e, f, out, s_n);
  if (tid == 0) {
    if (a.restart_rows > 0) {
      const int ri = a.restart_rows * g.mw;  // <= 65535 (the host checked)
      const uint8_t dri[6] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(ri >> 8), (uint8_t)ri};
      for (int i = 0; i < 6; i++) out[pos + i] = dri[i];
      pos += 6;
    }
    const uint8_t sos[14] = {0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00};
    for (int i = 0; i < 14; i++) out[pos + i] = sos[i];
    pos += 14;
    a.hdr[f] = pos;
    const unsigned long long end = (unsigned long long)pos + nbytes + carry + 2ull * (unsigned long long)(g.nint - 1);
    out[end] = 0xFF;
    out[end + 1] = 0xD9;
    a.out_len[f] = end + 2;
  }
}

// ---- stuffed bytes and RSTn markers ---------------------------------------------------------
// Chunk c = entropy bytes [c * IL_CH, ..): thread t takes 16 of them.  Byte j
// leaves at hdr + j + (0xFF bytes before j) + 2 * (intervals begun at or
// before j, the first apart); the marker of interval i goes in front of its
// first byte, written by the chunk that holds that byte (also when it is the
// chunk's first).  The chunk is laid out in LDS and leaves in whole words.
__global__ __launch_bounds__(256) void k_il_write(IlArgs a) {
  __shared__ uint32_t red[4];
  __shared__ uint32_t flags[IL_CH / 32];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[3 * IL_CH + 16];
  const int f = blockIdx.y, tid = threadIdx.x;
  if (a.err[f] || !a.out_len[f]) return;
  const IlFrame g = il_frame(a, f);
  const long long rs = il_rows(a.g) + 1;
  const unsigned long long nbytes = a.row_off[f * rs + g.rows] >> 3;
  const long long nch = (long long)((nbytes + IL_CH - 1) / IL_CH);
  const uint32_t *raw = a.raw + (long long)f * a.g.raw_fs;
  const unsigned long long *iv = a.ival_off + f * rs;
  uint8_t *out = a.out + (long long)f * a.g.out_cap + a.hdr[f];
  for (long long c = blockIdx.x; c < nch; c += gridDim.x) {
    const unsigned long long c0 = (unsigned long long)c * IL_CH;
    const int nb = (int)min(nbytes - c0, (unsigned long long)IL_CH);
    // intervals 1 .. m0 begin before c0: their markers left with earlier chunks.
    // (An interval that begins exactly at c0 is this chunk's: the chunk that
    // holds an interval's first byte writes its marker.)
    int lo = 0, hi = g.nint - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;  // >= 1
      if ((iv[mid] >> 3) < c0) lo = mid;
      else hi = mid - 1;
    }
    const int m0 = lo;
    __syncthreads();  // (flags, s_out: the chunk before is out)
    if (tid < IL_CH / 32) flags[tid] = 0;
    __syncthreads();
    for (int i = m0 + 1 + tid; i < g.nint; i += 256) {
      const unsigned long long bi = iv[i] >> 3;
      if (bi >= c0 + (unsigned long long)nb) break;
      atomicOr(&flags[(bi - c0) >> 5], 1u << ((bi - c0) & 31));
    }
    __syncthreads();
    const int j0 = 16 * tid;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    int rem = 0;
    if (j0 < nb) {
      v = *(const uint4 *)(raw + ((c0 + j0) >> 2));
      rem = min(nb - j0, 16);
    }
    const uint32_t fl = (flags[tid >> 1] >> (16 * (tid & 1))) & 0xFFFFu;
    const uint32_t nff = il_ff(v.x, rem) + il_ff(v.y, rem - 4) + il_ff(v.z, rem - 8) + il_ff(v.w, rem - 12);
    const uint32_t nmk = __popc(fl);
    // low half: bytes out; high half: markers
    const uint32_t mine = ((uint32_t)rem + nff + 2 * nmk) | (nmk << 16);
    uint32_t tot;
    const uint32_t excl = il_scan256(mine, red, tot) - mine;
    uint32_t o = excl & 0xFFFFu;
    int mk = m0 + (int)(excl >> 16);  // intervals begun before this thread's bytes
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (j < rem) {
        if ((fl >> j) & 1u) {  // interval mk + 1 begins here: RST(mk mod 8) closes interval mk
          s_out[o++] = 0xFF;
          s_out[o++] = (uint8_t)(0xD0 + (mk & 7));
          mk++;
        }
        const uint8_t by = (uint8_t)(w[j >> 2] >> (24 - 8 * (j & 3)));
        s_out[o++] = by;
        if (by == 0xFF) s_out[o++] = 0x00;
      }
    }
    __syncthreads();
    // out: head bytes to the first aligned word, whole words, tail bytes
    const uint32_t n = tot & 0xFFFFu;
    uint8_t *d = out + c0 + a.ffc[f * il_chunks(a.g) + c] + 2ull * (unsigned long long)m0;
    const uint32_t head = min(n, (uint32_t)((4 - ((uintptr_t)d & 3)) & 3));
    if (tid < head) d[tid] = s_out[tid];
    const uint32_t nw = (n - head) >> 2, sh = head;  // (s_out is word-aligned: the source shift is the head)
    const uint32_t *sw = (const uint32_t *)s_out;
    uint32_t *dw = (uint32_t *)(d + head);
    for (uint32_t k = tid; k < nw; k += 256) dw[k] = sh ? __builtin_amdgcn_alignbyte(sw[k + 1], sw[k], sh) : sw[k];
    const uint32_t tl = n - head - 4 * nw;
    if (tid < tl) d[head + 4 * nw + tid] = s_out[head + 4 * nw + tid];
  }
}

// ---- launches ----------------------------------------------------------------------------------
hipError_t launch_il_pad(const IlPadArgs &a, int n, hipStream_t s) {
  const long long lines = (long long)a.cw * 3 / 16 * a.ch;
  const long long gx = (lines + 255) / 256;
  hipLaunchKernelGGL(k_il_pad, dim3((unsigned)(gx < 2048 ? gx : 2048), n), dim3(256), 0, s, a);
  return hipGetLastError();
}

static dim3 il_block_grid(const IlArgs &a) { return dim3((unsigned)((a.g.nblk + 255) / 256), a.nframes); }

hipError_t launch_il_hist(const IlArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_il_hist, il_block_grid(a), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_il_entropy(const IlArgs &a, hipStream_t s) {
  const long long nch = il_chunks(a.g);
  const dim3 chunks((unsigned)(nch < 256 ? nch : 256), a.nframes);
  hipLaunchKernelGGL(k_il_bits, il_block_grid(a), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_il_rows, dim3(il_rows(a.g), a.nframes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_il_scan, dim3(a.nframes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_il_zero, dim3(64, a.nframes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_il_pack, il_block_grid(a), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_il_ffcount, chunks, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_il_head, dim3(a.nframes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_il_write, chunks, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace mij
