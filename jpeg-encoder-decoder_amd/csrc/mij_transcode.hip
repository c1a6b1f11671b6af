// mij_transcode.hip -- gfx950 kernels of lossless transcoding (DESIGN.md
// §4h): the coefficient planes the decoder left on the device, of any
// accepted sampling, become one interleaved baseline scan with tables
// optimised for it and restart intervals of whole MCU rows.  Nothing is
// dequantised: the planes, their MCU padding included, are coded as decoded.
//
//   (k_dec_dc / k_dec_dcbase, mij_decode.hip: prefix sums of the coded DC
//    differences over the source's scan order)
//   k_tc_abs      one absolute DC per block
//   k_tc_hist     symbol counts in the new scan's order (DC prediction per
//                 component, back to 0 at every restart)
//   (k_tables_1w builds the tables from the counts)
//   k_tc_bits     bits per block
//   k_tc_rows     bits per MCU row, MCU offsets inside their row
//   k_tc_scan     row offsets in the frame, intervals rounded up to bytes,
//                 the frame's bits (the host sizes scan words and output by them)
//   k_tc_zero     the words the packing ORs onto
//   k_tc_pack     every block's codes at its bit offset, interval pad bits
//   k_tc_ffcount  0xFF bytes per chunk
//   k_tc_head     headers, DRI, SOS, chunk offsets, EOI, the length
//   k_tc_write    stuffed bytes and RSTn markers
//
// The stages are those of the interleaved output format (mij_interleave.hip)
// and every dependency is a kernel boundary; what differs is the addressing:
// a per-frame descriptor (TcFrame) instead of the batch canvas, work arrays
// packed frame after frame, one grid row per frame.
#include "mij_ilcode.h"
#include "mij_transcode.h"

namespace mij {

namespace {

// the thread's block of frame F: false past the frame's blocks
struct TcBlk {
  const int16_t *coef;
  int diff, t0, m, k;
  bool closes;  // the last block of a restart interval
};
__device__ __forceinline__ bool tc_thread_block(const TcFrame &F, int i, TcBlk &b) {
  if (i >= F.nblk) return false;
  const int m = i / F.bpm, k = i - m * F.bpm;
  // the component of slot k, and the slot's place among the component's blocks
  const int n0 = F.c[0].hs * F.c[0].vs;
  int c = 0, j = k;
  if (k >= n0) {
    const int n1 = F.c[1].hs * F.c[1].vs;
    c = k - n0 < n1 ? 1 : 2;
    j = k - n0 - (c == 2 ? n1 : 0);
  }
  const TcComp C = F.c[c];
  const int my = m / F.mcus_x, mx = m - my * F.mcus_x;
  const int jy = j / C.hs, jx = j - jy * C.hs;
  const int blk = (my * C.vs + jy) * C.bw + mx * C.hs + jx;
  // the component's block before this one in scan order (-1: the interval starts here, predictor 0)
  int pred;
  if (j > 0) {
    pred = jx ? blk - 1 : blk - C.bw + C.hs - 1;
  } else if (mx == 0 && my % F.R == 0) {
    pred = -1;
  } else {  // the last block of the MCU before
    const int py = mx ? my : my - 1, px = mx ? mx - 1 : F.mcus_x - 1;
    pred = (py * C.vs + C.vs - 1) * C.bw + px * C.hs + C.hs - 1;
  }
  b.diff = (int)C.abs[blk] - (pred < 0 ? 0 : (int)C.abs[pred]);
  b.coef = C.plane + 64LL * blk;
  b.t0 = c ? 2 : 0;
  b.m = m;
  b.k = k;
  b.closes = k == F.bpm - 1 && mx == F.mcus_x - 1 && ((my + 1) % F.R == 0 || my == F.mcus_y - 1);
  return true;
}

}  // namespace

// ---- absolute DCs ------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tc_abs(const TcDc *jobs) {
  const TcDc j = jobs[blockIdx.y];
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= j.nblocks) return;
  const int s0 = s / j.seg * j.seg;
  uint32_t v = (uint32_t)j.pre[s] + j.tile[s / j.dc_tile];
  if (s0 > 0) v -= (uint32_t)j.pre[s0 - 1] + j.tile[(s0 - 1) / j.dc_tile];
  const int hv = j.hs * j.vs, m = s / hv, i = s - m * hv;
  const int my = m / j.mcus_x, mx = m - my * j.mcus_x, iy = i / j.hs, ix = i - iy * j.hs;
  j.abs[(my * j.vs + iy) * j.bw + mx * j.hs + ix] = (int16_t)v;  // < nblocks: a permutation of the plane's blocks
}

// ---- symbol counts in scan order -----------------------------------------------
__global__ __launch_bounds__(256) void k_tc_hist(TcArgs a) {
  __shared__ uint32_t h[4][256];
  const int f = blockIdx.y;
  const TcFrame &F = a.fr[f];
  if ((long long)blockIdx.x * 256 >= F.nblk) return;
  for (int i = threadIdx.x; i < 1024; i += 256) h[i >> 8][i & 255] = 0;
  __syncthreads();
  TcBlk b;
  if (tc_thread_block(F, blockIdx.x * 256 + threadIdx.x, b)) {
    // Absolute DCs are int16, so a difference has category <= 16, and 16 has no
    // code in any JPEG: the frame is refused, the later stages skip it and
    // nothing of it is written (DESIGN.md §4h "DC range").  Every lane that
    // finds one stores the same value; the symbol is still counted (16 < 256),
    // so that the table builder sees counts it can serve and leaves the code.
    if (il_class(b.diff) > 15) a.err[f] = FERR_DCRANGE;
    il_walk(b.coef, b.diff, [&](int ac, int sym, int, int) { atomicAdd(&h[b.t0 + ac][sym & 255], 1u); });
  }
  __syncthreads();
  uint32_t *gh = a.hist + (long long)f * 4 * 257;
  for (int i = threadIdx.x; i < 1024; i += 256) {
    const uint32_t v = h[i >> 8][i & 255];
    if (v) atomicAdd(&gh[(i >> 8) * 257 + (i & 255)], v);
  }
  // A one-component frame counts nothing for the second pair of tables, which
  // it neither uses nor writes: one count each, so that the builder, which
  // runs for all four, has a code to make and cannot fail the frame over them.
  if (F.ncomp == 1 && blockIdx.x == 0 && threadIdx.x < 2) gh[(2 + threadIdx.x) * 257] = 1u;
}

// ---- bits per block ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tc_bits(TcArgs a) {
  __shared__ uint32_t tab[4][256];
  const int f = blockIdx.y;
  if (a.err[f]) return;
  const TcFrame &F = a.fr[f];
  if ((long long)blockIdx.x * 256 >= F.nblk) return;
  for (int i = threadIdx.x; i < 1024; i += 256) tab[i >> 8][i & 255] = a.ehuf[(long long)f * 1024 + i];
  __syncthreads();
  TcBlk b;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (!tc_thread_block(F, i, b)) return;
  uint32_t bits = 0;
  il_walk(b.coef, b.diff, [&](int ac, int sym, int, int nv) { bits += (tab[b.t0 + ac][sym & 255] >> 16) + nv; });
  a.blk_bits[F.blk0 + i] = (uint16_t)bits;  // <= 32 + 63 * 31 + 3 * 16
}

// ---- bits per MCU row, MCU offsets inside the row -----------------------------------
__global__ __launch_bounds__(256) void k_tc_rows(TcArgs a) {
  __shared__ uint32_t red[4];
  const int f = blockIdx.y, r = blockIdx.x;
  if (a.err[f]) return;
  const TcFrame &F = a.fr[f];
  if (r >= F.mcus_y) return;
  const uint16_t *bb = a.blk_bits + F.blk0 + (long long)r * F.mcus_x * F.bpm;
  uint32_t *mo = a.mcu_off + F.mcu0 + (long long)r * F.mcus_x;
  uint32_t carry = 0;
  for (int c0 = 0; c0 < F.mcus_x; c0 += 256) {
    const int c = c0 + threadIdx.x;
    uint32_t v = 0;
    if (c < F.mcus_x)
      for (int k = 0; k < F.bpm; k++) v += bb[c * F.bpm + k];
    uint32_t tot;
    const uint32_t incl = il_scan256(v, red, tot);
    if (c < F.mcus_x) mo[c] = carry + incl - v;
    carry += tot;
  }
  if (threadIdx.x == 0) a.row_bits[F.row0 + r] = carry;
}

// ---- row offsets in the frame; every interval rounded up to a byte ------------------
__global__ __launch_bounds__(256) void k_tc_scan(TcArgs a) {
  __shared__ unsigned long long red[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (a.err[f]) {
    if (tid == 0) a.bits[f] = 0;
    return;
  }
  const TcFrame &F = a.fr[f];
  const int rows = F.mcus_y;
  const uint32_t *rb = a.row_bits + F.row0;
  unsigned long long *pre = a.row_pre + F.rowp0, *iv = a.ival_off + F.rowp0, *ro = a.row_off + F.rowp0;
  unsigned long long carry = 0;
  for (int r0 = 0; r0 < rows; r0 += 256) {
    const int r = r0 + tid;
    const unsigned long long v = r < rows ? rb[r] : 0ull;
    unsigned long long tot;
    const unsigned long long incl = il_scan256(v, red, tot);
    if (r < rows) pre[r] = carry + incl - v;
    carry += tot;
  }
  if (tid == 0) pre[rows] = carry;
  __syncthreads();  // (pre: this workgroup's stores, read below)
  carry = 0;
  for (int i0 = 0; i0 < F.nint; i0 += 256) {
    const int i = i0 + tid;
    unsigned long long v = 0;
    if (i < F.nint) v = (pre[min((i + 1) * F.R, rows)] - pre[i * F.R] + 7ull) & ~7ull;
    unsigned long long tot;
    const unsigned long long incl = il_scan256(v, red, tot);
    if (i < F.nint) iv[i] = carry + incl - v;
    carry += tot;
  }
  if (tid == 0) {
    iv[F.nint] = carry;
    ro[rows] = carry;
    a.bits[f] = carry;
  }
  __syncthreads();
  for (int r = tid; r < rows; r += 256) {
    const int i = r / F.R;
    ro[r] = iv[i] + pre[r] - pre[i * F.R];
  }
}

// ---- the scan words the packing ORs onto ----------------------------------------------
__global__ __launch_bounds__(256) void k_tc_zero(TcArgs a) {
  const int f = blockIdx.y;
  if (a.err[f]) return;
  const TcOut &O = a.o[f];
  // whole 16-byte lines up to the word after the last bit
  const long long n4 = min((long long)(a.bits[f] / 128 + 1), O.raw_words / 4);
  uint4 *p = (uint4 *)(a.raw + O.raw0);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- packing: thread = block, at its bit offset ----------------------------------------
// A block's first and last words are shared with its neighbours (atomic OR
// onto zeroed words); the words between are its own (plain stores).
__global__ __launch_bounds__(256) void k_tc_pack(TcArgs a) {
  __shared__ uint32_t tab[4][256];
  const int f = blockIdx.y;
  if (a.err[f]) return;
  const TcFrame &F = a.fr[f];
  if ((long long)blockIdx.x * 256 >= F.nblk) return;
  for (int i = threadIdx.x; i < 1024; i += 256) tab[i >> 8][i & 255] = a.ehuf[(long long)f * 1024 + i];
  __syncthreads();
  TcBlk b;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (!tc_thread_block(F, i, b)) return;
  const TcOut &O = a.o[f];
  const uint16_t *bb = a.blk_bits + F.blk0 + (long long)b.m * F.bpm;
  unsigned long long pos = a.row_off[F.rowp0 + b.m / F.mcus_x] + a.mcu_off[F.mcu0 + b.m];
  for (int k = 0; k < b.k; k++) pos += bb[k];
  uint32_t *raw = a.raw + O.raw0;
  unsigned long long wi = pos >> 5, acc = 0;
  int n = (int)(pos & 31);
  bool first = true;
  const unsigned long long wmax = (unsigned long long)O.raw_words;  // (sized by the frame's bits)
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
  il_walk(b.coef, b.diff, [&](int ac, int sym, int v, int nv) {
    const uint32_t e = tab[b.t0 + ac][sym & 255];
    const int len = (int)(e >> 16);
    put(e & ((1u << len) - 1u), len);
    put(il_mag(v, nv), nv);
  });
  // the interval's last block pads it to a byte with 1-bits
  if (b.closes) {
    const int np = (8 - (n & 7)) & 7;
    put((1u << np) - 1u, np);
  }
  if (n > 0 && wi < wmax) atomicOr(&raw[wi], (uint32_t)(acc >> 32));
}

// ---- 0xFF bytes per chunk -----------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tc_ffcount(TcArgs a) {
  __shared__ uint32_t red[4];
  const int f = blockIdx.y;
  if (a.err[f]) return;
  const TcOut &O = a.o[f];
  const unsigned long long nbytes = a.bits[f] >> 3;
  const long long nch = (long long)((nbytes + TC_CH - 1) / TC_CH);
  const uint32_t *raw = a.raw + O.raw0;
  for (long long c = blockIdx.x; c < nch; c += gridDim.x) {
    const unsigned long long b0 = (unsigned long long)c * TC_CH + 16 * threadIdx.x;
    uint32_t cnt = 0;
    if (b0 < nbytes) {  // (its line: inside the words k_tc_zero cleared)
      const uint4 v = *(const uint4 *)(raw + (b0 >> 2));
      const int rem = (int)min(nbytes - b0, 16ull);
      cnt = il_ff(v.x, rem) + il_ff(v.y, rem - 4) + il_ff(v.z, rem - 8) + il_ff(v.w, rem - 12);
    }
    uint32_t tot;
    il_scan256(cnt, red, tot);
    if (threadIdx.x == 0) a.ffc[O.chunk0 + c] = tot;
  }
}

// ---- headers, chunk offsets, EOI, length: one workgroup per frame --------------------------
// APP0, one DQT per table id in use (the source's bytes), the DHTs (two for a
// one-component frame), SOF0 with the source's component entries, DRI, SOS.
// Every other segment of the source is dropped.
__global__ __launch_bounds__(256) void k_tc_head(TcArgs a) {
  __shared__ uint32_t red[4];
  __shared__ int s_n[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (a.err[f]) {
    if (tid == 0) a.out_len[f] = 0;
    return;
  }
  const TcFrame &F = a.fr[f];
  const TcOut &O = a.o[f];
  const unsigned long long nbytes = a.bits[f] >> 3;
  const long long nch = (long long)((nbytes + TC_CH - 1) / TC_CH);
  uint32_t *ffc = a.ffc + O.chunk0;
  unsigned long long carry = 0;  // 0xFF bytes of the chunks before
  for (long long c0 = 0; c0 < nch; c0 += 256) {
    const long long c = c0 + tid;
    const uint32_t v = c < nch ? ffc[c] : 0u;
    uint32_t tot;
    const uint32_t incl = il_scan256(v, red, tot);
    if (c < nch) ffc[c] = (uint32_t)carry + incl - v;
    carry += tot;
  }
  const unsigned long long need = (unsigned long long)TC_HDR_MAX + nbytes + carry + 2ull * (unsigned long long)F.nint;
  if (need > (unsigned long long)O.out_cap) {  // (the host sized it for 2 * nbytes: not reached)
    if (tid == 0) {
      a.err[f] = FERR_OVERFLOW;
      a.out_len[f] = 0;
    }
    return;
  }
  uint8_t *out = a.out + O.out0;
  const HuffCode *hc = a.hc + (long long)f * 4;
  const int nc = F.ncomp, ntab = nc > 1 ? 4 : 2;
  {
    int hn = tid < 64 ? hc[tid >> 4].code_len_freq[1 + (tid & 15)] : 0;
    for (int o = 8; o; o >>= 1) hn += __shfl_xor(hn, o);  // sums over 16 lanes
    if (tid < 64 && (tid & 15) == 0) s_n[tid >> 4] = hn;
  }
  __syncthreads();
  int doff[5];  // DHT t starts at doff[t]; SOF0 at doff[ntab]
  doff[0] = 20 + 69 * F.ndqt;
  for (int t = 0; t < 4; t++) doff[t + 1] = doff[t] + (t < ntab ? 21 + s_n[t] : 0);
  const int o_sof = doff[4], o_dri = o_sof + 10 + 3 * nc, o_sos = o_dri + (F.ri ? 6 : 0);
  const int hlen = o_sos + 8 + 2 * nc;
  auto hbyte = [&](int i) -> uint8_t {
    if (i < 20) {
      const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 0x4A, 0x46, 0x49, 0x46,
                                0x00, 0x01, 0x01, 0x00, 0x00, 0x48, 0x00, 0x48, 0x00, 0x00};
      return app0[i];
    }
    if (i < doff[0]) {
      const int t = (i - 20) / 69, k = (i - 20) - 69 * t;
      const uint8_t m[5] = {0xFF, 0xDB, 0x00, 0x43, F.dqt_id[t]};
      return k < 5 ? m[k] : F.dqt[t][k - 5];
    }
    if (i < o_sof) {
      const int t = i >= doff[3] ? 3 : i >= doff[2] ? 2 : i >= doff[1] ? 1 : 0;
      const int k = i - doff[t], len = 19 + s_n[t];
      const uint8_t m[5] = {0xFF, 0xC4, (uint8_t)(len >> 8), (uint8_t)len, (uint8_t)((t & 1) << 4 | (t >> 1))};
      return k < 5 ? m[k] : k < 21 ? (uint8_t)hc[t].code_len_freq[k - 4] : (uint8_t)hc[t].sym_sorted[k - 21];
    }
    if (i < o_dri) {
      const int k = i - o_sof, len = 8 + 3 * nc;
      const uint8_t m[10] = {0xFF, 0xC0, (uint8_t)(len >> 8), (uint8_t)len, 0x08, (uint8_t)(F.h >> 8), (uint8_t)F.h,
                             (uint8_t)(F.w >> 8), (uint8_t)F.w, (uint8_t)nc};
      return k < 10 ? m[k] : F.sof[(k - 10) / 3][(k - 10) % 3];
    }
    if (i < o_sos) {
      const uint8_t m[6] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(F.ri >> 8), (uint8_t)F.ri};
      return m[i - o_dri];
    }
    const int k = i - o_sos;
    const uint8_t m[5] = {0xFF, 0xDA, 0x00, (uint8_t)(6 + 2 * nc), (uint8_t)nc};
    if (k < 5) return m[k];
    if (k < 5 + 2 * nc) {
      const int j = k - 5;
      return (j & 1) ? (uint8_t)((j >> 1) ? 0x11 : 0x00) : F.sof[j >> 1][0];
    }
    const uint8_t tail[3] = {0x00, 0x3F, 0x00};
    return tail[k - 5 - 2 * nc];
  };
  for (int i = tid; i < hlen; i += 256) out[i] = hbyte(i);  // hlen <= TC_HDR_MAX
  if (tid == 0) {
    a.hdr[f] = hlen;
    const unsigned long long end = (unsigned long long)hlen + nbytes + carry + 2ull * (unsigned long long)(F.nint - 1);
    out[end] = 0xFF;
    out[end + 1] = 0xD9;
    a.out_len[f] = end + 2;
  }
}

// ---- stuffed bytes and RSTn markers -----------------------------------------------------------
// Chunk c = entropy bytes [c * TC_CH, ..): thread t takes 16 of them.  Byte j
// leaves at hdr + j + (0xFF bytes before j) + 2 * (intervals begun at or
// before j, the first apart); the marker of interval i goes in front of its
// first byte, written by the chunk that holds that byte (also when it is the
// chunk's first).  The chunk is laid out in LDS and leaves in whole words.
__global__ __launch_bounds__(256) void k_tc_write(TcArgs a) {
  __shared__ uint32_t red[4];
  __shared__ uint32_t flags[TC_CH / 32];
  __shared__ __attribute__((aligned(16))) uint8_t s_out[3 * TC_CH + 16];
  const int f = blockIdx.y, tid = threadIdx.x;
  if (a.err[f] || !a.out_len[f]) return;
  const TcFrame &F = a.fr[f];
  const TcOut &O = a.o[f];
  const unsigned long long nbytes = a.bits[f] >> 3;
  const long long nch = (long long)((nbytes + TC_CH - 1) / TC_CH);
  const uint32_t *raw = a.raw + O.raw0;
  const unsigned long long *iv = a.ival_off + F.rowp0;
  uint8_t *out = a.out + O.out0 + a.hdr[f];
  for (long long c = blockIdx.x; c < nch; c += gridDim.x) {
    const unsigned long long c0 = (unsigned long long)c * TC_CH;
    const int nb = (int)min(nbytes - c0, (unsigned long long)TC_CH);
    // intervals 1 .. m0 begin before c0: their markers left with earlier chunks.
    // (An interval that begins exactly at c0 is this chunk's: the chunk that
    // holds an interval's first byte writes its marker.)
    int lo = 0, hi = F.nint - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;  // >= 1
      if ((iv[mid] >> 3) < c0) lo = mid;
      else hi = mid - 1;
    }
    const int m0 = lo;
    __syncthreads();  // (flags, s_out: the chunk before is out)
    if (tid < TC_CH / 32) flags[tid] = 0;
    __syncthreads();
    for (int i = m0 + 1 + tid; i < F.nint; i += 256) {
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
    uint8_t *d = out + c0 + a.ffc[O.chunk0 + c] + 2ull * (unsigned long long)m0;
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

// ---- launches ------------------------------------------------------------------------------------
hipError_t launch_tc_abs(const TcDc *jobs, int njobs, int max_blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_tc_abs, dim3((unsigned)((max_blocks + 255) / 256), njobs), dim3(256), 0, s, jobs);
  return hipGetLastError();
}

static dim3 tc_block_grid(const TcArgs &a) { return dim3((unsigned)((a.max_nblk + 255) / 256), a.nframes); }

hipError_t launch_tc_hist(const TcArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_tc_hist, tc_block_grid(a), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tc_sizes(const TcArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_tc_bits, tc_block_grid(a), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tc_rows, dim3(a.max_rows, a.nframes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tc_scan, dim3(a.nframes), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tc_write(const TcArgs &a, hipStream_t s) {
  const int nch = a.max_chunks < 1 ? 1 : a.max_chunks;
  const dim3 chunks((unsigned)(nch < 256 ? nch : 256), a.nframes);
  hipLaunchKernelGGL(k_tc_zero, dim3(64, a.nframes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tc_pack, tc_block_grid(a), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tc_ffcount, chunks, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tc_head, dim3(a.nframes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tc_write, chunks, dim3(256), 0, s, a);
  return hipGetLastError();
}

// The stages a progressive file's scans share with the one-scan coder
// (mij_progwrite.hip): each scan is a "frame" of TcArgs.
hipError_t launch_tc_layout(const TcArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_tc_rows, dim3(a.max_rows, a.nframes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_tc_scan, dim3(a.nframes), dim3(256), 0, s, a);
  return hipGetLastError();
}

static dim3 tc_chunk_grid(const TcArgs &a) {
  const int nch = a.max_chunks < 1 ? 1 : a.max_chunks;
  return dim3((unsigned)(nch < 256 ? nch : 256), a.nframes);
}

hipError_t launch_tc_zero(const TcArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_tc_zero, dim3(64, a.nframes), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tc_ffcount(const TcArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_tc_ffcount, tc_chunk_grid(a), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tc_stuffed(const TcArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_tc_write, tc_chunk_grid(a), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace mij
