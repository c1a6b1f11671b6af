// mij_progwrite.hip -- gfx950 kernels of progressive output:
// the coefficient planes the transcoder would code as one baseline scan
// become the scans of libjpeg's simple progression instead, each with tables
// optimised for it and restart intervals of whole rows of its own MCUs.
//
// A scan of a frame is a "segment": a TcFrame of its own (its units are the
// scan's MCUs: the frame's MCUs for the interleaved DC scans, the blocks of
// the component's own grid otherwise) beside a PwScan.  Per block of a scan
// the bits leave in this order: its own symbols, the EOBn code and extra bits
// if it heads an end-of-band run, the correction bits that trail its last
// symbol.  A run is its head followed by blocks without symbols of their own,
// so one prefix sum over those three places every bit, and no block needs
// another's bits: only the run's length at its head.
//
//   k_pw_class    per block of an AC scan: emits / trails / trailing bits
//   k_pw_runs     one wave per restart interval: the runs' heads and lengths
//   k_pw_hist     symbol counts per table (block symbols, one EOBn per head)
//   (k_tables_1w builds the tables, four per pseudo-frame)
//   k_pw_err      a frame whose table failed: all its scans fail
//   k_pw_bits     bits per block
//   (k_tc_rows, k_tc_scan: offsets, intervals rounded to bytes, bits per scan)
//   (k_tc_zero)
//   k_pw_pack     every block's bits at its offset, interval pad bits
//   (k_tc_ffcount)
//   k_pw_head     per frame: the headers of every scan behind the one before,
//                 chunk offsets, EOI, the length
//   (k_tc_write: stuffed bytes and RSTn markers of every scan)
#include "mij_ilcode.h"
#include "mij_progwrite.h"

namespace mij {

namespace {

// the thread's block of scan F: false past the scan's blocks
struct PwBlk {
  const int16_t *coef;
  int dc, pred_dc;
  bool has_pred;  // false: the interval starts here, predictor 0
  int c;          // the scan's component of the block
  int m, k;       // its unit and slot
  bool closes;    // the last block of a restart interval
};
__device__ __forceinline__ bool pw_block(const TcFrame &F, int i, PwBlk &b) {
  if (i >= F.nblk) return false;
  const int m = i / F.bpm, k = i - m * F.bpm;
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
  // < mcus_y * vs rows of bw >= mcus_x * hs blocks: inside the padded plane
  const int blk = (my * C.vs + jy) * C.bw + mx * C.hs + jx;
  int pred;
  if (j > 0) {
    pred = jx ? blk - 1 : blk - C.bw + C.hs - 1;
  } else if (mx == 0 && my % F.R == 0) {
    pred = -1;
  } else {  // the last block of the unit before
    const int py = mx ? my : my - 1, px = mx ? mx - 1 : F.mcus_x - 1;
    pred = (py * C.vs + C.vs - 1) * C.bw + px * C.hs + C.hs - 1;
  }
  b.dc = C.abs[blk];
  b.has_pred = pred >= 0;
  b.pred_dc = pred < 0 ? 0 : (int)C.abs[pred];
  b.coef = C.plane + 64LL * blk;
  b.c = c;
  b.m = m;
  b.k = k;
  b.closes = k == F.bpm - 1 && mx == F.mcus_x - 1 && ((my + 1) % F.R == 0 || my == F.mcus_y - 1);
  return true;
}

__device__ __forceinline__ unsigned long long above(int lane) { return lane >= 63 ? 0ull : ~0ull << (lane + 1); }

}  // namespace

// ---- what each block of an AC scan does to the runs ---------------------------------
__global__ __launch_bounds__(256) void k_pw_class(PwArgs a) {
  const int s = blockIdx.y;
  const PwScan S = a.sc[s];
  if (S.ss == 0) return;
  const TcFrame &F = a.seg.fr[s];
  const int i = blockIdx.x * 256 + threadIdx.x;
  PwBlk b;
  if (!pw_block(F, i, b)) return;
  a.info[F.blk0 + i] = (uint8_t)pw_classify(pw_masks(b.coef, S.ss, S.se, S.al), S.se, S.ah);
}

// ---- the runs of one restart interval: one wave walks its blocks 64 at a time --------
// A block with T set is in a run; the run's head is the latest block at or
// before it that has E set, follows a block without T, starts the interval,
// or follows a block at which a limit cut the run.  Inside a 64-block step
// every head but the cut ones is known from two ballots; a cut needs the
// count and the correction bits since the head (a wave prefix sum), and each
// cut moves the heads behind it, so the step is repeated from the first cut
// found: once per cut, and a cut needs more than 937 bits of at most 63 per
// block, or 0x7FFF blocks.  The run that is open at the step's end is carried
// (head, blocks, bits); its head's length is written when it closes.
// Every block's runlen is written exactly once.  A run is cut by the first
// block that takes it past 937 bits, and a block adds at most 63, so no run
// buffers more than 1000 bits (libjpeg's MAX_CORR_BITS) nor counts more than
// 0x7FFF blocks, which fits runlen's 16 bits.
__global__ __launch_bounds__(64) void k_pw_runs(PwArgs a) {
  const int s = blockIdx.y, iv = blockIdx.x, lane = threadIdx.x;
  const PwScan S = a.sc[s];
  if (S.ss == 0) return;
  const TcFrame &F = a.seg.fr[s];
  if (iv >= F.nint) return;
  const int u0 = iv * F.R * F.mcus_x, u1 = min((iv + 1) * F.R, F.mcus_y) * F.mcus_x;  // <= nblk (bpm is 1)
  const uint8_t *info = a.info + F.blk0;
  uint16_t *runlen = a.runlen + F.blk0;
  bool open = false;  // wave-uniform: the run carried into the step
  int H = 0, cnt0 = 0, be0 = 0;
  uint32_t next = u0 + lane < u1 ? info[u0 + lane] : 0u;
  for (int base = u0; base < u1; base += 64) {
    const int n = min(64, u1 - base);
    const uint32_t inf = next;
    if (base + 64 + lane < u1) next = info[base + 64 + lane];
    else next = 0u;
    const bool E = inf & 1u, T = inf & 2u;  // (both clear past the interval's end)
    const int tb = (int)(inf >> 2);
    const unsigned long long valid = n == 64 ? ~0ull : (1ull << n) - 1ull;
    const unsigned long long mE = __ballot(E), mT = __ballot(T);
    int P = tb;  // inclusive prefix sum of the trailing bits
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(P, o);
      if (lane >= o) P += u;
    }
    const int Pex = P - tb;
    const unsigned long long upto = ~above(lane);
    unsigned long long closed = 0, St = 0;
    int p = 0;  // the lanes before p are settled
    for (;;) {
      const unsigned long long inrun_prev = ((mT & ~closed) << 1) | (open ? 1ull : 0ull);
      St = mT & (mE | ~inrun_prev);
      const unsigned long long hm = St & upto;
      const int h = hm ? 63 - __clzll((long long)hm) : -1;
      const int pex_h = __shfl(Pex, h < 0 ? 0 : h);
      const int cnt = h < 0 ? cnt0 + lane + 1 : lane - h + 1;
      const int be = h < 0 ? be0 + P : P - pex_h;
      const bool lim = T && lane >= p && (cnt == PW_MAX_EOBRUN || be > PW_MAX_BE);
      const unsigned long long ml = __ballot(lim);
      if (!ml) break;
      const int q = __ffsll((long long)ml) - 1;
      closed |= 1ull << q;
      p = q + 1;
    }
    // the run ends in front of the next block that emits, heads a run or lies past the interval, or at a cut
    const unsigned long long B = mE | St | ~valid;
    const bool closed_last = closed >> 63;
    const int P63 = __shfl(P, 63);
    if (open) {
      if (B || closed_last) {
        if (lane == 0) runlen[H] = (uint16_t)(cnt0 + (B ? __ffsll((long long)B) - 1 : 64));
        open = false;
      } else {
        cnt0 += 64;
        be0 += P63;
      }
    }
    bool carries = false;
    if (lane < n) {
      int len = 0;
      if ((St >> lane) & 1ull) {
        const unsigned long long nb = B & above(lane);
        if (nb) len = __ffsll((long long)nb) - 1 - lane;
        else if (closed_last) len = 64 - lane;
        else carries = true;
      }
      if (!carries) runlen[base + lane] = (uint16_t)len;
    }
    const unsigned long long cm = __ballot(carries);
    if (cm) {  // (one lane at most: the step's last head)
      const int hl = __ffsll((long long)cm) - 1;
      open = true;
      H = base + hl;
      cnt0 = 64 - hl;
      be0 = P63 - __shfl(Pex, hl);
    }
  }
  if (open && lane == 0) runlen[H] = (uint16_t)cnt0;
}

// ---- symbol counts per table ----------------------------------------------------------
__global__ __launch_bounds__(256) void k_pw_hist(PwArgs a) {
  __shared__ uint32_t h[2][256];
  const int s = blockIdx.y;
  const PwScan S = a.sc[s];
  const TcFrame &F = a.seg.fr[s];
  // the slots a frame's tables leave unused: one count each, so that the builder has a code to make
  if (S.first && blockIdx.x == 0) {
    const PwFrame P = a.pf[S.frame];
    for (int t = P.ntab + threadIdx.x; t < 4 * P.npf; t += 256) a.seg.hist[((long long)P.pf0 * 4 + t) * 257] = 1u;
  }
  if (S.ntab == 0 || (long long)blockIdx.x * 256 >= F.nblk) return;
  for (int i = threadIdx.x; i < 512; i += 256) h[i >> 8][i & 255] = 0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  PwBlk b;
  if (pw_block(F, i, b)) {
    if (S.ss == 0) {
      int sym;
      uint32_t extra;
      pw_dc_first(b.dc, b.pred_dc, b.has_pred, S.al, sym, extra);
      atomicAdd(&h[b.c ? 1 : 0][sym], 1u);
    } else {
      const uint32_t inf = a.info[F.blk0 + i];
      if (inf & 1u) {
        unsigned long long tb;
        int tn;
        pw_walk_ac(b.coef, pw_masks(b.coef, S.ss, S.se, S.al), S.ss, S.ah, S.al,
                   [&](int sym, uint32_t, int) { atomicAdd(&h[0][sym & 255], 1u); }, [&](unsigned long long, int) {}, tb, tn);
      }
      const int len = a.runlen[F.blk0 + i];
      if (len) {
        int sym, n;
        uint32_t extra;
        pw_eobrun(len, sym, extra, n);
        atomicAdd(&h[0][sym], 1u);
      }
    }
  }
  __syncthreads();
  for (int i2 = threadIdx.x; i2 < 256 * S.ntab; i2 += 256) {
    const uint32_t v = h[i2 >> 8][i2 & 255];
    if (v) atomicAdd(&a.seg.hist[(long long)S.tab[i2 >> 8] * 257 + (i2 & 255)], v);
  }
}

// ---- a failed table fails its frame: every scan of it -------------------------------------
__global__ __launch_bounds__(256) void k_pw_err(PwArgs a) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= a.seg.nframes) return;
  const PwFrame P = a.pf[a.sc[s].frame];
  int e = 0;
  for (int q = 0; q < P.npf; q++)
    if (a.perr[P.pf0 + q]) e = a.perr[P.pf0 + q];
  a.seg.err[s] = e;
}

// ---- bits per block -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pw_bits(PwArgs a) {
  __shared__ uint32_t tab[2][256];
  const int s = blockIdx.y;
  if (a.seg.err[s]) return;
  const PwScan S = a.sc[s];
  const TcFrame &F = a.seg.fr[s];
  if ((long long)blockIdx.x * 256 >= F.nblk) return;
  for (int i = threadIdx.x; i < 256 * S.ntab; i += 256) tab[i >> 8][i & 255] = a.seg.ehuf[(long long)S.tab[i >> 8] * 256 + (i & 255)];
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  PwBlk b;
  if (!pw_block(F, i, b)) return;
  uint32_t bits = 0;
  if (S.ss == 0) {
    if (S.ah) {
      bits = 1;
    } else {
      int sym;
      uint32_t extra;
      pw_dc_first(b.dc, b.pred_dc, b.has_pred, S.al, sym, extra);
      bits = (tab[b.c ? 1 : 0][sym] >> 16) + sym;
    }
  } else {
    const uint32_t inf = a.info[F.blk0 + i];
    if (inf & 1u) {
      unsigned long long tb;
      int tn;
      pw_walk_ac(b.coef, pw_masks(b.coef, S.ss, S.se, S.al), S.ss, S.ah, S.al,
                 [&](int sym, uint32_t, int ne) { bits += (tab[0][sym & 255] >> 16) + ne; },
                 [&](unsigned long long, int nr) { bits += nr; }, tb, tn);
    }
    bits += inf >> 2;  // the trailing correction bits
    const int len = a.runlen[F.blk0 + i];
    if (len) {
      int sym, n;
      uint32_t extra;
      pw_eobrun(len, sym, extra, n);
      bits += (tab[0][sym] >> 16) + n;
    }
  }
  a.seg.blk_bits[F.blk0 + i] = (uint16_t)bits;  // <= 63 * (16 + 15) + 16 + 14 + 63
}

// ---- packing: thread = block, at its bit offset ------------------------------------------------
// As k_tc_pack: a block's first and last words are shared with its neighbours
// (atomic OR onto zeroed words); the words between are its own (plain
// stores).  Every store is guarded by the scan's words, which the host sized
// by the scan's bits.
__global__ __launch_bounds__(256) void k_pw_pack(PwArgs a) {
  __shared__ uint32_t tab[2][256];
  const int s = blockIdx.y;
  if (a.seg.err[s]) return;
  const PwScan S = a.sc[s];
  const TcFrame &F = a.seg.fr[s];
  if ((long long)blockIdx.x * 256 >= F.nblk) return;
  for (int i = threadIdx.x; i < 256 * S.ntab; i += 256) tab[i >> 8][i & 255] = a.seg.ehuf[(long long)S.tab[i >> 8] * 256 + (i & 255)];
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  PwBlk b;
  if (!pw_block(F, i, b)) return;
  const TcOut &O = a.seg.o[s];
  const uint16_t *bb = a.seg.blk_bits + F.blk0 + (long long)b.m * F.bpm;
  if (!bb[b.k] && !b.closes) return;
  unsigned long long pos = a.seg.row_off[F.rowp0 + b.m / F.mcus_x] + a.seg.mcu_off[F.mcu0 + b.m];
  for (int k = 0; k < b.k; k++) pos += bb[k];
  uint32_t *raw = a.seg.raw + O.raw0;
  unsigned long long wi = pos >> 5, acc = 0;
  int n = (int)(pos & 31);
  bool first = true;
  const unsigned long long wmax = (unsigned long long)O.raw_words;
  auto put = [&](uint32_t v, int len) {  // len <= 32, v < 2^len
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
  auto put_code = [&](int t, int sym) {
    const uint32_t e = tab[t][sym & 255];
    const int len = (int)(e >> 16);
    put(e & ((1u << len) - 1u), len);
  };
  auto put_raw = [&](unsigned long long v, int len) {  // len <= 63
    if (len > 32) {
      put((uint32_t)(v >> 32) & ((1u << (len - 32)) - 1u), len - 32);
      len = 32;
    }
    put(len == 32 ? (uint32_t)v : (uint32_t)v & ((1u << len) - 1u), len);
  };
  if (S.ss == 0) {
    if (S.ah) {
      put((uint32_t)(b.dc >> S.al) & 1u, 1);
    } else {
      int sym;
      uint32_t extra;
      pw_dc_first(b.dc, b.pred_dc, b.has_pred, S.al, sym, extra);
      put_code(b.c ? 1 : 0, sym);
      put(extra, sym);
    }
  } else {
    const uint32_t inf = a.info[F.blk0 + i];
    unsigned long long tb = 0;
    int tn = 0;
    if ((inf & 1u) || (inf >> 2))
      pw_walk_ac(b.coef, pw_masks(b.coef, S.ss, S.se, S.al), S.ss, S.ah, S.al,
                 [&](int sym, uint32_t extra, int ne) {
                   put_code(0, sym);
                   put(extra, ne);
                 },
                 put_raw, tb, tn);
    const int len = a.runlen[F.blk0 + i];
    if (len) {
      int sym, ne;
      uint32_t extra;
      pw_eobrun(len, sym, extra, ne);
      put_code(0, sym);
      put(extra, ne);
    }
    put_raw(tb, tn);
  }
  // the interval's last block pads it to a byte with 1-bits
  if (b.closes) {
    const int np = (8 - (n & 7)) & 7;
    put((1u << np) - 1u, np);
  }
  if (n > 0 && wi < wmax) atomicOr(&raw[wi], (uint32_t)(acc >> 32));
}

// ---- headers of every scan, chunk offsets, EOI, the length: one workgroup per frame ----------------
// SOI, APP0, the source's DQTs, SOF2 with the source's component entries;
// then per scan a DRI where the interval changes, the scan's DHTs, SOS, and
// room for its stuffed entropy data (k_tc_write fills it: hdr is where it
// begins); EOI.
__global__ __launch_bounds__(256) void k_pw_head(PwArgs a) {
  __shared__ uint32_t red[4];
  const int f = blockIdx.x, tid = threadIdx.x;
  const PwFrame P = a.pf[f];
  const TcFrame &F = a.fr[f];
  if (a.seg.err[P.seg0]) {  // (k_pw_err: the same for every scan of the frame)
    if (tid == 0) {
      a.ferr[f] = a.seg.err[P.seg0];
      a.flen[f] = 0;
    }
    if (tid < P.nseg) a.seg.out_len[P.seg0 + tid] = 0;
    return;
  }
  uint8_t *out = a.seg.out + P.out0;
  const int nc = F.ncomp;
  const int h0 = 20 + 69 * F.ndqt + 10 + 3 * nc;
  unsigned long long pos = (unsigned long long)h0;
  int ri_cur = 0;
  bool ok = true;
  for (int j = 0; j < P.nseg; j++) {
    const int s = P.seg0 + j;
    const PwScan S = a.sc[s];
    const TcFrame &G = a.seg.fr[s];
    const TcOut &O = a.seg.o[s];
    const unsigned long long nbytes = a.seg.bits[s] >> 3;
    const long long nch = (long long)((nbytes + TC_CH - 1) / TC_CH);
    uint32_t *ffc = a.seg.ffc + O.chunk0;
    unsigned long long carry = 0;  // 0xFF bytes of the chunks before
    for (long long c0 = 0; c0 < nch; c0 += 256) {
      const long long c = c0 + tid;
      const uint32_t v = c < nch ? ffc[c] : 0u;
      uint32_t tot;
      const uint32_t incl = il_scan256(v, red, tot);
      if (c < nch) ffc[c] = (uint32_t)carry + incl - v;
      carry += tot;
    }
    const int dri = G.ri != ri_cur ? 6 : 0;
    ri_cur = G.ri;
    int ns[2] = {0, 0};
    for (int t = 0; t < S.ntab; t++)
      for (int l = 1; l <= 16; l++) ns[t] += a.seg.hc[S.tab[t]].code_len_freq[l];
    const int o_dht1 = dri + (S.ntab > 0 ? 21 + ns[0] : 0), o_sos = o_dht1 + (S.ntab > 1 ? 21 + ns[1] : 0);
    const int hl = o_sos + 8 + 2 * S.ncomp;
    const unsigned long long ent = nbytes + carry + 2ull * (unsigned long long)(G.nint - 1);
    if (pos + hl + ent + 2ull > (unsigned long long)P.out_cap) {  // (the host sized it for 2 * nbytes: not reached)
      ok = false;
      break;
    }
    auto hbyte = [&](int i) -> uint8_t {
      if (i < dri) {
        const uint8_t m[6] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(G.ri >> 8), (uint8_t)G.ri};
        return m[i];
      }
      if (i < o_sos) {
        const int t = i >= o_dht1 ? 1 : 0, k = i - (t ? o_dht1 : dri), len = 19 + ns[t];
        const HuffCode &hc = a.seg.hc[S.tab[t]];
        // DC 00 / AC 10 for component 0, 01 / 11 for the others
        const uint8_t id = S.ss == 0 ? (uint8_t)t : (uint8_t)(0x10 | (S.comp ? 1 : 0));
        const uint8_t m[5] = {0xFF, 0xC4, (uint8_t)(len >> 8), (uint8_t)len, id};
        return k < 5 ? m[k] : k < 21 ? (uint8_t)hc.code_len_freq[k - 4] : (uint8_t)hc.sym_sorted[k - 21];
      }
      const int k = i - o_sos;
      const uint8_t m[5] = {0xFF, 0xDA, 0x00, (uint8_t)(6 + 2 * S.ncomp), (uint8_t)S.ncomp};
      if (k < 5) return m[k];
      if (k < 5 + 2 * S.ncomp) {
        const int q = k - 5, c = S.ncomp > 1 ? q >> 1 : S.comp;
        return (q & 1) ? (uint8_t)(c ? 0x11 : 0x00) : F.sof[c][0];
      }
      const uint8_t tail[3] = {(uint8_t)S.ss, (uint8_t)S.se, (uint8_t)(S.ah << 4 | S.al)};
      return tail[k - 5 - 2 * S.ncomp];
    };
    for (int i = tid; i < hl; i += 256) out[pos + i] = hbyte(i);  // pos + hl + ent + 2 <= out_cap
    if (tid == 0) {
      a.seg.hdr[s] = (int)(pos + hl);  // (the host refuses frames of 2 GiB)
      a.seg.out_len[s] = 1;
    }
    pos += hl + ent;
  }
  if (!ok) {
    __syncthreads();
    if (tid == 0) {
      a.ferr[f] = FERR_OVERFLOW;
      a.flen[f] = 0;
    }
    if (tid < P.nseg) a.seg.out_len[P.seg0 + tid] = 0;
    return;
  }
  auto head = [&](int i) -> uint8_t {
    if (i < 20) {
      const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 0x4A, 0x46, 0x49, 0x46,
                                0x00, 0x01, 0x01, 0x00, 0x00, 0x48, 0x00, 0x48, 0x00, 0x00};
      return app0[i];
    }
    if (i < 20 + 69 * F.ndqt) {
      const int t = (i - 20) / 69, k = (i - 20) - 69 * t;
      const uint8_t m[5] = {0xFF, 0xDB, 0x00, 0x43, F.dqt_id[t]};
      return k < 5 ? m[k] : F.dqt[t][k - 5];
    }
    const int k = i - 20 - 69 * F.ndqt, len = 8 + 3 * nc;
    const uint8_t m[10] = {0xFF, 0xC2, (uint8_t)(len >> 8), (uint8_t)len, 0x08, (uint8_t)(F.h >> 8), (uint8_t)F.h,
                           (uint8_t)(F.w >> 8), (uint8_t)F.w, (uint8_t)nc};
    return k < 10 ? m[k] : F.sof[(k - 10) / 3][(k - 10) % 3];
  };
  for (int i = tid; i < h0; i += 256) out[i] = head(i);
  if (tid == 0) {
    out[pos] = 0xFF;
    out[pos + 1] = 0xD9;
    a.ferr[f] = 0;
    a.flen[f] = pos + 2;
  }
}

// ---- launches -------------------------------------------------------------------------------------
static dim3 pw_block_grid(const PwArgs &a) { return dim3((unsigned)((a.seg.max_nblk + 255) / 256), a.seg.nframes); }

hipError_t launch_pw_count(const PwArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_pw_class, pw_block_grid(a), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_pw_runs, dim3(a.max_nint, a.seg.nframes), dim3(64), 0, s, a);
  hipLaunchKernelGGL(k_pw_hist, pw_block_grid(a), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pw_sizes(const PwArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_pw_err, dim3((a.seg.nframes + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_pw_bits, pw_block_grid(a), dim3(256), 0, s, a);
  return launch_tc_layout(a.seg, s);
}

hipError_t launch_pw_write(const PwArgs &a, hipStream_t s) {
  if (hipError_t e = launch_tc_zero(a.seg, s)) return e;
  hipLaunchKernelGGL(k_pw_pack, pw_block_grid(a), dim3(256), 0, s, a);
  if (hipError_t e = launch_tc_ffcount(a.seg, s)) return e;
  hipLaunchKernelGGL(k_pw_head, dim3(a.nframes), dim3(256), 0, s, a);
  return launch_tc_stuffed(a.seg, s);
}

}  // namespace mij
