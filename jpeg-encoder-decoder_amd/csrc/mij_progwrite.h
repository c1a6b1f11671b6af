// mij_progwrite.h -- progressive output: the scan script,
// what one block contributes to one scan under the token rules of libjpeg's
// jcphuff.c, and what mij_progwrite.hip (kernels) and mij_decode.hip (host)
// share.  The per-block routines are written once here: the kernels run them
// per lane, and tests/progwrite_check.cpp compiles the same text with a host
// compiler under the sanitizers.  Not public.
#pragma once
#include "mij_huff.h"

namespace mij {

constexpr int PW_MAX_SCANS = 10;
constexpr int PW_MAX_EOBRUN = 0x7FFF;  // blocks in one end-of-band run
constexpr int PW_MAX_BE = 937;         // buffered correction bits above which a run is cut (MAX_CORR_BITS - 64 + 1)
// bytes outside the entropy data at most: APP0 20 + 3 DQT x 69 + SOF2 19 + 10 scans x (DRI 6 + SOS 14) + 10 DHT x (21 + 256)
constexpr int PW_HDR_MAX = 20 + 3 * 69 + 19 + PW_MAX_SCANS * (6 + 14) + 10 * (21 + 256);

// One scan of the script: components (bit c), Ss, Se, Ah, Al.
struct PwScript {
  int comps, ss, se, ah, al;
};
// libjpeg's jpeg_simple_progression for YCbCr; a one-component frame takes the scans of component 0
constexpr PwScript PW_SCRIPT[PW_MAX_SCANS] = {{7, 0, 0, 0, 1},  {1, 1, 5, 0, 2},  {4, 1, 63, 0, 1}, {2, 1, 63, 0, 1},
                                             {1, 6, 63, 0, 2}, {1, 1, 63, 2, 1}, {7, 0, 0, 1, 0},  {4, 1, 63, 1, 0},
                                             {2, 1, 63, 1, 0}, {1, 1, 63, 1, 0}};

// One (frame, scan) as the kernels see it, beside the TcFrame that holds its
// geometry (mij_transcode.h): the kernels take Ss, Se, Ah, Al from here and
// assume nothing else about the script.
struct PwScan {
  int frame;     // of the call
  int ss, se, ah, al;
  int comp;      // the frame's component of a one-component scan (0 for an interleaved one)
  int ncomp;     // components in the scan
  int tab[2];    // table slots: DC first of component 0 / of the others; an AC scan's in tab[0]
  int ntab;      // tables the scan writes: 0 (DC refinement), 1, 2
  int first;     // the frame's first scan
};

MIJ_HUFF_FN int pw_nbits(uint32_t v) {  // bit length, 0 for 0
#if defined(__HIP_DEVICE_COMPILE__)
  return 32 - __clz((int)v);
#else
  return v ? 32 - __builtin_clz(v) : 0;
#endif
}

MIJ_HUFF_FN int pw_clz(unsigned long long v) {  // leading zeros, v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __clzll((long long)v);
#else
  return __builtin_clzll(v);
#endif
}
MIJ_HUFF_FN int pw_ctz(unsigned long long v) {  // index of the lowest set bit, v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((long long)v) - 1;
#else
  return __builtin_ctzll(v);
#endif
}
MIJ_HUFF_FN int pw_popc(unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}

// What an AC scan (Ss, Se, Al) needs of a block, one bit per coefficient k of
// the band, from t = |c| >> Al: nz, t != 0; one, t == 1; lsb, t & 1; neg,
// c < 0.  The block is read once, as eight 16-byte lines (it is 128-byte
// aligned in the arena); everything else the scan does with it is bit
// arithmetic, but the values of an Ah = 0 scan's new coefficients.
struct PwMasks {
  unsigned long long nz, one, lsb, neg;
};
MIJ_HUFF_FN PwMasks pw_masks(const int16_t *blk, int ss, int se, int al) {
  PwMasks m = {0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) {
    int16_t v[8];
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint4 *)v = ((const uint4 *)blk)[i];
#else
    memcpy(v, blk + 8 * i, sizeof v);
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 8; j++) {
      const int c = v[j], t = (c < 0 ? -c : c) >> al;
      const unsigned long long b = 1ull << (8 * i + j);
      if (t) m.nz |= b;
      if (t == 1) m.one |= b;
      if (t & 1) m.lsb |= b;
      if (c < 0) m.neg |= b;
    }
  }
  // 1 <= Ss <= Se <= 63
  const unsigned long long band = (se >= 63 ? ~0ull : (1ull << (se + 1)) - 1ull) & ~((1ull << ss) - 1ull);
  m.nz &= band;
  m.one &= band;
  m.lsb &= band;
  m.neg &= band;
  return m;
}

// What the block contributes to the AC scan (Ss, Se, Ah, Al), as far as the
// run stage needs it: bit 0 E, the block emits a symbol of its own (which
// ends the run before it); bit 1 T, zeros or correction bits trail its last
// symbol, so it opens or extends an end-of-band run; bits 2.. BR, the
// correction bits that trail (0 when Ah = 0).
//
// Bounds: the masks hold bits Ss..Se only (the host's script table has 1 <=
// Ss <= Se <= 63); BR counts coefficients of the band, so BR <= 63 and the
// result fits a byte.
MIJ_HUFF_FN uint32_t pw_classify(const PwMasks &m, int se, int ah) {
  const unsigned long long sym = ah == 0 ? m.nz : m.one;  // the coefficients that get a symbol
  const bool tr = !((sym >> se) & 1ull);
  int br = 0;
  if (ah) {
    unsigned long long big = m.nz & ~m.one;
    if (m.one) {
      const int last = 63 - pw_clz(m.one);
      big &= last >= 63 ? 0ull : ~0ull << (last + 1);
    }
    br = pw_popc(big);
  }
  return (sym ? 1u : 0u) | (tr ? 2u : 0u) | ((uint32_t)br << 2);
}

// The block's own symbols in stream order: sym(symbol, extra value, extra
// bits <= 15) per Huffman-coded symbol, raw(bits, count <= 63) for the
// correction bits that follow one.  The correction bits that trail the last
// symbol are returned in (tbits, tn): they leave after the EOBn code of the
// run the block heads, or with the run it extends.
//
// Bounds: every k is the index of a set bit of m.nz, Ss <= k <= Se <= 63,
// inside the block's 64 coefficients; each trip clears one bit, so the loop
// ends; a run r never exceeds the band's length, so the symbol is < 256;
// pending correction bits count coefficients of the band seen since the last
// symbol, <= 63, so they fit tbits.
template <class Sym, class Raw>
MIJ_HUFF_FN void pw_walk_ac(const int16_t *blk, const PwMasks &m, int ss, int ah, int al, const Sym &sym, const Raw &raw,
                            unsigned long long &tbits, int &tn) {
  const int eob = m.one ? 63 - pw_clz(m.one) : 0;  // the last coefficient that becomes nonzero in a refinement scan
  unsigned long long left = m.nz, br = 0;
  int r = 0, prev = ss - 1, nbr = 0;
  while (left) {
    const int k = pw_ctz(left);
    left &= left - 1ull;
    r += k - prev - 1;  // the zeros since the coefficient before
    prev = k;
    if (ah == 0) {
      for (; r > 15; r -= 16) sym(0xF0, 0u, 0);
      const int c = blk[k], t = (c < 0 ? -c : c) >> al;
      const int nb = pw_nbits((uint32_t)t) & 15;
      sym((r << 4) | nb, (uint32_t)(c < 0 ? ~t : t) & ((1u << nb) - 1u), nb);
      r = 0;
      continue;
    }
    for (; r > 15 && k <= eob; r -= 16) {
      sym(0xF0, 0u, 0);
      raw(br, nbr);
      br = 0;
      nbr = 0;
    }
    if (!((m.one >> k) & 1ull)) {  // already nonzero: its next bit waits for the next symbol
      br = (br << 1) | ((m.lsb >> k) & 1ull);
      nbr++;
      continue;
    }
    sym((r << 4) | 1, (m.neg >> k) & 1ull ? 0u : 1u, 1);
    raw(br, nbr);
    br = 0;
    nbr = 0;
    r = 0;
  }
  tbits = br;
  tn = nbr;
}

// The Huffman-coded difference of a DC first scan: v = dc >> Al (arithmetic)
// of the block and of its predecessor in scan order (0 at an interval's start).
MIJ_HUFF_FN void pw_dc_first(int dc, int pred_dc, int has_pred, int al, int &sym, uint32_t &extra) {
  const int d = (dc >> al) - (has_pred ? pred_dc >> al : 0);
  sym = pw_nbits((uint32_t)(d < 0 ? -d : d)) & 15;
  extra = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << sym) - 1u);
}

// The EOBn symbol and extra bits of a run of len blocks, 1 <= len <= PW_MAX_EOBRUN
MIJ_HUFF_FN void pw_eobrun(int len, int &sym, uint32_t &extra, int &n) {
  n = pw_nbits((uint32_t)len) - 1;
  sym = n << 4;
  extra = (uint32_t)len - (1u << n);
}

}  // namespace mij

#if defined(__HIPCC__)
#include "mij_transcode.h"

namespace mij {

// One frame's place in the call: its scans [seg0, seg0 + nseg) and its table
// slots.  The frame's headers are its TcFrame's (PwArgs::fr).
struct PwFrame {
  int seg0, nseg;
  int pf0, npf;   // the builder's pseudo-frames of four tables each
  int ntab;       // tables in use; the slots after them get one count each
  int pad;
  long long out0, out_cap;
};

// seg: the scans of every frame, frame after frame; TcArgs seg describes them
// to the shared stages of mij_transcode.hip (a scan there is a "frame": its
// units are MCUs, its rows MCU rows).
struct PwArgs {
  TcArgs seg;            // per scan: fr, o, bits, hdr, err, out_len, blk_bits, ... (nframes = scans)
  const PwScan *sc;      // per scan
  const PwFrame *pf;     // per frame
  const TcFrame *fr;     // per frame: headers
  int nframes;
  int max_nint;
  uint8_t *info;         // per scan block: pw_classify
  uint16_t *runlen;      // per scan block: blocks of the run it heads, 0: heads none
  const int *perr;       // per pseudo-frame, from the table builder
  int *ferr;             // per frame
  uint64_t *flen;        // per frame
};

hipError_t launch_pw_count(const PwArgs &a, hipStream_t s);  // classify, runs, counts
hipError_t launch_pw_sizes(const PwArgs &a, hipStream_t s);  // after the tables: bits per block ... per scan
hipError_t launch_pw_write(const PwArgs &a, hipStream_t s);  // after the read-back of the scans' bits

}  // namespace mij
#endif
