// mij_huff.h -- canonical Huffman decoding tables and the MSB-first bit
// window, shared by the baseline decoder's kernels (mij_decode.hip), the
// progressive decoder's per-unit routine (mij_progressive.h) and the host
// programs that check the latter on the CPU (tests/progressive_check.cpp).
// Plain C++ under a host compiler, __host__ __device__ under hipcc.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MIJ_HUFF_HD __host__ __device__
#define MIJ_HUFF_FN __host__ __device__ __forceinline__
#else
#define MIJ_HUFF_HD
#define MIJ_HUFF_FN inline __attribute__((always_inline))
#endif

namespace mij {

constexpr int LOOK = 9;

// One canonical Huffman table (ISO/IEC 10918-1 F.2.2.3 decoding procedure).
struct DecTab {
  uint16_t look[1 << LOOK];  // (length << 8) | symbol, 0 = longer than LOOK
  int32_t maxcode[18];       // largest code of each length, -1 if none
  int32_t valoff[17];        // index of the first symbol of a length - its code
  uint8_t val[256];
};

// MSB-first bit window over an unstuffed, 8-byte aligned, zero-padded scan
struct Bits {
  const unsigned long long *w;
  long long cw = -2;  // index of the word pair held (none yet)
  unsigned long long hi = 0, lo = 0;
  MIJ_HUFF_HD unsigned long long window(long long pos) {
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
MIJ_HUFF_FN int decode_one(Bits &br, long long pos, const DecTab &t, int &sym, int &val) {
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

// host: a DHT segment's counts and symbols -> the table; -1 if over-subscribed
inline int build_table(DecTab &t, const uint8_t counts[16], const uint8_t *syms, int nsyms) {
  memset(&t, 0, sizeof t);
  memcpy(t.val, syms, nsyms);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; l++) {
    const int c = counts[l - 1];
    t.valoff[l] = k - code;
    t.maxcode[l] = c ? code + c - 1 : -1;
    // over-subscribed: refused before the lookahead is filled, whose index
    // (code << sh) would otherwise leave the table (a DHT may claim 255
    // codes of 1 bit)
    if (code + c > (1 << l)) return -1;
    for (int i = 0; i < c; i++, k++, code++) {
      if (l <= LOOK) {
        const int sh = LOOK - l;
        for (int f = 0; f < (1 << sh); f++) t.look[(code << sh) | f] = (uint16_t)((l << 8) | syms[k]);
      }
    }
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  return 0;
}

}  // namespace mij
