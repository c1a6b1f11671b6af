// mij_progressive.h -- progressive JPEG (SOF2, 8-bit, Huffman): the host's
// parser with the scan-script checks of T.81 G.1.1.1, and the routine that
// decodes one restart interval of one scan into the coefficient planes
// (T.81 G.1.2 / G.2; the four procedures of libjpeg's jdphuff.c).  Both are
// written once here: the routine is what k_prog_scan runs per lane
// (mij_progressive.hip), and tests/progressive_check.cpp compiles the same
// text with a host compiler under the sanitizers.
#pragma once
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "mij_huff.h"

namespace mij {

constexpr int PROG_MAX_SCANS = 64;  // per stream; refused above (libjpeg's and mozjpeg's scripts use 6 to 12)

// per-scan status codes: 5 = the interval's bits end before its blocks do,
// 6 = invalid Huffman code or symbol, 8 = an EOB run reaches past the
// interval's last block, 9 = a coefficient index past Se
enum { PROG_OK = 0, PROG_SHORT = 5, PROG_CODE = 6, PROG_EOBRUN = 8, PROG_PAST_SE = 9 };

// One scan as the device sees it.  A scan of one component walks that
// component's own block grid ceil(w_c / 8) x ceil(h_c / 8): mcus_x is the
// grid's width and hs == vs == 1.  A scan of several components walks the
// frame's MCU grid, hs x vs blocks per component.  Either way block `slot`
// of MCU m lies at block row my * vs + slot_y, column mx * hs + slot_x of a
// plane whose rows are bw blocks apart (the padded plane's stride).
struct ProgScanDev {
  long long off[3];  // first int16 of each listed component's padded plane
  int ns, bpm;
  int ss, se, ah, al;
  int mcus_x, nmcus;
  int hs[3], vs[3], bw[3];
  int dc[3], ac;  // table indices; ac: the one component of an AC scan
  int slot_comp[6], slot_x[6], slot_y[6];
};

// The unit of work: one restart interval (a whole scan without DRI)
struct ProgUnit {
  long long data;   // byte offset of the UNSTUFFED interval in the blob (8-aligned, >= 16 zero bytes behind)
  long long nbits;  // its length in bits
  int scan;         // index into the ProgScanDev table
  int mcu0, nmcus;  // the scan's MCUs [mcu0, mcu0 + nmcus)
  int pad;
};

MIJ_HUFF_FN int16_t *prog_block(const ProgScanDev &S, int16_t *coefs, int mcu, int slot) {
  const int c = S.slot_comp[slot];
  const int my = mcu / S.mcus_x, mx = mcu - my * S.mcus_x;
  return coefs + S.off[c] + 64 * ((long long)(my * S.vs[c] + S.slot_y[slot]) * S.bw[c] + mx * S.hs[c] + S.slot_x[slot]);
}

// Decodes unit U sequentially from its first bit; returns a status code.
//
// Bounds, whatever the bits say.  Reads: every window is taken at pos <
// nbits (the checks precede each call) and covers words pos / 64 and pos /
// 64 + 1, at most 15 bytes past the interval's last byte; every slot ends in
// >= 16 zero bytes.  A symbol may end past nbits (in those zeros): that is
// PROG_SHORT, found before the next read.  Progress: every loop iteration
// below either consumes >= 1 bit at pos < nbits or advances k or the block,
// so the work is bounded by nbits + 64 * blocks.  Coefficients: k starts at
// Ss and a store at k is preceded by k <= Se <= 63 (PROG_PAST_SE otherwise).
// Blocks: the loops run over block index b < nmcus * bpm of the unit only; an
// EOB run is accepted only if it ends at or before the unit's last block
// (PROG_EOBRUN otherwise), so the run counter never skips past it.  Stores:
// MCU mcu0 + b / bpm < the scan's MCU count (the host checks mcu0 + nmcus <=
// mcus_x * mcus_y before any launch), so the block row is < mcus_y * vs <=
// the plane's block rows and the column < mcus_x * hs <= bw: inside the
// component's padded plane (prog_block).
MIJ_HUFF_HD inline int prog_decode_unit(const uint8_t *blob, const ProgUnit &U, const ProgScanDev &S, const DecTab *tabs,
                                   int16_t *coefs) {
  Bits br{(const unsigned long long *)(blob + U.data)};
  const long long nbits = U.nbits;
  long long pos = 0;
  int sym, val;
  if (S.ss == 0) {  // DC scan: first (a Huffman-coded difference, << Al) or refinement (one bit per block)
    int pred[3] = {0, 0, 0};
    for (int m = 0; m < U.nmcus; m++)
      for (int slot = 0; slot < S.bpm; slot++) {
        int16_t *b = prog_block(S, coefs, U.mcu0 + m, slot);
        if (pos >= nbits) return PROG_SHORT;
        if (S.ah == 0) {
          const int c = S.slot_comp[slot];
          const int n = decode_one(br, pos, tabs[S.dc[c]], sym, val);
          if (!n || sym > 15) return PROG_CODE;
          pos += n;
          pred[c] += val;
          b[0] = (int16_t)((uint32_t)pred[c] << S.al);
        } else {
          if (br.window(pos) >> 63) b[0] = (int16_t)(b[0] | (1 << S.al));
          pos++;
        }
      }
    return pos > nbits ? PROG_SHORT : PROG_OK;
  }
  // AC scan: one component, so bpm == 1 and MCU == block
  const DecTab &ac = tabs[S.ac];
  const int p1 = 1 << S.al, m1 = -(1 << S.al);
  long long eobrun = 0;  // blocks still covered by an end-of-band run, this one included
  for (int m = 0; m < U.nmcus; m++) {
    int16_t *b = prog_block(S, coefs, U.mcu0 + m, 0);
    int k = S.ss;
    if (S.ah == 0) {  // first pass over the band
      if (eobrun > 0) {
        eobrun--;
        continue;
      }
      while (k <= S.se) {
        if (pos >= nbits) return PROG_SHORT;
        const int n = decode_one(br, pos, ac, sym, val);
        if (!n) return PROG_CODE;
        pos += n;
        const int r = sym >> 4;
        if (sym & 15) {
          k += r;
          if (k > S.se) return PROG_PAST_SE;
          b[k++] = (int16_t)((uint32_t)val << S.al);
        } else if (r == 15) {
          k += 16;  // ZRL
        } else {    // EOBr: this block and (1 << r) + bits - 1 more
          eobrun = 1LL << r;
          if (r) {
            if (pos >= nbits) return PROG_SHORT;
            eobrun += (long long)(br.window(pos) >> (64 - r));
            pos += r;
          }
          if (eobrun > U.nmcus - m) return PROG_EOBRUN;
          eobrun--;
          break;
        }
      }
    } else {  // refinement: correction bits on nonzero history, new +-(1 << Al) values
      if (eobrun == 0) {
        while (k <= S.se) {
          if (pos >= nbits) return PROG_SHORT;
          const int n = decode_one(br, pos, ac, sym, val);
          if (!n) return PROG_CODE;
          pos += n;
          int r = sym >> 4;
          const int s = sym & 15;
          int newval = 0;
          if (s) {
            if (s != 1) return PROG_CODE;  // a new coefficient is +-1 at this bit
            newval = val > 0 ? p1 : m1;
          } else if (r != 15) {
            eobrun = 1LL << r;
            if (r) {
              if (pos >= nbits) return PROG_SHORT;
              eobrun += (long long)(br.window(pos) >> (64 - r));
              pos += r;
            }
            if (eobrun > U.nmcus - m) return PROG_EOBRUN;
            break;  // the rest of the band is handled as an end-of-band below
          }
          // over r zero-history coefficients (16 for ZRL), correcting the nonzero ones passed
          while (k <= S.se) {
            if (b[k]) {
              if (pos >= nbits) return PROG_SHORT;
              if ((br.window(pos) >> 63) && !(b[k] & p1)) b[k] = (int16_t)(b[k] + (b[k] >= 0 ? p1 : m1));
              pos++;
            } else if (--r < 0) {
              break;
            }
            k++;
          }
          if (newval) {
            if (k > S.se) return PROG_PAST_SE;
            b[k] = (int16_t)newval;
          }
          k++;
        }
      }
      if (eobrun > 0) {  // correction bits of what is left of the band
        for (; k <= S.se; k++)
          if (b[k]) {
            if (pos >= nbits) return PROG_SHORT;
            if ((br.window(pos) >> 63) && !(b[k] & p1)) b[k] = (int16_t)(b[k] + (b[k] >= 0 ? p1 : m1));
            pos++;
          }
        eobrun--;
      }
    }
  }
  return pos > nbits ? PROG_SHORT : PROG_OK;
}

// ---------------------------------------------------------------------------
// host: parsing
// ---------------------------------------------------------------------------
struct ProgIvl {
  long long data, end;  // raw bytes of one restart interval
};

struct ProgScan {
  int ns = 0;
  int comp[3] = {0, 0, 0};  // indices into the frame's components, ascending
  int tdi[3] = {-1, -1, -1}, tai = -1;  // the table snapshots in force (indices into ProgFrame::tabs)
  int ss = 0, se = 0, ah = 0, al = 0;
  int ri = 0;             // the restart interval in force, in the scan's own MCUs
  int mcus_x = 0, mcus_y = 0;  // the scan's own MCU grid
  int level = 0;
  std::vector<ProgIvl> ivl;
};

struct ProgFrame {
  int w = 0, h = 0, ncomp = 0;
  int cid[3] = {0, 0, 0}, hs[3] = {1, 1, 1}, vs[3] = {1, 1, 1}, tq[3] = {0, 0, 0};
  uint8_t decl_hv[3] = {0x11, 0x11, 0x11};
  int hmax = 1, vmax = 1, mcus_x = 0, mcus_y = 0;
  int bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};  // padded planes, in blocks
  int gw[3] = {0, 0, 0}, gh[3] = {0, 0, 0};  // the components' own block grids
  int adobe = -1;
  uint8_t dqt[4][64];
  bool have_dqt[4] = {false, false, false, false};
  std::vector<DecTab> tabs;  // one per DHT table definition, in stream order
  std::vector<ProgScan> scans;
  int levels = 0;
  char err[200] = "";
};

// 0, or 8 (MIJ_EJPEG) with the reason in F.err
// accept440: luma 1x2 is admitted too (MIJ_ACCEPT_440)
inline int prog_parse(const uint8_t *s, size_t n, ProgFrame &F, int frame, bool accept440 = false) {
#define PBAD(...)                                \
  do {                                           \
    snprintf(F.err, sizeof F.err, __VA_ARGS__);  \
    return 8;                                    \
  } while (0)
  auto be16 = [](const uint8_t *p) { return (p[0] << 8) | p[1]; };
  if (n < 4 || s[0] != 0xFF || s[1] != 0xD8) PBAD("stream %d: no SOI", frame);
  int cur[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};  // [Tc][Th] -> snapshot
  int ri = 0;
  int last_al[3][64];
  for (auto &row : last_al)
    for (int &v : row) v = -1;  // never coded
  size_t i = 2;
  while (i + 4 <= n) {
    if (s[i] != 0xFF) PBAD("stream %d: marker expected at byte %zu", frame, i);
    const int m = s[i + 1];
    if (m == 0xFF) {
      i++;
      continue;
    }
    if (m == 0xD9) break;
    if (m >= 0xD0 && m <= 0xD7) PBAD("stream %d: restart marker RST%d without a restart interval in force", frame, m - 0xD0);
    const int len = be16(s + i + 2);
    if (len < 2 || i + 2 + len > n) PBAD("stream %d: segment 0x%02X length %d", frame, m, len);
    const uint8_t *q = s + i + 4;
    const int body = len - 2;
    if (m == 0xDB) {
      if (!F.scans.empty()) PBAD("stream %d: DQT after the first scan of a progressive frame", frame);
      for (int o = 0; o < body; o += 65) {
        const int tq = q[o] & 15;
        if (q[o] >> 4) PBAD("stream %d: 16-bit DQT (Pq %d) is not baseline 8-bit", frame, q[o] >> 4);
        if (tq > 3 || o + 65 > body) PBAD("stream %d: DQT Tq %d / length", frame, tq);
        memcpy(F.dqt[tq], q + o + 1, 64);
        F.have_dqt[tq] = true;
      }
    } else if (m == 0xC4) {
      int o = 0;
      while (o + 17 <= body) {
        const int tc = q[o] >> 4, th = q[o] & 15;
        if (tc > 1 || th > 3) PBAD("stream %d: DHT Tc/Th %02X", frame, q[o]);
        int nsym = 0;
        for (int l = 0; l < 16; l++) nsym += q[o + 1 + l];
        if (nsym > 256 || o + 17 + nsym > body) PBAD("stream %d: DHT symbol count %d", frame, nsym);
        DecTab t;
        if (build_table(t, q + o + 1, q + o + 17, nsym)) PBAD("stream %d: DHT code over-subscribed", frame);
        cur[tc][th] = (int)F.tabs.size();
        F.tabs.push_back(t);
        o += 17 + nsym;
      }
    } else if (m == 0xC2) {
      if (F.ncomp) PBAD("stream %d: second SOF2", frame);
      if (body < 6) PBAD("stream %d: SOF2 length", frame);
      if (q[0] != 8) PBAD("stream %d: %d-bit samples (only 8-bit)", frame, q[0]);
      const int nc = q[5];
      if (nc != 1 && nc != 3) PBAD("stream %d: %d components (only greyscale and YCbCr)", frame, nc);
      if (body < 6 + 3 * nc) PBAD("stream %d: SOF2 length", frame);
      F.h = be16(q + 1);
      F.w = be16(q + 3);
      if (F.w <= 0 || F.h <= 0) PBAD("stream %d: %dx%d", frame, F.w, F.h);
      for (int c = 0; c < nc; c++) {
        const uint8_t *e = q + 6 + 3 * c;
        F.cid[c] = e[0];
        F.decl_hv[c] = e[1];
        F.hs[c] = e[1] >> 4;
        F.vs[c] = e[1] & 15;
        F.tq[c] = e[2];
        if (F.hs[c] < 1 || F.hs[c] > 4 || F.vs[c] < 1 || F.vs[c] > 4 || F.tq[c] > 3)
          PBAD("stream %d: SOF2 component %d sampling %dx%d / Tq %d", frame, c, F.hs[c], F.vs[c], F.tq[c]);
        for (int b = 0; b < c; b++)
          if (F.cid[b] == F.cid[c]) PBAD("stream %d: SOF2 repeats component id %d", frame, F.cid[c]);
      }
      if (nc == 1) {
        F.hs[0] = F.vs[0] = 1;
      } else {
        if (F.hs[1] != 1 || F.vs[1] != 1 || F.hs[2] != 1 || F.vs[2] != 1)
          PBAD("stream %d: chroma sampling %dx%d / %dx%d (only 1x1)", frame, F.hs[1], F.vs[1], F.hs[2], F.vs[2]);
        if (!(F.hs[0] <= 2 && F.vs[0] <= F.hs[0]) && !(accept440 && F.hs[0] == 1 && F.vs[0] == 2)) {
          if (accept440) PBAD("stream %d: luma sampling %dx%d (only 1x1, 2x1, 2x2, 1x2)", frame, F.hs[0], F.vs[0]);
          PBAD("stream %d: luma sampling %dx%d (only 1x1, 2x1, 2x2)", frame, F.hs[0], F.vs[0]);
        }
      }
      F.ncomp = nc;
      F.hmax = F.hs[0];
      F.vmax = F.vs[0];
      F.mcus_x = (F.w + 8 * F.hmax - 1) / (8 * F.hmax);
      F.mcus_y = (F.h + 8 * F.vmax - 1) / (8 * F.vmax);
      for (int c = 0; c < nc; c++) {
        F.bw[c] = F.mcus_x * F.hs[c];
        F.bh[c] = F.mcus_y * F.vs[c];
        const int wc = (F.w * F.hs[c] + F.hmax - 1) / F.hmax, hc = (F.h * F.vs[c] + F.vmax - 1) / F.vmax;
        F.gw[c] = (wc + 7) / 8;
        F.gh[c] = (hc + 7) / 8;
      }
    } else if (m == 0xC0 || m == 0xC1 || m == 0xC3 || (m >= 0xC5 && m <= 0xCF && m != 0xC8 && m != 0xCC)) {
      PBAD("stream %d: SOF 0x%02X in a progressive stream", frame, m);
    } else if (m == 0xDD) {
      if (body != 2) PBAD("stream %d: DRI length", frame);
      ri = be16(q);
    } else if (m == 0xEE) {
      if (body >= 12 && !memcmp(q, "Adobe", 5)) F.adobe = q[11];
    } else if (m == 0xDA) {
      if (!F.ncomp) PBAD("stream %d: SOS before SOF2", frame);
      if (body < 1 || body != 4 + 2 * q[0]) PBAD("stream %d: SOS length", frame);
      const int k = (int)F.scans.size();
      if (k >= PROG_MAX_SCANS) PBAD("stream %d: more than %d scans", frame, PROG_MAX_SCANS);
      ProgScan sc;
      sc.ns = q[0];
      if (sc.ns < 1 || sc.ns > F.ncomp) PBAD("stream %d scan %d: %d components in a %d-component frame", frame, k, sc.ns, F.ncomp);
      const uint8_t *tail = q + 1 + 2 * sc.ns;
      sc.ss = tail[0];
      sc.se = tail[1];
      sc.ah = tail[2] >> 4;
      sc.al = tail[2] & 15;
      if (sc.ss == 0 ? sc.se != 0 : (sc.se < sc.ss || sc.se > 63))
        PBAD("stream %d scan %d: Ss %d Se %d (a DC scan has Se 0, an AC scan Ss <= Se <= 63)", frame, k, sc.ss, sc.se);
      if (sc.ss > 0 && sc.ns != 1) PBAD("stream %d scan %d: AC scan of %d components (only 1)", frame, k, sc.ns);
      if (sc.al > 13) PBAD("stream %d scan %d: Al %d (at most 13)", frame, k, sc.al);
      for (int j = 0; j < sc.ns; j++) {
        int c = -1;
        for (int x = 0; x < F.ncomp; x++)
          if (q[1 + 2 * j] == F.cid[x]) c = x;
        if (c < 0 || (j && c <= sc.comp[j - 1]))
          PBAD("stream %d scan %d: SOS selectors are not SOF2 components in order", frame, k);
        sc.comp[j] = c;
        const int td = q[2 + 2 * j] >> 4, ta = q[2 + 2 * j] & 15;
        if (td > 3 || ta > 3) PBAD("stream %d scan %d: SOS table ids", frame, k);
        // a DC refinement scan reads no Huffman code at all
        if (sc.ss == 0 && sc.ah == 0 && (sc.tdi[j] = cur[0][td]) < 0)
          PBAD("stream %d scan %d: DC Huffman table %d missing before the scan", frame, k, td);
        if (sc.ss > 0 && (sc.tai = cur[1][ta]) < 0)
          PBAD("stream %d scan %d: AC Huffman table %d missing before the scan", frame, k, ta);
        if (sc.ss > 0 && last_al[c][0] < 0)
          PBAD("stream %d scan %d: AC scan of component %d before its DC scan", frame, k, c);
        for (int z = sc.ss; z <= sc.se; z++) {
          const int prev = last_al[c][z];
          if (prev < 0 ? sc.ah != 0 : (sc.ah != prev || sc.al != sc.ah - 1))
            PBAD("stream %d scan %d: component %d coefficient %d: Ah %d Al %d after %s %d (successive approximation "
                 "out of order)", frame, k, c, z, sc.ah, sc.al, prev < 0 ? "no scan," : "Al", prev < 0 ? 0 : prev);
          last_al[c][z] = sc.al;
        }
      }
      if (sc.ns == 1) {
        sc.mcus_x = F.gw[sc.comp[0]];
        sc.mcus_y = F.gh[sc.comp[0]];
      } else {
        sc.mcus_x = F.mcus_x;
        sc.mcus_y = F.mcus_y;
      }
      sc.ri = ri;
      sc.level = 1;
      for (const ProgScan &e : F.scans) {
        bool share = false;
        for (int a = 0; a < e.ns; a++)
          for (int b = 0; b < sc.ns; b++) share |= e.comp[a] == sc.comp[b];
        if (share && e.ss <= sc.se && sc.ss <= e.se) sc.level = std::max(sc.level, e.level + 1);
      }
      F.levels = std::max(F.levels, sc.level);
      // the entropy data: as the baseline parser finds it (mij_decode.hip)
      size_t e = i + 2 + len;
      long long start = (long long)e;
      const long long nm = (long long)sc.mcus_x * sc.mcus_y;
      const long long want = ri ? (nm + ri - 1) / ri : 1;
      for (;;) {
        const uint8_t *f = (const uint8_t *)memchr(s + e, 0xFF, n - e);
        if (!f || (size_t)(f - s) + 1 >= n) PBAD("stream %d: scan %d runs to the end", frame, k);
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
        if (b >= 0xD0 && b <= 0xD7 && ri) {
          const int iv = (int)sc.ivl.size();
          if (b != 0xD0 + (iv & 7))
            PBAD("stream %d scan %d: restart marker RST%d where RST%d is due (interval %d)", frame, k, b - 0xD0, iv & 7, iv);
          if (iv + 1 >= want) PBAD("stream %d scan %d: more restart markers than its %lld intervals need", frame, k, want);
          sc.ivl.push_back({start, (long long)e});
          e += 2;
          start = (long long)e;
          continue;
        }
        break;
      }
      sc.ivl.push_back({start, (long long)e});
      if ((long long)sc.ivl.size() != want)
        PBAD("stream %d scan %d: %zu restart intervals, %lld expected (%lld MCUs, interval %d)", frame, k, sc.ivl.size(),
             want, nm, ri);
      F.scans.push_back(sc);
      i = e;
      continue;
    }
    i += 2 + len;
  }
  if (!F.ncomp) PBAD("stream %d: no SOF2", frame);
  if (F.ncomp == 3 && (F.adobe == 0 || F.adobe == 2))
    PBAD("stream %d: Adobe APP14 transform %d (RGB / YCCK), only YCbCr", frame, F.adobe);
  for (int c = 0; c < F.ncomp; c++) {
    if (!F.have_dqt[F.tq[c]]) PBAD("stream %d: DQT %d of component %d missing", frame, F.tq[c], c);
    for (int z = 0; z < 64; z++)
      if (last_al[c][z] != 0) {
        if (last_al[c][z] < 0) PBAD("stream %d: incomplete scan script: component %d coefficient %d is never coded", frame, c, z);
        PBAD("stream %d: incomplete scan script: component %d coefficient %d ends at Al %d", frame, c, z, last_al[c][z]);
      }
  }
  return 0;
#undef PBAD
}

// The device tables of frame F's scans and units.  off[c]: first int16 of
// component c's padded plane; piece(scan, interval) -> (blob offset,
// unstuffed bytes); tab0: index of F.tabs[0] in the call's table array.
// Scans and units are appended in stream order.  Returns -1 if an interval
// would hold no MCU.
template <class PieceFn>
inline int prog_tables(const ProgFrame &F, const long long off[3], int tab0, PieceFn piece,
                       std::vector<ProgScanDev> &scans, std::vector<ProgUnit> &units) {
  for (size_t k = 0; k < F.scans.size(); k++) {
    const ProgScan &sc = F.scans[k];
    ProgScanDev S;
    memset(&S, 0, sizeof S);
    S.ns = sc.ns;
    S.ss = sc.ss, S.se = sc.se, S.ah = sc.ah, S.al = sc.al;
    S.mcus_x = sc.mcus_x;
    S.nmcus = sc.mcus_x * sc.mcus_y;
    for (int j = 0; j < sc.ns; j++) {
      const int c = sc.comp[j];
      S.off[j] = off[c];
      S.hs[j] = sc.ns == 1 ? 1 : F.hs[c];
      S.vs[j] = sc.ns == 1 ? 1 : F.vs[c];
      S.bw[j] = F.bw[c];
      S.dc[j] = sc.tdi[j] < 0 ? 0 : tab0 + sc.tdi[j];
      for (int y = 0; y < S.vs[j]; y++)
        for (int x = 0; x < S.hs[j]; x++) {  // at most 2 * 2 + 1 + 1 = 6
          S.slot_comp[S.bpm] = j;
          S.slot_x[S.bpm] = x;
          S.slot_y[S.bpm] = y;
          S.bpm++;
        }
    }
    S.ac = sc.tai < 0 ? 0 : tab0 + sc.tai;
    const int ri = sc.ri ? sc.ri : S.nmcus;
    for (size_t i = 0; i < sc.ivl.size(); i++) {
      ProgUnit U;
      long long at, len;
      piece((int)k, (int)i, at, len);
      U.data = at;
      U.nbits = 8 * len;
      U.scan = (int)scans.size();
      const long long m0 = (long long)i * ri;
      if (m0 >= S.nmcus) return -1;
      U.mcu0 = (int)m0;
      U.nmcus = std::min(ri, S.nmcus - U.mcu0);
      U.pad = 0;
      units.push_back(U);
    }
    scans.push_back(S);
  }
  return 0;
}

}  // namespace mij

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace mij {

// one component of one progressive frame, for the hand-over (k_prog_dcdiff)
struct ProgDcJob {
  long long off;  // first int16 of its padded plane
  int nblocks, bw, hs, vs, mcus_x;
  int pad;
};

// the progressive path's own device buffers (a decoder that never sees a
// progressive stream allocates none)
struct ProgBuffers {
  DecTab *tabs = nullptr;
  ProgScanDev *scans = nullptr;
  ProgUnit *units = nullptr;
  int *status = nullptr;
  ProgDcJob *dcjobs = nullptr;
  int16_t *dcabs = nullptr;
  size_t tabs_cap = 0, scans_cap = 0, units_cap = 0, status_cap = 0, dcjobs_cap = 0, dcabs_cap = 0;
};

enum { PROG_MAP_LANE = 0, PROG_MAP_WAVE = 1 };  // one unit per lane / per wave

// Runs the units (sorted by level; level_end[l] = one past the last unit of
// level l + 1; the caller has zeroed the planes), one launch per level, then
// the hand-over kernels over dcjobs unless a scan ended in a status code;
// status[s] per scan on return.  arena_blocks: 64-coefficient blocks of the
// whole arena, the size of the hand-over's scratch.  Synchronous.
int prog_run(hipStream_t stream, ProgBuffers &B, const uint8_t *d_blob, int16_t *d_coef, long long arena_blocks,
             const std::vector<DecTab> &tabs, const std::vector<ProgScanDev> &scans, const std::vector<ProgUnit> &units,
             const std::vector<int> &level_end, const std::vector<ProgDcJob> &dcjobs, int mapping,
             std::vector<int> &status);
void prog_free(ProgBuffers &B);

}  // namespace mij
#endif
