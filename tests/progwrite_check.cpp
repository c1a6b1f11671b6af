// progwrite_check.cpp -- the per-block routines of progressive output
// (csrc/mij_progwrite.h) compiled by a host compiler under the
// address and undefined-behaviour sanitizers: the text the kernels run per
// lane.  A program of its own (tests/test_progwrite_model.py builds and runs
// it); nothing here touches a GPU.
//
//   progwrite_check IN OUT
//
// IN: int32 nscans, then per scan int32 ss, se, ah, al, nblocks, interval
// (blocks per restart interval), then nblocks records of int32 table (DC
// first scans: 0 for component 0, 1 for the others), int32 predecessor (index
// of the block whose DC predicts this one, -1: none) and 64 int16
// coefficients, in scan order.  OUT: per scan and interval the tokens as four
// int32 each (table or -1 for a raw bit, symbol, extra value, extra bits),
// every raw bit a token of its own, and (-2, 0, 0, 0) after every interval.
// The runs are resolved here one block after another from pw_classify's flags;
// the blocks then leave in the order the kernels give them: own symbols, the
// EOBn code of the run the block heads, its trailing correction bits.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mij_progwrite.h"

struct Rec {
  int32_t table, pred;
  int16_t c[64];
};

static std::vector<int32_t> out;

static void tok(int t, int sym, uint32_t extra, int n) {
  out.push_back(t);
  out.push_back(sym);
  out.push_back((int32_t)extra);
  out.push_back(n);
}

static void raw_bits(unsigned long long v, int n) {
  for (int i = n - 1; i >= 0; i--) tok(-1, 0, (uint32_t)((v >> i) & 1), 1);
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t nscans = 0;
  if (fread(&nscans, 4, 1, f) != 1) return 2;
  for (int s = 0; s < nscans; s++) {
    int32_t h[6];
    if (fread(h, 4, 6, f) != 6) return 2;
    const int ss = h[0], se = h[1], ah = h[2], al = h[3], nb = h[4], iv = h[5];
    std::vector<Rec> blk(nb);
    if (nb && fread(blk.data(), sizeof(Rec), nb, f) != (size_t)nb) return 2;
    for (int i0 = 0; i0 < nb; i0 += iv) {
      const int i1 = i0 + iv < nb ? i0 + iv : nb;
      if (ss == 0) {
        for (int i = i0; i < i1; i++) {
          if (ah) {
            tok(-1, 0, (uint32_t)(blk[i].c[0] >> al) & 1u, 1);
            continue;
          }
          int sym;
          uint32_t extra;
          const int p = blk[i].pred;
          mij::pw_dc_first(blk[i].c[0], p < 0 ? 0 : blk[p].c[0], p >= 0, al, sym, extra);
          tok(blk[i].table, sym, extra, sym);
        }
      } else {
        std::vector<uint32_t> info(i1 - i0);
        std::vector<int> runlen(i1 - i0, 0);
        bool open = false;
        int H = 0, cnt = 0, be = 0;
        for (int i = i0; i < i1; i++) {
          const uint32_t inf = info[i - i0] = mij::pw_classify(mij::pw_masks(blk[i].c, ss, se, al), se, ah);
          if ((inf & 1u) && open) {
            runlen[H] = cnt;
            open = false;
          }
          if (inf & 2u) {
            if (!open) {
              open = true;
              H = i - i0;
              cnt = be = 0;
            }
            cnt++;
            be += (int)(inf >> 2);
            if (cnt == mij::PW_MAX_EOBRUN || be > mij::PW_MAX_BE) {
              runlen[H] = cnt;
              open = false;
            }
          }
        }
        if (open) runlen[H] = cnt;
        for (int i = i0; i < i1; i++) {
          unsigned long long tb = 0;
          int tn = 0;
          mij::pw_walk_ac(blk[i].c, mij::pw_masks(blk[i].c, ss, se, al), ss, ah, al,
                          [&](int sym, uint32_t extra, int n) { tok(0, sym, extra, n); }, raw_bits, tb, tn);
          if (tn != (int)(info[i - i0] >> 2)) return 3;  // pw_classify counts what pw_walk_ac leaves
          if (runlen[i - i0]) {
            int sym, n;
            uint32_t extra;
            mij::pw_eobrun(runlen[i - i0], sym, extra, n);
            tok(0, sym, extra, n);
          }
          raw_bits(tb, tn);
        }
      }
      tok(-2, 0, 0, 0);
    }
  }
  fclose(f);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  if (!out.empty() && fwrite(out.data(), 4, out.size(), o) != out.size()) return 2;
  fclose(o);
  printf("ok %zu tokens\n", out.size() / 4);
  return 0;
}
