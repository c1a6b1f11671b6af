// progressive_check.cpp -- the progressive decoder's host parser and per-unit
// decode routine (csrc/mij_progressive.h, the text k_prog_scan runs per lane)
// on the CPU, as a program of its own so that it can be built with
// -fsanitize=address,undefined (tests/test_progressive_model.py):
//
//   progressive_check {<file.jpg> <coefs.bin | -> <expect>}...
//
// Each stream is parsed, staged as the library stages it (every restart
// interval of every scan unstuffed into an 8-aligned slot with exactly 16
// zero bytes behind it, the blob not a byte longer, so that a read past the
// documented bound is a sanitizer error) and decoded scan by scan into zeroed
// planes laid out as the decoder's arena.  expect: "ok" (decodes; with a
// coefficient file, int16 padded planes with absolute DCs back to back, the
// planes must equal it), "status" (a scan ends in a status code), "status:N"
// (in code N), "refused" (the parser refuses it), "any" (whatever happens,
// it happens inside the bounds).  Prints one line per stream; exit status 0
// if every expectation held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mij_progressive.h"

static std::vector<uint8_t> slurp(const char *path) {
  std::vector<uint8_t> v;
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

static size_t unstuff(uint8_t *dst, const uint8_t *s, size_t b, size_t e) {
  size_t o = 0;
  while (b < e) {
    dst[o++] = s[b];
    if (s[b] == 0xFF && b + 1 < e && s[b + 1] == 0x00) b++;
    b++;
  }
  return o;
}

static bool one(const char *jpg_path, const char *coef_path, const std::string &expect) {
  const std::vector<uint8_t> jpg = slurp(jpg_path);
  mij::ProgFrame F;
  std::string outcome;
  int status = 0;
  bool equal = true;
  if (mij::prog_parse(jpg.data(), jpg.size(), F, 0)) {
    outcome = std::string("refused: ") + F.err;
  } else {
    struct Piece {
      size_t at, len;
    };
    std::vector<std::vector<Piece>> pieces(F.scans.size());
    size_t off = 0;
    for (size_t k = 0; k < F.scans.size(); k++)
      for (const auto &iv : F.scans[k].ivl) {
        pieces[k].push_back({off, (size_t)(iv.end - iv.data)});
        off = (off + (size_t)(iv.end - iv.data) + 16 + 7) & ~(size_t)7;
      }
    // the exact bound: the last slot's 16 zero bytes (and its alignment) end the allocation
    std::vector<unsigned long long> store(off / 8, 0);
    uint8_t *blob = (uint8_t *)store.data();
    for (size_t k = 0; k < F.scans.size(); k++)
      for (size_t i = 0; i < pieces[k].size(); i++)
        pieces[k][i].len = unstuff(blob + pieces[k][i].at, jpg.data(), (size_t)F.scans[k].ivl[i].data,
                                   (size_t)F.scans[k].ivl[i].end);
    long long offs[3] = {0, 0, 0}, units = 0;
    for (int c = 0; c < F.ncomp; c++) {
      offs[c] = units;
      units += 64LL * F.bw[c] * F.bh[c];
    }
    std::vector<int16_t> coefs((size_t)units, 0);
    std::vector<mij::ProgScanDev> scans;
    std::vector<mij::ProgUnit> work;
    auto piece = [&](int k, int i, long long &at, long long &len) {
      at = (long long)pieces[k][i].at;
      len = (long long)pieces[k][i].len;
    };
    if (mij::prog_tables(F, offs, 0, piece, scans, work)) {
      outcome = "refused: a restart interval has no MCUs";
    } else {
      int bad_scan = -1;
      for (const mij::ProgUnit &U : work) {
        const int st = mij::prog_decode_unit(blob, U, scans[U.scan], F.tabs.data(), coefs.data());
        if (st && !status) {
          status = st;
          bad_scan = U.scan;
        }
      }
      if (status) {
        outcome = "status " + std::to_string(status) + " in scan " + std::to_string(bad_scan);
      } else {
        outcome = "ok, " + std::to_string(F.scans.size()) + " scans, " + std::to_string(F.levels) + " levels";
        if (strcmp(coef_path, "-")) {
          const std::vector<uint8_t> want = slurp(coef_path);
          equal = want.size() == coefs.size() * 2 && !memcmp(want.data(), coefs.data(), want.size());
          outcome += equal ? ", coefficients equal" : ", coefficients DIFFER";
        }
      }
    }
  }
  bool held;
  if (expect == "ok") held = outcome.compare(0, 2, "ok") == 0 && equal;
  else if (expect == "status") held = status != 0;
  else if (expect.compare(0, 7, "status:") == 0) held = status == atoi(expect.c_str() + 7);
  else if (expect == "refused") held = outcome.compare(0, 7, "refused") == 0;
  else held = expect == "any";
  printf("%s %s: %s (expected %s)\n", held ? "PASS" : "FAIL", jpg_path, outcome.c_str(), expect.c_str());
  return held;
}

int main(int argc, char **argv) {
  if (argc < 4 || (argc - 1) % 3) {
    fprintf(stderr, "usage: %s {<file.jpg> <coefs.bin | -> <ok | status | status:N | refused | any>}...\n", argv[0]);
    return 2;
  }
  int failed = 0;
  for (int a = 1; a + 2 < argc; a += 3) failed += !one(argv[a], argv[a + 1], argv[a + 2]);
  printf("%d streams, %d failed\n", (argc - 1) / 3, failed);
  return failed ? 1 : 0;
}
