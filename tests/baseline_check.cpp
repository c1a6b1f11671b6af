// baseline_check.cpp -- the baseline decoder's table builder and symbol
// decoder (csrc/mij_huff.h: build_table, Bits, decode_one, the text
// k_dec_sync and k_dec_write run per lane) on the CPU, as a program of its
// own so that it can be built with -fsanitize=address,undefined
// (tests/test_baseline_sweep_model.py):
//
//   baseline_check <case.txt>...
//
// A case file is what tests/baseline_sweep.py's writer knows about one
// stream, as decimal numbers and hex:
//
//   ntab                      then per table: tc th, 16 counts, nsyms, the symbols
//   nivl                      then per restart interval:
//     nbytes nsyms used       the unstuffed bytes in hex (one line), then per
//     ti sym val bits         symbol: its table's index, the symbol, the value
//                             F.2.2.1 EXTEND gives (0 without magnitude bits)
//                             and code length + magnitude bits
//
// Every table must build; every interval is staged as the library stages it
// (8-aligned, zero-padded) in a buffer that ends with the last word a window
// may cover by the decoder's documented bound, so that a read past that bound
// is a sanitizer error, and walked symbol by symbol, once
// with one bit window carried along, as the kernels carry it, and once with a
// fresh window per symbol; symbol, value and bits consumed must be the
// writer's, and the walk must end on the interval's last used bit.  Last,
// over-subscribed DHTs go to build_table, which must refuse them (-1) without
// touching anything outside the table, and two complete codes, which it must
// take.  Prints one line per case; exit status 0 if everything held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mij_huff.h"

static int fail(const char *path, const char *what, long a = 0, long b = 0, long c = 0) {
  printf("%s: FAILED: %s (%ld, %ld, %ld)\n", path, what, a, b, c);
  return 1;
}

static int num(FILE *f) {
  int v;
  if (fscanf(f, "%d", &v) != 1) {
    fprintf(stderr, "short case file\n");
    exit(2);
  }
  return v;
}

static int one(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  const int ntab = num(f);
  std::vector<mij::DecTab> tabs(ntab);
  for (int t = 0; t < ntab; t++) {
    num(f);  // tc
    num(f);  // th
    uint8_t counts[16];
    for (int l = 0; l < 16; l++) counts[l] = (uint8_t)num(f);
    const int nsyms = num(f);
    std::vector<uint8_t> syms(nsyms);  // exactly nsyms: a read past them is a sanitizer error
    for (int i = 0; i < nsyms; i++) syms[i] = (uint8_t)num(f);
    if (mij::build_table(tabs[t], counts, syms.data(), nsyms)) return fail(path, "build_table refused table", t);
  }
  const int nivl = num(f);
  long total = 0;
  for (int iv = 0; iv < nivl; iv++) {
    const int nbytes = num(f), nsyms = num(f), used = num(f);
    // the words a window may cover at pos < 8 * nbytes: pos / 64 and pos / 64 + 1
    const size_t size = nbytes > 0 ? 8 * (size_t)((nbytes - 1) / 8) + 16 : 16;
    uint8_t *slot = (uint8_t *)aligned_alloc(8, size);
    memset(slot, 0, size);
    for (int i = 0; i < nbytes; i++) {
      unsigned v;
      if (fscanf(f, "%2x", &v) != 1) exit(2);
      slot[i] = (uint8_t)v;
    }
    mij::Bits carried{(const unsigned long long *)slot};
    long long pos = 0;
    for (int s = 0; s < nsyms; s++) {
      const int ti = num(f), want_sym = num(f), want_val = num(f), want_bits = num(f);
      if (pos >= 8LL * nbytes) return fail(path, "symbol past the interval", iv, s);
      int sym = -1, val = -1;
      const int n = mij::decode_one(carried, pos, tabs[ti], sym, val);
      if (n != want_bits || sym != want_sym || val != want_val)
        return fail(path, "carried window: bits / symbol / value differ", iv, s, n);
      mij::Bits fresh{(const unsigned long long *)slot};
      int sym2 = -1, val2 = -1;
      const int n2 = mij::decode_one(fresh, pos, tabs[ti], sym2, val2);
      if (n2 != n || sym2 != sym || val2 != val) return fail(path, "fresh window differs from the carried one", iv, s);
      pos += n;
    }
    if (pos != used) return fail(path, "the walk does not end on the last used bit", iv, (long)pos, used);
    total += nsyms;
    free(slot);
  }
  fclose(f);
  printf("%s: ok, %d tables, %d intervals, %ld symbols\n", path, ntab, nivl, total);
  return 0;
}

static int tables() {
  int bad = 0;
  mij::DecTab *t = new mij::DecTab;  // on the heap, alone: a store past it is a sanitizer error
  uint8_t syms[256];
  for (int i = 0; i < 256; i++) syms[i] = (uint8_t)i;
  struct {
    const char *what;
    uint8_t counts[16];
    int want;
  } cases[] = {
      {"three codes of 1 bit", {3}, -1},
      {"255 codes of 1 bit", {255}, -1},
      {"one code too many at 16 bits", {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3}, -1},
      {"five codes of 2 bits after none of 1", {0, 5}, -1},
      {"over-subscribed at the first length past the lookahead", {1, 1, 1, 1, 1, 1, 1, 1, 1, 3}, -1},
      {"a complete code, the all-ones code word included", {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2}, 0},
      {"one code of 1 bit and 128 of 8", {1, 0, 0, 0, 0, 0, 0, 128}, 0},
  };
  for (auto &c : cases) {
    int n = 0;
    for (int l = 0; l < 16; l++) n += c.counts[l];
    const int rc = mij::build_table(*t, c.counts, syms, n);
    if (rc != c.want) {
      printf("build_table: FAILED: %s: %d, expected %d\n", c.what, rc, c.want);
      bad = 1;
    }
  }
  delete t;
  if (!bad) printf("build_table: ok, over-subscribed codes refused\n");
  return bad;
}

int main(int argc, char **argv) {
  int bad = 0;
  for (int i = 1; i < argc; i++) bad |= one(argv[i]);
  bad |= tables();
  return bad;
}
