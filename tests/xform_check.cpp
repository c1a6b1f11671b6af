// xform_check.cpp -- csrc/mij_xform.h on the host: the mapping k_xf_blocks
// applies, (plane geometry, operation, destination block, zigzag position)
// -> (source block, source position, sign), printed as a table that
// tests/test_transform_model.py compares with the numpy model's permutation.
//
//   xform_check <sbw> <ox> <oy> <dbw> <dbh> <op>
//
// one line per destination block (raster order) and position:
// "source_block source_position sign"
#include <cstdio>
#include <cstdlib>

#include "mij_xform.h"

int main(int argc, char **argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: %s <sbw> <ox> <oy> <dbw> <dbh> <op>\n", argv[0]);
    return 2;
  }
  mij::XfGeo g;
  g.sbw = atoi(argv[1]);
  g.ox = atoi(argv[2]);
  g.oy = atoi(argv[3]);
  g.dbw = atoi(argv[4]);
  g.dbh = atoi(argv[5]);
  const int op = atoi(argv[6]);
  if (op < 0 || op >= mij::XF_OPS || g.sbw < 1 || g.dbw < 1 || g.dbh < 1 || g.ox < 0 || g.oy < 0) return 2;
  g.bits = mij::xf_op_bits(op);
  const uint64_t neg = mij::xf_neg_mask(g.bits);
  for (int d = 0; d < g.dbw * g.dbh; d++) {
    const int by = d / g.dbw, bx = d - by * g.dbw;  // as the kernel splits it
    const int s = mij::xf_src_block(g, by, bx);
    for (int z = 0; z < 64; z++) printf("%d %d %d\n", s, mij::xf_src_pos(g.bits, z), (neg >> z) & 1 ? -1 : 1);
  }
  return 0;
}
