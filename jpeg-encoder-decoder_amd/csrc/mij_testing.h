/* mij_testing.h -- test-only entry points of libmijpeg.so.  Not part of the
 * public C ABI (include/mijpeg.h); the test suite binds them by name. */
#ifndef MIJ_TESTING_H
#define MIJ_TESTING_H
#include "mijpeg.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Fault injection: v > 0 makes the next encode's packing start frame 0's luma
 * pack ticket at v, as a stale ticket word would (pack group 0 never runs,
 * the groups after it wait on its look-back word); the frame must fail with
 * MIJ_EHANG within the device-wait bound instead of hanging the launch.
 * Consumed by that encode.  Returns the value armed before (0 once consumed),
 * or -2 on bad arguments. */
int mij_test_stale_ticket(mij_batch *b, int v);

/* The launch plan of the batch's most recent encode (mij_batch_encode; with
 * b == NULL, of the most recent mij_encode_regions call): what encode_frames,
 * ent_args and run_entropy decided, stored by them where they decide it.
 * Host state only -- no launch, copy or synchronisation.  A call between the
 * encode and this one that goes through the same host functions (the band
 * and assembly calls, mij_batch_dct) overwrites the fields it decides anew.
 * Copies the first min(n, MIJ_PLAN_FIELDS) fields to out and returns
 * MIJ_PLAN_FIELDS, or -2 on bad arguments. */
enum {
  MIJ_PLAN_NFRAMES = 0,     /* frames of the last entropy call (a sub-batch's with overlap) */
  MIJ_PLAN_F0,              /* its first frame */
  MIJ_PLAN_ENTROPY_CALLS,   /* entropy calls of the encode (sub-batches) */
  MIJ_PLAN_DC_LAST,         /* DC tables inside k_segdc_actab */
  MIJ_PLAN_ACTAB,           /* AC tables beside the segment DCs (k_segdc_actab) */
  MIJ_PLAN_TABLES,          /* k_tables launch: 0 none, 2 DC tables only, 4 all four */
  MIJ_PLAN_SEGDC,           /* segment-first DCs: 0 none (K1 wrote them), 1 k_seg_dc,
                               2 inside k_segdc_actab, 3 inside k_tables' DC waves */
  MIJ_PLAN_SEAM,
  MIJ_PLAN_FF_PACK,
  MIJ_PLAN_SEAM_IN_SCAN,    /* seams fixed inside k_emit_scan, no k_seam_fix launch */
  MIJ_PLAN_EMIT_SLOTS,
  MIJ_PLAN_PACK_LS_LUMA,    /* pack groups of 32 << ls segments */
  MIJ_PLAN_PACK_LS_CHROMA,
  MIJ_PLAN_PACK_WIDE,
  MIJ_PLAN_HIST_FILL_SKIPPED, /* the histogram fill before K1 was skipped */
  MIJ_PLAN_K1_MODE,         /* mode bits of the last K1 launch (2 tokens, 3 tokens +
                               coefficient planes, 6 tokens from the planes: split) */
  MIJ_PLAN_DC_ONLY,         /* that K1 stored no token stream for all-AC-zero chroma
                               segments (seg_ntok bit 31; the pack builds their tokens
                               from the raw DCs) */
  MIJ_PLAN_FIELDS
};
int mij_test_last_plan(mij_batch *b, int *out, int n);

/* Capacity injection: the next mij_batch_encode_sampled at a sampling other
 * than MIJ_SAMP_420 gives `frame` an output capacity of at most `cap` bytes
 * (the public interface always sizes it for the worst case); that frame must
 * fail alone with MIJ_ENOSPC.  Consumed by that encode.  Host state only.
 * Returns 0, or -2 on bad arguments. */
int mij_test_sampled_out_cap(mij_batch *b, int frame, long long cap);
/* The lane mapping of the progressive decoder's k_prog_scan:
 * 0 = one unit (restart interval of a scan) per lane; 1 = one unit per wave,
 * the default.  Both give the same planes; scripts/bench_progressive.py
 * times them.  Returns the previous mapping, or -2 on bad arguments. */
int mij_test_prog_mapping(mij_decoder *d, int mapping);

#ifdef __cplusplus
}
#endif
#endif
