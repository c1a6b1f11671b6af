/*
 * mijpeg.h -- C ABI of the MI355X-native (gfx950) JPEG block-encode path.
 *
 * Drop-in replacement for the reference's encoder
 * (MattiaDallaCosta/JPEG-encoder-decoder include/encoder.h:10-12,
 * include/structs.h:5-18): a C host that includes this header instead of
 * encoder.h and links libmijpeg.so gets the same three entry points with the
 * same signatures, argument meaning, buffer ownership and output bytes; the
 * work runs as HIP kernels on the GPU.  See INTEGRATION.md.
 *
 * Plain C types only: no HIP/torch types cross this boundary.
 */
#ifndef MIJPEG_H
#define MIJPEG_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- types: layout-identical to the reference --------------------------- */

/* include/structs.h:5-13 (ISO/IEC 10918-1 K.2 table state). */
typedef struct __huff_code {
    int sym_freq[257];
    int code_len[257];
    int next[257];
    int code_len_freq[32];
    int sym_sorted[256];
    int sym_code_len[256];
    int sym_code[256];
} huff_code;

/* include/structs.h:15-18: a sub-rectangle of the input frame; w and h must
 * be multiples of 16 (the reference silently produced garbage otherwise,
 * this library rejects them, see mij_last_error). */
typedef struct {
    int x, y;
    int w, h;
} area_t;

/* ---- drop-in entry points ------------------------------------------------ */

/* Replaces encoder.h:10 / encoder.c:158-178.  `in` is a BGR888 frame whose
 * row stride is the reference's compile-time WIDTH (define.h:3, 320 px) or
 * the value set with mij_set_input_stride().  Writes the quantized, zigzagged
 * coefficients with DC differences into Y[w*h], Cb[w*h/4], Cr[w*h/4] (block
 * raster order per component). */
void rgb_to_dct(uint8_t *in, int16_t *Y, int16_t *Cb, int16_t *Cr, area_t dims);

/* Replaces encoder.h:11 / encoder.c:360-381: fills the four optimized
 * Huffman tables (Luma[0]=DC, Luma[1]=AC, Chroma[0]=DC, Chroma[1]=AC);
 * every field ends in the state the reference leaves it in. */
void init_huffman(int16_t *Y, int16_t *Cb, int16_t *Cr, area_t dims,
                  huff_code Luma[2], huff_code Chroma[2]);

/* Replaces encoder.h:12 / encoder.c:549-644: writes the JFIF stream to `f`
 * (may be NULL here, unlike the reference) and to jpg[], returns its size
 * (0 on error).  jpg must hold mij_max_jpg_bytes(w, h) bytes to be safe. */
size_t write_jpg(FILE *f, uint8_t *jpg, int16_t *Y, int16_t *Cb, int16_t *Cr,
                 area_t dims, huff_code Luma[2], huff_code Chroma[2]);

/* ---- extensions ----------------------------------------------------------- */

/* Runtime replacement for define.h:3 WIDTH (input row stride in pixels used
 * by rgb_to_dct).  Default 320.  Returns 0 or an error code. */
int mij_set_input_stride(int stride_px);

/* Quality factor for the drop-in calls, scaled like utils/original.c:504-509.
 * Default 50 == the reference's fixed tables (encoder.c:18-36). */
int mij_set_quality(int quality);

/* Error reporting (the reference has none: encoder.c returns void). */
enum {
    MIJ_OK = 0,
    MIJ_EINVAL = 1,     /* dims not multiples of 16, bad stride/quality, ... */
    MIJ_ENODEV = 2,     /* no usable HIP device / runtime */
    MIJ_EHIP = 3,       /* a HIP runtime call failed */
    MIJ_ENOSPC = 4,     /* output capacity too small */
    MIJ_ETABLE = 5,     /* Huffman construction outside the reference's
                           defined behaviour (code length >= 32 etc.) */
    MIJ_EPPM = 6,       /* PPM rejected by the rules of utils/original.c:294-365 */
    MIJ_EIO = 7,        /* file could not be opened, read or written */
    MIJ_EJPEG = 8,      /* decoder: not a baseline stream of the accepted subset (8-bit SOF0, greyscale
                         * or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan or the encoder's three
                         * scans), or corrupt; the message names the stream and the reason */
    MIJ_EHANG = 9       /* a device-side wait (pack look-back, ticket) outlasted its
                           bound: the frame's device state was corrupted; the
                           frame fails instead of the launch hanging */
};
int mij_last_error(void);
const char *mij_strerror(int code);
/* Text of the calling thread's last failure ("" before any): what was wrong
 * with which argument, beyond the code mij_last_error returns. */
const char *mij_last_message(void);

/* Worst-case size of an encoded w x h frame (all 63 AC coefficients coded at
 * 27 bits, every byte stuffed). */
size_t mij_max_jpg_bytes(int w, int h);

/* Whole path host->host (rgb_to_dct -> init_huffman -> write_jpg without the
 * host round trips of the three-call split).  `bgr` + stride_px describe the
 * frame, dims the region.  Returns MIJ_OK and the size in *out_len. */
int mij_encode(const uint8_t *bgr, int stride_px, area_t dims, int quality,
               uint8_t *out, size_t cap, size_t *out_len);

/* ---- device-resident batch pipeline (throughput path) ---------------------
 * A batch object owns the device buffers for up to max_frames frames of one
 * geometry; frames are independent (own tables, own JFIF stream).  All work
 * is queued on the batch's HIP stream; outputs stay in HBM until fetched. */
typedef struct mij_batch mij_batch;

mij_batch *mij_batch_create(int device, int width, int height, int max_frames,
                            int quality);
void mij_batch_destroy(mij_batch *b);
/* packed BGR888 frames (width*height*3 bytes each) from host memory into
 * batch slots first .. first+nframes-1 */
int mij_batch_upload(mij_batch *b, const uint8_t *bgr, int first, int nframes);
/* or point the batch at frames already in device memory (not owned):
 * frame i starts at d_bgr + i*frame_stride, rows pitch bytes apart
 * (pointer, pitch and frame stride 16-byte aligned: K1 streams rows with
 * 16-byte LDS-DMA loads) */
int mij_batch_set_input(mij_batch *b, const void *d_bgr, long long frame_stride,
                        int pitch);
int mij_batch_encode(mij_batch *b, int nframes);     /* full path, async */
/* pipeline: fused (default) -- K1 emits the symbol tokens directly, the
 * coefficient planes never reach HBM; split (set_split(b, 1)) -- K1 writes
 * zigzag coefficient planes and a second pass tokenizes them.  Same output
 * bytes either way. */
int mij_batch_set_split(mij_batch *b, int on);
/* fused pipeline: encode in nsub sub-batches (1 = off, at most 16), the
 * entropy stages of sub-batch k on a second stream behind K1 of sub-batch k,
 * concurrent with K1 of sub-batch k + 1.  Same output bytes; stage timing
 * then reports K1 over all sub-batches ([0]) and the whole encode ([7]). */
int mij_batch_set_overlap(mij_batch *b, int nsub);
/* Entropy-stage variants of the fused pipeline.  Every setting gives the
 * same output bytes; the defaults are the measured-fastest ones and the
 * others exist for A/B timing (bench.py --opt NAME=V) and are covered by
 * tests/test_options.py.
 *   MIJ_OPT_SEAM          1 (default): every scan word stored whole, shared
 *                         group edge words ORed in afterwards; 0: edge words
 *                         ORed onto zeroed scan buffers (the band paths' form)
 *   MIJ_OPT_FF_PACK       1 (default, seam mode only): the packing counts the
 *                         0xFF bytes of every output chunk; 0: a counting pass
 *   MIJ_OPT_ACTAB         1 (default): on batches of >= 16 frames the AC
 *                         tables are built beside the segment DCs; 0: after
 *   MIJ_OPT_SEGDC_FUSED   0 (default); 1: the segment DCs inside the table
 *                         kernel's DC waves
 *   MIJ_OPT_PACK_WIDE     -1 (default: the wide window from quality 85);
 *                         0 / 1 force the default / wide pack window
 *   MIJ_OPT_EMIT_SLOTS    0 (default: chosen from frame count, size and Q);
 *                         > 0: JFIF-assembly workgroups per frame
 *   MIJ_OPT_OVERLAP_PRIO  1 (default): the overlap stream (set_overlap) at
 *                         the highest priority; 0: the lowest
 *   (7 is reserved: an internal fault-injection hook of the test suite,
 *   not settable through this call)
 *   MIJ_OPT_PACK_SEGS     -1 (default: chosen from the quality); otherwise
 *                         ly + 4 * lc (0..15): the packing's groups take
 *                         32 << ly luma and 32 << lc chroma segments */
enum {
  MIJ_OPT_SEAM = 0,
  MIJ_OPT_FF_PACK = 1,
  MIJ_OPT_ACTAB = 2,
  MIJ_OPT_SEGDC_FUSED = 3,
  MIJ_OPT_PACK_WIDE = 4,
  MIJ_OPT_EMIT_SLOTS = 5,
  MIJ_OPT_OVERLAP_PRIO = 6,
  /* 7: reserved */
  MIJ_OPT_PACK_SEGS = 8,
  MIJ_OPT_COUNT = 9
};
int mij_batch_set_option(mij_batch *b, int opt, int value);
int mij_batch_get_option(mij_batch *b, int opt);
/* input frames in R, G, B byte order (PPM files, brain.c:25-42) instead of the
 * encoder's B, G, R (encoder.c:133); the channels are swapped inside K1, at no
 * cost.  Both pipelines. */
int mij_batch_set_rgb(mij_batch *b, int on);
/* fused pipeline only: also keep the coefficient planes (for
 * mij_batch_coefs); the split pipeline always has them */
int mij_batch_keep_coefs(mij_batch *b, int on);
int mij_batch_dct(mij_batch *b, int nframes);        /* K1 only, async */
/* Measurement only (bench.py): K1's memory traffic without its arithmetic --
 * the coefficient variant's persistent grid, tile claims, LDS-DMA of the BGR
 * tiles one tile ahead and whole-line coefficient + raw-DC stores -- on
 * frames 0..n-1, timed like mij_batch_dct; the coefficient planes are left
 * holding garbage.  Its time is the floor of K1's access pattern on this GPU.
 * Plain B, G, R batches only; async. */
int mij_batch_pattern_floor(mij_batch *b, int nframes);
int mij_batch_sync(mij_batch *b);
int mij_batch_output(mij_batch *b, int frame, uint8_t *dst, size_t cap,
                     size_t *len);
int mij_batch_lengths(mij_batch *b, size_t *lens, int nframes);
/* quantized zigzag coefficient planes of a frame; diffed != 0 applies the DC
 * differencing of encoder.c:168-177 (as rgb_to_dct returns them) */
int mij_batch_coefs(mij_batch *b, int frame, int16_t *Y, int16_t *Cb,
                    int16_t *Cr, int diffed);
int mij_batch_tables(mij_batch *b, int frame, huff_code out[4]);
/* timing: when enabled, HIP events bracket each stage of the next encode;
 * mij_batch_stage_ms returns up to n (<= MIJ_NSTAGES) stage durations (ms) of
 * the last one: [0]=K1 colour+DCT+quant (+tokens when fused), [1]=fix (FP64
 * re-encode of the blocks K1 listed), [2]=tokenize (split pipeline),
 * [3]=stats (segment DC fixup, fused pipeline), [4]=tables, [5]=pack
 * (segment bits + offsets + bit packing), [6]=emit (JFIF assembly),
 * [7]=whole encode */
#define MIJ_NSTAGES 8
int mij_batch_set_timing(mij_batch *b, int on);
int mij_batch_stage_ms(mij_batch *b, float *ms, int n);
/* the same for each of the last `steps` encodes (<= 64) issued while timing
 * was on, oldest first: ms[step*MIJ_NSTAGES + stage]; returns the count filled */
int mij_batch_stage_history(mij_batch *b, float *ms, int steps);
/* symbol tokens K1 stored in the token buffer for the last encode of nframes
 * frames (4 bytes each; used for the bandwidth accounting of the fused
 * kernel).  DC-only chroma segments, whose tokens the packing builds from the
 * raw DCs instead of a stored stream, add nothing to it. */
unsigned long long mij_batch_token_count(mij_batch *b, int nframes);
/* {w, h, 8x8 blocks per frame, segments per frame, K1 tiles per frame,
 *  the pack kernel's LDS window in words at the batch's quality}: the first n */
int mij_batch_geometry(mij_batch *b, long long *out, int n);
/* FP64 fix-ups since creation: blocks re-encoded by the fix-up kernel after
 * K1 (split pipeline) plus coefficients replayed in place (fused pipeline) */
unsigned long long mij_batch_replays(mij_batch *b);
/* the batch's hipStream_t, as an opaque pointer */
void *mij_batch_stream(mij_batch *b);
/* Enqueue the batch's work on the caller's stream (null: its own again).
 * Work enqueued after the switch runs after the work enqueued before it (an
 * event on the old stream).  The root's assembler runs its assembly on the
 * band batch's stream this way (sharding.encode_banded_dev), so the band's
 * word move, the assembly and the next step's K1 follow each other in one
 * queue instead of through cross-queue waits (~13 us each on config 4).
 * Switch back (null) before destroying either batch. */
int mij_batch_set_stream(mij_batch *b, void *stream);

/* ---- region batches: many areas of one frame -----
 * The reference's workload (main.c:142-155): the change detector returns up
 * to 100 rectangles of a frame and each is encoded on its own with
 * rgb_to_dct / init_huffman / write_jpg.  A region batch does all of them in
 * one launch sequence: the batch is created with the largest region's size
 * (the canvas) and slot i holds region i, w_i x h_i, at the top-left of its
 * slot.  Each region gets its own tables and JFIF (SOF0 = w_i x h_i); the
 * bytes are those of the three drop-in calls on that region. */
/* per-frame sizes of the next encodes (multiples of 16, at most the batch
 * geometry); wh = {w0, h0, w1, h1, ...}; NULL restores the batch geometry.
 * A full-frame mij_batch_upload / mij_batch_set_input also restores it: call
 * this after uploading when the uploaded frames are smaller than the canvas. */
int mij_batch_set_frame_dims(mij_batch *b, const int *wh, int nframes);
/* regions of a device-resident BGR frame (rows pitch bytes apart) into
 * slots 0..n-1 (one gather launch) and their sizes as the frame dims */
int mij_batch_gather_regions(mij_batch *b, const void *d_frame, long long pitch,
                             int frame_w, int frame_h, const area_t *regions, int n);
/* the same from a host frame of stride_px pixels per row (uploaded once) */
int mij_batch_upload_regions(mij_batch *b, const uint8_t *bgr, int stride_px, int frame_h,
                             const area_t *regions, int n);
/* one call: every region of a host BGR frame to its own JPEG; the n streams
 * are written back to back into out (cap bytes), their lengths into lens */
int mij_encode_regions(const uint8_t *bgr, int stride_px, int frame_h, const area_t *regions,
                       int n, int quality, uint8_t *out, size_t cap, size_t *lens);

/* ---- frames of any size: the interleaved output format -----
 * The calls above write the reference's shape: width and height multiples of
 * 16, three one-component scans.  These write what every other baseline
 * encoder writes, for any 1 <= w, h <= 65535 inside the batch canvas: the
 * frame is edge-extended to multiples of 16 (last column, then last row,
 * replicated), colour conversion, 4:2:0, DCT, quantisation and zigzag are
 * those of the calls above on the extended frame, SOF0 carries the true w and
 * h, and the entropy data is ONE interleaved scan (MCU = Y Y Y Y Cb Cr, DC
 * prediction per component in that order) with its own four optimised
 * tables.  restart_rows = r > 0 adds a DRI of Ri = r * ceil(w / 16) MCUs and
 * RSTn markers every r MCU rows (each interval padded with 1-bits, prediction
 * back to 0); 0: none.  Every 0xFF of entropy data, pad bytes included, is
 * followed by 0x00.  mij_decoder_decode / mij_decode read these streams. */

/* Worst-case size of such a stream: that of the padded frame, 2 bytes per
 * restart marker, the DRI segment.  0 for sizes outside 1..65535 or
 * Ri > 65535. */
size_t mij_max_jpg_bytes_any(int w, int h, int restart_rows);
/* n device-resident frames of any size, pointer alignment and pitch (frame i
 * at d_px + i*frame_stride, rows pitch bytes apart, wh = {w0, h0, w1, h1,
 * ...}, sizes may differ) edge-extended into slots 0..n-1 in one launch; the
 * padded sizes become the frame dims (as with mij_batch_gather_regions) and
 * the true sizes are remembered for mij_batch_encode_interleaved.  With
 * mij_batch_set_rgb on, the source bytes are R, G, B (set it before this
 * call).  A later mij_batch_upload, _set_input, _set_frame_dims or region
 * call forgets the true sizes.  The source is read in aligned 4-byte words:
 * up to 3 bytes before d_px and up to 3 bytes past the last row's last pixel
 * may be read (never used), always inside an aligned word that also holds
 * bytes of the frame, so inside its allocation's pages. */
int mij_batch_pad_input(mij_batch *b, const void *d_px, long long frame_stride, long long pitch,
                        const int *wh, int n);
/* the same for one host frame of stride_px pixels per row into slot `slot`;
 * the other slots keep what they hold */
int mij_batch_upload_any(mij_batch *b, const uint8_t *px, int stride_px, int w, int h, int slot);
/* slots 0..nframes-1 (all holding padded input: MIJ_EINVAL otherwise, and
 * for Ri > 65535) to interleaved streams; asynchronous on the batch's stream;
 * results through mij_batch_output / _lengths / _tables, and the padded
 * frames' coefficient planes through mij_batch_coefs.  A frame that fails
 * (tables, capacity) has length 0 and its error code.  The first use
 * allocates this format's buffers and, with restart intervals, grows the
 * per-frame output capacity to mij_max_jpg_bytes_any of the canvas. */
int mij_batch_encode_interleaved(mij_batch *b, int nframes, int restart_rows);
/* One call, host to host, mirror of mij_decode: px holds w x h pixels in
 * `order` (MIJ_PIX_BGR / MIJ_PIX_RGB), rows stride_px pixels apart.  *out_len
 * (may be NULL) receives the stream's size, or with MIJ_ENOSPC -- returned
 * before any device work when cap < mij_max_jpg_bytes_any(w, h,
 * restart_rows), so cap 0 asks for it -- that bound. */
int mij_encode_any(const uint8_t *px, int stride_px, int w, int h, int order, int quality,
                   int restart_rows, uint8_t *out, size_t cap, size_t *out_len);

/* ---- a chosen chroma sampling -------------------------------
 * The interleaved format above at 4:2:0, 4:2:2, 4:4:4 or greyscale.  Hmax x
 * Vmax is 2x2, 2x1, 1x1, 1x1 and an MCU 8 Hmax x 8 Vmax pixels; the frame is
 * edge-extended to whole MCUs (the padded slots hold that extension for every
 * sampling).  Every pixel gets Y, Cb, Cr by the reference's expressions,
 * truncated; 4:4:4 chroma is those bytes, 4:2:2 chroma (a + b) / 2 over a
 * horizontal pair of them, greyscale has one component (one DQT, two DHT).
 * DCT, truncating quantisation, clip and zigzag are the reference's on every
 * 8x8 block of every plane, luma table for component 0, chroma table for the
 * others.  restart_rows counts MCU rows of the sampling's grid (8 pixel rows
 * for all but 4:2:0): Ri = r * ceil(w / (8 Hmax)).  MIJ_SAMP_420 is, byte for
 * byte, mij_batch_encode_interleaved / mij_encode_any. */
enum { MIJ_SAMP_420 = 0, MIJ_SAMP_422 = 1, MIJ_SAMP_444 = 2, MIJ_SAMP_GRAY = 3 };
/* Worst-case size of such a stream: the per-block worst case of
 * mij_max_jpg_bytes times the sampling's blocks, headers, the DRI segment, 2
 * bytes per restart marker; mij_max_jpg_bytes_any for MIJ_SAMP_420.  0 for
 * sizes outside 1..65535, an unknown sampling, restart_rows < 0 or
 * Ri > 65535.  Host only. */
size_t mij_max_jpg_bytes_sampled(int w, int h, int sampling, int restart_rows);
/* mij_batch_encode_interleaved at a sampling: slots 0..nframes-1 must hold
 * padded input (mij_batch_pad_input / _upload_any) with mij_batch_set_rgb
 * unchanged since; results through mij_batch_output / _lengths.  Waits for
 * the device once mid-call (the frames' bit counts size the scan words).  A
 * frame that fails (tables, capacity) has length 0 and its error code.  The
 * first call with a sampling other than MIJ_SAMP_420 allocates this path's
 * buffers, which grow with later calls, and grows the per-frame output
 * capacity to mij_max_jpg_bytes_sampled of the canvas. */
int mij_batch_encode_sampled(mij_batch *b, int nframes, int sampling, int restart_rows);
/* The planes the last mij_batch_encode_sampled (or mij_batch_encode_libjpeg,
 * below) coded, as mij_decoder_layout and mij_decoder_component show a
 * decoded stream's: layout = {w, h, ncomp,
 * hmax, vmax, mcus_x, mcus_y, Ri, 1} then {h, v, tq, blocks across, blocks
 * down} per component (MIJ_ENOSPC under 9 + 5 * ncomp ints); a component =
 * its padded plane, raster blocks of 64 zigzag coefficients, DC absolute. */
int mij_batch_sampled_layout(mij_batch *b, int frame, int *out, int n);
int mij_batch_sampled_component(mij_batch *b, int frame, int comp, int16_t *dst, size_t cap);
/* mij_encode_any at a sampling.  Every MIJ_EINVAL, and MIJ_ENOSPC with
 * mij_max_jpg_bytes_sampled(w, h, sampling, restart_rows) in *out_len when
 * cap is under it, come before any device work. */
int mij_encode_sampled(const uint8_t *px, int stride_px, int w, int h, int order, int quality,
                       int sampling, int restart_rows, uint8_t *out, size_t cap, size_t *out_len);

/* ---- encoding as libjpeg does --------------------------------
 * The same streams with libjpeg's arithmetic in front of the entropy coder,
 * so that the DQTs and every quantised coefficient are those of the file
 * libjpeg (cjpeg, Pillow's save(quality, subsampling), ImageMagick) writes for
 * the same pixels, quality and sampling: the Annex K tables on the IJG scale
 * (s = 5000 / Q under 50, else 200 - 2 Q; (base s + 50) / 100 in 1..255);
 * fixed-point colour conversion; chroma downsampled without smoothing, (a + b
 * + bias) >> 1 with bias 0, 1, ... at 4:2:2 and (a + b + c + d + bias) >> 2
 * with bias 1, 2, ... at 4:2:0; pixels replicated to the right, and downward
 * to a whole row group, the component's last sample row below that; the
 * blocks of the MCU padding that hold no sample with no AC and the DC of the
 * block before them in the MCU; the "islow" integer DCT; a quantiser that
 * rounds the magnitude.  Huffman tables and headers are this library's own:
 * the files are not byte-equal to libjpeg's, their decoded pixels are.
 *
 * mij_libjpeg_tables: the luma then the chroma table of a quality, 64 bytes
 * each in zigzag order as mij_decoder_info reports a stream's; MIJ_EINVAL
 * outside 1..100.  Host only. */
int mij_libjpeg_tables(int quality, uint8_t dqt[128]);
/* mij_batch_encode_sampled with that arithmetic, the batch's quality read on
 * the IJG scale, at all four MIJ_SAMP_* (4:2:0 too goes through this path,
 * not through mij_batch_encode_interleaved): the same preconditions,
 * refusals, mid-call wait, buffer growth and result calls.  Afterwards
 * mij_batch_sampled_layout / _component serve its planes: they follow the
 * last mij_batch_encode_sampled or mij_batch_encode_libjpeg. */
int mij_batch_encode_libjpeg(mij_batch *b, int nframes, int sampling, int restart_rows);
/* mij_encode_sampled with that arithmetic.  Every MIJ_EINVAL, and MIJ_ENOSPC
 * with mij_max_jpg_bytes_sampled(w, h, sampling, restart_rows) in *out_len
 * when cap is under it, come before any device work. */
int mij_encode_libjpeg(const uint8_t *px, int stride_px, int w, int h, int order, int quality,
                       int sampling, int restart_rows, uint8_t *out, size_t cap, size_t *out_len);

/* ---- PPM ingest -----------------------------------
 * Header rules of the reference's reader, utils/original.c:294-365, kept
 * exactly: "P6" then a newline straight after it; then lines up to the first
 * one that does not start with '#' (comment lines, :303-316), which must hold
 * "W H" (sscanf "%d %d", :318); W and H multiples of 16 (:324-328); the depth
 * read with fscanf("%d\n") -- which also swallows whitespace bytes that begin
 * the pixel data, so such a file then fails the length check, as in the
 * reference -- must be 255 (:330-337); the bytes left must be exactly 3*W*H
 * (:339-344).  Extra rules where the reference is undefined: a line longer
 * than 1023 bytes or missing its newline is a parse error, W or H <= 0 is
 * rejected.  Errors: MIJ_EIO (open/read), MIJ_EPPM (rules above). */
int mij_ppm_header(const char *path, int *w, int *h, long long *data_offset);
/* pixels of a PPM into dst (rows dst_pitch bytes apart); to_bgr != 0 swaps
 * to the encoder's B, G, R order (what rgb_to_dct / mij_encode expect) */
int mij_ppm_read(const char *path, uint8_t *dst, size_t cap, int dst_pitch, int to_bgr);

/* ---- streaming encoder: PPM files -> .jpg files ----------------------------
 * Frames of one geometry flow through two batches in ping-pong: host threads
 * read chunk k+1 into pinned memory (no channel swap: K1 reads RGB) while the
 * GPU encodes chunk k; each chunk is uploaded, encoded, its lengths fetched,
 * its JPEG bytes copied back and written by host threads, all overlapped with
 * the other batch's chunk.  Output bytes are those of mij_encode /
 * write_jpg for the same image. */
typedef struct mij_stream mij_stream;
mij_stream *mij_stream_create(int device, int width, int height, int chunk_frames,
                              int quality, int host_threads);
void mij_stream_destroy(mij_stream *s);
/* encode n PPM files (all width x height) to out_paths; stops at the first
 * failing file (its index in *failed, -1 if none) */
int mij_stream_encode_files(mij_stream *s, const char *const *in_paths,
                            const char *const *out_paths, int n, int *failed);
/* in-memory variant: n RGB frames (packed rows) -> outs[i] (caps[i] bytes),
 * lengths in lens[i] */
int mij_stream_encode_frames(mij_stream *s, const uint8_t *const *rgb, int n,
                             uint8_t *const *outs, const size_t *caps, size_t *lens);
/* seconds of the last encode_*: {wall, host read, host write, gpu (events),
 * frames, bytes in, bytes out} */
#define MIJ_STREAM_NSTATS 7
int mij_stream_stats(mij_stream *s, double *out, int n);

/* ---- one large frame over several ranks -------
 * Rank r encodes band r -- an MCU-row range [row0, row0 + rows) with rows a
 * multiple of 16 -- of each of n frames as frames 0..n-1 of its own batch
 * (created for width x rows, input pointing at the band's first row).  The
 * caller moves four small things between ranks (sharding.py does it with
 * torch.distributed / RCCL):
 *   1. mij_band_analyze    -> last raw DC per component      [n*3]  all-gather
 *   2. mij_band_histograms(previous band's last DCs, 0 for band 0)
 *                          -> the band's symbol counts       [n*4*257] all-reduce(sum)
 *   3. mij_band_tables(summed counts) -> bits per scan       [n*3]  all-gather, exclusive scan
 *   4. mij_band_pack(global bit offset of the band in each scan)
 *      mij_band_words(frame, comp) -> packed big-endian words; word 0 is
 *      global word offset/32 of that scan (bits before the offset are 0)  gather
 * One rank assembles on a batch of the whole frame: mij_assemble_begin
 * (summed counts -> tables), mij_assemble_words per band and component (OR:
 * neighbouring bands share at most one word), mij_assemble_end(total bits per
 * scan) -> 0xFF stuffing, pads, headers; then mij_batch_output. */
int mij_band_analyze(mij_batch *b, int n, int16_t *last_dc);
int mij_band_histograms(mij_batch *b, int n, const int16_t *prev_dc, uint32_t *hist);
int mij_band_tables(mij_batch *b, int n, const uint32_t *hist, unsigned long long *bits);
int mij_band_pack(mij_batch *b, int n, const unsigned long long *bit_offset,
                  unsigned long long *nwords);
int mij_band_words(mij_batch *b, int frame, int comp, void *dst, size_t cap_words,
                   int dst_on_device);
int mij_assemble_begin(mij_batch *b, int n, const uint32_t *hist);
int mij_assemble_words(mij_batch *b, int frame, int comp, unsigned long long first_word,
                       const void *src, size_t nwords, int src_on_device);
int mij_assemble_end(mij_batch *b, int n, const unsigned long long *total_bits);
/* The same exchange in one call per side (what sharding.encode_banded uses):
 * mij_band_words_all copies every scan's band words of frames 0..n-1, in
 * (frame, comp) order, into one buffer (word counts from mij_band_pack);
 * mij_assemble_pieces ORs pieces of one buffer (the gathered band words of
 * all ranks) into the scans in one launch: piece i = pieces[4i..4i+3] =
 * {frame * 3 + comp, first word in the scan, first word in src, words}.  Both
 * return once the copy is done (src / dst may be reused).
 * mij_assembler_create makes a batch that only assembles (tables, scan
 * buffers, outputs: no input, coefficient or token buffers); use it with
 * mij_assemble_begin / _pieces / _words / _end and the output calls. */
int mij_band_words_all(mij_batch *b, int n, void *dst, size_t cap_words, int dst_on_device);
int mij_assemble_pieces(mij_batch *b, const void *src, size_t src_words, int src_on_device,
                        const unsigned long long *pieces, int npieces);
mij_batch *mij_assembler_create(int device, int width, int height, int max_frames, int quality);

/* The same exchange steps, device-resident: every pointer is device memory
 * and every call only enqueues work on the batch's stream (mij_batch_stream)
 * -- nothing waits for the host, so the caller's collectives (RCCL on that
 * same stream) run between the calls.  Shapes: last/prev int16 [n][4]
 * (component c at [f][c]), hist uint32 [n][4][257],
 * bits uint64 [3n + 1] (a band's bits per (frame, scan), then its word
 * count), allbits uint64 [world][3n + 1] (every band's bits, rank order).
 *   band_analyze_async     K1 over the band; its last raw DCs -> d_last
 *   band_histograms_async  the segments' first DC tokens from the previous
 *                          band's last DCs (d_prev; null for band 0: zeros);
 *                          the band's histograms -> d_hist (sum them over
 *                          the bands)
 *   band_tables_async      tables from the summed histograms; an upper bound
 *                          of the band's words (its histograms weighted by
 *                          the code lengths, +3 per frame) -> *d_bound, so
 *                          the caller can size the word exchange while the
 *                          band packs
 *   band_pack_async        every scan of the band packed from bit 0 -> d_bits
 *   band_words_async       moves those words, (frame, scan) order, to d_dst
 *                          (cap_words long; words beyond it are dropped and
 *                          the root's assembly fails those frames)
 *   assemble_tables_async  (root) the tables from the summed histograms (may
 *                          run while the bands pack)
 *   assemble_async         (root) every band's words shifted to its bit
 *                          position (the sum of the earlier bands' bits) and
 *                          OR-ed into the scans from d_src (band r's words at
 *                          row r, stride_words apart), then the JFIF
 *                          assembly; read the frames with mij_batch_output.
 * Replaces the host protocol's mij_band_analyze / _histograms / _tables /
 * _pack / _words_all and mij_assemble_begin / _pieces / _end. */
int mij_band_analyze_async(mij_batch *b, int n, int16_t *d_last);
int mij_band_histograms_async(mij_batch *b, int n, const int16_t *d_prev, uint32_t *d_hist);
int mij_band_tables_async(mij_batch *b, int n, const uint32_t *d_ghist, uint64_t *d_bound);
int mij_band_pack_async(mij_batch *b, int n, uint64_t *d_bits);
int mij_band_words_async(mij_batch *b, int n, uint32_t *d_dst, size_t cap_words);
int mij_assemble_tables_async(mij_batch *b, int n, const uint32_t *d_ghist);
int mij_assemble_async(mij_batch *b, int n, const uint64_t *d_allbits, int world, const uint32_t *d_src,
                       size_t stride_words);
/* A device-to-host copy of `bytes` on the batch's stream (the word bounds
 * and stuffed totals of the device protocol, read by the host to size the
 * word exchange): ordered after the collectives and launches enqueued on
 * that stream before it, so the caller waits for just those (an event on the
 * batch's stream) and not for a copy queued behind the packing on another
 * stream.  h_dst must be pinned host memory. */
int mij_copy_to_host_async(mij_batch *b, void *h_dst, const void *d_src, size_t bytes);
/* Distributed JFIF emission (the config-4 bands, sharding.encode_banded_dev
 * with emit="bands"): after mij_band_pack_async and the all-gather of every
 * band's d_bits into d_allbits [world][3n + 1], band `rank` stuffs the bytes
 * of the final scans that lie wholly inside it (encoder.c:403-408) into
 * d_dst (cap bytes), frames and scans in order; d_rec [n][3][4] (u64) gets
 * per scan {stuffed bytes, band bits, head bits << 8 | head count, tail bits
 * << 8 | tail count} (head: the <= 7 bits completing the byte the bands
 * before began; tail: the bits after the last whole byte) and *d_total the
 * band's stuffed bytes.  The band's scan words are consumed. */
int mij_band_stuff_async(mij_batch *b, int n, const uint64_t *d_allbits, int world, int rank,
                         uint64_t *d_rec, uint64_t *d_total, uint8_t *d_dst, size_t cap);
/* root, after mij_assemble_tables_async: frames 0..n-1 from every band's
 * records d_allrec [world][n][3][4] and stuffed bytes d_src [world][stride]:
 * headers, the seam bytes between bands (stuffed when 0xFF), the pads
 * (encoder.c:425-432), EOI, the interiors copied into place */
int mij_assemble_stuffed_async(mij_batch *b, int n, const uint64_t *d_allrec, int world,
                               const uint8_t *d_src, size_t stride);

/* ---- diagnostics used by the test-suite -----------------------------------*/
/* 16x16x64 i8 MFMA layout probe: A, B are 64 lanes x 16 int8, D 64 x 4 int32 */
int mij_probe_mfma(const int8_t *A, const int8_t *B, int32_t *D);
/* colour-exception bitmaps as built on the device: 3 x 1024 words; bit
 * (R<<7 | G>>1) of table 0 (Y), (G<<7 | B>>1) of table 1 (Cb, R == G),
 * (G<<7 | R>>1) of table 2 (Cr, B == G); see DESIGN.md */
int mij_colour_lut(uint32_t *out);
/* Tests: runs the coefficient K1 (as mij_batch_dct) on frames 0..n-1 of a
 * plain B, G, R batch through its audit variant and copies out every
 * block's fast-path decisions: masks[(f * nblk + blk) * 4 + g] bit k set =
 * zigzag coefficient 16 g + k straddled a truncation boundary (replayed in
 * FP64), blocks in the batch's coefficient order (Y, Cb, Cr). */
int mij_batch_audit(mij_batch *b, int nframes, uint16_t *masks);
/* Tests: the four optimized tables of frames 0..n-1 built from given counts
 * hist[f][4][257] (DC-Y, AC-Y, DC-C, AC-C; entry 256 is ignored, the
 * reserved count of encoder.c:367 is 1); read them with mij_batch_tables.
 * MIJ_ETABLE when a frame's counts have no valid table (mij_last_message). */
int mij_batch_build_tables(mij_batch *b, int n, const uint32_t *hist);
/* name of the code object target the library was built for ("gfx950") */
const char *mij_build_target(void);

/* ---- change detector (reference main/brain.c) ------
 * The reference's per-frame loop (main.c:136-163) subsamples the camera frame
 * 4x4 (brain.c:16-45), compares it with the stored subsampled frame
 * (brain.c:104-233: weighted colour distance > 600 per subsampled pixel,
 * runs of differing pixels joined into at most 100 areas, enlarged to
 * multiples of 16 in frame pixels) and encodes each area.  Here the
 * subsample and the per-pixel test run as one HIP kernel over a
 * device-resident frame that writes one bit per subsampled pixel; the run
 * joining, which is sequential in the reference and keeps its quirks (see
 * DESIGN.md), runs on the host over the runs of that bit mask. */

/* include/structs.h:20-22 */
typedef struct {
    int beg, end, row, done;
} pair_t;

typedef struct mij_detector mij_detector;
/* frame geometry: width and height multiples of 4 (the reference: 320x240);
 * the stored plane starts as zeros, like main.c:33's static `saved` */
mij_detector *mij_detector_create(int device, int width, int height);
void mij_detector_destroy(mij_detector *d);
/* brain.c:16-45 on a device BGR frame (rows pitch bytes apart, pitch and
 * pointer 4-byte aligned) into the detector's current plane */
int mij_detector_subsample(mij_detector *d, const void *d_frame, long long pitch);
/* brain.c:104-233: current plane vs stored plane -> outs[100], *count */
int mij_detector_compare(mij_detector *d, area_t outs[100], int *count);
/* subsample + compare in one kernel launch (main.c:140-143) */
int mij_detector_step(mij_detector *d, const void *d_frame, long long pitch, area_t outs[100],
                      int *count);
/* the step's kernel alone, asynchronous on the detector's stream (the mask
 * stays on the device; for timing) */
int mij_detector_launch(mij_detector *d, const void *d_frame, long long pitch);
/* brain.c:53-60 / main.c:161: stored plane := current plane (device copy) */
int mij_detector_store(mij_detector *d);
/* host BGR frame (height rows pitch bytes apart; pitch 0 = 3*width) into the
 * detector's frame buffer, same pitch; *d_frame receives its device address */
int mij_detector_upload(mij_detector *d, const uint8_t *bgr, long long pitch, const void **d_frame);
/* plane 0 = current, 1 = stored, in the reference's layout (R, G, B bytes per
 * subsampled pixel, (width/4)*(height/4)*3 bytes): read back / set */
int mij_detector_get_plane(mij_detector *d, int which, uint8_t *rgb);
int mij_detector_set_plane(mij_detector *d, int which, const uint8_t *rgb);
/* the kernel's bit mask of the last compare: one row of `words` 64-bit words
 * per subsampled row (bit x%64 of word x/64 = pixel x differs) */
int mij_detector_mask(mij_detector *d, unsigned long long *dst, size_t cap_words, int *words);
void *mij_detector_stream(mij_detector *d);

/* ---- round-trip verifier ---------------------------
 * The reference has no decoder.  mij_decoder turns baseline JFIF streams of
 * the shape encoder.c:549-644 writes (8-bit, Y 2x2 + Cb + Cr 1x1, three
 * one-component scans, no restarts) back into the encoder's coefficient
 * layout: per component, blocks in raster order, 64 zigzag-ordered
 * quantized coefficients, DC as the coded difference (= rgb_to_dct's
 * output), so encode -> decode can be checked bit-exactly at any size.
 * Entropy decoding runs on the GPU, one lane per 512-bit chunk of every
 * scan, the chunks' entry states found by self-synchronisation.
 * From the decoded planes the same object gives pixels
 * (mij_decoder_reconstruct) and, without leaving the coefficient domain, a
 * losslessly re-coded stream (mij_decoder_transcode), each on request. */
typedef struct mij_decoder mij_decoder;
mij_decoder *mij_decoder_create(int device, int max_w, int max_h, int max_frames);
void mij_decoder_destroy(mij_decoder *d);
/* n host streams; synchronous; MIJ_EJPEG names the stream on failure */
int mij_decoder_decode(mij_decoder *d, const uint8_t *const *jpgs, const size_t *lens, int n);
/* frame size and the two DQT tables (zigzag order) of stream `frame` */
int mij_decoder_info(mij_decoder *d, int frame, int *w, int *h, uint8_t dqt[128]);
/* Y[w*h], Cb[w*h/4], Cr[w*h/4] of stream `frame` (host copies) */
int mij_decoder_coefs(mij_decoder *d, int frame, int16_t *Y, int16_t *Cb, int16_t *Cr);
/* self-synchronisation passes the last decode needed */
int mij_decoder_passes(mij_decoder *d);
/* device address of stream `frame`'s planes (Y, then Cb, then Cr) */
void *mij_decoder_device_coefs(mij_decoder *d, int frame);

/* ---- progressive files -----------------------------------------
 * Opt-in: with MIJ_ACCEPT_PROGRESSIVE set, mij_decoder_decode (and the
 * loader's decoder) also takes 8-bit Huffman progressive streams (SOF2),
 * greyscale or YCbCr under the sampling and Adobe rules of the baseline
 * files below, up to 64 scans, DC and AC Huffman table ids 0..3, DHT and DRI
 * between scans, restart intervals counted in each scan's own MCUs.  The
 * scan script must be legal and complete (T.81 G.1.1.1): MIJ_EJPEG names the
 * stream, the scan and the rule otherwise, before any device work.  Each
 * restart interval of each scan is decoded sequentially by one GPU wave (one
 * lane of it working) into the same arena, scans that depend on each other in successive launches
 * ("levels"); afterwards the frame is served exactly as an interleaved
 * baseline frame without restart intervals: layout, component, reconstruct
 * at every scale, transcode and transform work unchanged, and one call may
 * mix all three kinds of stream.  Corrupt entropy data gives MIJ_EJPEG,
 * "stream %d scan %d: corrupt entropy data (code)": 5 the bits end early,
 * 6 invalid code, 8 an end-of-band run past its restart interval, 9 a
 * coefficient index past Se.
 * The mask holds until changed and is 0 at creation: with the bit clear
 * nothing differs from a library without it, SOF2 is refused as not
 * baseline.  Unknown bits: MIJ_EINVAL, the mask unchanged.  The one-shot
 * calls (mij_decode, mij_decode_scaled, mij_transcode, mij_transform,
 * mij_thumbnail*) always refuse SOF2.
 *
 * MIJ_ACCEPT_440: three-component streams with luma 1x2 and
 * chroma 1x1 ("4:4:0": what jpegtran, a phone gallery or this library's own
 * transforms make of a 4:2:2 file turned by a quarter), baseline, and
 * progressive when MIJ_ACCEPT_PROGRESSIVE is set as well.  The MCU is 8 x 16,
 * two luma blocks top then bottom; the chroma planes are w x ceil(h / 2) and
 * are upsampled as libjpeg's h1v2_fancy_upsample does (at 1/8 scale each row
 * twice), the pixels libjpeg's byte for byte at every scale.  Such a frame
 * is served like any other: layout, component, reconstruct at every scale,
 * transcode (SOF H/V bytes 0x12 0x11 0x11), transform, thumbnails, the loader.
 * With the bit set a transposing operation of mij_decoder_transform on a
 * frame whose H != V is planned with every component's H and V swapped
 * (4:2:2 -> 4:4:0, 4:4:0 -> 4:2:2, as jpegtran does) instead of refused.
 * With the bit clear nothing differs from a library without it; the one-shot
 * calls always refuse luma 1x2 and that operation.  Bit value 2 is unknown. */
#define MIJ_ACCEPT_PROGRESSIVE 1
#define MIJ_ACCEPT_440 4
int mij_decoder_accept(mij_decoder *d, unsigned mask);
/* of stream `frame` of the last decode (any pointer may be NULL): 1 if it was
 * progressive; its scans (a baseline file: 1, the encoder's shape: 3); the
 * dependent launches its scans were sorted into (not progressive: 1).
 * mij_decoder_passes counts self-synchronising passes only: 0 for a call of
 * progressive streams alone. */
int mij_decoder_scan_info(mij_decoder *d, int frame, int *progressive, int *nscans, int *levels);
/* Host only: width and height from the frame header (SOFn of any kind, found
 * in front of the first SOS; no other rule is applied), for sizing a decoder
 * before a stream that the one-shot calls refuse.  1 if found, else 0 with
 * *w and *h untouched (either may be NULL). */
int mij_jpeg_size(const uint8_t *jpg, size_t len, int *w, int *h);

/* ---- ordinary baseline files -------------------------------------------------
 * mij_decoder_decode also accepts what libjpeg, Pillow, cameras and browsers
 * write: 8-bit baseline (SOF0, Huffman), greyscale or YCbCr with luma 1x1
 * (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) -- with MIJ_ACCEPT_440 also 1x2
 * (4:4:0) -- and chroma 1x1, any width and height
 * up to the decoder's, one interleaved scan, DQT ids 0..3, arbitrary
 * component ids, restart intervals.  Such a frame's planes are padded to
 * whole MCUs; mij_decoder_coefs / _planes are defined as the encoder's layout
 * and return MIJ_EINVAL on it: use the three calls below, which work on
 * every frame.  All frames of a call share one set of device buffers, packed
 * in the order of the call.  Each buffer's first allocation takes what
 * max_frames frames of max_w x max_h of the encoder's shape need (the
 * coefficients' at mij_decoder_create, the others' at first use) and grows
 * (is freed and allocated again) only when a call's padded planes need more;
 * a decoder that only sees the encoder's streams never reallocates.
 *
 * layout: out[0..8] = w, h, components, max H, max V, MCUs across, MCUs
 * down, restart interval (0 = none), 1 if one interleaved scan; then per
 * component H, V, Tq, blocks across, blocks down of its padded plane.
 * MIJ_ENOSPC if n < 9 + 5 * components (at most 24). */
#define MIJ_LAYOUT_MAX 24
int mij_decoder_layout(mij_decoder *d, int frame, int *out, int n);
/* host copy of component comp's padded plane: blocks in raster order, 64
 * zigzag-ordered quantized coefficients each, the DC ABSOLUTE (the view
 * libjpeg's jpeg_read_coefficients gives); cap in coefficients */
int mij_decoder_component(mij_decoder *d, int frame, int comp, int16_t *dst, size_t cap);

/* ---- decode to pixels -------------------------------------------------------
 * The decoded coefficients through libjpeg's integer ("islow") IDCT, its h2v2
 * "fancy" chroma upsampling and its fixed-point colour conversion, on the
 * GPU: on the streams libjpeg decodes correctly the pixels are libjpeg's byte
 * for byte (DESIGN.md "Decode to pixels" states the arithmetic and the one
 * kind of stream on which the two differ). */
enum { MIJ_PIX_BGR = 0, MIJ_PIX_RGB = 1 };
/* all frames of the last mij_decoder_decode -> planes and pixels; async on
 * the decoder's stream; buffers allocated on first use, so a decoder used
 * only as verifier costs what it costs without this call */
int mij_decoder_reconstruct(mij_decoder *d, int order);
/* host copy of frame's w*h pixels, rows pitch bytes apart (0 = 3*w; the bytes
 * between rows are not written); waits */
int mij_decoder_pixels(mij_decoder *d, int frame, uint8_t *dst, size_t cap, long long pitch);
/* the IDCT output before upsampling: Y[w*h], Cb[w*h/4], Cr[w*h/4] */
int mij_decoder_planes(mij_decoder *d, int frame, uint8_t *Y, uint8_t *Cb, uint8_t *Cr);
/* host copy of component comp's padded sample plane after the IDCT (8 *
 * blocks across bytes per row, 8 * blocks down rows), before upsampling:
 * tells an IDCT error from an upsampling error; cap in bytes */
int mij_decoder_plane(mij_decoder *d, int frame, int comp, uint8_t *dst, size_t cap);
/* device address of frame's pixels, rows *pitch bytes apart: 3*w rounded up
 * to 16 (for widths that are multiples of 16 that is 3*w, packed rows, usable
 * with mij_batch_set_input); the bytes of a row past 3*w hold anything.
 * Valid until the next decode.  The pixels are complete once the decoder's
 * stream has reached this point */
void *mij_decoder_device_pixels(mij_decoder *d, int frame, long long *pitch);
/* HIP-event times of the last reconstruct: {dc + idct, colour}; waits */
int mij_decoder_reconstruct_ms(mij_decoder *d, float ms[2]);
/* the decoder's stream, like mij_batch_stream */
void *mij_decoder_stream(mij_decoder *d);
/* one call, host to host, mirror of mij_encode: out receives w*h packed
 * pixels, *w and *h (either may be NULL) the stream's size, as soon as its
 * headers are read: also with MIJ_ENOSPC, which is returned before any
 * device work, so a call with cap 0 asks for the size.  MIJ_EINVAL for
 * a pixels / planes / device_pixels call before reconstruct or after a newer
 * decode, MIJ_ENOSPC for a short cap (everywhere above) */
int mij_decode(const uint8_t *jpg, size_t len, int order, uint8_t *out, size_t cap, int *w, int *h);

/* ---- decode at 1/2, 1/4, 1/8 scale ---------------------------
 * What djpeg -scale 1/N and Pillow's Image.draft give: libjpeg's reduced
 * IDCTs make 4x4, 2x2 or 1x1 samples of every block (4:2:0 chroma twice that,
 * so it needs no upsampling), and the pixels are libjpeg's byte for byte.  The
 * output is ceil(w * s / 8) x ceil(h * s / 8) with s = 8 / denom.
 *
 * mij_decoder_reconstruct_scaled: as mij_decoder_reconstruct, at 1/denom;
 * denom 1 IS mij_decoder_reconstruct, 2, 4, 8 as above, anything else
 * MIJ_EINVAL before any device work.  Afterwards mij_decoder_pixels,
 * _device_pixels (pitch: 3 * scaled width rounded up to 16) and
 * _reconstruct_ms serve the scaled result, mij_decoder_plane gives the
 * component's scaled padded plane (mij_decoder_scaled_layout: rows x pitch
 * bytes; the bytes of a row past S * blocks across are 0), and
 * mij_decoder_planes returns MIJ_EINVAL.  A later reconstruct of either
 * kind replaces the result; transcode and transform are not affected. */
int mij_decoder_reconstruct_scaled(mij_decoder *d, int order, int denom);
/* host only, valid after a decode, denom 1, 2, 4 or 8 (else MIJ_EINVAL):
 * out[0..2] = scaled width, scaled height,
 * components; then per component the IDCT's output size S (S x S samples per
 * block), the component's real width and height in samples, the bytes
 * between rows of its padded plane and that plane's rows.  MIJ_ENOSPC if
 * n < 3 + 5 * components (at most 18) */
#define MIJ_SCALED_LAYOUT_MAX 18
int mij_decoder_scaled_layout(mij_decoder *d, int frame, int denom, int *out, int n);
/* mirror of mij_decode at 1/denom: *w and *h receive the SCALED size as soon
 * as the headers are read, also with MIJ_ENOSPC (cap 0 asks for the size
 * without a device) */
int mij_decode_scaled(const uint8_t *jpg, size_t len, int order, int denom, uint8_t *out, size_t cap, int *w,
                      int *h);

/* ---- resize: thumbnails at any size --------------------------
 * What PIL.Image.resize(size, resample) gives for BOX, BILINEAR and BICUBIC
 * (no `box`, no `reducing_gap`), byte for byte, on 3-byte interleaved 8-bit
 * pixels in device memory: Pillow's fixed-point resampler (22-bit weights from
 * double-precision coefficients, int32 sums, horizontal pass to an 8-bit
 * intermediate, then vertical; a pass whose sizes are equal is skipped, both
 * equal is a copy).  The channels are resampled alike, so the byte order does
 * not matter.  Sizes are 1..65535 a side.
 *
 * A source image is any device pointer and pitch (>= 3 * w), no alignment
 * asked, so it may be a rectangle inside a larger image (crop, then resize).
 * It is read as mij_batch_pad_input reads: whole aligned 4-byte words that hold
 * at least one byte of the image's rows.  Frames of a call may all differ in
 * both sizes.  The results live in the resizer's buffers, which grow on
 * demand: rows 3 * out_w rounded up to 16 bytes apart (the bytes past 3 *
 * out_w hold anything), as mij_decoder_device_pixels lays them out, so they go
 * to mij_batch_pad_input unchanged.
 *
 * MIJ_EINVAL before any device work, the message naming the frame and the
 * argument: an unknown filter, a size outside 1..65535, a pitch under 3 * w,
 * n outside 1..max_frames, a null image, a pixels call before a resize.  A
 * refused call leaves the previous result served. */
enum { MIJ_RS_BOX = 0, MIJ_RS_BILINEAR = 1, MIJ_RS_BICUBIC = 2 };
typedef struct { const void *px; long long pitch; int w, h; } mij_image;   /* device memory */
typedef struct mij_resizer mij_resizer;
mij_resizer *mij_resizer_create(int device, int max_frames);
void mij_resizer_destroy(mij_resizer *r);
/* n device images to out_wh = {w0, h0, w1, h1, ...}; async on the resizer's stream */
int mij_resizer_resize(mij_resizer *r, const mij_image *src, const int *out_wh, int n, int filter);
/* device address of frame's pixels and their pitch; valid until the next
 * resize, complete once the resizer's stream has reached this point */
void *mij_resizer_device_pixels(mij_resizer *r, int frame, long long *pitch);
/* host copy, rows pitch bytes apart (0 = 3 * out_w); MIJ_ENOSPC for a short cap; waits */
int mij_resizer_pixels(mij_resizer *r, int frame, uint8_t *dst, size_t cap, long long pitch);
int mij_resizer_ms(mij_resizer *r, float ms[2]);           /* {horizontal, vertical}; waits */
void *mij_resizer_stream(mij_resizer *r);
int mij_resizer_set_stream(mij_resizer *r, void *stream);  /* as mij_batch_set_stream */
/* host to host; cap 0 asks for the size (MIJ_ENOSPC, before any device work) */
int mij_resize(const uint8_t *px, int stride_px, int w, int h, int out_w, int out_h, int filter,
               uint8_t *out, size_t cap);
/* jpg -> jpg at exactly out_w x out_h: mij_decoder_reconstruct_scaled at
 * mij_thumbnail_denom, a resize of the whole scaled image, then
 * mij_batch_pad_input + mij_batch_encode_interleaved (4:2:0, no restart
 * intervals: mij_encode_any's stream), all on one stream, the pixels never
 * leaving the device.  Refuses what mij_decode refuses, with its message;
 * MIJ_ENOSPC with mij_max_jpg_bytes_any(out_w, out_h, 0) in *out_len when cap
 * is under it, before any device work */
int mij_thumbnail(const uint8_t *jpg, size_t len, int out_w, int out_h, int filter, int quality,
                  uint8_t *out, size_t cap, size_t *out_len);
/* mij_thumbnail with mij_batch_encode_libjpeg at `sampling` (MIJ_SAMP_*) at
 * the end: the coefficients of Image.draft -> resize -> save(quality,
 * subsampling).  The same refusals; the bound is mij_max_jpg_bytes_sampled(
 * out_w, out_h, sampling, 0) */
int mij_thumbnail_libjpeg(const uint8_t *jpg, size_t len, int out_w, int out_h, int filter, int quality,
                          int sampling, uint8_t *out, size_t cap, size_t *out_len);
/* Pillow's Image.draft rule: the largest of 8, 4, 2, 1 that is <= min(w /
 * out_w, h / out_h) in integer division, 1 if none is (and for sizes < 1) */
int mij_thumbnail_denom(int w, int h, int out_w, int out_h);   /* host only */

/* ---- pixels to tensors ----------------------------------------
 * The last stage of an input pipeline: n device images of 3-byte pixels, all
 * of one size w x h, into ONE dense tensor [n, 3, h, w] (MIJ_T_NCHW) or
 * [n, h, w, 3] (MIJ_T_NHWC) in caller-owned device memory, for instance a
 * torch tensor's data_ptr().  The element tensor channel c gets for source
 * byte v is torchvision's to_tensor followed by normalize, in IEEE single
 * precision, round to nearest even:
 *     t = (float)v / 255.0f;   t = t - mean[c];   t = t / std[c];
 * MIJ_T_F32 stores t, MIJ_T_F16 / MIJ_T_BF16 t rounded to nearest even (what
 * tensor.to(torch.float16 / torch.bfloat16) gives), MIJ_T_U8 stores v (mean
 * and std are not read).  The values come from a table built on the host, so
 * they are the same bits on every device.  swap = 1: tensor channel c reads
 * pixel byte 2 - c (BGR pixels, RGB tensor).  mirror: one flag per frame (NULL:
 * none); output column x of a flagged frame reads source column w - 1 - x.
 *
 * A source image is what mij_resizer_resize takes: any device pointer, any
 * pitch >= 3 * w, read in whole aligned 4-byte words that hold at least one
 * byte of the image's rows.  d_dst is 16-byte aligned and holds
 * mij_tensor_bytes(n, w, h, dtype) bytes.  The run is asynchronous on the
 * tensorizer's stream.  d_dst == NULL: the tensor goes to a buffer the
 * tensorizer owns (it grows on demand; cap_bytes is not read), served by
 * mij_tensorizer_device and mij_tensorizer_read until the next such run.
 *
 * Refused with MIJ_EINVAL before any device work, the message naming the frame
 * and the argument, decided in this order: an unknown dtype or layout; swap
 * outside 0 / 1; for the float dtypes a mean that is not finite or a std that
 * is 0 or not finite; a null src; n outside 1..max_frames; per frame a null
 * image, a size outside 1..65535, a pitch under 3 * w, a size other than
 * frame 0's; a d_dst that is not 16-byte aligned; then MIJ_ENOSPC for
 * cap_bytes under mij_tensor_bytes (the message gives the need: a cap of 0
 * asks for it); a null tensorizer last.  A refused call leaves the previous
 * owned result served. */
enum { MIJ_T_U8 = 0, MIJ_T_F16 = 1, MIJ_T_BF16 = 2, MIJ_T_F32 = 3 };
enum { MIJ_T_NCHW = 0, MIJ_T_NHWC = 1 };
typedef struct { int dtype, layout, swap; float mean[3], std[3]; } mij_tensor_spec;
typedef struct mij_tensorizer mij_tensorizer;
mij_tensorizer *mij_tensorizer_create(int device, int max_frames);
void mij_tensorizer_destroy(mij_tensorizer *t);
int mij_tensorizer_run(mij_tensorizer *t, const mij_image *src, const uint8_t *mirror /* n flags or NULL */,
                       int n, const mij_tensor_spec *spec, void *d_dst, size_t cap_bytes);
/* bytes of the tensor; 0 for n < 1, a size outside 1..65535, an unknown dtype */
size_t mij_tensor_bytes(int n, int w, int h, int dtype);   /* host only */
/* the owned buffer of the last run with d_dst == NULL and its size; complete
 * once the tensorizer's stream has reached this point; NULL (MIJ_EINVAL)
 * before such a run */
void *mij_tensorizer_device(mij_tensorizer *t, size_t *bytes);
/* host copy of it; MIJ_ENOSPC for a short cap; waits */
int mij_tensorizer_read(mij_tensorizer *t, void *dst, size_t cap);
int mij_tensorizer_ms(mij_tensorizer *t, float *ms);       /* HIP-event time of the last run; waits */
void *mij_tensorizer_stream(mij_tensorizer *t);
int mij_tensorizer_set_stream(mij_tensorizer *t, void *stream);  /* as mij_batch_set_stream */

/* The chain that ends in it: n stored JPEGs to one tensor.  A loader owns a
 * decoder (for streams up to max_w x max_h), a resizer and a tensorizer on one
 * stream.  mij_loader_load:
 *   decode     the n streams, of any accepted kind and differing sizes, in one
 *              mij_decoder_decode;
 *   scale      one mij_decoder_reconstruct_scaled(order, d) for the call:
 *              d = denom (1, 2, 4, 8), or with denom 0 the smallest
 *              mij_thumbnail_denom(crop w, crop h, out_w, out_h) over the
 *              frames, so that no frame is enlarged from fewer samples than
 *              it needs (mij_loader_denom gives the last call's d);
 *   crop       crops[i] = (x, y, w, h) in full-size pixels, inside the frame,
 *              w, h >= 1 (NULL: whole frames) becomes the scaled image's
 *              rectangle x0 = x / d, y0 = y / d, x1 = min(ceil(W / d),
 *              ceil((x + w) / d)), y1 likewise;
 *   resize     every rectangle to out_w x out_h with `filter` (MIJ_RS_*) in
 *              one mij_resizer_resize;
 *   tensorize  the results into d_dst (or the owned buffer) as
 *              mij_tensorizer_run does, with its spec, mirror flags, cap and
 *              refusals.
 * Asynchronous from the reconstruct on, on mij_loader_stream.  Refused before
 * any device work: what mij_decode refuses of a stream's headers, with its
 * code and message; MIJ_EINVAL for a bad spec, n, out size, filter, denom,
 * order, a stream larger than the loader's, a crop that is empty or outside
 * its frame, a misaligned d_dst; MIJ_ENOSPC for a short cap; a null loader
 * last. */
typedef struct mij_loader mij_loader;
mij_loader *mij_loader_create(int device, int max_w, int max_h, int max_frames);
void mij_loader_destroy(mij_loader *l);
int mij_loader_load(mij_loader *l, const uint8_t *const *jpgs, const size_t *lens, int n,
                    const area_t *crops /* n, full-size pixels, or NULL */, const uint8_t *mirror,
                    int out_w, int out_h, int filter, int denom /* 1,2,4,8; 0 = auto */,
                    int order, const mij_tensor_spec *spec, void *d_dst, size_t cap_bytes);
int mij_loader_denom(mij_loader *l);                       /* of the last load; 0 before one */
int mij_loader_accept(mij_loader *l, unsigned mask);       /* mij_decoder_accept of the loader's decoder */
void *mij_loader_device(mij_loader *l, size_t *bytes);     /* as mij_tensorizer_device */
int mij_loader_read(mij_loader *l, void *dst, size_t cap); /* as mij_tensorizer_read */
/* {entropy decode (mij_decoder_decode's span on the stream, its host parsing
 * included), reconstruct, resize, tensorize} of the last load, ms; waits */
int mij_loader_ms(mij_loader *l, float ms[4]);
void *mij_loader_stream(mij_loader *l);

/* ---- lossless transcoding ------------------------------------
 * What jpegtran -optimize does, on the GPU: every frame of the last decode,
 * of either kind above, becomes one standard interleaved baseline stream
 * with the SAME quantized coefficients (the blocks of the MCU padding as
 * decoded), sampling, size, component ids and DQT bytes; only the entropy
 * code is rebuilt.  Huffman tables are optimised for the new scan (DC/AC of
 * component 0, DC/AC of components 1 and 2 together; a greyscale file gets
 * two), restart intervals are restart_rows whole MCU rows of the source's
 * MCU grid (0: none; DRI = restart_rows * MCUs across, written whenever
 * restart_rows > 0), whatever interval the source had.  Headers: SOI, the
 * JFIF APP0 of mij_encode_any, one DQT per table id in use (ascending),
 * DHTs, SOF0 with the source's component entries verbatim, DRI, one SOS.
 * Every other segment of the source is DROPPED: APPn (EXIF, ICC, Adobe,
 * the source's JFIF density), COM, its Huffman tables.  A three-scan stream
 * of mij_encode becomes byte for byte what mij_encode_any writes for the
 * same frame.  Decoding the result gives the source's coefficients, so any
 * decoder gives the source's pixels.
 *
 * MIJ_EINVAL before any device work for restart_rows < 0 or an interval over
 * 65535 MCUs in any frame (the message names it), and for a call before a
 * successful decode.  The call waits for the device (the frames' bit counts
 * size its buffers, which are allocated on first use and grow; a decoder
 * that never transcodes allocates none).  It neither needs nor disturbs
 * mij_decoder_reconstruct: both may follow one decode, in either order.  A
 * frame whose tables cannot be built (MIJ_ETABLE from the two calls below,
 * length 0) does not fail the others.
 *
 * DC range.  A block's absolute DC is the sum of its interval's coded
 * differences modulo 2^16, as int16: what mij_decoder_component reports,
 * what the pixels are made from and what is coded here.  A stream no 8-bit
 * image gives can put neighbouring DCs of the new scan more than 32767
 * apart; that difference is of category 16, which no JPEG can carry.  Such a
 * frame is refused: MIJ_EJPEG from the two calls below, with a message naming
 * the frame, length 0, nothing written; the other frames of the call are
 * served.  So a stream this call returns always decodes, here and in
 * libjpeg, to the source's coefficients.  (mij_transcode, one frame, fails
 * as a whole.  Progressive output, MIJ_OUT_PROGRESSIVE, cannot meet the
 * case: its first DC scan codes the DCs halved.) */
int mij_decoder_transcode(mij_decoder *d, int restart_rows);
/* host copy of frame's stream; *len (may be NULL) its size, also with
 * MIJ_ENOSPC (cap 0, dst NULL asks for it); waits.  MIJ_EINVAL before a
 * transcode or after a newer decode */
int mij_decoder_transcoded(mij_decoder *d, int frame, uint8_t *dst, size_t cap, size_t *len);
/* device address and size of frame's stream, valid until the next decode or
 * transcode; NULL (and mij_last_error) where the call above fails */
void *mij_decoder_device_transcoded(mij_decoder *d, int frame, size_t *len);
/* HIP-event time of the last transcode (ms), its mid-call wait for the bit
 * counts included; waits */
int mij_decoder_transcode_ms(mij_decoder *d, float *ms);
/* one call, host to host; cap 0 asks for the size (MIJ_ENOSPC, the exact
 * length in *out_len).  A stream the decoder refuses returns its MIJ_EJPEG
 * and message */
int mij_transcode(const uint8_t *jpg, size_t len, int restart_rows, uint8_t *out, size_t cap, size_t *out_len);

/* ---- lossless transforms --------------------------------------
 * The other half of jpegtran, in the coefficient domain: flip, transpose,
 * rotation by 90/180/270 and MCU-aligned crop of every frame of the last
 * decode, then coded as mij_decoder_transcode codes it.  No coefficient is
 * requantised: blocks move, coefficients inside them are transposed and
 * change sign.  Order: crop, then the edge rule, then the operation.
 *   crop (x, y, w, h) in source pixels: x a multiple of 8*Hmax, y of 8*Vmax,
 *   w, h >= 1, inside the frame; the result is w x h, a partial last MCU
 *   keeps the source's blocks beyond the crop.  NULL: the whole frame.
 *   edge rule: an operation that mirrors the source's width (FLIP_H, ROT180,
 *   TRANSVERSE, ROT270) needs it to be whole MCUs, one that mirrors its height
 *   (FLIP_V, ROT180, TRANSVERSE, ROT90) likewise; otherwise the call is
 *   refused (jpegtran -perfect) or, with MIJ_XF_TRIM, the dimension is cut
 *   down to whole MCUs first (jpegtran -trim).
 *   headers as mij_decoder_transcode writes them; a transposing operation
 *   swaps width and height and the nibbles of every SOF0 H/V byte and
 *   transposes every DQT.  APPn / COM segments are dropped, an EXIF
 *   orientation with them.  restart_rows counts MCU rows of the OUTPUT.
 * MIJ_EINVAL before any device work, naming the frame and the reason: an
 * unknown op or flag bit; a crop that is misaligned, empty or outside the
 * frame; a mirrored dimension that is not whole MCUs without MIJ_XF_TRIM, or
 * of which nothing is left with it; a transposing operation on a frame with a
 * component whose H != V (4:2:2, 4:4:0) unless the decoder has MIJ_ACCEPT_440
 * set, with which it can read the result (H and V of every component swap:
 * the trim and whole-MCU rules use the source's MCU, the output grid and
 * restart_rows the output's); an
 * interval over 65535 MCUs of the output grid.  One refused frame refuses the
 * call.  MIJ_XF_NONE without a crop is mij_decoder_transcode, byte for byte.
 * The results are read with mij_decoder_transcoded, _device_transcoded and
 * _transcode_ms: "the last transcode" there is the last transcode or
 * transform.  The transformed planes live in buffers allocated at the first
 * transform; the decoded planes stay as they are (reconstruct and transcode
 * may follow). */
enum { MIJ_XF_NONE = 0, MIJ_XF_FLIP_H, MIJ_XF_FLIP_V, MIJ_XF_TRANSPOSE, MIJ_XF_TRANSVERSE,
       MIJ_XF_ROT90, MIJ_XF_ROT180, MIJ_XF_ROT270 };        /* jpegtran's JXFORM order; ROT90 is clockwise */
enum { MIJ_XF_TRIM = 1 };                                    /* flags */
int mij_decoder_transform(mij_decoder *d, int op, int flags, const area_t *crop, int restart_rows);
/* one call, host to host, as mij_transcode: cap 0 asks for the size; the
 * refusals above come before any device work */
int mij_transform(const uint8_t *jpg, size_t len, int op, int flags, const area_t *crop,
                  int restart_rows, uint8_t *out, size_t cap, size_t *out_len);
/* EXIF orientation 1..8 of a stream (APP1 "Exif", IFD0 tag 0x0112); 1 when
 * there is none or it is malformed.  Host only */
int mij_exif_orientation(const uint8_t *jpg, size_t len);   /* 1..8; 1 when there is none; host only */
/* the operation that makes an image of that orientation upright (NONE for
 * anything outside 1..8) */
int mij_orientation_op(int orientation);                    /* the op that makes it upright */

/* ---- progressive output ----------------------------------------
 * What jpegtran -progressive does: mij_decoder_transcode and
 * mij_decoder_transform write every frame as a progressive file (SOF2)
 * instead of one baseline scan.  Sticky like mij_decoder_accept; the default
 * is MIJ_OUT_BASELINE, under which both calls write the bytes described
 * above.  The same
 * coefficients, sampling, size, component ids and DQT bytes as the baseline
 * output; the scans are libjpeg's jpeg_simple_progression (ten for YCbCr:
 * DC with Al 1, Y 1-5 Al 2, Cr and Cb 1-63 Al 1, Y 6-63 Al 2, Y refined to
 * Al 1, DC refined, Cr, Cb, Y refined to Al 0; the six of component 0 for
 * greyscale), coded by the rules of libjpeg's jcphuff.c with one optimised
 * Huffman table per scan and component group, written in front of its scan
 * (DC ids 0 / 1, AC ids 0 / 1 for component 0 / the others).  A scan of one
 * component covers the blocks of that component's own ceil(w_c / 8) x
 * ceil(h_c / 8) grid, so AC coefficients of MCU-padding blocks outside it
 * are not coded (jpegtran does the same; no pixel changes).  restart_rows = r
 * gives every scan the interval r x (its own MCUs across), a DRI wherever
 * that changes; MIJ_EINVAL before any device work when r < 0 or an interval
 * of any scan of any frame exceeds 65535 (the message names the frame).  A
 * frame for which any table cannot be built gets length 0 and MIJ_ETABLE;
 * the others succeed.  mij_decoder_transcoded, _device_transcoded and
 * _transcode_ms serve the result as before.  The tables are this library's,
 * not libjpeg's: the bytes differ from jpegtran's, the decoded coefficients
 * do not. */
enum { MIJ_OUT_BASELINE = 0, MIJ_OUT_PROGRESSIVE = 1 };
int mij_decoder_output(mij_decoder *d, int format);
/* one call, host to host, as mij_transcode, from a baseline or a progressive
 * stream to a progressive one; cap 0 asks for the size */
int mij_transcode_progressive(const uint8_t *jpg, size_t len, int restart_rows, uint8_t *out, size_t cap,
                              size_t *out_len);

/* Drop-in entry points of include/brain.h:7-10, on frames of
 * mij_set_input_stride() x mij_set_frame_height() pixels (define.h:3-4,
 * 320x240 by default).  subsample writes the PPM copy to f when f is not
 * NULL (brain.c:22, :29-42).  compare uses differences (2 rows of WIDTH/8
 * runs, main.c:35) as scratch like the reference.  Errors: mij_last_error. */
int mij_set_frame_height(int height);
void subsample(FILE *f, uint8_t *in, uint8_t *out);
void store(uint8_t *in, uint8_t *saved);
uint8_t compare(uint8_t *in, uint8_t *saved, area_t *outs, pair_t (*differences)[]);
void enlargeAdjust(area_t *a);

#ifdef __cplusplus
}
#endif
#endif /* MIJPEG_H */
