/*
 * transcode_jpg.c -- C host for libmijpeg.so's lossless transcoding, next to
 * decode_jpg.c.
 *
 * Re-codes a baseline JPEG (what decode_jpg accepts) without touching its
 * quantized coefficients, as jpegtran -optimize does: one interleaved scan,
 * Huffman tables optimised for it, restart intervals of restart_rows MCU rows
 * (0, the default: none).  Every decoder gives the same pixels from the
 * output as from the input.  APPn / COM segments are not carried over.
 * Entropy decoding and coding both run on the GPU.
 *
 *   transcode_jpg [options] <in.jpg> <out.jpg> [restart_rows]
 *
 * With options, the other half of jpegtran, as lossless (mij_decoder_transform):
 *   -flip h|v  -rotate 90|180|270  -transpose  -transverse
 *   -auto             the operation that makes the file's EXIF orientation upright
 *   -crop WxH+X+Y     X and Y multiples of the MCU size
 *   -trim             cut a mirrored edge down to whole MCUs instead of refusing it
 *   --progressive     also take progressive files (MIJ_ACCEPT_PROGRESSIVE):
 *                     "progressive in, optimised baseline out"
 *   --440             also take 4:4:0 files, luma 1x2 (MIJ_ACCEPT_440); a
 *                     transposing operation then turns 4:2:2 into 4:4:0 and
 *                     back instead of being refused
 *   --write-progressive   write a progressive file (jpegtran -progressive,
 *                     mij_decoder_output): libjpeg's ten-scan script, tables
 *                     optimised per scan; restart_rows counts rows of each
 *                     scan's own MCUs
 * restart_rows then counts MCU rows of the output.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mijpeg.h"

static uint8_t *read_file(const char *path, size_t *len) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return NULL; }
    long n = -1;
    if (!fseek(f, 0, SEEK_END)) n = ftell(f);
    uint8_t *buf = n > 0 ? malloc((size_t)n) : NULL;
    if (!buf || fseek(f, 0, SEEK_SET) || fread(buf, 1, (size_t)n, f) != (size_t)n) {
        fprintf(stderr, "%s: cannot read\n", path);
        free(buf);
        fclose(f);
        return NULL;
    }
    fclose(f);
    *len = (size_t)n;
    return buf;
}

static int fail(const char *what, int rc) {
    fprintf(stderr, "%s: %s: %s\n", what, mij_strerror(rc), mij_last_message());
    return 1;
}

static int usage(const char *prog) {
    fprintf(stderr, "usage: %s [--progressive] [--440] [--write-progressive] [-flip h|v] [-rotate 90|180|270] [-transpose] [-transverse] [-auto] [-trim]\n"
            "       [-crop WxH+X+Y] <in.jpg> <out.jpg> [restart_rows]\n", prog);
    return 2;
}

int main(int argc, char **argv) {
    const char *prog = argv[0];
    int op = MIJ_XF_NONE, flags = 0, have_crop = 0, have_xf = 0, automatic = 0, write_progressive = 0;
    unsigned accept = 0;
    area_t crop = {0, 0, 0, 0};
    while (argc > 1 && argv[1][0] == '-' && argv[1][1]) {
        const char *o = argv[1], *v = argc > 2 ? argv[2] : "";
        int used = 1;
        if (!strcmp(o, "--progressive")) {
            accept |= MIJ_ACCEPT_PROGRESSIVE;
            argc--;
            argv++;
            continue;
        }
        if (!strcmp(o, "--440")) {
            accept |= MIJ_ACCEPT_440;
            argc--;
            argv++;
            continue;
        }
        if (!strcmp(o, "--write-progressive")) {
            write_progressive = 1;
            argc--;
            argv++;
            continue;
        }
        if (!strcmp(o, "-flip") && (!strcmp(v, "h") || !strcmp(v, "v"))) {
            op = v[0] == 'h' ? MIJ_XF_FLIP_H : MIJ_XF_FLIP_V, used = 2;
        } else if (!strcmp(o, "-rotate") && (!strcmp(v, "90") || !strcmp(v, "180") || !strcmp(v, "270"))) {
            op = !strcmp(v, "90") ? MIJ_XF_ROT90 : !strcmp(v, "180") ? MIJ_XF_ROT180 : MIJ_XF_ROT270, used = 2;
        } else if (!strcmp(o, "-transpose")) {
            op = MIJ_XF_TRANSPOSE;
        } else if (!strcmp(o, "-transverse")) {
            op = MIJ_XF_TRANSVERSE;
        } else if (!strcmp(o, "-auto")) {
            automatic = 1;
        } else if (!strcmp(o, "-trim")) {
            flags |= MIJ_XF_TRIM;
        } else if (!strcmp(o, "-crop") && sscanf(v, "%dx%d+%d+%d", &crop.w, &crop.h, &crop.x, &crop.y) == 4) {
            have_crop = 1, used = 2;
        } else {
            return usage(prog);
        }
        have_xf = 1;
        argc -= used;
        argv += used;
    }
    if (argc != 3 && argc != 4) return usage(prog);
    const int restart_rows = argc == 4 ? atoi(argv[3]) : 0;
    size_t len = 0;
    uint8_t *jpg = read_file(argv[1], &len);
    if (!jpg) return 1;
    if (automatic) op = mij_orientation_op(mij_exif_orientation(jpg, len));
    /* the frame size, for the decoder: mij_decode reports it with MIJ_ENOSPC
     * before any device work */
    int w = 0, h = 0;
    uint8_t probe;
    int rc;
    if (accept) {  /* the one-shot calls refuse SOF2 and luma 1x2: the size from the frame header itself */
        w = h = 16;
        mij_jpeg_size(jpg, len, &w, &h);
        if (w < 1) w = 1;
        if (h < 1) h = 1;
    } else {
        rc = mij_decode(jpg, len, MIJ_PIX_RGB, &probe, 0, &w, &h);
        if (rc != MIJ_ENOSPC) return fail(argv[1], rc);
    }
    mij_decoder *d = mij_decoder_create(0, (w + 15) / 16 * 16, (h + 15) / 16 * 16, 1);
    if (!d) return fail("mij_decoder_create", mij_last_error());
    if (accept && (rc = mij_decoder_accept(d, accept)) != MIJ_OK) return fail("mij_decoder_accept", rc);
    if (write_progressive && (rc = mij_decoder_output(d, MIJ_OUT_PROGRESSIVE)) != MIJ_OK) return fail("mij_decoder_output", rc);
    const uint8_t *streams[1] = {jpg};
    if ((rc = mij_decoder_decode(d, streams, &len, 1)) != MIJ_OK) return fail(argv[1], rc);
    rc = have_xf ? mij_decoder_transform(d, op, flags, have_crop ? &crop : NULL, restart_rows)
                 : mij_decoder_transcode(d, restart_rows);
    if (rc != MIJ_OK) return fail(argv[1], rc);
    size_t n = 0;
    if (!mij_decoder_device_transcoded(d, 0, &n)) return fail(argv[1], mij_last_error());
    uint8_t *out = malloc(n);
    if (!out) { fprintf(stderr, "out of memory\n"); return 1; }
    if ((rc = mij_decoder_transcoded(d, 0, out, n, &n)) != MIJ_OK) return fail(argv[1], rc);
    FILE *f = fopen(argv[2], "wb");
    if (!f || fwrite(out, 1, n, f) != n || fclose(f)) {
        perror(argv[2]);
        return 1;
    }
    printf("%s: %dx%d, %zu -> %zu bytes -> %s\n", argv[1], w, h, len, n, argv[2]);
    mij_decoder_destroy(d);
    free(out);
    free(jpg);
    return 0;
}
