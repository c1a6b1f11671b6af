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
 *   transcode_jpg <in.jpg> <out.jpg> [restart_rows]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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

int main(int argc, char **argv) {
    if (argc != 3 && argc != 4) {
        fprintf(stderr, "usage: %s <in.jpg> <out.jpg> [restart_rows]\n", argv[0]);
        return 2;
    }
    const int restart_rows = argc == 4 ? atoi(argv[3]) : 0;
    size_t len = 0;
    uint8_t *jpg = read_file(argv[1], &len);
    if (!jpg) return 1;
    /* the frame size, for the decoder: mij_decode reports it with MIJ_ENOSPC
     * before any device work */
    int w = 0, h = 0;
    uint8_t probe;
    int rc = mij_decode(jpg, len, MIJ_PIX_RGB, &probe, 0, &w, &h);
    if (rc != MIJ_ENOSPC) return fail(argv[1], rc);
    mij_decoder *d = mij_decoder_create(0, (w + 15) / 16 * 16, (h + 15) / 16 * 16, 1);
    if (!d) return fail("mij_decoder_create", mij_last_error());
    const uint8_t *streams[1] = {jpg};
    if ((rc = mij_decoder_decode(d, streams, &len, 1)) != MIJ_OK) return fail(argv[1], rc);
    if ((rc = mij_decoder_transcode(d, restart_rows)) != MIJ_OK) return fail(argv[1], rc);
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
