/*
 * decode_jpg.c -- C host for libmijpeg.so's decoder, next to encode_ppm.c.
 *
 * Turns a baseline JPEG (8-bit; greyscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0; any
 * size; one interleaved scan with or without restart intervals, as libjpeg,
 * cameras and browsers write it, or the encoder's own three scans) into a P6
 * PPM through mij_decode: entropy decoding, IDCT, chroma upsampling and
 * colour conversion all run on the GPU.  Anything else is refused with the
 * reason.
 *
 *   decode_jpg <in.jpg> <out.ppm>
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

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <in.jpg> <out.ppm>\n", argv[0]);
        return 2;
    }
    size_t len = 0;
    uint8_t *jpg = read_file(argv[1], &len);
    if (!jpg) return 1;
    /* the frame size is in SOF0: 65535 x 65535 at most, found by a first call
     * that reports the size and MIJ_ENOSPC before any device work */
    int w = 0, h = 0;
    uint8_t probe;
    int rc = mij_decode(jpg, len, MIJ_PIX_RGB, &probe, 0, &w, &h);
    if (rc != MIJ_ENOSPC) {
        fprintf(stderr, "%s: %s: %s\n", argv[1], mij_strerror(rc), mij_last_message());
        return 1;
    }
    size_t cap = (size_t)3 * w * h;
    uint8_t *px = malloc(cap);
    if (!px) { fprintf(stderr, "out of memory\n"); return 1; }
    rc = mij_decode(jpg, len, MIJ_PIX_RGB, px, cap, &w, &h);
    if (rc != MIJ_OK) {
        fprintf(stderr, "%s: %s: %s\n", argv[1], mij_strerror(rc), mij_last_message());
        return 1;
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f || fprintf(f, "P6\n%d %d\n255\n", w, h) < 0 || fwrite(px, 1, cap, f) != cap || fclose(f)) {
        perror(argv[2]);
        return 1;
    }
    printf("%s: %dx%d -> %s\n", argv[1], w, h, argv[2]);
    free(px);
    free(jpg);
    return 0;
}
