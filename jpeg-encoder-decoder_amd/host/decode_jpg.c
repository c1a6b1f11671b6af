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
 * With -scale 1/2, 1/4 or 1/8 the image comes out at that scale through
 * mij_decode_scaled, as djpeg -scale gives it (libjpeg's reduced IDCTs).
 *
 * With --progressive progressive files are decoded too, through a decoder
 * object with MIJ_ACCEPT_PROGRESSIVE set (the one-shot calls refuse them).
 * With --440 4:4:0 files, luma 1x2, are decoded too, the same way
 * (MIJ_ACCEPT_440).  The options may come in any order.
 *
 *   decode_jpg [--progressive] [--440] [-scale 1/N] <in.jpg> <out.ppm>
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

int main(int argc, char **argv) {
    int denom = 1;
    unsigned accept = 0;
    const char *prog = argv[0];
    while (argc > 1 && argv[1][0] == '-' && argv[1][1]) {
        int used = 1;
        if (!strcmp(argv[1], "--progressive")) {
            accept |= MIJ_ACCEPT_PROGRESSIVE;
        } else if (!strcmp(argv[1], "--440")) {
            accept |= MIJ_ACCEPT_440;
        } else if (!strcmp(argv[1], "-scale") && argc > 2) {
            char tail = 0;
            if (sscanf(argv[2], "1/%d%c", &denom, &tail) != 1 || (denom != 1 && denom != 2 && denom != 4 && denom != 8)) {
                fprintf(stderr, "%s: -scale %s: 1/1, 1/2, 1/4 or 1/8\n", prog, argv[2]);
                return 2;
            }
            used = 2;
        } else {
            break;  /* the usage message below */
        }
        argv += used;
        argc -= used;
    }
    if (argc != 3) {
        fprintf(stderr, "usage: %s [--progressive] [--440] [-scale 1/N] <in.jpg> <out.ppm>\n", prog);
        return 2;
    }
    size_t len = 0;
    uint8_t *jpg = read_file(argv[1], &len);
    if (!jpg) return 1;
    /* the frame size is in SOF0: 65535 x 65535 at most, found by a first call
     * that reports the size and MIJ_ENOSPC before any device work */
    int w = 0, h = 0;
    uint8_t probe;
    if (accept) {
        int fw = 16, fh = 16;
        mij_jpeg_size(jpg, len, &fw, &fh);
        mij_decoder *d = mij_decoder_create(0, fw < 16 ? 16 : (fw + 15) / 16 * 16, fh < 16 ? 16 : (fh + 15) / 16 * 16, 1);
        const uint8_t *streams[1] = {jpg};
        int lay[3 + 5 * 3];
        int prc = d ? mij_decoder_accept(d, accept) : mij_last_error();
        if (!prc) prc = mij_decoder_decode(d, streams, &len, 1);
        if (!prc) prc = mij_decoder_reconstruct_scaled(d, MIJ_PIX_RGB, denom);
        if (!prc) prc = mij_decoder_scaled_layout(d, 0, denom, lay, 3 + 5 * 3);
        const size_t pcap = !prc ? (size_t)3 * lay[0] * lay[1] : 0;
        uint8_t *ppx = !prc ? malloc(pcap) : NULL;
        int bad = 0;
        if (!prc && !ppx) {
            fprintf(stderr, "out of memory\n");
            bad = 1;
        }
        if (!prc && !bad) prc = mij_decoder_pixels(d, 0, ppx, pcap, 0);
        if (prc) {
            fprintf(stderr, "%s: %s: %s\n", argv[1], mij_strerror(prc), mij_last_message());
            bad = 1;
        }
        if (!bad) {
            FILE *pf = fopen(argv[2], "wb");
            if (!pf || fprintf(pf, "P6\n%d %d\n255\n", lay[0], lay[1]) < 0 || fwrite(ppx, 1, pcap, pf) != pcap || fclose(pf)) {
                perror(argv[2]);
                bad = 1;
            } else {
                printf("%s: %dx%d -> %s\n", argv[1], lay[0], lay[1], argv[2]);
            }
        }
        if (d) mij_decoder_destroy(d);
        free(ppx);
        free(jpg);
        return bad;
    }
    int rc = mij_decode_scaled(jpg, len, MIJ_PIX_RGB, denom, &probe, 0, &w, &h);
    if (rc != MIJ_ENOSPC) {
        fprintf(stderr, "%s: %s: %s\n", argv[1], mij_strerror(rc), mij_last_message());
        return 1;
    }
    size_t cap = (size_t)3 * w * h;
    uint8_t *px = malloc(cap);
    if (!px) { fprintf(stderr, "out of memory\n"); return 1; }
    rc = mij_decode_scaled(jpg, len, MIJ_PIX_RGB, denom, px, cap, &w, &h);
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
