/*
 * thumbnail_jpg.c -- C host for libmijpeg.so's thumbnailer, next to
 * decode_jpg.c and transcode_jpg.c.
 *
 * Makes a JPEG of exactly WxH pixels from a baseline JPEG (what decode_jpg
 * accepts): decoded at the largest of 1/8, 1/4, 1/2, 1/1 scale that still
 * covers WxH (Pillow's Image.draft rule), resampled to WxH as Pillow's
 * Image.resize does, encoded as mij_encode_any encodes (4:2:0, one scan).  The
 * pixels never leave the GPU (mij_thumbnail).
 *
 *   thumbnail_jpg [-filter box|bilinear|bicubic] [-quality Q] [--libjpeg [--sampling 444|422|420|gray]]
 *                 WxH <in.jpg> <out.jpg>
 *
 * Defaults: bicubic, quality 75.  With --libjpeg the last stage is
 * mij_thumbnail_libjpeg: libjpeg's quantisation tables and coefficients for
 * that quality, at the --sampling (4:2:0 unless given), the ones Pillow's
 * draft -> resize -> save writes.
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
    fprintf(stderr, "usage: %s [-filter box|bilinear|bicubic] [-quality Q] [--libjpeg [--sampling 444|422|420|gray]] "
                    "WxH <in.jpg> <out.jpg>\n", prog);
    return 2;
}

int main(int argc, char **argv) {
    const char *prog = argv[0];
    int filter = MIJ_RS_BICUBIC, quality = 75, libjpeg = 0, sampling = -1;
    while (argc > 2 && argv[1][0] == '-' && argv[1][1]) {
        const char *o = argv[1], *v = argv[2];
        if (!strcmp(o, "--libjpeg")) { /* no value */
            libjpeg = 1;
            argc--;
            argv++;
            continue;
        }
        if (!strcmp(o, "--sampling")) {
            static const char *const names[4] = {"420", "422", "444", "gray"};
            for (int k = 0; k < 4; k++)
                if (!strcmp(v, names[k])) sampling = k;
            if (sampling < 0) return usage(prog);
        }
        else if (!strcmp(o, "-filter") && !strcmp(v, "box")) filter = MIJ_RS_BOX;
        else if (!strcmp(o, "-filter") && !strcmp(v, "bilinear")) filter = MIJ_RS_BILINEAR;
        else if (!strcmp(o, "-filter") && !strcmp(v, "bicubic")) filter = MIJ_RS_BICUBIC;
        else if (!strcmp(o, "-quality")) quality = atoi(v);
        else return usage(prog);
        argc -= 2;
        argv += 2;
    }
    if (sampling >= 0 && !libjpeg) {
        fprintf(stderr, "--sampling needs --libjpeg: the default arithmetic writes 4:2:0\n");
        return 2;
    }
    if (sampling < 0) sampling = MIJ_SAMP_420;
    int ow = 0, oh = 0;
    if (argc != 4 || sscanf(argv[1], "%dx%d", &ow, &oh) != 2) return usage(prog);
    size_t len = 0, n = 0;
    uint8_t *jpg = read_file(argv[2], &len);
    if (!jpg) return 1;
    /* the output's bound: mij_thumbnail reports it with MIJ_ENOSPC before any device work */
    int rc = libjpeg ? mij_thumbnail_libjpeg(jpg, len, ow, oh, filter, quality, sampling, NULL, 0, &n)
                     : mij_thumbnail(jpg, len, ow, oh, filter, quality, NULL, 0, &n);
    if (rc != MIJ_ENOSPC) return fail(argv[2], rc);
    uint8_t *out = malloc(n);
    if (!out) { fprintf(stderr, "out of memory\n"); return 1; }
    rc = libjpeg ? mij_thumbnail_libjpeg(jpg, len, ow, oh, filter, quality, sampling, out, n, &n)
                 : mij_thumbnail(jpg, len, ow, oh, filter, quality, out, n, &n);
    if (rc != MIJ_OK) return fail(argv[2], rc);
    FILE *f = fopen(argv[3], "wb");
    if (!f || fwrite(out, 1, n, f) != n || fclose(f)) {
        perror(argv[3]);
        return 1;
    }
    printf("%s: %zu bytes -> %dx%d, %zu bytes -> %s\n", argv[2], len, ow, oh, n, argv[3]);
    free(out);
    free(jpg);
    return 0;
}
