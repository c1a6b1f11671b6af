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
 *   thumbnail_jpg [-filter box|bilinear|bicubic] [-quality Q] [--libjpeg [--sampling 444|422|420|gray]] [--440]
 *                 WxH <in.jpg> <out.jpg>
 *
 * Defaults: bicubic, quality 75.  With --libjpeg the last stage is
 * mij_thumbnail_libjpeg: libjpeg's quantisation tables and coefficients for
 * that quality, at the --sampling (4:2:0 unless given), the ones Pillow's
 * draft -> resize -> save writes.  With --440 4:4:0 files (luma 1x2) are taken
 * too: the same stages on one stream through a decoder object with
 * MIJ_ACCEPT_440 set (the one-shot calls refuse them).
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
    fprintf(stderr, "usage: %s [-filter box|bilinear|bicubic] [-quality Q] [--libjpeg [--sampling 444|422|420|gray]] [--440] "
                    "WxH <in.jpg> <out.jpg>\n", prog);
    return 2;
}

/* mij_thumbnail / mij_thumbnail_libjpeg spelt out on a decoder that accepts 4:4:0 */
static int thumbnail_440(const uint8_t *jpg, size_t len, int ow, int oh, int filter, int quality, int libjpeg,
                         int sampling, uint8_t *out, size_t cap, size_t *n) {
    int w = 16, h = 16, rc;
    if (ow < 1 || oh < 1 || ow > 65535 || oh > 65535 || quality < 1 || quality > 100) {
        fprintf(stderr, "out size %dx%d (1..65535 each), quality %d (1..100)\n", ow, oh, quality);
        return MIJ_EINVAL;
    }
    mij_jpeg_size(jpg, len, &w, &h);
    if (w < 1) w = 1;
    if (h < 1) h = 1;
    mij_decoder *d = mij_decoder_create(0, (w + 15) / 16 * 16, (h + 15) / 16 * 16, 1);
    mij_resizer *r = d ? mij_resizer_create(0, 1) : NULL;
    mij_batch *b = r ? mij_batch_create(0, (ow + 15) / 16 * 16, (oh + 15) / 16 * 16, 1, quality) : NULL;
    rc = b ? MIJ_OK : mij_last_error();
    if (!rc) rc = mij_decoder_accept(d, MIJ_ACCEPT_440);
    if (!rc) rc = mij_resizer_set_stream(r, mij_decoder_stream(d));
    if (!rc) rc = mij_batch_set_stream(b, mij_decoder_stream(d));
    const uint8_t *streams[1] = {jpg};
    if (!rc) rc = mij_decoder_decode(d, streams, &len, 1);
    if (!rc) rc = mij_decoder_info(d, 0, &w, &h, NULL);
    const int denom = mij_thumbnail_denom(w, h, ow, oh);
    if (!rc) rc = mij_decoder_reconstruct_scaled(d, MIJ_PIX_BGR, denom);
    mij_image im = {NULL, 0, (w + denom - 1) / denom, (h + denom - 1) / denom};
    if (!rc && !(im.px = mij_decoder_device_pixels(d, 0, &im.pitch))) rc = mij_last_error();
    const int wh[2] = {ow, oh};
    if (!rc) rc = mij_resizer_resize(r, &im, wh, 1, filter);
    long long pitch = 0;
    const void *px = !rc ? mij_resizer_device_pixels(r, 0, &pitch) : NULL;
    if (!rc && !px) rc = mij_last_error();
    if (!rc) rc = mij_batch_pad_input(b, px, 0, pitch, wh, 1);
    if (!rc) rc = libjpeg ? mij_batch_encode_libjpeg(b, 1, sampling, 0) : mij_batch_encode_interleaved(b, 1, 0);
    if (!rc) rc = mij_batch_output(b, 0, out, cap, n);
    /* the borrowers of the decoder's stream first; a failure's message stays in place */
    if (b) mij_batch_destroy(b);
    if (r) mij_resizer_destroy(r);
    if (d) mij_decoder_destroy(d);
    return rc;
}

int main(int argc, char **argv) {
    const char *prog = argv[0];
    int filter = MIJ_RS_BICUBIC, quality = 75, libjpeg = 0, sampling = -1, accept440 = 0;
    while (argc > 2 && argv[1][0] == '-' && argv[1][1]) {
        const char *o = argv[1], *v = argv[2];
        if (!strcmp(o, "--libjpeg")) { /* no value */
            libjpeg = 1;
            argc--;
            argv++;
            continue;
        }
        if (!strcmp(o, "--440")) { /* no value */
            accept440 = 1;
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
    if (accept440) {
        n = libjpeg ? mij_max_jpg_bytes_sampled(ow, oh, sampling, 0) : mij_max_jpg_bytes_any(ow, oh, 0);
        uint8_t *buf = malloc(n ? n : 1);
        if (!buf) { fprintf(stderr, "out of memory\n"); free(jpg); return 1; }
        int bad = 0;
        int trc = thumbnail_440(jpg, len, ow, oh, filter, quality, libjpeg, sampling, buf, n, &n);
        if (trc != MIJ_OK) {
            bad = fail(argv[2], trc);
        } else {
            FILE *tf = fopen(argv[3], "wb");
            if (!tf || fwrite(buf, 1, n, tf) != n || fclose(tf)) {
                perror(argv[3]);
                bad = 1;
            } else {
                printf("%s: %zu bytes -> %dx%d, %zu bytes -> %s\n", argv[2], len, ow, oh, n, argv[3]);
            }
        }
        free(buf);
        free(jpg);
        return bad;
    }
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
