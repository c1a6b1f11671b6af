/*
 * encode_ppm.c -- C host for libmijpeg.so.
 *
 * Reproduces the reference caller's sequence (main.c:144-152:
 * rgb_to_dct -> init_huffman -> write_jpg on caller-owned buffers) on a PPM
 * file, with the PPM checks of utils/original.c:294-365 (P6, '#' comments,
 * depth 255, width/height multiples of 16).  The PPM is RGB; the encoder's
 * input convention is BGR888 (encoder.c:133), so channels are swapped on load.
 *
 *   encode_ppm <in.ppm> <out.jpg> [quality] [x y w h] [--fused]
 *   encode_ppm <in.ppm> <out.jpg> [quality] --sampling 444|422|420|gray
 *   encode_ppm <in.ppm> <out.jpg> [quality] --libjpeg [--sampling 444|422|420|gray]
 *
 * With --sampling the PPM may have any size and becomes one standard
 * interleaved baseline stream at that chroma sampling (mij_encode_sampled).
 * With --libjpeg the stream has libjpeg's quantisation tables and
 * coefficients for that quality and sampling, 4:2:0 unless --sampling says
 * otherwise (mij_encode_libjpeg).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mijpeg.h"

static uint8_t *read_ppm_bgr(const char *path, int *w, int *h, int any_size) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return NULL; }
    char magic[3] = {0};
    if (fread(magic, 1, 2, f) != 2 || strcmp(magic, "P6")) {
        fprintf(stderr, "%s: not a P6 PPM\n", path);
        fclose(f);
        return NULL;
    }
    int vals[3], n = 0;
    while (n < 3) {
        int c = fgetc(f);
        if (c == EOF) break;
        if (c == '#') { while (c != '\n' && c != EOF) c = fgetc(f); continue; }
        if (c == ' ' || c == '\t' || c == '\n' || c == '\r') continue;
        ungetc(c, f);
        if (fscanf(f, "%d", &vals[n]) != 1) break;
        n++;
    }
    fgetc(f); /* single whitespace after the depth */
    if (n != 3 || vals[2] != 255 || vals[0] <= 0 || vals[1] <= 0 || (!any_size && (vals[0] % 16 || vals[1] % 16))) {
        fprintf(stderr, "%s: need depth 255 and dimensions %s\n", path, any_size ? "above 0" : "multiple of 16");
        fclose(f);
        return NULL;
    }
    *w = vals[0];
    *h = vals[1];
    size_t np = (size_t)*w * *h;
    uint8_t *px = malloc(np * 3);
    if (!px || fread(px, 3, np, f) != np) {
        fprintf(stderr, "%s: truncated pixel data\n", path);
        free(px);
        fclose(f);
        return NULL;
    }
    fclose(f);
    for (size_t i = 0; i < np; i++) { uint8_t t = px[3 * i]; px[3 * i] = px[3 * i + 2]; px[3 * i + 2] = t; }
    return px;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s <in.ppm> <out.jpg> [quality] [x y w h] [--fused]\n"
                        "       %s <in.ppm> <out.jpg> [quality] --sampling 444|422|420|gray\n"
                        "       %s <in.ppm> <out.jpg> [quality] --libjpeg [--sampling 444|422|420|gray]\n",
                argv[0], argv[0], argv[0]);
        return 2;
    }
    int fused = 0, sampling = -1, libjpeg = 0;
    for (int i = 3; i < argc; i++)
        if (!strcmp(argv[i], "--libjpeg")) { /* the option leaves the argument list */
            libjpeg = 1;
            for (int j = i; j + 1 < argc; j++) argv[j] = argv[j + 1];
            argc--;
            break;
        }
    for (int i = 3; i + 1 < argc; i++)
        if (!strcmp(argv[i], "--sampling")) { /* the option and its value leave the argument list */
            static const char *const names[4] = {"420", "422", "444", "gray"};
            for (int k = 0; k < 4; k++)
                if (!strcmp(argv[i + 1], names[k])) sampling = k;
            if (sampling < 0) {
                fprintf(stderr, "--sampling %s: one of 444, 422, 420, gray\n", argv[i + 1]);
                return 2;
            }
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    if (!strcmp(argv[argc - 1], "--fused")) { fused = 1; argc--; }
    if (libjpeg && sampling < 0) sampling = MIJ_SAMP_420;
    int W, H;
    uint8_t *raw = read_ppm_bgr(argv[1], &W, &H, sampling >= 0);
    if (!raw) return 1;
    int quality = argc > 3 ? atoi(argv[3]) : 50;
    if (sampling >= 0) {
        size_t bound = mij_max_jpg_bytes_sampled(W, H, sampling, 0), n = 0;
        uint8_t *out = malloc(bound ? bound : 1);
        if (!out || (libjpeg ? mij_encode_libjpeg : mij_encode_sampled)(raw, W, W, H, MIJ_PIX_BGR, quality, sampling, 0, out,
                                                                         bound, &n) != MIJ_OK) {
            fprintf(stderr, "%s: %s\n", argv[1], mij_last_message());
            return 1;
        }
        FILE *f = fopen(argv[2], "wb");
        if (!f || fwrite(out, 1, n, f) != n) { perror(argv[2]); return 1; }
        fclose(f);
        printf("%s: %dx%d Q=%d sampling %d%s -> %zu bytes\n", argv[2], W, H, quality, sampling,
               libjpeg ? ", libjpeg's arithmetic" : "", n);
        free(raw);
        free(out);
        return 0;
    }
    area_t dims = {0, 0, W, H};
    if (argc > 7) { dims.x = atoi(argv[4]); dims.y = atoi(argv[5]); dims.w = atoi(argv[6]); dims.h = atoi(argv[7]); }
    size_t cap = mij_max_jpg_bytes(dims.w, dims.h);
    uint8_t *jpg = malloc(cap ? cap : 1);
    size_t size = 0;
    if (fused) {
        if (mij_encode(raw, W, dims, quality, jpg, cap, &size) != MIJ_OK) return 1;
        FILE *f = fopen(argv[2], "wb");
        if (!f || fwrite(jpg, 1, size, f) != size) { perror(argv[2]); return 1; }
        fclose(f);
    } else {
        /* caller-owned buffers as in main.c:25-37 */
        int16_t *Y = malloc(sizeof(int16_t) * dims.w * dims.h);
        int16_t *Cb = malloc(sizeof(int16_t) * dims.w * dims.h / 4);
        int16_t *Cr = malloc(sizeof(int16_t) * dims.w * dims.h / 4);
        huff_code Luma[2], Chroma[2];
        mij_set_input_stride(W); /* define.h:3 WIDTH, now a runtime value */
        if (mij_set_quality(quality) != MIJ_OK) return 1;
        rgb_to_dct(raw, Y, Cb, Cr, dims);
        if (mij_last_error()) return 1;
        init_huffman(Y, Cb, Cr, dims, Luma, Chroma);
        if (mij_last_error()) return 1;
        FILE *f = fopen(argv[2], "wb");
        if (!f) { perror(argv[2]); return 1; }
        size = write_jpg(f, jpg, Y, Cb, Cr, dims, Luma, Chroma);
        fclose(f);
        if (!size) return 1;
        free(Y); free(Cb); free(Cr);
    }
    printf("%s: %dx%d region (%d,%d %dx%d) Q=%d -> %zu bytes\n", argv[2], W, H, dims.x, dims.y,
           dims.w, dims.h, quality, size);
    free(raw);
    free(jpg);
    return 0;
}
