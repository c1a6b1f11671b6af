// mij_tensor.hip -- pixels to tensors: n device images of
// 3-byte interleaved 8-bit pixels, all of one size, into one dense
// [n, 3, h, w] or [n, h, w, 3] tensor of uint8, float16, bfloat16 or float32,
// scaled by 1/255 and normalised per channel (the arithmetic: mij_tensor.h),
// optionally with the channels swapped and single frames mirrored; and the
// chain that ends in it (mij_loader_*: decode, reconstruct at a scale, crop +
// resize, tensorize on one stream).
//
//   k_tensorize   one launch over every frame of a call.  A workgroup owns
//                 TZ_ROWS rows of TZ_SEG pixels of one frame.  The bytes of
//                 those pixels come into LDS as they lie in memory, in whole
//                 aligned dwords (the source has any alignment and pitch),
//                 the host-built table lut[3][256] beside them.  The tile's
//                 output is TZ_ROWS lines of 3 * TZ_SEG elements (NHWC) or
//                 3 * TZ_ROWS lines of TZ_SEG elements (NCHW: one per channel
//                 plane and row); a line is cut at the 16-byte boundaries of
//                 the destination, and a lane takes one such piece: it looks
//                 its 16, 8 or 4 elements up and stores them with one
//                 16-byte store, or, at a line's unaligned head and tail, one
//                 element at a time.  The kernel is specialised by element
//                 size and layout; the dtype is in the table.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "mij_host.h"
#include "mij_resize.h"
#include "mij_tensor.h"

#define HIP_TRY(x)                                                                 \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess)                                                          \
      return mij_fail(MIJ_EHIP, "%s failed: %s", #x, hipGetErrorString(e_));       \
  } while (0)

namespace mij {

// aligned dwords that hold the 3 * TZ_SEG bytes of a row segment begun up to 3 bytes into the first
constexpr int TZ_WORDS = (3 * TZ_SEG + 3 + 3) / 4;
constexpr int TZ_LUT_BYTES = 3 * 256 * 4;  // the table at the widest element

struct TzJob {
  const uint8_t *src;
  long long spitch;
  int mirror, pad;
};

#define TZ_GLOBAL __attribute__((address_space(1)))
typedef uint32_t tz_u32x4 __attribute__((ext_vector_type(4)));

// Bounds.  Every index below comes from w, h, the pitch and the tile
// constants, which the host checked (1..65535 a side, pitch >= 3 * w, grid =
// n * tiles_x * tiles_y), none from pixel data; a source byte only indexes the
// 256 entries of its channel's table.  Source reads stay inside aligned dwords
// that hold at least one byte of the row being read (the contract
// mij_batch_pad_input documents).  Stores stay inside [A0, A1), the line's own
// elements of the dense tensor: a 16-byte store only where all 16 bytes are.
template <int ES, bool NHWC>
__global__ __launch_bounds__(256) void k_tensorize(const TzJob *jobs, const uint32_t *lut, uint8_t *dst, int w, int h,
                                                   int tiles_x, int tiles_y, int swap) {
  __shared__ uint32_t s_lut[3 * 256 * ES / 4];
  __shared__ uint32_t s_src[TZ_ROWS][TZ_WORDS];
  const int per = tiles_x * tiles_y;
  const int f = (int)blockIdx.x / per, t = (int)blockIdx.x - f * per;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int x0 = tx * TZ_SEG, nx = min(TZ_SEG, w - x0);    // nx >= 1: tiles_x = ceil(w / TZ_SEG)
  const int y0 = ty * TZ_ROWS, ny = min(TZ_ROWS, h - y0);  // ny >= 1 likewise
  const TzJob J = jobs[f];
  const bool mirror = J.mirror != 0;
  // output columns x0 .. x0 + nx - 1 read source columns sx0 .. sx0 + nx - 1 (mirrored: from the right)
  const int sx0 = mirror ? w - x0 - nx : x0;
  const uintptr_t seg0 = (uintptr_t)J.src + (long long)y0 * J.spitch + 3LL * sx0;  // row y0's first byte
  for (int i = threadIdx.x; i < 3 * 256 * ES / 4; i += 256) s_lut[i] = lut[i];
  for (int i = threadIdx.x; i < TZ_ROWS * TZ_WORDS; i += 256) {
    const int r = i / TZ_WORDS, j = i - r * TZ_WORDS;
    const uintptr_t start = seg0 + (long long)r * J.spitch, a0 = start & ~(uintptr_t)3;
    const int nwords = (int)((start + 3u * (unsigned)nx - a0 + 3) >> 2);  // <= TZ_WORDS
    if (r < ny && j < nwords) s_src[r][j] = *(TZ_GLOBAL const uint32_t *)(a0 + 4ull * j);
  }
  __syncthreads();

  constexpr int EPC = 16 / ES;                                   // elements of a 16-byte piece
  constexpr int PIECES = (NHWC ? 3 : 1) * TZ_SEG * ES / 16 + 1;  // pieces of a line at most, its first begun anywhere
  const int lines = NHWC ? ny : 3 * ny, le = NHWC ? 3 * nx : nx;
  for (int item = threadIdx.x; item < lines * PIECES; item += 256) {
    const int line = item / PIECES, k = item - line * PIECES;
    const int r = NHWC ? line : line / 3, c = NHWC ? 0 : line - 3 * r;
    const long long y = y0 + r;
    const long long e0 = NHWC ? (((long long)f * h + y) * w + x0) * 3 : (((long long)f * 3 + c) * h + y) * w + x0;
    const uintptr_t A0 = (uintptr_t)dst + (unsigned long long)e0 * ES, A1 = A0 + (unsigned long long)le * ES;
    const uintptr_t C = (A0 & ~(uintptr_t)15) + 16ull * k;
    const uintptr_t lo = C > A0 ? C : A0, hi = C + 16 < A1 ? C + 16 : A1;
    if (lo >= hi) continue;
    // the row's bytes in LDS: byte b of source pixel sx0 + p at sb[3 * p + b]
    const uint8_t *sb = (const uint8_t *)s_src[r] + ((seg0 + (long long)r * J.spitch) & 3);
    // element i of the line: column x0 + xr, channel cc
    const int i0 = (int)((lo - A0) / ES);
    int xr = NHWC ? i0 / 3 : i0, cc = NHWC ? i0 - 3 * xr : c;
    auto next = [&]() -> uint32_t {
      const int p = mirror ? nx - 1 - xr : xr;
      const uint32_t v = sb[3 * p + tz_src_channel(cc, swap)];
      const int at = 256 * cc + (int)v;
      uint32_t e;
      if (ES == 1) e = ((const uint8_t *)s_lut)[at];
      else if (ES == 2) e = ((const uint16_t *)s_lut)[at];
      else e = s_lut[at];
      if (NHWC) {
        if (++cc == 3) cc = 0, xr++;
      } else {
        xr++;
      }
      return e;
    };
    if (hi - lo == 16) {
      uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < EPC; j++) o[j * ES / 4] |= next() << (8 * (j * ES % 4));
      tz_u32x4 v4;
      v4.x = o[0], v4.y = o[1], v4.z = o[2], v4.w = o[3];
      *(TZ_GLOBAL tz_u32x4 *)lo = v4;
    } else {
      for (uintptr_t a = lo; a < hi; a += ES) {
        const uint32_t e = next();
        if (ES == 1) *(TZ_GLOBAL uint8_t *)a = (uint8_t)e;
        else if (ES == 2) *(TZ_GLOBAL uint16_t *)a = (uint16_t)e;
        else *(TZ_GLOBAL uint32_t *)a = e;
      }
    }
  }
}

}  // namespace mij

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
namespace {

size_t round_to(size_t v, size_t m) { return (v + m - 1) / m * m; }
bool tz_side(int v) { return v >= 1 && v <= mij::TZ_MAX_SIDE; }

// the spec's refusals; mean and std only where they are used
int tz_check_spec(const char *what, const mij_tensor_spec *s) {
  if (!s) return mij_fail(MIJ_EINVAL, "%s: null spec", what);
  if (s->dtype < 0 || s->dtype >= mij::TZ_DTYPES)
    return mij_fail(MIJ_EINVAL, "%s: dtype %d (MIJ_T_U8, MIJ_T_F16, MIJ_T_BF16 or MIJ_T_F32)", what, s->dtype);
  if (s->layout < 0 || s->layout >= mij::TZ_LAYOUTS)
    return mij_fail(MIJ_EINVAL, "%s: layout %d (MIJ_T_NCHW or MIJ_T_NHWC)", what, s->layout);
  if (s->swap != 0 && s->swap != 1) return mij_fail(MIJ_EINVAL, "%s: swap %d (0 or 1)", what, s->swap);
  if (s->dtype != MIJ_T_U8)
    for (int c = 0; c < 3; c++) {
      if (!isfinite(s->mean[c])) return mij_fail(MIJ_EINVAL, "%s: mean[%d] is not finite", what, c);
      if (!isfinite(s->std[c]) || s->std[c] == 0.0f)
        return mij_fail(MIJ_EINVAL, "%s: std[%d] is %g (finite and not 0)", what, c, (double)s->std[c]);
    }
  return MIJ_OK;
}

// a caller's destination: 16-byte aligned and long enough (none: the owned buffer)
int tz_check_dst(const char *what, const void *d_dst, size_t cap, size_t need) {
  if (!d_dst) return MIJ_OK;
  if ((uintptr_t)d_dst & 15) return mij_fail(MIJ_EINVAL, "%s: d_dst %p is not 16-byte aligned", what, d_dst);
  if (cap < need) return mij_fail(MIJ_ENOSPC, "%s: need %zu bytes", what, need);
  return MIJ_OK;
}

}  // namespace

extern "C" size_t mij_tensor_bytes(int n, int w, int h, int dtype) {
  const int es = mij::tz_esize(dtype);
  if (n < 1 || !tz_side(w) || !tz_side(h) || !es) return 0;
  unsigned long long b = 3ULL * (unsigned)es * (unsigned)w * (unsigned)h;  // under 2^36
  if (__builtin_mul_overflow(b, (unsigned long long)n, &b) || b > SIZE_MAX) return 0;
  return (size_t)b;
}

struct mij_tensorizer {
  int dev = 0, cap = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};  // around the launch
  hipEvent_t ev_up = nullptr;             // the staging buffer's upload is done
  hipEvent_t ev_switch = nullptr;
  uint8_t *d_own = nullptr;               // the owned destination
  size_t own_cap = 0, own_bytes = 0;
  bool own_valid = false, ran = false;
  uint8_t *h_stage = nullptr, *d_stage = nullptr;  // the jobs, then the table: one copy per call
  size_t jobs_bytes = 0;
};

static void tensorizer_free(mij_tensorizer *t) {
  if (!t) return;
  hipSetDevice(t->dev);
  if (t->stream) hipStreamSynchronize(t->stream);
  if (t->own_stream && t->own_stream != t->stream) hipStreamSynchronize(t->own_stream);
  hipFree(t->d_own);
  hipFree(t->d_stage);
  if (t->h_stage) hipHostFree(t->h_stage);
  for (hipEvent_t e : {t->ev[0], t->ev[1], t->ev_up, t->ev_switch})
    if (e) hipEventDestroy(e);
  if (t->own_stream) hipStreamDestroy(t->own_stream);
  delete t;
}

extern "C" mij_tensorizer *mij_tensorizer_create(int device, int max_frames) {
  mij_clear_error();
  if (max_frames < 1) {
    mij_fail(MIJ_EINVAL, "tensorizer_create: max_frames %d", max_frames);
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    mij_fail(MIJ_ENODEV, "no HIP device %d (the HIP path has no CPU fallback)", device);
    return nullptr;
  }
  auto *t = new mij_tensorizer();
  t->dev = device;
  t->cap = max_frames;
  t->jobs_bytes = round_to((size_t)max_frames * sizeof(mij::TzJob), 256);
  auto init = [&]() -> int {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&t->own_stream, hipStreamNonBlocking));
    t->stream = t->own_stream;
    for (hipEvent_t &e : t->ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_up, hipEventDisableTiming));
    HIP_TRY(hipMalloc((void **)&t->d_stage, t->jobs_bytes + mij::TZ_LUT_BYTES));
    HIP_TRY(hipHostMalloc((void **)&t->h_stage, t->jobs_bytes + mij::TZ_LUT_BYTES));
    return MIJ_OK;
  };
  if (init()) {
    tensorizer_free(t);
    return nullptr;
  }
  return t;
}

extern "C" void mij_tensorizer_destroy(mij_tensorizer *t) { tensorizer_free(t); }

extern "C" void *mij_tensorizer_stream(mij_tensorizer *t) { return t ? (void *)t->stream : nullptr; }

extern "C" int mij_tensorizer_set_stream(mij_tensorizer *t, void *stream) {
  mij_clear_error();
  if (!t) return mij_fail(MIJ_EINVAL, "tensorizer_set_stream: null tensorizer");
  HIP_TRY(hipSetDevice(t->dev));
  const hipStream_t s = stream ? (hipStream_t)stream : t->own_stream;
  if (s == t->stream) return MIJ_OK;
  if (s != t->own_stream) {  // a caller's stream: it must belong to the tensorizer's device
    hipDevice_t sdev, tdev;
    if (hipStreamGetDevice(s, &sdev) != hipSuccess || hipDeviceGet(&tdev, t->dev) != hipSuccess || sdev != tdev)
      return mij_fail(MIJ_EINVAL, "tensorizer_set_stream: not a stream of the tensorizer's device %d", t->dev);
  }
  // the new stream runs after everything enqueued so far on the old one
  if (!t->ev_switch) HIP_TRY(hipEventCreateWithFlags(&t->ev_switch, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(t->ev_switch, t->stream));
  HIP_TRY(hipStreamWaitEvent(s, t->ev_switch, 0));
  t->stream = s;
  return MIJ_OK;
}

// Everything mij_tensorizer_run refuses, decided from the arguments alone and
// in the order include/mijpeg.h lists it; the object itself comes last, so a
// caller (and the suite, on a machine without a device) can ask with none.
static int tz_check_run(const char *what, const mij_tensorizer *t, const mij_image *src, int n, const mij_tensor_spec *spec,
                        const void *d_dst, size_t cap_bytes, size_t *need) {
  if (int rc = tz_check_spec(what, spec)) return rc;
  if (!src) return mij_fail(MIJ_EINVAL, "%s: null src", what);
  if (n < 1 || (t && n > t->cap)) {
    if (t) return mij_fail(MIJ_EINVAL, "%s: n %d (1..%d, the tensorizer's max_frames)", what, n, t->cap);
    return mij_fail(MIJ_EINVAL, "%s: n %d (1..max_frames)", what, n);
  }
  for (int i = 0; i < n; i++) {
    const mij_image &s = src[i];
    if (!s.px) return mij_fail(MIJ_EINVAL, "%s: frame %d: src.px is null", what, i);
    if (!tz_side(s.w) || !tz_side(s.h))
      return mij_fail(MIJ_EINVAL, "%s: frame %d: src is %dx%d (1..65535 each)", what, i, s.w, s.h);
    if (s.pitch < 3LL * s.w)
      return mij_fail(MIJ_EINVAL, "%s: frame %d: src.pitch %lld under 3*%d bytes", what, i, s.pitch, s.w);
    if (s.w != src[0].w || s.h != src[0].h)
      return mij_fail(MIJ_EINVAL, "%s: frame %d: src is %dx%d, frame 0 %dx%d (the frames of a call have one size)", what, i,
                      s.w, s.h, src[0].w, src[0].h);
  }
  *need = mij_tensor_bytes(n, src[0].w, src[0].h, spec->dtype);
  const long long tiles = (long long)((src[0].w + mij::TZ_SEG - 1) / mij::TZ_SEG) * ((src[0].h + mij::TZ_ROWS - 1) / mij::TZ_ROWS);
  if (!*need || tiles * n > 0x7FFFFFFFLL)
    return mij_fail(MIJ_EINVAL, "%s: n %d frames of %dx%d make more than 2^31 tiles in one call", what, n, src[0].w, src[0].h);
  if (int rc = tz_check_dst(what, d_dst, cap_bytes, *need)) return rc;
  if (!t) return mij_fail(MIJ_EINVAL, "%s: null tensorizer", what);
  return MIJ_OK;
}

// the checked run: the caller has been through tz_check_run
static int tz_run(mij_tensorizer *t, const mij_image *src, const uint8_t *mirror, int n, const mij_tensor_spec *spec,
                  void *d_dst, size_t need) {
  const int w = src[0].w, h = src[0].h;
  HIP_TRY(hipSetDevice(t->dev));
  HIP_TRY(hipEventSynchronize(t->ev_up));  // the last call's upload has left the staging buffer
  uint8_t *dst = (uint8_t *)d_dst;
  if (!dst) {
    if (need > t->own_cap) {  // the result moves; the stream may still use the old buffer
      t->own_valid = false;
      HIP_TRY(hipStreamSynchronize(t->stream));
      hipFree(t->d_own);
      t->d_own = nullptr;
      t->own_cap = 0;
      const size_t cap = need + need / 4 + 4096;
      HIP_TRY(hipMalloc((void **)&t->d_own, cap));
      t->own_cap = cap;
    }
    dst = t->d_own;
    t->own_valid = false;
  }
  mij::TzJob *jobs = (mij::TzJob *)t->h_stage;
  for (int i = 0; i < n; i++) jobs[i] = {(const uint8_t *)src[i].px, src[i].pitch, mirror && mirror[i] ? 1 : 0, 0};
  const int es = mij::tz_esize(spec->dtype);
  mij::tz_build_lut(spec->dtype, spec->mean, spec->std, t->h_stage + t->jobs_bytes);
  const size_t lut_bytes = (size_t)3 * 256 * es;
  HIP_TRY(hipMemcpyAsync(t->d_stage, t->h_stage, t->jobs_bytes + lut_bytes, hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipEventRecord(t->ev_up, t->stream));
  const mij::TzJob *d_jobs = (const mij::TzJob *)t->d_stage;
  const uint32_t *d_lut = (const uint32_t *)(t->d_stage + t->jobs_bytes);
  const int tiles_x = (w + mij::TZ_SEG - 1) / mij::TZ_SEG, tiles_y = (h + mij::TZ_ROWS - 1) / mij::TZ_ROWS;
  const dim3 grid((unsigned)((long long)n * tiles_x * tiles_y));
  t->ran = false;
  HIP_TRY(hipEventRecord(t->ev[0], t->stream));
#define TZ_LAUNCH(ES, NHWC)                                                                                       \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(mij::k_tensorize<ES, NHWC>), grid, dim3(256), 0, t->stream, d_jobs, d_lut, dst, w, \
                     h, tiles_x, tiles_y, spec->swap)
  const bool nhwc = spec->layout == MIJ_T_NHWC;
  if (es == 1) {
    if (nhwc) TZ_LAUNCH(1, true);
    else TZ_LAUNCH(1, false);
  } else if (es == 2) {
    if (nhwc) TZ_LAUNCH(2, true);
    else TZ_LAUNCH(2, false);
  } else {
    if (nhwc) TZ_LAUNCH(4, true);
    else TZ_LAUNCH(4, false);
  }
#undef TZ_LAUNCH
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(t->ev[1], t->stream));
  t->ran = true;
  if (!d_dst) {
    t->own_bytes = need;
    t->own_valid = true;
  }
  return MIJ_OK;
}

extern "C" int mij_tensorizer_run(mij_tensorizer *t, const mij_image *src, const uint8_t *mirror, int n,
                                  const mij_tensor_spec *spec, void *d_dst, size_t cap_bytes) {
  mij_clear_error();
  size_t need = 0;
  if (int rc = tz_check_run("tensorizer_run", t, src, n, spec, d_dst, cap_bytes, &need)) return rc;
  return tz_run(t, src, mirror, n, spec, d_dst, need);
}

extern "C" void *mij_tensorizer_device(mij_tensorizer *t, size_t *bytes) {
  mij_clear_error();
  if (bytes) *bytes = 0;
  if (!t) {
    mij_fail(MIJ_EINVAL, "tensorizer_device: null tensorizer");
    return nullptr;
  }
  if (!t->own_valid) {
    mij_fail(MIJ_EINVAL, "tensorizer_device: no mij_tensorizer_run into the tensorizer's own buffer before it");
    return nullptr;
  }
  if (bytes) *bytes = t->own_bytes;
  return t->d_own;
}

extern "C" int mij_tensorizer_read(mij_tensorizer *t, void *dst, size_t cap) {
  mij_clear_error();
  if (!t) return mij_fail(MIJ_EINVAL, "tensorizer_read: null tensorizer");
  if (!t->own_valid)
    return mij_fail(MIJ_EINVAL, "tensorizer_read: no mij_tensorizer_run into the tensorizer's own buffer before it");
  if (cap < t->own_bytes) return mij_fail(MIJ_ENOSPC, "tensorizer_read: need %zu bytes", t->own_bytes);
  if (!dst) return mij_fail(MIJ_EINVAL, "tensorizer_read: dst is NULL");
  HIP_TRY(hipSetDevice(t->dev));
  HIP_TRY(hipMemcpyAsync(dst, t->d_own, t->own_bytes, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  return MIJ_OK;
}

extern "C" int mij_tensorizer_ms(mij_tensorizer *t, float *ms) {
  mij_clear_error();
  if (!t || !ms) return mij_fail(MIJ_EINVAL, "tensorizer_ms: bad args");
  if (!t->ran) return mij_fail(MIJ_EINVAL, "tensorizer_ms: no mij_tensorizer_run before it");
  HIP_TRY(hipSetDevice(t->dev));
  HIP_TRY(hipEventSynchronize(t->ev[1]));
  HIP_TRY(hipEventElapsedTime(ms, t->ev[0], t->ev[1]));
  return MIJ_OK;
}

// ---------------------------------------------------------------------------
// the chain: stored JPEGs to one tensor
// ---------------------------------------------------------------------------
struct mij_loader {
  int dev = 0, max_w = 0, max_h = 0, cap = 0;
  mij_decoder *d = nullptr;
  mij_resizer *r = nullptr;
  mij_tensorizer *t = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};  // around the entropy decode
  int denom = 0;                          // of the last load
  bool valid = false;
};

static void loader_free(mij_loader *l) {
  if (!l) return;
  // the borrowers of the decoder's stream first; each waits for what it enqueued there
  mij_tensorizer_destroy(l->t);
  mij_resizer_destroy(l->r);
  if (l->d) hipSetDevice(l->dev);
  for (hipEvent_t e : l->ev)
    if (e) hipEventDestroy(e);
  mij_decoder_destroy(l->d);
  delete l;
}

extern "C" mij_loader *mij_loader_create(int device, int max_w, int max_h, int max_frames) {
  mij_clear_error();
  if (!tz_side(max_w) || !tz_side(max_h) || max_frames < 1) {
    mij_fail(MIJ_EINVAL, "loader_create: max size %dx%d (1..65535 each), max_frames %d", max_w, max_h, max_frames);
    return nullptr;
  }
  auto *l = new mij_loader();
  l->dev = device;
  l->max_w = max_w;
  l->max_h = max_h;
  l->cap = max_frames;
  auto init = [&]() -> int {
    if (!(l->d = mij_decoder_create(device, (max_w + 15) / 16 * 16, (max_h + 15) / 16 * 16, max_frames))) return mij_last_error();
    if (!(l->r = mij_resizer_create(device, max_frames))) return mij_last_error();
    if (!(l->t = mij_tensorizer_create(device, max_frames))) return mij_last_error();
    // one stream for every stage: the decoder's
    if (int rc = mij_resizer_set_stream(l->r, mij_decoder_stream(l->d))) return rc;
    if (int rc = mij_tensorizer_set_stream(l->t, mij_decoder_stream(l->d))) return rc;
    HIP_TRY(hipSetDevice(device));
    for (hipEvent_t &e : l->ev) HIP_TRY(hipEventCreate(&e));
    return MIJ_OK;
  };
  if (init()) {
    loader_free(l);  // (leaves the failure's message in place)
    return nullptr;
  }
  return l;
}

extern "C" void mij_loader_destroy(mij_loader *l) { loader_free(l); }

extern "C" void *mij_loader_stream(mij_loader *l) { return l ? mij_decoder_stream(l->d) : nullptr; }

extern "C" int mij_loader_accept(mij_loader *l, unsigned mask) {
  mij_clear_error();
  if (!l) return mij_fail(MIJ_EINVAL, "loader_accept: null loader");
  return mij_decoder_accept(l->d, mask);
}

extern "C" int mij_loader_denom(mij_loader *l) { return l && l->valid ? l->denom : 0; }

extern "C" int mij_loader_load(mij_loader *l, const uint8_t *const *jpgs, const size_t *lens, int n, const area_t *crops,
                               const uint8_t *mirror, int out_w, int out_h, int filter, int denom, int order,
                               const mij_tensor_spec *spec, void *d_dst, size_t cap_bytes) {
  mij_clear_error();
  const char *what = "loader_load";
  // the arguments, then the streams' headers, then the loader itself: nothing below needs a device
  if (int rc = tz_check_spec(what, spec)) return rc;
  if (!jpgs || !lens) return mij_fail(MIJ_EINVAL, "%s: null %s", what, !jpgs ? "jpgs" : "lens");
  if (n < 1 || (l && n > l->cap)) {
    if (l) return mij_fail(MIJ_EINVAL, "%s: n %d (1..%d, the loader's max_frames)", what, n, l->cap);
    return mij_fail(MIJ_EINVAL, "%s: n %d (1..max_frames)", what, n);
  }
  if (!tz_side(out_w) || !tz_side(out_h))
    return mij_fail(MIJ_EINVAL, "%s: out size %dx%d (1..65535 each)", what, out_w, out_h);
  if (filter < 0 || filter >= mij::RS_FILTERS)
    return mij_fail(MIJ_EINVAL, "%s: filter %d (MIJ_RS_BOX, MIJ_RS_BILINEAR or MIJ_RS_BICUBIC)", what, filter);
  if (denom != 0 && denom != 1 && denom != 2 && denom != 4 && denom != 8)
    return mij_fail(MIJ_EINVAL, "%s: denom %d (1, 2, 4, 8, or 0: chosen from the sizes)", what, denom);
  if (order != MIJ_PIX_BGR && order != MIJ_PIX_RGB) return mij_fail(MIJ_EINVAL, "%s: pixel order %d", what, order);
  std::vector<area_t> rect(n);  // the crops in full-size pixels
  int d_auto = 8;
  for (int i = 0; i < n; i++) {
    if (!jpgs[i]) return mij_fail(MIJ_EINVAL, "%s: frame %d: stream is NULL", what, i);
    // the headers: what mij_decode refuses is refused here, with its code and message
    int w = 0, h = 0;
    if (int rc = mij_parse_size_accept(what, jpgs[i], lens[i], i, l ? mij_decoder_accepted(l->d) : 0, &w, &h)) return rc;
    if (l && (w > l->max_w || h > l->max_h))
      return mij_fail(MIJ_EINVAL, "%s: frame %d: %dx%d exceeds the loader's %dx%d", what, i, w, h, l->max_w, l->max_h);
    area_t a = {0, 0, w, h};
    if (crops) {
      a = crops[i];
      if (a.w < 1 || a.h < 1 || a.x < 0 || a.y < 0 || (long long)a.x + a.w > w || (long long)a.y + a.h > h)
        return mij_fail(MIJ_EINVAL, "%s: frame %d: crop %dx%d at (%d, %d) is empty or outside the %dx%d frame", what, i,
                        a.w, a.h, a.x, a.y, w, h);
    }
    rect[i] = a;
    d_auto = std::min(d_auto, mij_thumbnail_denom(a.w, a.h, out_w, out_h));
  }
  const int dn = denom ? denom : d_auto;
  const size_t need = mij_tensor_bytes(n, out_w, out_h, spec->dtype);
  const long long tiles = (long long)((out_w + mij::TZ_SEG - 1) / mij::TZ_SEG) * ((out_h + mij::TZ_ROWS - 1) / mij::TZ_ROWS);
  if (!need || tiles * n > 0x7FFFFFFFLL)
    return mij_fail(MIJ_EINVAL, "%s: n %d frames of %dx%d make more than 2^31 tiles in one call", what, n, out_w, out_h);
  if (int rc = tz_check_dst(what, d_dst, cap_bytes, need)) return rc;
  if (!l) return mij_fail(MIJ_EINVAL, "%s: null loader", what);

  HIP_TRY(hipSetDevice(l->dev));
  const hipStream_t stream = (hipStream_t)mij_decoder_stream(l->d);
  l->valid = false;
  HIP_TRY(hipEventRecord(l->ev[0], stream));
  if (int rc = mij_decoder_decode(l->d, jpgs, lens, n)) return rc;
  HIP_TRY(hipEventRecord(l->ev[1], stream));
  if (int rc = mij_decoder_reconstruct_scaled(l->d, order, dn)) return rc;
  // the crop's rectangle of the scaled image: every scaled pixel that holds a sample of it
  std::vector<mij_image> im(n);
  std::vector<int> wh(2 * (size_t)n);
  for (int i = 0; i < n; i++) {
    const area_t &a = rect[i];
    const uint8_t *px = (const uint8_t *)mij_decoder_device_pixels(l->d, i, &im[i].pitch);
    if (!px) return mij_last_error();
    const int x0 = a.x / dn, y0 = a.y / dn, x1 = (a.x + a.w + dn - 1) / dn, y1 = (a.y + a.h + dn - 1) / dn;
    im[i].px = px + (long long)y0 * im[i].pitch + 3LL * x0;
    im[i].w = x1 - x0;
    im[i].h = y1 - y0;
    wh[2 * i] = out_w;
    wh[2 * i + 1] = out_h;
  }
  if (int rc = mij_resizer_resize(l->r, im.data(), wh.data(), n, filter)) return rc;
  for (int i = 0; i < n; i++) {
    if (!(im[i].px = mij_resizer_device_pixels(l->r, i, &im[i].pitch))) return mij_last_error();
    im[i].w = out_w;
    im[i].h = out_h;
  }
  size_t need_t = 0;
  if (int rc = tz_check_run(what, l->t, im.data(), n, spec, d_dst, cap_bytes, &need_t)) return rc;
  if (int rc = tz_run(l->t, im.data(), mirror, n, spec, d_dst, need_t)) return rc;
  l->denom = dn;
  l->valid = true;
  return MIJ_OK;
}

extern "C" void *mij_loader_device(mij_loader *l, size_t *bytes) {
  if (!l) {
    mij_clear_error();
    if (bytes) *bytes = 0;
    mij_fail(MIJ_EINVAL, "loader_device: null loader");
    return nullptr;
  }
  return mij_tensorizer_device(l->t, bytes);
}

extern "C" int mij_loader_read(mij_loader *l, void *dst, size_t cap) {
  if (!l) {
    mij_clear_error();
    return mij_fail(MIJ_EINVAL, "loader_read: null loader");
  }
  return mij_tensorizer_read(l->t, dst, cap);
}

extern "C" int mij_loader_ms(mij_loader *l, float ms[4]) {
  mij_clear_error();
  if (!l || !ms) return mij_fail(MIJ_EINVAL, "loader_ms: bad args");
  if (!l->valid) return mij_fail(MIJ_EINVAL, "loader_ms: no mij_loader_load before it");
  float rec[2], rs[2];
  if (int rc = mij_tensorizer_ms(l->t, &ms[3])) return rc;  // waits for the whole chain
  if (int rc = mij_decoder_reconstruct_ms(l->d, rec)) return rc;
  if (int rc = mij_resizer_ms(l->r, rs)) return rc;
  HIP_TRY(hipSetDevice(l->dev));
  HIP_TRY(hipEventElapsedTime(&ms[0], l->ev[0], l->ev[1]));
  ms[1] = rec[0] + rec[1];
  ms[2] = rs[0] + rs[1];
  return MIJ_OK;
}
