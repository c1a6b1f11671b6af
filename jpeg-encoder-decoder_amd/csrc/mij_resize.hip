// mij_resize.hip -- the separable resampler for 3-byte interleaved 8-bit
// pixels: Pillow's Image.resize for BOX, BILINEAR and
// BICUBIC, byte for byte (the arithmetic: mij_resize.h), as two gfx950
// kernels, each one launch over every frame of a call, and the C API around
// them (mij_resizer_*, mij_resize, mij_thumbnail).
//
//   k_rs_h   horizontal pass.  A workgroup owns RS_TX output pixels of RS_TY
//            rows, one row per wave, one output pixel per lane.  The bytes
//            under the tile's windows come into LDS as they lie in memory,
//            in whole aligned 16-byte lines (the source has any alignment;
//            at a span's two ends only the aligned dwords that hold its
//            bytes are read), RS_CH pixels at a time, and are spread there
//            to one dword per pixel; the tile's weights (one contiguous
//            piece of the table) are staged beside them when they fit, else
//            read from the table.  A lane then walks its window: one LDS
//            dword and three multiply-adds per tap.  A workgroup takes up to
//            RS_RG such tiles one below the other.
//   k_rs_v   vertical pass, and the copy of a frame that needs no pass.  A
//            workgroup owns 256 bytes of RS_TY output rows, one row per
//            wave; a lane owns 4 consecutive bytes and walks the window's
//            rows, so every load is a coalesced dword per lane (re-aligned
//            when the source is a caller's image) and the weights are
//            uniform per wave.
//
// A frame with both passes goes source -> intermediate (in_h rows of out_w
// pixels, the resizer's own buffer) -> output; with one pass straight from
// the source to the output.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "mij_host.h"
#include "mij_resize.h"

#define HIP_TRY(x)                                                                 \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess)                                                          \
      return mij_fail(MIJ_EHIP, "%s failed: %s", #x, hipGetErrorString(e_));       \
  } while (0)

namespace mij {

constexpr int RS_TX = 64;     // output pixels of a k_rs_h tile (one per lane)
constexpr int RS_TY = 4;      // rows of a tile (one per wave), both kernels
constexpr int RS_RG = 8;      // k_rs_h: tiles one below the other a workgroup takes at most
constexpr int RS_CH = 768;    // source pixels of a row staged at a time
constexpr int RS_RAW = 3 * RS_CH / 16 + 2;  // 16-byte lines that hold them, wherever the first begins
constexpr int RS_WCAP = 4096; // weights staged per tile (RS_TX rows of ksize <= 64)
constexpr int RS_VB = 256;    // bytes of a row a k_rs_v tile covers (4 per lane)

// One pass over one frame.  Bounds: every index below comes from sizes the
// host checked (1..65535 a side, pitch >= 3 * width) and from the axis table
// the host built (rs_build_axis: 0 <= xmin, xmin + count <= in_n, count <=
// ksize), none from pixel data.  Reads of the source stay inside aligned
// dwords that hold at least one byte of the row being read (the contract
// mij_batch_pad_input documents); stores go to the resizer's own buffers,
// whose rows are 3 * width rounded up to 16 bytes apart, and stay inside a
// row's pitch.
struct RsJob {
  const uint8_t *src;
  uint8_t *dst;
  long long spitch, dpitch;
  int in_n, out_n;   // the axis: source and output extent (pixels for k_rs_h, rows for k_rs_v)
  int other;         // the other axis: rows (k_rs_h), bytes of a row (k_rs_v)
  int tab;           // the axis table's first int32 in the table buffer; -1: copy (k_rs_v)
  int ksize;
  int wg0;           // the job's first workgroup in the kernel's grid
  int tiles_x;       // tiles across
  int rg;            // k_rs_h: groups of RS_TY rows a workgroup takes, one after the other
};

// the job a workgroup belongs to: the last whose wg0 <= wg (as the k_dec_* kernels find theirs)
__device__ __forceinline__ int rs_job_of(const RsJob *jobs, int n, int wg) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].wg0 <= wg) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The jobs' pointers come out of a table in memory, where the compiler takes them for generic ones and
// would use flat loads and stores (which also wait on the LDS counter); they are global memory.
#define RS_GLOBAL __attribute__((address_space(1)))
typedef RS_GLOBAL const uint32_t *rs_gu32;
typedef uint32_t rs_u32x4 __attribute__((ext_vector_type(4)));

// The aligned 16-byte line at address c, of which only the aligned dwords that
// hold a byte of [start, end) are read: one 16-byte load inside a row's span,
// dword loads at its two ends.  The others are 0.
__device__ __forceinline__ uint4 rs_load_line(uintptr_t c, uintptr_t start, uintptr_t end) {
  if (c >= (start & ~(uintptr_t)3) && c + 16 <= ((end + 3) & ~(uintptr_t)3)) {
    const rs_u32x4 v = *(RS_GLOBAL const rs_u32x4 *)c;
    return make_uint4(v.x, v.y, v.z, v.w);
  }
  uint32_t v[4];
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = c + 4 * j + 4 > start && c + 4 * j < end ? *(rs_gu32)(c + 4 * j) : 0u;
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// 4 bytes from byte b of a row of nb bytes that starts at any address; bytes
// past the row's end read as 0 and the dword that would hold only such bytes
// is not touched
__device__ __forceinline__ uint32_t rs_load_dword(const uint8_t *row, int b, int nb) {
  const uint8_t *a = row + b;
  const uint32_t sh = (uint32_t)((uintptr_t)a & 3);
  const rs_gu32 w = (rs_gu32)(a - sh);
  const uint32_t lo = w[0];
  const uint32_t hi = sh && b + 4 - (int)sh < nb ? w[1] : 0u;
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

// a lane's taps inside the staged piece [c0, c1); wrow is its row of weights, in LDS or in the table
__device__ __forceinline__ void rs_h_taps(const uint32_t *px, const int32_t *wrow, int k0, int k1, int c0, int xmin,
                                          int32_t acc[3]) {
#pragma unroll 4
  for (int k = k0; k < k1; k++) {
    const uint32_t v = px[k - c0];
    const int32_t w = wrow[k - xmin];
    acc[0] = rs_tap(acc[0], v & 255u, w);
    acc[1] = rs_tap(acc[1], (v >> 8) & 255u, w);
    acc[2] = rs_tap(acc[2], v >> 16, w);
  }
}

__global__ __launch_bounds__(256) void k_rs_h(const RsJob *jobs, int njobs, const int32_t *tabs) {
  __shared__ uint32_t s_px[RS_TY][RS_CH];
  __shared__ uint4 s_raw[RS_TY][RS_RAW];
  __shared__ int32_t s_w[RS_WCAP];
  const RsJob J = jobs[rs_job_of(jobs, njobs, blockIdx.x)];
  const int tile = (int)blockIdx.x - J.wg0;
  const int ty = tile / J.tiles_x, tx = tile - ty * J.tiles_x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x0 = tx * RS_TX, nx = min(RS_TX, J.out_n - x0);  // nx >= 1: tiles_x = ceil(out_n / RS_TX)
  const int32_t *bounds = tabs + J.tab, *wt = bounds + 2LL * J.out_n;
  // the tile's span of source pixels: xmin and xmin + count never decrease with the output index
  const int span0 = bounds[2 * x0], xl = x0 + nx - 1, span1 = bounds[2 * xl] + bounds[2 * xl + 1];
  const int x = x0 + min(lane, nx - 1);
  const int xmin = bounds[2 * x], xend = xmin + bounds[2 * x + 1];
  const bool wlds = nx * J.ksize <= RS_WCAP;  // uniform
  if (wlds) {
    const int32_t *wsrc = wt + (long long)x0 * J.ksize;
    for (int i = threadIdx.x; i < nx * J.ksize; i += 256) s_w[i] = wsrc[i];
  }
  // J.rg groups of RS_TY rows, one after the other: the job, the bounds and the weights are fetched once
  for (int g = 0; g < J.rg; g++) {
    const int yg = (ty * J.rg + g) * RS_TY;
    if (yg >= J.other) break;  // uniform over the workgroup
    const int y = yg + wave;
    const bool row_live = y < J.other, live = row_live && lane < nx;
    const uint8_t *srow = J.src + (long long)min(y, J.other - 1) * J.spitch;
    int32_t acc[3] = {RS_ACC0, RS_ACC0, RS_ACC0};
    for (int c0 = span0; c0 < span1; c0 += RS_CH) {  // uniform over the workgroup
      const int c1 = min(c0 + RS_CH, span1);
      __syncthreads();  // the previous piece is consumed (and, the first time, the weights are staged)
      // the piece's bytes as they lie in memory, in whole aligned 16-byte lines (c1 <= in_n)
      const uintptr_t start = (uintptr_t)srow + 3ull * c0, end = (uintptr_t)srow + 3ull * c1;
      const uintptr_t line0 = start & ~(uintptr_t)15;
      const int nlines = (int)((end - line0 + 15) >> 4);  // <= RS_RAW: 3 * RS_CH bytes, begun up to 15 bytes into a line
      if (row_live)
        for (int i = lane; i < nlines; i += 64) s_raw[wave][i] = rs_load_line(line0 + 16ull * i, start, end);
      __syncthreads();
      // one dword per pixel, 0x00c2c1c0, from the two dwords around its 3 bytes (the second may lie past the
      // piece, inside s_raw: its bytes are masked off)
      const uint32_t *raw = (const uint32_t *)s_raw[wave];
      for (int p = c0 + lane; row_live && p < c1; p += 64) {
        const uint32_t o = (uint32_t)(start - line0) + 3u * (uint32_t)(p - c0);
        s_px[wave][p - c0] = __builtin_amdgcn_alignbyte(raw[(o >> 2) + 1], raw[o >> 2], o & 3u) & 0xFFFFFFu;
      }
      __syncthreads();
      const int k0 = max(xmin, c0), k1 = min(xend, c1);
      if (live) {
        if (wlds) rs_h_taps(s_px[wave], s_w + (x - x0) * J.ksize, k0, k1, c0, xmin, acc);
        else rs_h_taps(s_px[wave], wt + (long long)x * J.ksize, k0, k1, c0, xmin, acc);
      }
    }
    if (live) {
      RS_GLOBAL uint8_t *d = (RS_GLOBAL uint8_t *)(J.dst + (long long)y * J.dpitch + 3LL * x);
      d[0] = (uint8_t)rs_clip(acc[0]);
      d[1] = (uint8_t)rs_clip(acc[1]);
      d[2] = (uint8_t)rs_clip(acc[2]);
    }
  }
}

__global__ __launch_bounds__(256) void k_rs_v(const RsJob *jobs, int njobs, const int32_t *tabs) {
  const RsJob J = jobs[rs_job_of(jobs, njobs, blockIdx.x)];
  const int tile = (int)blockIdx.x - J.wg0;
  const int ty = tile / J.tiles_x, tx = tile - ty * J.tiles_x;
  const int y = ty * RS_TY + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // uniform per wave
  const int b = tx * RS_VB + 4 * (int)(threadIdx.x & 63), nb = J.other;
  if (y >= J.out_n || b >= nb) return;
  RS_GLOBAL uint32_t *d = (RS_GLOBAL uint32_t *)(J.dst + (long long)y * J.dpitch + b);  // dword-aligned; b + 4 <= the pitch
  if (J.tab < 0) {  // no pass: the frame is copied
    *d = rs_load_dword(J.src + (long long)y * J.spitch, b, nb);
    return;
  }
  const int32_t *bounds = tabs + J.tab;
  const int ymin = bounds[2 * y], n = bounds[2 * y + 1];  // ymin + n <= in_n
  const int32_t *w = bounds + 2LL * J.out_n + (long long)y * J.ksize;
  const uint8_t *s = J.src + (long long)ymin * J.spitch;
  int32_t acc[4] = {RS_ACC0, RS_ACC0, RS_ACC0, RS_ACC0};
#pragma unroll 4
  for (int k = 0; k < n; k++) {
    const uint32_t v = rs_load_dword(s + (long long)k * J.spitch, b, nb);
    const int32_t wk = w[k];
    acc[0] = rs_tap(acc[0], v & 255u, wk);
    acc[1] = rs_tap(acc[1], (v >> 8) & 255u, wk);
    acc[2] = rs_tap(acc[2], (v >> 16) & 255u, wk);
    acc[3] = rs_tap(acc[3], v >> 24, wk);
  }
  *d = rs_clip(acc[0]) | (rs_clip(acc[1]) << 8) | (rs_clip(acc[2]) << 16) | (rs_clip(acc[3]) << 24);
}

}  // namespace mij

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
namespace {

long long round_to(long long v, long long m) { return (v + m - 1) / m * m; }
long long rs_pitch(int w) { return round_to(3LL * w, 16); }
bool rs_side(int v) { return v >= 1 && v <= mij::RS_MAX_SIDE; }

struct RsFrame {
  int w = 0, h = 0;
  long long pitch = 0, off = 0;  // in the output buffer
};

}  // namespace

struct mij_resizer {
  int dev = 0, cap = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // before the horizontal launch, between, after the vertical
  hipEvent_t ev_up = nullptr;                      // the staging buffer's upload is done
  hipEvent_t ev_switch = nullptr;
  uint8_t *d_mid = nullptr, *d_out = nullptr;      // the intermediates; the results
  size_t mid_cap = 0, out_cap = 0;
  uint8_t *h_stage = nullptr, *d_stage = nullptr;  // both job tables, then the axis tables: one copy per call
  size_t stage_cap = 0;
  std::vector<RsFrame> frames;                     // of the last resize
  std::vector<double> k;                           // rs_build_axis' scratch
  bool valid = false;
};

static void resizer_free(mij_resizer *r) {
  if (!r) return;
  hipSetDevice(r->dev);
  if (r->stream) hipStreamSynchronize(r->stream);
  if (r->own_stream && r->own_stream != r->stream) hipStreamSynchronize(r->own_stream);
  hipFree(r->d_mid);
  hipFree(r->d_out);
  hipFree(r->d_stage);
  if (r->h_stage) hipHostFree(r->h_stage);
  for (hipEvent_t e : {r->ev[0], r->ev[1], r->ev[2], r->ev_up, r->ev_switch})
    if (e) hipEventDestroy(e);
  if (r->own_stream) hipStreamDestroy(r->own_stream);
  delete r;
}

extern "C" mij_resizer *mij_resizer_create(int device, int max_frames) {
  mij_clear_error();
  if (max_frames < 1) {
    mij_fail(MIJ_EINVAL, "resizer_create: max_frames %d", max_frames);
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    mij_fail(MIJ_ENODEV, "no HIP device %d (the HIP path has no CPU fallback)", device);
    return nullptr;
  }
  auto *r = new mij_resizer();
  r->dev = device;
  r->cap = max_frames;
  auto init = [&]() -> int {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&r->own_stream, hipStreamNonBlocking));
    r->stream = r->own_stream;
    for (hipEvent_t &e : r->ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventCreateWithFlags(&r->ev_up, hipEventDisableTiming));
    return MIJ_OK;
  };
  if (init()) {
    resizer_free(r);
    return nullptr;
  }
  return r;
}

extern "C" void mij_resizer_destroy(mij_resizer *r) { resizer_free(r); }

extern "C" void *mij_resizer_stream(mij_resizer *r) { return r ? (void *)r->stream : nullptr; }

extern "C" int mij_resizer_set_stream(mij_resizer *r, void *stream) {
  mij_clear_error();
  if (!r) return mij_fail(MIJ_EINVAL, "resizer_set_stream: null resizer");
  HIP_TRY(hipSetDevice(r->dev));
  const hipStream_t s = stream ? (hipStream_t)stream : r->own_stream;
  if (s == r->stream) return MIJ_OK;
  if (s != r->own_stream) {  // a caller's stream: it must belong to the resizer's device
    hipDevice_t sdev, rdev;
    if (hipStreamGetDevice(s, &sdev) != hipSuccess || hipDeviceGet(&rdev, r->dev) != hipSuccess || sdev != rdev)
      return mij_fail(MIJ_EINVAL, "resizer_set_stream: not a stream of the resizer's device %d", r->dev);
  }
  // the new stream runs after everything enqueued so far on the old one
  if (!r->ev_switch) HIP_TRY(hipEventCreateWithFlags(&r->ev_switch, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(r->ev_switch, r->stream));
  HIP_TRY(hipStreamWaitEvent(s, r->ev_switch, 0));
  r->stream = s;
  return MIJ_OK;
}

// frees and allocates again when `need` is more than the buffer holds (the
// stream is idle by then: its work may still use the old buffer)
static int rs_grow(mij_resizer *r, uint8_t *&p, size_t &cap, size_t need) {
  if (need <= cap) return MIJ_OK;
  HIP_TRY(hipStreamSynchronize(r->stream));
  hipFree(p);
  p = nullptr;
  cap = 0;
  need += need / 4 + 4096;
  HIP_TRY(hipMalloc((void **)&p, need));
  cap = need;
  return MIJ_OK;
}

static int rs_check_filter(const char *what, int filter) {
  if (filter < 0 || filter >= mij::RS_FILTERS)
    return mij_fail(MIJ_EINVAL, "%s: filter %d (MIJ_RS_BOX, MIJ_RS_BILINEAR or MIJ_RS_BICUBIC)", what, filter);
  return MIJ_OK;
}

extern "C" int mij_resizer_resize(mij_resizer *r, const mij_image *src, const int *out_wh, int n, int filter) {
  mij_clear_error();
  if (!r) return mij_fail(MIJ_EINVAL, "resizer_resize: null resizer");
  if (!src || !out_wh) return mij_fail(MIJ_EINVAL, "resizer_resize: null %s", !src ? "src" : "out_wh");
  if (n < 1 || n > r->cap) return mij_fail(MIJ_EINVAL, "resizer_resize: n %d (1..%d, the resizer's max_frames)", n, r->cap);
  if (rs_check_filter("resizer_resize", filter)) return MIJ_EINVAL;
  for (int i = 0; i < n; i++) {
    const mij_image &s = src[i];
    if (!s.px) return mij_fail(MIJ_EINVAL, "resizer_resize: frame %d: src.px is null", i);
    if (!rs_side(s.w) || !rs_side(s.h))
      return mij_fail(MIJ_EINVAL, "resizer_resize: frame %d: src is %dx%d (1..65535 each)", i, s.w, s.h);
    if (s.pitch < 3LL * s.w)
      return mij_fail(MIJ_EINVAL, "resizer_resize: frame %d: src.pitch %lld under 3*%d bytes", i, s.pitch, s.w);
    if (!rs_side(out_wh[2 * i]) || !rs_side(out_wh[2 * i + 1]))
      return mij_fail(MIJ_EINVAL, "resizer_resize: frame %d: out_wh is %dx%d (1..65535 each)", i, out_wh[2 * i],
                      out_wh[2 * i + 1]);
  }
  // the plan: per-frame buffers, the axis tables (shared by equal axes), the jobs of each kernel
  using mij::RsJob;
  std::vector<RsFrame> frames(n);
  std::vector<RsJob> hj, vj;
  std::vector<int> hf, vf;  // their frames
  std::map<std::tuple<int, int>, long long> tab_of;  // (in, out) -> first word
  std::vector<std::tuple<int, int, long long>> tabs;
  long long tab_words = 0, mid_bytes = 0, out_bytes = 0, hwgs = 0, vwgs = 0;
  auto table = [&](int in, int out) {
    auto it = tab_of.find({in, out});
    if (it != tab_of.end()) return it->second;
    const long long at = tab_words;
    tab_of[{in, out}] = at;
    tabs.push_back({in, out, at});
    tab_words += mij::rs_table_words(in, out, filter);
    return at;
  };
  auto h_tiles = [](const RsJob &j) { return (long long)j.tiles_x * ((j.other + mij::RS_TY * j.rg - 1) / (mij::RS_TY * j.rg)); };
  std::vector<long long> mid_off(n, -1);
  for (int i = 0; i < n; i++) {
    const mij_image &s = src[i];
    RsFrame &F = frames[i];
    F.w = out_wh[2 * i];
    F.h = out_wh[2 * i + 1];
    F.pitch = rs_pitch(F.w);
    F.off = out_bytes;
    out_bytes += round_to(F.pitch * F.h, 256);
    const bool hp = F.w != s.w, vp = F.h != s.h;
    if (hp && vp) {
      mid_off[i] = mid_bytes;
      mid_bytes += round_to(F.pitch * s.h, 256);
    }
    if (hp) {
      RsJob j;
      memset(&j, 0, sizeof j);
      j.in_n = s.w;
      j.out_n = F.w;
      j.other = s.h;
      j.ksize = mij::rs_ksize(s.w, F.w, filter);
      j.tiles_x = (F.w + mij::RS_TX - 1) / mij::RS_TX;
      // a workgroup takes up to RS_RG tiles one below the other (the job, bounds and weights fetched once for
      // all of them), a frame's column of tiles still making 32 workgroups or more
      j.rg = std::max(1, std::min(mij::RS_RG, s.h / (32 * mij::RS_TY)));
      table(s.w, F.w);
      hwgs += h_tiles(j);
      hj.push_back(j);
      hf.push_back(i);
    }
    if (vp || !hp) {  // (neither pass: k_rs_v copies the frame)
      RsJob j;
      memset(&j, 0, sizeof j);
      j.in_n = s.h;
      j.out_n = F.h;
      j.other = 3 * F.w;
      j.ksize = vp ? mij::rs_ksize(s.h, F.h, filter) : 0;
      j.tab = vp ? 0 : -1;
      j.tiles_x = (3 * F.w + mij::RS_VB - 1) / mij::RS_VB;
      if (vp) table(s.h, F.h);
      vwgs += (long long)j.tiles_x * ((F.h + mij::RS_TY - 1) / mij::RS_TY);
      vj.push_back(j);
      vf.push_back(i);
    }
  }
  if (hwgs > 0x7FFFFFFFLL || vwgs > 0x7FFFFFFFLL || tab_words > 0x7FFFFFFFLL)
    return mij_fail(MIJ_EINVAL, "resizer_resize: %d frames make more than 2^31 tiles or table words in one call", n);
  const size_t jobs_bytes = (size_t)round_to((long long)((hj.size() + vj.size()) * sizeof(RsJob)), 256);
  const size_t stage_bytes = jobs_bytes + (size_t)tab_words * 4;

  HIP_TRY(hipSetDevice(r->dev));
  if (r->ev_up) HIP_TRY(hipEventSynchronize(r->ev_up));  // the last call's upload has left the staging buffer
  if (stage_bytes > r->stage_cap) {
    HIP_TRY(hipStreamSynchronize(r->stream));
    hipFree(r->d_stage);
    if (r->h_stage) hipHostFree(r->h_stage);
    r->d_stage = r->h_stage = nullptr;
    r->stage_cap = 0;
    const size_t cap = stage_bytes + stage_bytes / 4 + 4096;
    HIP_TRY(hipMalloc((void **)&r->d_stage, cap));
    HIP_TRY(hipHostMalloc((void **)&r->h_stage, cap));
    r->stage_cap = cap;
  }
  if (rs_grow(r, r->d_mid, r->mid_cap, (size_t)mid_bytes)) return mij_last_error();
  if (out_bytes > (long long)r->out_cap) r->valid = false;  // the results move
  if (rs_grow(r, r->d_out, r->out_cap, (size_t)out_bytes)) return mij_last_error();

  int32_t *h_tabs = (int32_t *)(r->h_stage + jobs_bytes);
  for (const auto &[in, out, at] : tabs) {
    const int ks = mij::rs_ksize(in, out, filter);
    if ((int)r->k.size() < ks) r->k.resize(ks);
    if (!mij::rs_sum_fits(mij::rs_build_axis(in, out, filter, h_tabs + at, r->k.data())))
      return mij_fail(MIJ_EINVAL, "resizer_resize: the weights of %d -> %d leave int32 (DESIGN.md 4m)", in, out);
  }
  RsJob *h_jobs = (RsJob *)r->h_stage;
  long long wg = 0;
  for (size_t q = 0; q < hj.size(); q++) {
    RsJob &j = hj[q];
    const int i = hf[q];
    const bool vp = frames[i].h != src[i].h;
    j.src = (const uint8_t *)src[i].px;
    j.spitch = src[i].pitch;
    j.dst = vp ? r->d_mid + mid_off[i] : r->d_out + frames[i].off;
    j.dpitch = frames[i].pitch;
    j.tab = (int)tab_of[{j.in_n, j.out_n}];
    j.wg0 = (int)wg;
    wg += h_tiles(j);
  }
  wg = 0;
  for (size_t q = 0; q < vj.size(); q++) {
    RsJob &j = vj[q];
    const int i = vf[q];
    const bool hp = frames[i].w != src[i].w;
    j.src = hp ? r->d_mid + mid_off[i] : (const uint8_t *)src[i].px;
    j.spitch = hp ? frames[i].pitch : src[i].pitch;
    j.dst = r->d_out + frames[i].off;
    j.dpitch = frames[i].pitch;
    if (j.tab >= 0) j.tab = (int)tab_of[{j.in_n, j.out_n}];
    j.wg0 = (int)wg;
    wg += (long long)j.tiles_x * ((j.out_n + mij::RS_TY - 1) / mij::RS_TY);
  }
  if (!hj.empty()) memcpy(h_jobs, hj.data(), hj.size() * sizeof(RsJob));
  if (!vj.empty()) memcpy(h_jobs + hj.size(), vj.data(), vj.size() * sizeof(RsJob));
  HIP_TRY(hipMemcpyAsync(r->d_stage, r->h_stage, stage_bytes, hipMemcpyHostToDevice, r->stream));
  HIP_TRY(hipEventRecord(r->ev_up, r->stream));
  const RsJob *d_jobs = (const RsJob *)r->d_stage;
  const int32_t *d_tabs = (const int32_t *)(r->d_stage + jobs_bytes);
  r->valid = false;
  HIP_TRY(hipEventRecord(r->ev[0], r->stream));
  if (hwgs) {
    hipLaunchKernelGGL(mij::k_rs_h, dim3((unsigned)hwgs), dim3(256), 0, r->stream, d_jobs, (int)hj.size(), d_tabs);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(r->ev[1], r->stream));
  if (vwgs) {
    hipLaunchKernelGGL(mij::k_rs_v, dim3((unsigned)vwgs), dim3(256), 0, r->stream, d_jobs + hj.size(), (int)vj.size(),
                       d_tabs);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(r->ev[2], r->stream));
  r->frames = std::move(frames);
  r->valid = true;
  return MIJ_OK;
}

static int rs_frame(mij_resizer *r, int frame, const char *what) {
  if (!r) return mij_fail(MIJ_EINVAL, "%s: null resizer", what);
  if (!r->valid) return mij_fail(MIJ_EINVAL, "%s: no mij_resizer_resize before it", what);
  if (frame < 0 || frame >= (int)r->frames.size())
    return mij_fail(MIJ_EINVAL, "%s: frame %d of %d", what, frame, (int)r->frames.size());
  return MIJ_OK;
}

extern "C" void *mij_resizer_device_pixels(mij_resizer *r, int frame, long long *pitch) {
  mij_clear_error();
  if (rs_frame(r, frame, "resizer_device_pixels")) return nullptr;
  if (pitch) *pitch = r->frames[frame].pitch;
  return r->d_out + r->frames[frame].off;
}

extern "C" int mij_resizer_pixels(mij_resizer *r, int frame, uint8_t *dst, size_t cap, long long pitch) {
  mij_clear_error();
  if (int rc = rs_frame(r, frame, "resizer_pixels")) return rc;
  if (!dst) return mij_fail(MIJ_EINVAL, "resizer_pixels: dst is NULL");
  const RsFrame &F = r->frames[frame];
  const long long row = 3LL * F.w;
  if (pitch == 0) pitch = row;
  if (pitch < row) return mij_fail(MIJ_EINVAL, "resizer_pixels: pitch %lld < %lld", pitch, row);
  const unsigned long long need = (unsigned long long)(F.h - 1) * pitch + row;
  if (cap < need) return mij_fail(MIJ_ENOSPC, "resizer_pixels: need %llu bytes", need);
  HIP_TRY(hipSetDevice(r->dev));
  HIP_TRY(hipMemcpy2DAsync(dst, (size_t)pitch, r->d_out + F.off, (size_t)F.pitch, (size_t)row, F.h,
                           hipMemcpyDeviceToHost, r->stream));
  HIP_TRY(hipStreamSynchronize(r->stream));
  return MIJ_OK;
}

extern "C" int mij_resizer_ms(mij_resizer *r, float ms[2]) {
  mij_clear_error();
  if (!r || !ms) return mij_fail(MIJ_EINVAL, "resizer_ms: bad args");
  if (!r->valid) return mij_fail(MIJ_EINVAL, "resizer_ms: no mij_resizer_resize before it");
  HIP_TRY(hipSetDevice(r->dev));
  HIP_TRY(hipEventSynchronize(r->ev[2]));
  HIP_TRY(hipEventElapsedTime(&ms[0], r->ev[0], r->ev[1]));
  HIP_TRY(hipEventElapsedTime(&ms[1], r->ev[1], r->ev[2]));
  return MIJ_OK;
}

extern "C" int mij_resize(const uint8_t *px, int stride_px, int w, int h, int out_w, int out_h, int filter,
                          uint8_t *out, size_t cap) {
  mij_clear_error();
  if (rs_check_filter("mij_resize", filter)) return MIJ_EINVAL;
  if (!rs_side(w) || !rs_side(h) || !rs_side(out_w) || !rs_side(out_h))
    return mij_fail(MIJ_EINVAL, "mij_resize: %dx%d to %dx%d (1..65535 each)", w, h, out_w, out_h);
  const unsigned long long need = 3ULL * out_w * out_h;
  if (cap < need) return mij_fail(MIJ_ENOSPC, "mij_resize: need %llu bytes", need);
  if (!px || !out || stride_px < w)
    return mij_fail(MIJ_EINVAL, "mij_resize: null buffer or stride %d under the width %d", stride_px, w);
  mij_resizer *r = mij_resizer_create(mij_drop_device(), 1);
  if (!r) return mij_last_error();
  uint8_t *d_src = nullptr;
  auto run = [&]() -> int {
    const size_t row = 3 * (size_t)w;
    HIP_TRY(hipMalloc((void **)&d_src, row * h + 16));
    HIP_TRY(hipMemcpy2DAsync(d_src, row, px, 3 * (size_t)stride_px, row, h, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));  // a pageable source
    const mij_image im = {d_src, (long long)row, w, h};
    const int wh[2] = {out_w, out_h};
    if (int rc = mij_resizer_resize(r, &im, wh, 1, filter)) return rc;
    return mij_resizer_pixels(r, 0, out, cap, 0);
  };
  const int rc = run();
  resizer_free(r);  // (waits for its stream; leaves the failure's message in place)
  hipFree(d_src);
  return rc;
}

extern "C" int mij_thumbnail_denom(int w, int h, int out_w, int out_h) {
  if (w < 1 || h < 1 || out_w < 1 || out_h < 1) return 1;
  const int scale = std::min(w / out_w, h / out_h);
  for (int d = 8; d > 1; d >>= 1)
    if (d <= scale) return d;
  return 1;
}

// sampling < 0: the reference's arithmetic at 4:2:0 (mij_thumbnail); otherwise
// libjpeg's at that MIJ_SAMP_* (mij_thumbnail_libjpeg)
static int thumbnail(const char *what, const uint8_t *jpg, size_t len, int out_w, int out_h, int filter, int quality,
                     int sampling, uint8_t *out, size_t cap, size_t *out_len) {
  mij_clear_error();
  if (out_len) *out_len = 0;
  if (rs_check_filter(what, filter)) return MIJ_EINVAL;
  if (!rs_side(out_w) || !rs_side(out_h))
    return mij_fail(MIJ_EINVAL, "%s: out size %dx%d (1..65535 each)", what, out_w, out_h);
  if (quality < 1 || quality > 100) return mij_fail(MIJ_EINVAL, "%s: quality %d (1..100)", what, quality);
  if (sampling > MIJ_SAMP_GRAY) return mij_fail(MIJ_EINVAL, "%s: sampling %d (MIJ_SAMP_420 .. MIJ_SAMP_GRAY)", what, sampling);
  if (!jpg) return mij_fail(MIJ_EINVAL, "%s: jpg is NULL", what);
  // the headers, through mij_decode asked for the size: what it refuses is refused here, with its message
  int w = 0, h = 0;
  uint8_t probe;
  if (int rc = mij_decode(jpg, len, MIJ_PIX_BGR, &probe, 0, &w, &h); rc != MIJ_ENOSPC) return rc;
  mij_clear_error();
  const size_t bound = sampling < 0 ? mij_max_jpg_bytes_any(out_w, out_h, 0) : mij_max_jpg_bytes_sampled(out_w, out_h, sampling, 0);
  if (out_len) *out_len = bound;
  if (cap < bound) return mij_fail(MIJ_ENOSPC, "%s: need %zu bytes for %dx%d", what, bound, out_w, out_h);
  if (!out) return mij_fail(MIJ_EINVAL, "%s: out is NULL", what);
  const int denom = mij_thumbnail_denom(w, h, out_w, out_h);
  const int dev = mij_drop_device();
  mij_decoder *d = nullptr;
  mij_resizer *r = nullptr;
  mij_batch *b = nullptr;
  auto run = [&]() -> int {
    if (!(d = mij_decoder_create(dev, (w + 15) / 16 * 16, (h + 15) / 16 * 16, 1))) return mij_last_error();
    if (!(r = mij_resizer_create(dev, 1))) return mij_last_error();
    if (!(b = mij_batch_create(dev, (out_w + 15) / 16 * 16, (out_h + 15) / 16 * 16, 1, quality))) return mij_last_error();
    // one stream for all three stages: the decoder's
    if (int rc = mij_resizer_set_stream(r, mij_decoder_stream(d))) return rc;
    if (int rc = mij_batch_set_stream(b, mij_decoder_stream(d))) return rc;
    if (int rc = mij_decoder_decode(d, &jpg, &len, 1)) return rc;
    if (int rc = mij_decoder_reconstruct_scaled(d, MIJ_PIX_BGR, denom)) return rc;
    mij_image im;
    if (!(im.px = mij_decoder_device_pixels(d, 0, &im.pitch))) return mij_last_error();
    im.w = (w + denom - 1) / denom;
    im.h = (h + denom - 1) / denom;
    const int wh[2] = {out_w, out_h};
    if (int rc = mij_resizer_resize(r, &im, wh, 1, filter)) return rc;
    long long pitch = 0;
    const void *px = mij_resizer_device_pixels(r, 0, &pitch);
    if (!px) return mij_last_error();
    if (int rc = mij_batch_pad_input(b, px, 0, pitch, wh, 1)) return rc;
    if (int rc = sampling < 0 ? mij_batch_encode_interleaved(b, 1, 0) : mij_batch_encode_libjpeg(b, 1, sampling, 0)) return rc;
    size_t n = 0;
    if (int rc = mij_batch_output(b, 0, out, cap, &n)) return rc;
    if (out_len) *out_len = n;
    return MIJ_OK;
  };
  const int rc = run();
  // the borrowers of the decoder's stream first; each waits for what it enqueued there, and a failure's
  // message stays in place
  mij_batch_destroy(b);
  resizer_free(r);
  mij_decoder_destroy(d);
  return rc;
}

extern "C" int mij_thumbnail(const uint8_t *jpg, size_t len, int out_w, int out_h, int filter, int quality,
                             uint8_t *out, size_t cap, size_t *out_len) {
  return thumbnail("mij_thumbnail", jpg, len, out_w, out_h, filter, quality, -1, out, cap, out_len);
}

extern "C" int mij_thumbnail_libjpeg(const uint8_t *jpg, size_t len, int out_w, int out_h, int filter, int quality,
                                     int sampling, uint8_t *out, size_t cap, size_t *out_len) {
  if (sampling < MIJ_SAMP_420) {
    mij_clear_error();
    if (out_len) *out_len = 0;
    return mij_fail(MIJ_EINVAL, "mij_thumbnail_libjpeg: sampling %d (MIJ_SAMP_420 .. MIJ_SAMP_GRAY)", sampling);
  }
  return thumbnail("mij_thumbnail_libjpeg", jpg, len, out_w, out_h, filter, quality, sampling, out, cap, out_len);
}
