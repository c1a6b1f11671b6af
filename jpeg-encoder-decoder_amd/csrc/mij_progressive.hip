// mij_progressive.hip -- progressive JPEG on the device: the
// scans of every progressive frame of a call, decoded into the decoder's
// arena of coefficient planes, and the hand-over that leaves those planes as
// an interleaved baseline frame without restart intervals leaves them.
//
// The unit of work is one restart interval of one scan (a whole scan without
// DRI), decoded sequentially from its first bit by mij_progressive.h's
// prog_decode_unit: EOB runs span blocks, and a refinement scan's bit
// consumption depends on which coefficients are already nonzero, so nothing
// inside a unit can start early.  Parallelism is units x scans x frames:
// the host sorts each frame's scans into levels (a scan's level is 1 + the
// highest level of an earlier scan sharing a component and an overlapping
// band), and one launch per level runs every unit of that level of every
// frame.  Scans of one level touch disjoint coefficients; units of one scan
// touch disjoint blocks.
#include <hip/hip_runtime.h>

#include "mij_host.h"
#include "mij_progressive.h"

#define HIP_TRY(x)                                                                 \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess)                                                          \
      return mij_fail(MIJ_EHIP, "%s failed: %s", #x, hipGetErrorString(e_));       \
  } while (0)

namespace mij {

// units [u0, u1).  WAVE: one unit per wave, lane 0 alone works: no
// divergence, 1/64 of the lanes, and the default, 2.5 times as fast as the
// other on 64 streams of 1920x1088.  Otherwise one unit per
// lane, 64 lanes per workgroup (the host orders a level's units by scan,
// then frame, then interval, so a wave's lanes run the same procedure; their
// symbols still differ, and lanes that diverge serialise).
template <bool WAVE>
__global__ __launch_bounds__(64) void k_prog_scan(const uint8_t *blob, const ProgUnit *units, const ProgScanDev *scans,
                                                  const DecTab *tabs, int16_t *coefs, int *status, int u0, int u1) {
  const int u = u0 + (WAVE ? (int)blockIdx.x : (int)(blockIdx.x * 64 + threadIdx.x));
  if (u >= u1 || (WAVE && threadIdx.x)) return;
  const ProgUnit U = units[u];
  const int st = prog_decode_unit(blob, U, scans[U.scan], tabs, coefs);
  if (st) atomicMax(&status[U.scan], st);
}

// scan-order index -> raster index in the padded plane (interleaved order)
__device__ __forceinline__ int prog_scan_to_raster(const ProgDcJob &j, int s) {
  const int hv = j.hs * j.vs, m = s / hv, i = s - m * hv;
  const int my = m / j.mcus_x, mx = m - my * j.mcus_x, iy = i / j.hs, ix = i - iy * j.hs;
  return (my * j.vs + iy) * j.bw + mx * j.hs + ix;
}

// Hand-over, in two launches (the second reads its neighbour's DC, so the
// absolute values are first copied aside): block s of a component, in the
// interleaved scan's order, gets DC(s) - DC(s - 1), DC(-1) = 0, which is
// what the baseline path leaves for a frame without restart intervals.
// blockIdx.y: the job; dcabs: one int16 per block of the arena.
__global__ __launch_bounds__(256) void k_prog_dcabs(const ProgDcJob *jobs, const int16_t *coefs, int16_t *dcabs) {
  const ProgDcJob j = jobs[blockIdx.y];
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < j.nblocks) dcabs[j.off / 64 + r] = coefs[j.off + 64LL * r];
}

__global__ __launch_bounds__(256) void k_prog_dcdiff(const ProgDcJob *jobs, int16_t *coefs, const int16_t *dcabs) {
  const ProgDcJob j = jobs[blockIdx.y];
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= j.nblocks) return;
  const int16_t *a = dcabs + j.off / 64;
  const int r = prog_scan_to_raster(j, s);
  const int prev = s ? a[prog_scan_to_raster(j, s - 1)] : 0;
  coefs[j.off + 64LL * r] = (int16_t)(a[r] - prev);
}

template <class T>
static int prog_grow(T *&p, size_t &cap, size_t need) {
  if (need <= cap) return MIJ_OK;
  hipFree(p);
  p = nullptr;
  cap = 0;
  need += need / 4 + 16;
  HIP_TRY(hipMalloc((void **)&p, need * sizeof(T)));
  cap = need;
  return MIJ_OK;
}

void prog_free(ProgBuffers &B) {
  for (void *p : {(void *)B.tabs, (void *)B.scans, (void *)B.units, (void *)B.status, (void *)B.dcjobs, (void *)B.dcabs})
    hipFree(p);
  B = ProgBuffers();
}

int prog_run(hipStream_t stream, ProgBuffers &B, const uint8_t *d_blob, int16_t *d_coef, long long arena_blocks,
             const std::vector<DecTab> &tabs, const std::vector<ProgScanDev> &scans, const std::vector<ProgUnit> &units,
             const std::vector<int> &level_end, const std::vector<ProgDcJob> &dcjobs, int mapping,
             std::vector<int> &status) {
  const size_t ns = scans.size(), nu = units.size(), nj = dcjobs.size();
  if (int rc = prog_grow(B.tabs, B.tabs_cap, tabs.size())) return rc;
  if (int rc = prog_grow(B.scans, B.scans_cap, ns)) return rc;
  if (int rc = prog_grow(B.units, B.units_cap, nu)) return rc;
  if (int rc = prog_grow(B.status, B.status_cap, ns)) return rc;
  if (int rc = prog_grow(B.dcjobs, B.dcjobs_cap, nj)) return rc;
  if (int rc = prog_grow(B.dcabs, B.dcabs_cap, (size_t)arena_blocks)) return rc;
  HIP_TRY(hipMemcpyAsync(B.tabs, tabs.data(), tabs.size() * sizeof(DecTab), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(B.scans, scans.data(), ns * sizeof(ProgScanDev), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(B.units, units.data(), nu * sizeof(ProgUnit), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(B.dcjobs, dcjobs.data(), nj * sizeof(ProgDcJob), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(B.status, 0, ns * sizeof(int), stream));
  int u0 = 0;
  for (int u1 : level_end) {
    if (u1 > u0) {
      if (mapping == PROG_MAP_WAVE)
        hipLaunchKernelGGL(k_prog_scan<true>, dim3(u1 - u0), dim3(64), 0, stream, d_blob, B.units, B.scans, B.tabs, d_coef,
                           B.status, u0, u1);
      else
        hipLaunchKernelGGL(k_prog_scan<false>, dim3((u1 - u0 + 63) / 64), dim3(64), 0, stream, d_blob, B.units, B.scans,
                           B.tabs, d_coef, B.status, u0, u1);
    }
    u0 = u1;
  }
  HIP_TRY(hipGetLastError());
  status.assign(ns, 0);
  HIP_TRY(hipMemcpyAsync(status.data(), B.status, ns * sizeof(int), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int st : status)
    if (st) return MIJ_OK;  // the caller reports it; the planes are not handed over
  int maxb = 1;
  for (const ProgDcJob &j : dcjobs) maxb = std::max(maxb, j.nblocks);
  for (size_t j0 = 0; j0 < nj; j0 += 32768) {  // grid.y is a 16-bit quantity
    const dim3 grid((maxb + 255) / 256, (unsigned)std::min<size_t>(32768, nj - j0));
    hipLaunchKernelGGL(k_prog_dcabs, grid, dim3(256), 0, stream, B.dcjobs + j0, d_coef, B.dcabs);
    hipLaunchKernelGGL(k_prog_dcdiff, grid, dim3(256), 0, stream, B.dcjobs + j0, d_coef, B.dcabs);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(stream));
  return MIJ_OK;
}

}  // namespace mij
