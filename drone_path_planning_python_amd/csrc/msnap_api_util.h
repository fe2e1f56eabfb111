// What the translation units that define C-ABI entry points share (msnap_api.hip and every unit that holds its own
// subsystem's entries; msnap_timeopt.hip holds those of all five time-allocation modes): the argument checks, the entry
// macro and the one staging helper every host-pointer call goes through.
#pragma once

#include <math.h>

#include <initializer_list>

#include "msnap_internal.h"

namespace msnap {

inline int check_seg(const msnap_ctx *ctx, int n_seg) {
  if (n_seg < 1 || n_seg > ctx->max_segments) return MSNAP_ESEGMENTS;
  return MSNAP_OK;
}

// An entry point and its _device twin share one argument check.  It returns MSNAP_OK to go on, an error code, or
// kNoWork when the call has nothing to compute (the entry point then returns MSNAP_OK).
constexpr int kNoWork = 1;

// the start of such an entry point: anything but MSNAP_OK from the check is returned, then the device is selected
#define MSNAP_ENTER(ctx, check)                                   \
  do {                                                            \
    const int rc__ = (check);                                     \
    if (rc__) return rc__ == msnap::kNoWork ? MSNAP_OK : rc__;    \
    MSNAP_HIP(ctx, hipSetDevice((ctx)->device));                  \
  } while (0)

// One host region of a host-pointer call: `in` is copied to the device before the launch, the device copy back to
// `out` after it.  Either may be null; both set: the launch updates the region in place.
struct Region {
  const void *in;
  void *out;
  size_t bytes;
};
inline Region upload(const void *h, size_t bytes) { return {h, nullptr, bytes}; }
inline Region download(void *h, size_t bytes) { return {nullptr, h, bytes}; }

// a staged region's device address, for any pointer parameter of a launcher
struct DevPtr {
  void *p;
  template <class T>
  operator T *() const { return static_cast<T *>(p); }
};

// A host-pointer call.  The regions are carved, 256-byte aligned, out of the context's one staging arena (a region of
// no bytes still gets a valid, non-null address); the inputs are copied in on ctx->stream, `launch` runs on their
// device addresses, the outputs are copied back and the stream is synchronised once.  A failed launch returns its
// code with nothing copied back.
template <size_t K, class Launch>
int staged(msnap_ctx *ctx, const Region (&r)[K], Launch &&launch) {
  size_t off[K], total = 0;
  for (size_t k = 0; k < K; ++k) {
    off[k] = total;
    total += r[k].bytes ? (r[k].bytes + 255) & ~(size_t)255 : 256;
  }
  int rc = ensure(ctx, ctx->host_stage, total);
  if (rc) return rc;
  DevPtr d[K];
  for (size_t k = 0; k < K; ++k) {
    d[k].p = (char *)ctx->host_stage.p + off[k];
    if (r[k].in && r[k].bytes)
      MSNAP_HIP(ctx, hipMemcpyAsync(d[k].p, r[k].in, r[k].bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  if ((rc = launch(d))) return rc;
  for (size_t k = 0; k < K; ++k)
    if (r[k].out && r[k].bytes)
      MSNAP_HIP(ctx, hipMemcpyAsync(r[k].out, d[k].p, r[k].bytes, hipMemcpyDeviceToHost, ctx->stream));
  MSNAP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MSNAP_OK;
}

// bytes of a batch's coefficients [n_drones][n_seg][4][order + 1] and durations [n_drones][n_seg]
inline size_t coef_bytes(const msnap_ctx *ctx, int n_drones, int n_seg) {
  return (size_t)n_drones * n_seg * 4 * (ctx->order + 1) * 8;
}
inline size_t dur_bytes(int n_drones, int n_seg) { return (size_t)n_drones * n_seg * 8; }

// every pointer of the list is required: the last step of an argument check
inline int all_required(std::initializer_list<const void *> ptrs) {
  for (const void *p : ptrs)
    if (!p) return MSNAP_EINVAL;
  return MSNAP_OK;
}

// a batch of n_drones paths of n_seg segments whose every pointer is required
inline int batch_args(const msnap_ctx *ctx, int n_drones, int n_seg, std::initializer_list<const void *> ptrs) {
  if (!ctx || n_drones < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, n_seg)) return rc;
  if (n_drones == 0) return kNoWork;
  return all_required(ptrs);
}

// The launch of a kernel that carries one tile of kDronesPerWave drones per wave in `lds_bytes` of dynamic LDS
// (K13, K15, K21).  Beyond 64 KiB a kernel has to be told: an attribute of the function, no stream operation.
template <class... P, class... A>
int launch_tiles(msnap_ctx *ctx, void (*kernel)(P...), size_t lds_bytes, int n_drones, A... args) {
  if (lds_bytes > 64 * 1024)
    MSNAP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLdsBytes));
  const int ntiles = (n_drones + kDronesPerWave - 1) / kDronesPerWave;
  hipLaunchKernelGGL(kernel, dim3(ntiles), dim3(kWave), lds_bytes, ctx->stream, static_cast<P>(args)...);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

// the numbers of a window call (msnap_window.h): a time resolution > 0 and, where there is one, a threshold >= 0
inline bool window_levels_valid(double t_res, double threshold = 0.0) {
  return isfinite(threshold) && threshold >= 0.0 && isfinite(t_res) && t_res > 0.0;
}

}  // namespace msnap
