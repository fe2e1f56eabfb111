// C-ABI of libmsnap.so (include/msnap.h): context management, host-pointer
// wrappers, stream / timer plumbing.  All compute happens in the HIP kernels of the other translation units (SRCS of
// the Makefile, one subsystem each).  The units of the later subsystems -- msnap_timeopt.hip for all five
// time-allocation modes, msnap_clearance.hip, msnap_pairs.hip, msnap_mesh_clearance.hip, msnap_extent.hip,
// msnap_states.hip, msnap_periodic.hip -- hold their own entry points, on the helpers of msnap_api_util.h; there is no
// CPU fallback.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>

#include "msnap_internal.h"
#include "msnap_api_util.h"
#include "msnap_collide.h"

namespace msnap {

int record_hip_error(msnap_ctx *ctx, hipError_t e, const char *what) {
  if (ctx) snprintf(ctx->hip_err, sizeof(ctx->hip_err), "%s: %s", what, hipGetErrorString(e));
  return MSNAP_EHIP;
}

int handover_form(const msnap_ctx *ctx, const void *ptr, const void *pos, int n, int n_samples) {
  if (!ptr) return 0;
  for (const auto &h : ctx->handover)
    if (h.ptr == ptr) return (h.pos == pos && h.n == n && h.s == n_samples) ? h.form : 0;
  return 0;
}

bool stream_is_capturing(const msnap_ctx *ctx) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return ctx->stream && hipStreamIsCapturing(ctx->stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

int ensure(msnap_ctx *ctx, DevBuf &b, size_t bytes) {
  const bool capturing = stream_is_capturing(ctx);
  if (bytes <= b.cap) {
    // the launch about to be captured records pointers into this block: from now on a graph may replay on it
    if (capturing) b.in_graph = true;
    return MSNAP_OK;
  }
  // growing synchronises the stream and frees the old block: neither is legal while the stream is being
  // captured into a graph, and a capture must not silently record a launch on a buffer that is about to go
  if (capturing) return MSNAP_ECAPTURE;
  if (b.p && b.in_graph) {
    // a graph captured earlier may replay on the old block at any time: it is retired, not freed (msnap.h,
    // "Stream capture"); work queued on it eagerly stays valid for the same reason
    RetiredBuf *r = new (std::nothrow) RetiredBuf{b.p, b.cap, ctx->retired};
    if (!r) return MSNAP_ENOMEM;
    ctx->retired = r;
    b.p = nullptr;
    b.cap = 0;
    b.in_graph = false;
  } else if (b.p) {
    MSNAP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    MSNAP_HIP(ctx, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
  }
  size_t cap = bytes + bytes / 4 + 256;
  hipError_t e = hipMalloc(&b.p, cap);
  if (e != hipSuccess) {
    b.p = nullptr;
    record_hip_error(ctx, e, "hipMalloc");
    return MSNAP_ENOMEM;
  }
  b.cap = cap;
  return MSNAP_OK;
}

struct OptionName {
  const char *name, *env;
};
static const OptionName kOptions[] = {
    {"solve_grid_waves", "MSNAP_SOLVE_GRID_WAVES"}, {"gemm_grid_waves", "MSNAP_GEMM_GRID_WAVES"},
    {"twist_max_drones", "MSNAP_TWIST_MAX_DRONES"}, {"no_twist", "MSNAP_NO_TWIST"}, {"twist_waves", "MSNAP_TWIST_WAVES"},
    {"collide_waves_per_cu", "MSNAP_COLLIDE_WAVES_PER_CU"}, {"pipe_chunk_mb", "MSNAP_PIPE_CHUNK_MB"},
    {"collide_sample_parts", "MSNAP_COLLIDE_SAMPLE_PARTS"}, {"no_twin", "MSNAP_NO_TWIN"}, {"no_grid_sample", "MSNAP_NO_GRID_SAMPLE"}, {"gemm_stream_waves_per_cu", "MSNAP_GEMM_STREAM_WAVES_PER_CU"}, {"mesh_waves_per_cu", "MSNAP_MESH_WAVES_PER_CU"}, {"collide_no_cull", "MSNAP_COLLIDE_NO_CULL"}, {"collide_cull_min_drones", "MSNAP_COLLIDE_CULL_MIN_DRONES"}, {"collide_cull_mode", "MSNAP_COLLIDE_CULL_MODE"}, {"twin_max_drones", "MSNAP_TWIN_MAX_DRONES"},
};

void note_kernel(msnap_ctx *ctx, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(ctx->last_kernel, sizeof(ctx->last_kernel), fmt, ap);
  va_end(ap);
}

static bool option_is_read_only(const char *name) { return !strncmp(name, "collide_last_", 13); }

static int *option_slot(msnap_ctx *ctx, const char *name) {
  if (!strcmp(name, "solve_grid_waves")) return &ctx->solve_grid_waves;
  if (!strcmp(name, "gemm_grid_waves")) return &ctx->gemm_grid_waves;
  if (!strcmp(name, "twist_max_drones")) return &ctx->twist_max_drones;
  if (!strcmp(name, "no_twist")) return &ctx->no_twist;
  if (!strcmp(name, "twist_waves")) return &ctx->twist_waves;
  if (!strcmp(name, "no_twin")) return &ctx->no_twin;
  if (!strcmp(name, "no_grid_sample")) return &ctx->no_grid_sample;
  if (!strcmp(name, "gemm_stream_waves_per_cu")) return &ctx->gemm_stream_waves_per_cu;
  if (!strcmp(name, "mesh_waves_per_cu")) return &ctx->mesh_waves_per_cu;
  if (!strcmp(name, "twin_max_drones")) return &ctx->twin_max_drones;
  if (!strcmp(name, "collide_waves_per_cu")) return &ctx->collide_waves_per_cu;
  if (!strcmp(name, "collide_sample_parts")) return &ctx->collide_sample_parts;
  if (!strcmp(name, "collide_no_sym")) return &ctx->collide_no_sym;
  if (!strcmp(name, "collide_no_cull")) return &ctx->collide_no_cull;
  if (!strcmp(name, "collide_cull_min_drones")) return &ctx->collide_cull_min_drones;
  if (!strcmp(name, "collide_cull_mode")) return &ctx->collide_cull_mode;
  if (!strcmp(name, "collide_last_cull")) return &ctx->collide_last_cull;
  if (!strcmp(name, "collide_last_shares")) return &ctx->collide_last_shares;
  if (!strcmp(name, "collide_last_sym")) return &ctx->collide_last_sym;   // (read: what the last pass did)
  if (!strcmp(name, "collide_last_handover")) return &ctx->collide_last_handover;
  if (!strcmp(name, "own_stream_priority")) return &ctx->own_stream_priority;   // (read side; set has its own branch)
  return nullptr;
}

}  // namespace msnap

using namespace msnap;

extern "C" {

int msnap_version(void) { return MSNAP_VERSION_NUM; }

const char *msnap_strerror(int code) {
  switch (code) {
    case MSNAP_OK: return "ok";
    case MSNAP_EINVAL: return "invalid argument";
    case MSNAP_EHIP: return "HIP runtime error (see msnap_last_hip_error)";
    case MSNAP_EORDER: return "unsupported polynomial order (7 or 9)";
    case MSNAP_ESEGMENTS: return "segment count out of range for this context, or not the prepared grid's";
    case MSNAP_ENOMEM: return "out of memory";
    case MSNAP_ENODEVICE: return "no usable gfx950 device";
    case MSNAP_ENOGRID: return "no time grid prepared on this context (msnap_grid_prepare)";
    case MSNAP_ECAPTURE: return "a scratch buffer would have to grow during stream capture: run the call once outside the capture first";
    default: return "unknown msnap error";
  }
}

const char *msnap_last_hip_error(const msnap_ctx *ctx) { return ctx ? ctx->hip_err : ""; }

const char *msnap_last_kernel(const msnap_ctx *ctx) { return ctx ? ctx->last_kernel : ""; }

int msnap_create(msnap_ctx **out, int device_id, int order, int max_segments) {
  if (!out) return MSNAP_EINVAL;
  *out = nullptr;
  if (order != 7 && order != 9) return MSNAP_EORDER;
  if (max_segments < 1) return MSNAP_ESEGMENTS;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MSNAP_ENODEVICE;
  if (device_id < 0 || device_id >= ndev) return MSNAP_ENODEVICE;
  msnap_ctx *ctx = new (std::nothrow) msnap_ctx();
  if (!ctx) return MSNAP_ENOMEM;
  ctx->device = device_id;
  ctx->order = order;
  ctx->khalf = (order + 1) / 2;
  ctx->max_segments = max_segments;
  // the only place the environment is read: seeds of the msnap_set_option knobs
  for (const OptionName &o : kOptions) {
    const char *e = getenv(o.env);
    if (e && atol(e) > 0) (void)msnap_set_option(ctx, o.name, atol(e));
  }
  int rc = MSNAP_OK;
  do {
    if (hipSetDevice(device_id) != hipSuccess) { rc = MSNAP_ENODEVICE; break; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) ctx->n_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) { rc = MSNAP_EHIP; break; }
    ctx->stream = ctx->own_stream;
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) { rc = MSNAP_EHIP; break; }
    if (hipHostMalloc((void **)&ctx->cull_hint, 64, hipHostMallocDefault) != hipSuccess) {
      ctx->cull_hint = nullptr;      // (the pairwise pass then never has a hint and keeps its default evaluator)
      (void)hipGetLastError();
    } else {
      *ctx->cull_hint = 0;
    }
    rc = solve_kernel_setup(ctx);
  } while (0);
  if (rc != MSNAP_OK) {
    msnap_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return MSNAP_OK;
}

void msnap_destroy(msnap_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
  (void)msnap_release_graph_buffers(ctx, nullptr);
  if (ctx->mesh_tests) (void)hipFree(ctx->mesh_tests);
  for (msnap::DevBuf *b : {&ctx->scratch, &ctx->limits_work, &ctx->extent_work, &ctx->clearance_work,&ctx->mesh_clearance_work, &ctx->pairs_work, &ctx->host_stage, &ctx->collide_work, &ctx->grid_t,
                           &ctx->grid_wp, &ctx->grid_op, &ctx->grid_dur, &ctx->grid_status, &ctx->grid_frag})
    if (b->p) (void)hipFree(b->p);
  for (int k = 0; k < 2; ++k) {
    if (ctx->pipe_stream[k]) (void)hipStreamSynchronize(ctx->pipe_stream[k]);
    for (auto &b : ctx->pipe[k])
      if (b.p) (void)hipFree(b.p);
    if (ctx->pipe_stream[k]) (void)hipStreamDestroy(ctx->pipe_stream[k]);
  }
  if (ctx->pipe_start) (void)hipEventDestroy(ctx->pipe_start);
  if (ctx->bounce) (void)hipHostFree(ctx->bounce);
  if (ctx->cull_hint) (void)hipHostFree(ctx->cull_hint);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

int msnap_release_graph_buffers(msnap_ctx *ctx, size_t *bytes) {
  if (!ctx) return MSNAP_EINVAL;
  size_t freed = 0;
  int rc = MSNAP_OK;
  (void)hipSetDevice(ctx->device);
  while (ctx->retired) {
    RetiredBuf *r = ctx->retired;
    ctx->retired = r->next;
    if (hipFree(r->p) != hipSuccess) rc = MSNAP_EHIP;      // (hipFree waits for the device's outstanding work)
    freed += r->cap;
    delete r;
  }
  if (bytes) *bytes = freed;
  return rc;
}

int msnap_set_stream(msnap_ctx *ctx, void *hip_stream) {
  if (!ctx) return MSNAP_EINVAL;
  ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return MSNAP_OK;
}

int msnap_use_own_stream(msnap_ctx *ctx) {
  if (!ctx) return MSNAP_EINVAL;
  ctx->stream = ctx->own_stream;
  return MSNAP_OK;
}

int msnap_set_option(msnap_ctx *ctx, const char *name, long value) {
  if (!ctx || !name || value < 0 || value > (1L << 30)) return MSNAP_EINVAL;
  if (!strcmp(name, "pipe_chunk_mb")) {
    ctx->pipe_chunk_bytes = (size_t)(value > 0 ? value : 64) << 20;
    return MSNAP_OK;
  }
  if (!strcmp(name, "own_stream_priority")) {
    // 0 = default, 1 = the lowest priority the device offers, 2 = the highest: the context's own stream is
    // re-created (work queued on it is drained first; an external stream set by msnap_set_stream stays)
    if (value > 2) return MSNAP_EINVAL;
    MSNAP_HIP(ctx, hipSetDevice(ctx->device));
    int least = 0, greatest = 0;
    MSNAP_HIP(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t fresh = nullptr;
    MSNAP_HIP(ctx, hipStreamCreateWithPriority(&fresh, hipStreamNonBlocking,
                                               value == 1 ? least : value == 2 ? greatest : 0));
    const bool current = ctx->stream == ctx->own_stream;
    if (ctx->own_stream) {
      (void)hipStreamSynchronize(ctx->own_stream);
      (void)hipStreamDestroy(ctx->own_stream);
    }
    ctx->own_stream = fresh;
    if (current) ctx->stream = fresh;
    ctx->own_stream_priority = (int)value;
    return MSNAP_OK;
  }
  if (!strcmp(name, "mesh_count_tests")) {
    MSNAP_HIP(ctx, hipSetDevice(ctx->device));
    MSNAP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (value && !ctx->mesh_tests) MSNAP_HIP(ctx, hipMalloc(&ctx->mesh_tests, 8));
    if (ctx->mesh_tests) MSNAP_HIP(ctx, hipMemset(ctx->mesh_tests, 0, 8));
    if (!value && ctx->mesh_tests) {
      (void)hipFree(ctx->mesh_tests);
      ctx->mesh_tests = nullptr;
    }
    return MSNAP_OK;
  }
  if (option_is_read_only(name)) return MSNAP_EINVAL;      // "collide_last_*": what the last pass did
  if (!strcmp(name, "twist_waves") && value != 0 && value != 1 && value != 2 && value != 4) return MSNAP_EINVAL;
  int *slot = option_slot(ctx, name);
  if (!slot) return MSNAP_EINVAL;
  *slot = (int)value;
  return MSNAP_OK;
}

int msnap_get_option(const msnap_ctx *ctx, const char *name, long *value) {
  if (!ctx || !name || !value) return MSNAP_EINVAL;
  if (!strcmp(name, "pipe_chunk_mb")) {
    *value = (long)(ctx->pipe_chunk_bytes >> 20);
    return MSNAP_OK;
  }
  if (!strcmp(name, "mesh_count_tests")) {   // the count since it was last set (synchronises the stream)
    unsigned long long n = 0;
    if (ctx->mesh_tests) {
      if (stream_is_capturing(ctx)) return MSNAP_ECAPTURE;
      if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
          hipMemcpy(&n, ctx->mesh_tests, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return MSNAP_EHIP;
    }
    *value = (long)n;
    return MSNAP_OK;
  }
  if (!strcmp(name, "collide_last_group_pairs") || !strcmp(name, "collide_last_survivors") ||
      !strcmp(name, "collide_last_by_groups") || !strcmp(name, "collide_last_pairs_evaluated")) {
    // counts the last broad-phase pass left on the device (synchronises the stream; not during a capture)
    int32_t shares = ctx->collide_last_shares, groups = 0;
    const bool culled = ctx->collide_last_cull && ctx->collide_meta;
    if (culled) {
      if (stream_is_capturing(ctx)) return MSNAP_ECAPTURE;
      if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
          hipMemcpy(&shares, ctx->collide_meta + kMetaTotal, sizeof shares, hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(&groups, ctx->collide_meta + kMetaGroups, sizeof groups, hipMemcpyDeviceToHost) != hipSuccess)
        return MSNAP_EHIP;
    }
    // (a large swarm's group evaluator ran only if its survivors fit the list: kGroupCapLarge slots)
    const bool by_groups = culled && (ctx->collide_last_by_groups == 1 || (ctx->collide_last_by_groups == 2 && groups <= kGroupCapLarge));
    if (!strcmp(name, "collide_last_group_pairs")) *value = groups;
    else if (!strcmp(name, "collide_last_survivors")) *value = shares;
    else if (!strcmp(name, "collide_last_by_groups")) *value = by_groups ? 1 : 0;
    else *value = !culled ? -1 : by_groups ? (long)groups * 64 : (long)shares * 1024;
    return MSNAP_OK;
  }
  const int *slot = option_slot(const_cast<msnap_ctx *>(ctx), name);
  if (!slot) return MSNAP_EINVAL;
  *value = *slot;
  return MSNAP_OK;
}

int msnap_host_alloc(void **ptr, size_t bytes) {
  if (!ptr) return MSNAP_EINVAL;
  *ptr = nullptr;
  if (bytes == 0) return MSNAP_OK;
  hipError_t e = hipHostMalloc(ptr, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    *ptr = nullptr;
    (void)hipGetLastError();
    return e == hipErrorNoDevice ? MSNAP_ENODEVICE : MSNAP_ENOMEM;
  }
  return MSNAP_OK;
}

int msnap_host_free(void *ptr) {
  if (!ptr) return MSNAP_OK;
  return hipHostFree(ptr) == hipSuccess ? MSNAP_OK : MSNAP_EHIP;
}

void *msnap_get_stream(msnap_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int msnap_sync(msnap_ctx *ctx) {
  if (!ctx) return MSNAP_EINVAL;
  MSNAP_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MSNAP_OK;
}

int msnap_timer_start(msnap_ctx *ctx) {
  if (!ctx) return MSNAP_EINVAL;
  MSNAP_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return MSNAP_OK;
}

int msnap_timer_stop(msnap_ctx *ctx, float *elapsed_ms) {
  if (!ctx || !elapsed_ms) return MSNAP_EINVAL;
  MSNAP_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  MSNAP_HIP(ctx, hipEventSynchronize(ctx->ev1));
  MSNAP_HIP(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
  return MSNAP_OK;
}

// ------------------------------------------------------------------ solve
// Host-pointer solve (msnap_solve_batch / msnap_solve_grid): H2D, kernel, D2H.
// Batches whose coefficients exceed one chunk (ctx->pipe_chunk_bytes) are cut into chunks of
// drones that alternate between two streams, each with its own device staging set, so chunk
// c+1's upload and kernel overlap chunk c's download; with page-locked host buffers
// (msnap_host_alloc) both copy engines then run at PCIe rate, with pageable memory the HIP
// runtime serialises the copies and the result is the same as one big copy.  Device staging is
// bounded by two chunks, whatever the batch size.
constexpr size_t kBounceMax = 1u << 20;   // bytes of inputs + outputs that take the single-bounce path

static int solve_host(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t, int shared,
                      bool use_grid, double *coef, double *dur, int32_t *status) {
  const size_t m = (size_t)n_seg + 1, nc = ctx->order + 1;
  const size_t pd_wp = m * 4 * 8, pd_t = m * 8;                       // bytes per drone
  const size_t pd_coef = (size_t)n_seg * 4 * nc * 8, pd_dur = (size_t)n_seg * 8, pd_st = 4;
  size_t chunk = ctx->pipe_chunk_bytes / pd_coef;
  chunk -= chunk % kDronesPerWave;
  if (chunk < 4096) chunk = 4096;
  const size_t N = n_drones;
  int rc;
  auto launch = [&](size_t n, const double *dwp, const double *dt, double *dcoef, double *ddur, int32_t *dst) {
    return use_grid ? launch_solve_grid(ctx, (int)n, dwp, dcoef, ddur, dst)
                    : launch_solve(ctx, (int)n, n_seg, dwp, dt, shared, dcoef, ddur, dst);
  };
  // Small batches (the reference's own call is ONE trajectory): everything goes through one
  // page-locked bounce buffer laid out like the device staging block [wp | t | coef | dur | status],
  // so a call is one upload, the kernel, one download and one synchronise instead of five pageable
  // copies (60 -> ~30 us per call).
  auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t b_t = t ? (shared ? 1 : N) * pd_t : 0;
  const size_t o_t = up256(N * pd_wp), in_bytes = up256(o_t + b_t);                  // [wp | t]
  const size_t o_coef = in_bytes, o_dur = o_coef + up256(N * pd_coef), o_st = o_dur + up256(N * pd_dur);
  const size_t out_bytes = o_st + up256(N * pd_st) - o_coef;                          // [coef | dur | status]
  if (in_bytes + out_bytes <= kBounceMax && !solve_uses_global_scratch(ctx, n_seg)) {
    if (!ctx->bounce) {
      if (hipHostMalloc(&ctx->bounce, kBounceMax, hipHostMallocDefault) != hipSuccess) {
        ctx->bounce = nullptr;
        (void)hipGetLastError();
      } else {
        ctx->bounce_cap = kBounceMax;
      }
    }
    if (ctx->bounce && (rc = ensure(ctx, ctx->host_stage, kBounceMax)) == MSNAP_OK) {
      char *hb = (char *)ctx->bounce, *db = (char *)ctx->host_stage.p;
      memcpy(hb, wp, N * pd_wp);
      if (t) memcpy(hb + o_t, t, b_t);
      MSNAP_HIP(ctx, hipMemcpyAsync(db, hb, in_bytes, hipMemcpyHostToDevice, ctx->stream));
      rc = launch(N, (const double *)db, (const double *)(db + o_t), (double *)(db + o_coef), (double *)(db + o_dur),
                  (int32_t *)(db + o_st));
      if (rc) return rc;
      MSNAP_HIP(ctx, hipMemcpyAsync(hb + o_coef, db + o_coef, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
      MSNAP_HIP(ctx, hipStreamSynchronize(ctx->stream));
      memcpy(coef, hb + o_coef, N * pd_coef);
      memcpy(dur, hb + o_dur, N * pd_dur);
      memcpy(status, hb + o_st, N * pd_st);
      return MSNAP_OK;
    }
  }
  if (N <= chunk || solve_uses_global_scratch(ctx, n_seg))      // one shot on the context's stream
    return staged(ctx, {upload(wp, N * pd_wp), upload(t, b_t), download(coef, N * pd_coef), download(dur, N * pd_dur),
                        download(status, N * pd_st)},
                  [&](const DevPtr *d) { return launch(N, d[0], d[1], d[2], d[3], d[4]); });

  for (int k = 0; k < 2; ++k)
    if (!ctx->pipe_stream[k])
      MSNAP_HIP(ctx, hipStreamCreateWithFlags(&ctx->pipe_stream[k], hipStreamNonBlocking));
  if (!ctx->pipe_start) MSNAP_HIP(ctx, hipEventCreateWithFlags(&ctx->pipe_start, hipEventDisableTiming));
  const bool per_drone_t = t && !shared;
  for (int k = 0; k < 2; ++k) {
    if ((rc = ensure(ctx, ctx->pipe[k][0], chunk * pd_wp))) return rc;
    if (per_drone_t && (rc = ensure(ctx, ctx->pipe[k][1], chunk * pd_t))) return rc;
    if ((rc = ensure(ctx, ctx->pipe[k][2], chunk * pd_coef))) return rc;
    if ((rc = ensure(ctx, ctx->pipe[k][3], chunk * pd_dur))) return rc;
    if ((rc = ensure(ctx, ctx->pipe[k][4], chunk * pd_st))) return rc;
  }
  if (t && shared) {
    if ((rc = ensure(ctx, ctx->host_stage, pd_t))) return rc;
    MSNAP_HIP(ctx, hipMemcpyAsync(ctx->host_stage.p, t, pd_t, hipMemcpyHostToDevice, ctx->stream));
  }
  // the chunk streams start after whatever the context's stream holds (incl. the shared grid upload)
  MSNAP_HIP(ctx, hipEventRecord(ctx->pipe_start, ctx->stream));
  hipStream_t const user_stream = ctx->stream;
  rc = MSNAP_OK;
  hipError_t herr = hipSuccess;
  const char *what = "";
#define PIPE_HIP(call)                                   \
  if (rc == MSNAP_OK && herr == hipSuccess) {            \
    herr = (call);                                       \
    if (herr != hipSuccess) what = #call;                \
  }
  for (int k = 0; k < 2; ++k) PIPE_HIP(hipStreamWaitEvent(ctx->pipe_stream[k], ctx->pipe_start, 0));
  size_t c = 0;
  for (size_t d0 = 0; d0 < N && rc == MSNAP_OK && herr == hipSuccess; d0 += chunk, ++c) {
    const size_t n = (N - d0 < chunk) ? N - d0 : chunk;
    const int k = (int)(c & 1);
    hipStream_t s = ctx->pipe_stream[k];
    DevBuf *b = ctx->pipe[k];
    PIPE_HIP(hipMemcpyAsync(b[0].p, (const char *)wp + d0 * pd_wp, n * pd_wp, hipMemcpyHostToDevice, s));
    if (per_drone_t)
      PIPE_HIP(hipMemcpyAsync(b[1].p, (const char *)t + d0 * pd_t, n * pd_t, hipMemcpyHostToDevice, s));
    if (herr != hipSuccess) break;
    ctx->stream = s;   // the launchers enqueue on ctx->stream
    rc = launch(n, (const double *)b[0].p, per_drone_t ? (const double *)b[1].p : (const double *)ctx->host_stage.p,
                (double *)b[2].p, (double *)b[3].p, (int32_t *)b[4].p);
    ctx->stream = user_stream;
    PIPE_HIP(hipMemcpyAsync((char *)coef + d0 * pd_coef, b[2].p, n * pd_coef, hipMemcpyDeviceToHost, s));
    PIPE_HIP(hipMemcpyAsync((char *)dur + d0 * pd_dur, b[3].p, n * pd_dur, hipMemcpyDeviceToHost, s));
    PIPE_HIP(hipMemcpyAsync((char *)status + d0 * pd_st, b[4].p, n * pd_st, hipMemcpyDeviceToHost, s));
  }
#undef PIPE_HIP
  // always drain both streams, also on the error path: the staging sets must be idle on return
  for (int k = 0; k < 2; ++k) {
    hipError_t e = hipStreamSynchronize(ctx->pipe_stream[k]);
    if (herr == hipSuccess && e != hipSuccess) { herr = e; what = "hipStreamSynchronize(pipe)"; }
  }
  if (rc != MSNAP_OK) return rc;
  if (herr != hipSuccess) return record_hip_error(ctx, herr, what);
  return MSNAP_OK;
}

int msnap_solve_batch_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp,
                             const double *t, int shared_times, double *coef, double *dur,
                             int32_t *status) {
  MSNAP_ENTER(ctx, batch_args(ctx, n_drones, n_seg, {wp, t, coef, dur, status}));
  return launch_solve(ctx, n_drones, n_seg, wp, t, shared_times ? 1 : 0, coef, dur, status);
}

int msnap_solve_batch(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, const double *t,
                      int shared_times, double *coef, double *dur, int32_t *status) {
  MSNAP_ENTER(ctx, batch_args(ctx, n_drones, n_seg, {wp, t, coef, dur, status}));
  return solve_host(ctx, n_drones, n_seg, wp, t, shared_times ? 1 : 0, /*use_grid=*/false, coef, dur, status);
}

// ------------------------------------------------------------------ shared grid (K2)
int msnap_grid_prepare_device(msnap_ctx *ctx, int n_seg, const double *t) {
  if (!ctx || !t) return MSNAP_EINVAL;
  int rc = check_seg(ctx, n_seg);
  if (rc) return rc;
  MSNAP_HIP(ctx, hipSetDevice(ctx->device));
  return launch_grid_prepare(ctx, n_seg, t, 1);
}

int msnap_grid_prepare(msnap_ctx *ctx, int n_seg, const double *t) {
  if (!ctx || !t) return MSNAP_EINVAL;
  int rc = check_seg(ctx, n_seg);
  if (rc) return rc;
  MSNAP_HIP(ctx, hipSetDevice(ctx->device));
  rc = launch_grid_prepare(ctx, n_seg, t, 0);
  if (rc) return rc;
  MSNAP_HIP(ctx, hipStreamSynchronize(ctx->stream));   // t is pageable host memory
  return MSNAP_OK;
}

int msnap_grid_segments(const msnap_ctx *ctx) {
  if (!ctx) return MSNAP_EINVAL;
  return ctx->grid_ready ? ctx->grid_seg : 0;
}

static int grid_solve_args(const msnap_ctx *ctx, int n_drones, int n_seg, const void *wp, const void *coef,
                           const void *dur, const void *status) {
  if (!ctx || n_drones < 0) return MSNAP_EINVAL;
  if (!ctx->grid_ready) return MSNAP_ENOGRID;
  if (n_seg != ctx->grid_seg) return MSNAP_ESEGMENTS;      // the caller's buffers are sized for another grid
  if (n_drones == 0) return kNoWork;
  return (!wp || !coef || !dur || !status) ? MSNAP_EINVAL : MSNAP_OK;
}

int msnap_solve_grid_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, double *coef, double *dur,
                            int32_t *status) {
  MSNAP_ENTER(ctx, grid_solve_args(ctx, n_drones, n_seg, wp, coef, dur, status));
  return launch_solve_grid(ctx, n_drones, wp, coef, dur, status);
}

int msnap_solve_grid(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, double *coef, double *dur,
                     int32_t *status) {
  MSNAP_ENTER(ctx, grid_solve_args(ctx, n_drones, n_seg, wp, coef, dur, status));
  return solve_host(ctx, n_drones, ctx->grid_seg, wp, nullptr, 1, /*use_grid=*/true, coef, dur, status);
}

// ------------------------------------------------------------------ pack
int msnap_pack_pol_matrix_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef,
                                 const double *dur, float *out) {
  MSNAP_ENTER(ctx, batch_args(ctx, n_drones, n_seg, {coef, dur, out}));
  return launch_pack(ctx, n_drones, n_seg, coef, dur, out);
}

int msnap_pack_pol_matrix(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef,
                          const double *dur, float *out) {
  MSNAP_ENTER(ctx, batch_args(ctx, n_drones, n_seg, {coef, dur, out}));
  const size_t b_out = (size_t)n_drones * n_seg * (1 + 4 * (ctx->order + 1)) * 4;
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      download(out, b_out)},
                [&](const DevPtr *d) { return launch_pack(ctx, n_drones, n_seg, d[0], d[1], d[2]); });
}

// ------------------------------------------------------------------ formation transform
static int transform_args(const msnap_ctx *ctx, int n_poses, int n_offsets, const void *rb_pose, const void *offsets,
                          const void *out) {
  if (!ctx || n_poses < 0 || n_offsets < 0) return MSNAP_EINVAL;
  if (n_poses == 0 || n_offsets == 0) return kNoWork;
  return (!rb_pose || !offsets || !out) ? MSNAP_EINVAL : MSNAP_OK;
}

int msnap_formation_transform_device(msnap_ctx *ctx, int n_poses, int n_offsets, const double *rb_pose,
                                     const double *offsets, double *out) {
  MSNAP_ENTER(ctx, transform_args(ctx, n_poses, n_offsets, rb_pose, offsets, out));
  return launch_formation_transform(ctx, n_poses, n_offsets, rb_pose, offsets, out);
}

int msnap_formation_transform(msnap_ctx *ctx, int n_poses, int n_offsets, const double *rb_pose,
                              const double *offsets, double *out) {
  MSNAP_ENTER(ctx, transform_args(ctx, n_poses, n_offsets, rb_pose, offsets, out));
  return staged(ctx, {upload(rb_pose, (size_t)n_poses * 7 * 8), upload(offsets, (size_t)n_offsets * 3 * 8),
                      download(out, (size_t)n_offsets * n_poses * 7 * 8)},
                [&](const DevPtr *d) { return launch_formation_transform(ctx, n_poses, n_offsets, d[0], d[1], d[2]); });
}

// ------------------------------------------------------------------ sampler
static int sample_args_ok(const msnap_ctx *ctx, int n_drones, int n_samples, int n_axes, double dt) {
  if (!ctx || n_drones < 0 || n_samples < 0) return 0;
  if (n_axes != 3 && n_axes != 4) return 0;
  if (!(dt >= 0.0)) return 0;
  return 1;
}

static int sample_args(const msnap_ctx *ctx, int n_drones, int n_seg, const void *coef, const void *dur, double dt,
                       int n_samples, int n_axes, const void *pos) {
  if (!sample_args_ok(ctx, n_drones, n_samples, n_axes, dt)) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, n_seg)) return rc;
  if (n_drones == 0 || n_samples == 0) return kNoWork;
  return (!coef || !dur || !pos) ? MSNAP_EINVAL : MSNAP_OK;
}

int msnap_sample_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                        double dt, int n_samples, int n_axes, double *pos) {
  MSNAP_ENTER(ctx, sample_args(ctx, n_drones, n_seg, coef, dur, dt, n_samples, n_axes, pos));
  return launch_sample(ctx, n_drones, n_seg, coef, dur, dt, n_samples, n_axes, pos, nullptr, false);
}

size_t msnap_collide_rows_t_doubles(int n_rows, int n_samples) {
  if (n_rows <= 0 || n_samples <= 0) return 0;
  return ((size_t)n_rows + kRowBlock - 1) / kRowBlock * kRowBlock * (size_t)n_samples * 3;
}

int msnap_formation_collide_reads_rows_t(const msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples) {
  (void)row_offset;
  if (!ctx || n_rows <= 0 || n_cols <= 0 || n_samples < 6) return 0;      // (paths shorter than one sample chunk: plain loops)
  return 1;
}

int msnap_formation_collide_takes_broad_phase(const msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples) {
  if (!ctx || n_rows <= 0 || n_cols <= 0 || n_samples < 1 || row_offset < 0) return 0;
  return formation_collide_takes_broad_phase(ctx, n_rows, row_offset, n_cols, n_samples, ctx->collide_no_sym) ? 1 : 0;
}

int msnap_formation_whole_pass_pays(msnap_ctx *ctx, int n_drones, int n_ranks, int *pays) {
  if (!ctx || !pays || n_drones < 0 || n_ranks < 1) return MSNAP_EINVAL;
  *pays = 0;
  long evaluated = -1, shares = 0, groups = 0;
  int rc = msnap_get_option(ctx, "collide_last_pairs_evaluated", &evaluated);
  if (rc) return rc;
  if (evaluated < 0 || n_drones < 2) return MSNAP_OK;      // the last pass evaluated all pairs: the parts divide them
  // (what the NEXT whole passes of this swarm evaluate: the evaluator follows these counts from then on)
  if ((rc = msnap_get_option(ctx, "collide_last_survivors", &shares)) || (rc = msnap_get_option(ctx, "collide_last_group_pairs", &groups)))
    return rc;
  evaluated = collide_counts_by_groups(ctx, ctx->collide_last_n, (int)shares, (int)groups) ? groups * 64 : shares * 1024;
  // whole pass on every rank: the sort / bound / select launches + the surviving pairs at about 2/3 of the all-pairs
  // kernel's pace; parts: 1 / n_ranks of all pairs + transposition, merge, fold and the second collective -- the fixed
  // costs of the two sides are about equal (measured at 4096 drones), which leaves the arithmetic
  const double all_pairs = 0.5 * (double)n_drones * (double)(n_drones - 1);
  *pays = ((double)evaluated / all_pairs) * 1.5 * (double)n_ranks < 1.0 ? 1 : 0;
  return MSNAP_OK;
}

// What the pass over these drones as a whole swarm will read from the sampler's second output, put on record for that
// pass: behind the broad phase the boxes and sort keys (true: the sampler has the samples in LDS; the pass then needs
// no key launch), otherwise the transposed row image (false) -- paired with the positions `pos` they were computed
// from.  A buffer seen before keeps its slot.
static bool record_handover(msnap_ctx *ctx, const double *pos, const double *pos_t, int n_drones, int n_samples) {
  const bool keys = formation_collide_takes_broad_phase(ctx, n_drones, 0, n_drones, n_samples, ctx->collide_no_sym);
  msnap_ctx::Handover *rec = nullptr;
  for (auto &h : ctx->handover)
    if (h.ptr == (const void *)pos_t) rec = &h;
  if (!rec) rec = &ctx->handover[ctx->handover_next++ % 8];
  *rec = {pos_t, pos, n_drones, n_samples, keys ? 2 : 1};
  return keys;
}

int msnap_sample_collide_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                double dt, int n_samples, double *pos, double *pos_t) {
  const int rc = sample_args(ctx, n_drones, n_seg, coef, dur, dt, n_samples, 3, pos);
  MSNAP_ENTER(ctx, rc == MSNAP_OK && !pos_t ? MSNAP_EINVAL : rc);
  const bool keys = record_handover(ctx, pos, pos_t, n_drones, n_samples);
  return launch_sample(ctx, n_drones, n_seg, coef, dur, dt, n_samples, 3, pos, pos_t, keys);
}

int msnap_solve_grid_sample_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *wp, double dt, int n_samples,
                                   double *coef, double *dur, int32_t *status, double *pos, double *pos_t) {
  if (!sample_args_ok(ctx, n_drones, n_samples, 3, dt)) return MSNAP_EINVAL;
  if (!ctx->grid_ready) return MSNAP_ENOGRID;
  if (n_seg != ctx->grid_seg) return MSNAP_ESEGMENTS;
  if (n_drones == 0) return MSNAP_OK;
  if (!wp || !coef || !dur || !status) return MSNAP_EINVAL;
  MSNAP_HIP(ctx, hipSetDevice(ctx->device));
  if (n_samples == 0) return launch_solve_grid(ctx, n_drones, wp, coef, dur, status);
  if (!pos) return MSNAP_EINVAL;
  const bool keys = pos_t && record_handover(ctx, pos, pos_t, n_drones, n_samples);
  return launch_grid_sample(ctx, n_drones, wp, dt, n_samples, coef, dur, status, pos, pos_t, keys);
}

int msnap_sample(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, double dt,
                 int n_samples, int n_axes, double *pos) {
  MSNAP_ENTER(ctx, sample_args(ctx, n_drones, n_seg, coef, dur, dt, n_samples, n_axes, pos));
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      download(pos, (size_t)n_drones * n_samples * n_axes * 8)},
                [&](const DevPtr *d) {
                  return launch_sample(ctx, n_drones, n_seg, d[0], d[1], dt, n_samples, n_axes, d[2], nullptr, false);
                });
}

// ------------------------------------------------------------------ flatness evaluator
static int eval_flat_args(const msnap_ctx *ctx, int n_drones, int n_seg, const void *coef, const void *dur,
                          int n_samples, const void *ts, const void *out) {
  if (!ctx || n_drones < 0 || n_samples < 0) return MSNAP_EINVAL;
  if (int rc = check_seg(ctx, n_seg)) return rc;
  if (n_drones == 0 || n_samples == 0) return kNoWork;
  return (!coef || !dur || !ts || !out) ? MSNAP_EINVAL : MSNAP_OK;
}

int msnap_eval_flat_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                           int n_samples, const double *ts, double *out) {
  MSNAP_ENTER(ctx, eval_flat_args(ctx, n_drones, n_seg, coef, dur, n_samples, ts, out));
  return launch_eval_flat(ctx, n_drones, n_seg, coef, dur, n_samples, ts, out);
}

int msnap_eval_flat(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                    int n_samples, const double *ts, double *out) {
  MSNAP_ENTER(ctx, eval_flat_args(ctx, n_drones, n_seg, coef, dur, n_samples, ts, out));
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      upload(ts, (size_t)n_samples * 8), download(out, (size_t)n_drones * n_samples * 13 * 8)},
                [&](const DevPtr *d) { return launch_eval_flat(ctx, n_drones, n_seg, d[0], d[1], n_samples, d[2], d[3]); });
}

// ------------------------------------------------------------------ snap cost
int msnap_snap_cost_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                           double *cost) {
  MSNAP_ENTER(ctx, batch_args(ctx, n_drones, n_seg, {coef, dur, cost}));
  return launch_snap_cost(ctx, n_drones, n_seg, coef, dur, cost);
}

int msnap_snap_cost(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, double *cost) {
  MSNAP_ENTER(ctx, batch_args(ctx, n_drones, n_seg, {coef, dur, cost}));
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      download(cost, (size_t)n_drones * 4 * 8)},
                [&](const DevPtr *d) { return launch_snap_cost(ctx, n_drones, n_seg, d[0], d[1], d[2]); });
}

// ------------------------------------------------------------------ formation collide
static int collide_args(const msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples,
                        const void *pos_rows, const void *pos_cols, double radius, const void *min_dist,
                        const void *partner, const void *hit) {
  if (!ctx || n_rows < 0 || n_cols < 0 || n_samples < 1 || row_offset < 0 || !(radius >= 0.0)) return MSNAP_EINVAL;
  if (n_rows == 0) return kNoWork;
  return (!pos_rows || (n_cols > 0 && !pos_cols) || !min_dist || !partner || !hit) ? MSNAP_EINVAL : MSNAP_OK;
}

int msnap_formation_collide_device(msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples,
                                   const double *pos_rows, const double *pos_cols, double radius,
                                   double *min_dist, int32_t *partner, int32_t *hit) {
  MSNAP_ENTER(ctx, collide_args(ctx, n_rows, row_offset, n_cols, n_samples, pos_rows, pos_cols, radius, min_dist,
                                partner, hit));
  return launch_formation_collide(ctx, n_rows, row_offset, n_cols, n_samples, pos_rows, pos_cols, radius,
                                  min_dist, partner, hit, nullptr, ctx->collide_no_sym);
}

int msnap_formation_collide_t_device(msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples,
                                     const double *pos_rows_t, const double *pos_rows, const double *pos_cols,
                                     double radius, double *min_dist, int32_t *partner, int32_t *hit) {
  const int rc = collide_args(ctx, n_rows, row_offset, n_cols, n_samples, pos_rows, pos_cols, radius, min_dist,
                              partner, hit);
  MSNAP_ENTER(ctx, rc == MSNAP_OK && !pos_rows_t ? MSNAP_EINVAL : rc);
  return launch_formation_collide(ctx, n_rows, row_offset, n_cols, n_samples, pos_rows, pos_cols, radius,
                                  min_dist, partner, hit, pos_rows_t, ctx->collide_no_sym);
}

int msnap_formation_collide(msnap_ctx *ctx, int n_rows, int row_offset, int n_cols, int n_samples,
                            const double *pos_rows, const double *pos_cols, double radius, double *min_dist,
                            int32_t *partner, int32_t *hit) {
  MSNAP_ENTER(ctx, collide_args(ctx, n_rows, row_offset, n_cols, n_samples, pos_rows, pos_cols, radius, min_dist,
                                partner, hit));
  const size_t E = (size_t)n_samples * 3, b_rows = (size_t)n_rows * E * 8, R = n_rows;
  // The once-per-pair evaluation credits column-side minima to the ROW drones, which is only right when
  // pos_rows is the slice [row_offset, row_offset + n_rows) of pos_cols.  Host arrays can be compared: a
  // caller whose rows are some other set of drones gets the one-sided evaluation instead of wrong partners.
  const bool no_sym = ctx->collide_no_sym ||
                      ((long long)row_offset + n_rows <= n_cols && pos_rows != pos_cols + row_offset * E &&
                       memcmp(pos_rows, pos_cols + row_offset * E, b_rows) != 0);
  return staged(ctx, {upload(pos_rows, b_rows), upload(pos_cols, (size_t)n_cols * E * 8), download(min_dist, R * 8),
                      download(partner, R * 4), download(hit, R * 4)},
                [&](const DevPtr *d) {
                  return launch_formation_collide(ctx, n_rows, row_offset, n_cols, n_samples, d[0], d[1], radius, d[2],
                                                  d[3], d[4], nullptr, no_sym);
                });
}

// ------------------------------------------------------------------ formation pass in parts (one per rank)
size_t msnap_formation_part_bytes(int n_drones) {
  if (n_drones < 0) return 0;
  return ((size_t)n_drones * (sizeof(double) + sizeof(int32_t)) + 7) & ~(size_t)7;
}

// (`device`: the parts are device memory, read as doubles: 8-byte aligned)
static int part_args(const msnap_ctx *ctx, int n_drones, int n_samples, const void *pos_all, int part, int n_parts,
                     const void *part_out, bool device) {
  if (!ctx || n_drones < 0 || n_samples < 1 || n_parts < 1 || part < 0 || part >= n_parts) return MSNAP_EINVAL;
  if (n_drones == 0) return kNoWork;
  return (!pos_all || !part_out || (device && ((uintptr_t)part_out & 7))) ? MSNAP_EINVAL : MSNAP_OK;
}

static int finish_args(const msnap_ctx *ctx, int n_drones, int n_parts, const void *parts, int row_offset, int n_rows,
                       double radius, const void *min_dist, const void *partner, const void *hit, bool device) {
  if (!ctx || n_drones < 0 || n_parts < 1 || row_offset < 0 || n_rows < 0 || !(radius >= 0.0)) return MSNAP_EINVAL;
  if ((long long)row_offset + n_rows > n_drones) return MSNAP_EINVAL;
  if (n_rows == 0) return kNoWork;
  return (!parts || !min_dist || !partner || !hit || (device && ((uintptr_t)parts & 7))) ? MSNAP_EINVAL : MSNAP_OK;
}

int msnap_formation_collide_part_device(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos_all, int part,
                                        int n_parts, void *part_out) {
  MSNAP_ENTER(ctx, part_args(ctx, n_drones, n_samples, pos_all, part, n_parts, part_out, true));
  return launch_formation_collide_part(ctx, n_drones, n_samples, pos_all, part, n_parts, (double *)part_out,
                                       (int32_t *)((unsigned char *)part_out + (size_t)n_drones * sizeof(double)));
}

int msnap_formation_collide_finish_device(msnap_ctx *ctx, int n_drones, int n_parts, const void *parts, int row_offset,
                                          int n_rows, double radius, double *min_dist, int32_t *partner, int32_t *hit) {
  MSNAP_ENTER(ctx, finish_args(ctx, n_drones, n_parts, parts, row_offset, n_rows, radius, min_dist, partner, hit, true));
  return launch_formation_collide_finish(ctx, n_drones, n_parts, parts, msnap_formation_part_bytes(n_drones),
                                         row_offset, n_rows, radius, min_dist, partner, hit);
}

int msnap_formation_collide_part(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos_all, int part,
                                 int n_parts, void *part_out) {
  MSNAP_ENTER(ctx, part_args(ctx, n_drones, n_samples, pos_all, part, n_parts, part_out, false));
  return staged(ctx, {upload(pos_all, (size_t)n_drones * n_samples * 3 * 8),
                      download(part_out, msnap_formation_part_bytes(n_drones))},
                [&](const DevPtr *d) {
                  return msnap_formation_collide_part_device(ctx, n_drones, n_samples, d[0], part, n_parts, d[1]);
                });
}

int msnap_formation_collide_finish(msnap_ctx *ctx, int n_drones, int n_parts, const void *parts, int row_offset,
                                   int n_rows, double radius, double *min_dist, int32_t *partner, int32_t *hit) {
  MSNAP_ENTER(ctx, finish_args(ctx, n_drones, n_parts, parts, row_offset, n_rows, radius, min_dist, partner, hit, false));
  const size_t R = n_rows;
  return staged(ctx, {upload(parts, msnap_formation_part_bytes(n_drones) * (size_t)n_parts), download(min_dist, R * 8),
                      download(partner, R * 4), download(hit, R * 4)},
                [&](const DevPtr *d) {
                  return msnap_formation_collide_finish_device(ctx, n_drones, n_parts, d[0], row_offset, n_rows, radius,
                                                               d[1], d[2], d[3]);
                });
}

// ------------------------------------------------------------------ mesh sweep
static int sweep_args(const msnap_ctx *ctx, int n_drones, int n_samples, const void *pos, int n_tris, const void *tris,
                      double radius, const void *min_dist, const void *hit) {
  if (!ctx || n_drones < 0 || n_samples < 1 || n_tris < 0 || !(radius >= 0.0)) return MSNAP_EINVAL;
  if (n_drones == 0) return kNoWork;
  return (!pos || (n_tris > 0 && !tris) || !min_dist || !hit) ? MSNAP_EINVAL : MSNAP_OK;
}

int msnap_mesh_sweep_device(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos, int n_tris,
                            const double *tris, double radius, double *min_dist, int32_t *hit) {
  MSNAP_ENTER(ctx, sweep_args(ctx, n_drones, n_samples, pos, n_tris, tris, radius, min_dist, hit));
  return launch_mesh_sweep(ctx, n_drones, n_samples, pos, n_tris, tris, radius, min_dist, hit);
}

int msnap_mesh_sweep(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos, int n_tris,
                     const double *tris, double radius, double *min_dist, int32_t *hit) {
  MSNAP_ENTER(ctx, sweep_args(ctx, n_drones, n_samples, pos, n_tris, tris, radius, min_dist, hit));
  return staged(ctx, {upload(pos, (size_t)n_drones * n_samples * 3 * 8), upload(tris, (size_t)n_tris * 9 * 8),
                      download(min_dist, (size_t)n_drones * 8), download(hit, (size_t)n_drones * 4)},
                [&](const DevPtr *d) {
                  return launch_mesh_sweep(ctx, n_drones, n_samples, d[0], n_tris, d[1], radius, d[2], d[3]);
                });
}

// ------------------------------------------------------------------ mesh-vs-mesh validity
static int validity_args(const msnap_ctx *ctx, int n_states, const void *states, int n_rtris, const void *rtris,
                         int n_etris, const void *etris, const void *valid) {
  if (!ctx || n_states < 0 || n_rtris < 0 || n_etris < 0) return MSNAP_EINVAL;
  if (n_states == 0) return kNoWork;
  return (!states || !valid || (n_rtris > 0 && !rtris) || (n_etris > 0 && !etris)) ? MSNAP_EINVAL : MSNAP_OK;
}

int msnap_mesh_validity_device(msnap_ctx *ctx, int n_states, const double *states, int n_rtris, const double *rtris,
                               int n_etris, const double *etris, int32_t *valid) {
  MSNAP_ENTER(ctx, validity_args(ctx, n_states, states, n_rtris, rtris, n_etris, etris, valid));
  return launch_mesh_validity(ctx, n_states, states, n_rtris, rtris, n_etris, etris, valid);
}

int msnap_mesh_validity(msnap_ctx *ctx, int n_states, const double *states, int n_rtris, const double *rtris,
                        int n_etris, const double *etris, int32_t *valid) {
  MSNAP_ENTER(ctx, validity_args(ctx, n_states, states, n_rtris, rtris, n_etris, etris, valid));
  return staged(ctx, {upload(states, (size_t)n_states * 4 * 8), upload(rtris, (size_t)n_rtris * 9 * 8),
                      upload(etris, (size_t)n_etris * 9 * 8), download(valid, (size_t)n_states * 4)},
                [&](const DevPtr *d) { return launch_mesh_validity(ctx, n_states, d[0], n_rtris, d[1], n_etris, d[2], d[3]); });
}

// ------------------------------------------------------------------ dynamic limits (msnap_limits.hip)
// `limits_rc`: check_limits of a retiming (limits is a host array in both versions), which comes after the shape and
// before an empty batch returns
static int limits_args(const msnap_ctx *ctx, int n_drones, int n_seg, std::initializer_list<const void *> ptrs,
                       int limits_rc = MSNAP_OK) {
  if (int rc = check_limits_args(ctx, n_drones, n_seg)) return rc;
  if (limits_rc) return limits_rc;
  if (n_drones == 0) return kNoWork;
  return all_required(ptrs);
}

int msnap_dynamic_peaks_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                               double *peak, double *t_peak, int32_t *status) {
  MSNAP_ENTER(ctx, limits_args(ctx, n_drones, n_seg, {coef, dur, peak, t_peak, status}));
  const int rc = ensure(ctx, ctx->limits_work, lane_doubles(n_drones, n_seg) * sizeof(double));
  if (rc) return rc;
  return launch_peaks(ctx, n_drones, n_seg, coef, dur, (double *)ctx->limits_work.p, peak, t_peak, status);
}

int msnap_dynamic_peaks(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, double *peak,
                        double *t_peak, int32_t *status) {
  MSNAP_ENTER(ctx, limits_args(ctx, n_drones, n_seg, {coef, dur, peak, t_peak, status}));
  const size_t b_pk = (size_t)n_drones * 4 * 8;
  return staged(ctx, {upload(coef, coef_bytes(ctx, n_drones, n_seg)), upload(dur, dur_bytes(n_drones, n_seg)),
                      download(peak, b_pk), download(t_peak, b_pk), download(status, (size_t)n_drones * 4)},
                [&](const DevPtr *d) {
                  return msnap_dynamic_peaks_device(ctx, n_drones, n_seg, d[0], d[1], d[2], d[3], d[4]);
                });
}

int msnap_time_scale_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                            const double *scale, double *coef_out, double *dur_out) {
  MSNAP_ENTER(ctx, limits_args(ctx, n_drones, n_seg, {coef, dur, scale, coef_out, dur_out}));
  return launch_time_scale(ctx, n_drones, n_seg, coef, dur, scale, coef_out, dur_out);
}

// (the host versions stage coef and dur once and scale them in place)
int msnap_time_scale(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                     const double *scale, double *coef_out, double *dur_out) {
  MSNAP_ENTER(ctx, limits_args(ctx, n_drones, n_seg, {coef, dur, scale, coef_out, dur_out}));
  return staged(ctx, {{coef, coef_out, coef_bytes(ctx, n_drones, n_seg)}, {dur, dur_out, dur_bytes(n_drones, n_seg)},
                      upload(scale, (size_t)n_drones * 8)},
                [&](const DevPtr *d) { return launch_time_scale(ctx, n_drones, n_seg, d[0], d[1], d[2], d[0], d[1]); });
}

int msnap_retime_to_limits_device(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                                  const double limits[4], int flags, double *coef_out, double *dur_out,
                                  double *scale) {
  MSNAP_ENTER(ctx, limits_args(ctx, n_drones, n_seg, {coef, dur, coef_out, dur_out, scale}, check_limits(limits, flags)));
  return launch_retime(ctx, n_drones, n_seg, coef, dur, limits, flags, coef_out, dur_out, scale);
}

int msnap_retime_to_limits(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                           const double limits[4], int flags, double *coef_out, double *dur_out, double *scale) {
  MSNAP_ENTER(ctx, limits_args(ctx, n_drones, n_seg, {coef, dur, coef_out, dur_out, scale}, check_limits(limits, flags)));
  return staged(ctx, {{coef, coef_out, coef_bytes(ctx, n_drones, n_seg)}, {dur, dur_out, dur_bytes(n_drones, n_seg)},
                      download(scale, (size_t)n_drones * 8)},
                [&](const DevPtr *d) {
                  return launch_retime(ctx, n_drones, n_seg, d[0], d[1], limits, flags, d[0], d[1], d[2]);
                });
}

}  // extern "C"
