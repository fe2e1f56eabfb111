// The small kernels either side of the solve: the float32 pol-matrix pack (a7), the
// formation transform (a8), the flatness evaluator (f1), the snap cost and its
// gradient, the mesh sweep and the mesh validity test.  The sampler is
// msnap_sample.hip, the pairwise pass msnap_collide.hip.  gfx950, wave64.
#include <math.h>

#include <cstdlib>

#include "msnap_internal.h"
#include "msnap_energy.h"
#include "msnap_tri.h"
#include "msnap_wave.h"

namespace msnap {

// ------------------------------------------------------------------------------------
// a7: matrix[M][1 + 4*ncoef] float32 = [T | x | y | z | yaw]
// (reference scripts/drones_pols_generator.py:63-77)
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
pack_kernel(const double *__restrict__ coef, const double *__restrict__ dur, float *__restrict__ out,
            size_t n_rows /* N*M */, int nc) {
  const int ncol = 1 + 4 * nc;
  const size_t total = n_rows * (size_t)ncol;
  uniform_for<size_t>(threadIdx.x, total, (size_t)gridDim.x * blockDim.x, [&](size_t idx) {
    const size_t row = idx / ncol;
    const int col = (int)(idx - row * ncol);
    const double v = (col == 0) ? dur[row] : coef[row * (size_t)(4 * nc) + (col - 1)];
    out[idx] = (float)v;
  }, (size_t)blockIdx.x * blockDim.x);
}

int launch_pack(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, float *out) {
  const size_t rows = (size_t)n_drones * n_seg;
  const int nc = ctx->order + 1;
  const size_t total = rows * (1 + 4 * nc);
  size_t blocks = (total + 255) / 256;
  if (blocks > (size_t)ctx->n_cu * 8) blocks = (size_t)ctx->n_cu * 8;
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, coef, dur, out, rows, nc);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

// ------------------------------------------------------------------------------------
// a8: p' = R(q_rb) p_k + t_rb ;  q' = quaternion of R(q_rb)
// (reference scripts/drones_traj_generator.py:67-82 through tf2_geometry_msgs
// do_transform_pose -> PyKDL Frame product; KDL is not vendored in the
// reference: Rotation::Quaternion / Rotation::GetQuaternion restated from the
// published orocos_kdl frames.cpp.  The drone poses carry identity orientation,
// drones_traj_generator.py:31,38.)
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
formation_kernel(const double *__restrict__ rb, const double *__restrict__ off, double *__restrict__ out,
                 int P, int Kn) {
#pragma clang fp contract(off)
  // A wave's 64 (offset, pose) items own 448 CONSECUTIVE output doubles; written per lane they would be
  // seven 8-B stores at a 56-B stride.  Through a per-wave LDS image (stride 7 is odd: conflict-free both
  // ways) they leave as seven stores of 512 contiguous bytes.
  __shared__ double image[4][kWave * 7];
  const int lane = threadIdx.x & (kWave - 1);
  double *img = image[threadIdx.x / kWave];
  const size_t total = (size_t)P * Kn;
  const size_t span = (size_t)gridDim.x * blockDim.x;
  const size_t trips = (total + span - 1) / span;      // the same for every wave: no partly exited wave below
  for (size_t trip = 0; trip < trips; ++trip) {
    const size_t wave_base = trip * span + (size_t)blockIdx.x * blockDim.x + (threadIdx.x - lane);
    const size_t idx = wave_base + lane;
    if (idx < total) {
    const int k = (int)(idx / P);
    const int p = (int)(idx - (size_t)k * P);
    const double *r = rb + (size_t)p * 7;
    const double tx = r[0], ty = r[1], tz = r[2];
    const double x = r[3], y = r[4], z = r[5], w = r[6];
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const double m00 = w2 + x2 - y2 - z2, m01 = 2 * x * y - 2 * w * z, m02 = 2 * x * z + 2 * w * y;
    const double m10 = 2 * x * y + 2 * w * z, m11 = w2 - x2 + y2 - z2, m12 = 2 * y * z - 2 * w * x;
    const double m20 = 2 * x * z - 2 * w * y, m21 = 2 * y * z + 2 * w * x, m22 = w2 - x2 - y2 + z2;
    const double ox = off[k * 3 + 0], oy = off[k * 3 + 1], oz = off[k * 3 + 2];
    double *o = img + lane * 7;
    o[0] = m00 * ox + m01 * oy + m02 * oz + tx;
    o[1] = m10 * ox + m11 * oy + m12 * oz + ty;
    o[2] = m20 * ox + m21 * oy + m22 * oz + tz;
    // Rotation::GetQuaternion
    const double trace = m00 + m11 + m22;
    double qx, qy, qz, qw;
    if (trace > 1e-12) {
      const double s = 0.5 / sqrt(trace + 1.0);
      qw = 0.25 / s;
      qx = (m21 - m12) * s;
      qy = (m02 - m20) * s;
      qz = (m10 - m01) * s;
    } else if (m00 > m11 && m00 > m22) {
      const double s = 2.0 * sqrt(1.0 + m00 - m11 - m22);
      qw = (m21 - m12) / s;
      qx = 0.25 * s;
      qy = (m01 + m10) / s;
      qz = (m02 + m20) / s;
    } else if (m11 > m22) {
      const double s = 2.0 * sqrt(1.0 + m11 - m00 - m22);
      qw = (m02 - m20) / s;
      qx = (m01 + m10) / s;
      qy = 0.25 * s;
      qz = (m12 + m21) / s;
    } else {
      const double s = 2.0 * sqrt(1.0 + m22 - m00 - m11);
      qw = (m10 - m01) / s;
      qx = (m02 + m20) / s;
      qy = (m12 + m21) / s;
      qz = 0.25 * s;
    }
    o[3] = qx;
    o[4] = qy;
    o[5] = qz;
    o[6] = qw;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    const size_t ebase = wave_base * 7, nelem = total * 7;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const int e = j * kWave + lane;
      if (ebase + e < nelem) out[ebase + e] = img[e];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
  }
}

int launch_formation_transform(msnap_ctx *ctx, int n_poses, int n_offsets, const double *rb_pose,
                               const double *offsets, double *out) {
  const size_t total = (size_t)n_poses * n_offsets;
  size_t blocks = (total + 255) / 256;
  if (blocks > (size_t)ctx->n_cu * 8) blocks = (size_t)ctx->n_cu * 8;
  hipLaunchKernelGGL(formation_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, rb_pose, offsets,
                     out, n_poses, n_offsets);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

// ------------------------------------------------------------------------------------
// f1: Trajectory.eval / Polynomial4D.eval -- differential-flatness outputs
// (reference src/optimizations/uav_trajectory.py:64-85 and :119-127: piece lookup with
// '<=', derivative polynomials built as (i+1)*p[i+1], Horner with separate multiply and
// add, thrust = acc + (0,0,9.81), body axes from yaw, omega from the jerk).
//   out[d][s] = pos[3] vel[3] acc[3] omega[3] yaw ; NaN when t is outside [0, duration]
// ------------------------------------------------------------------------------------
template <int NC>
__device__ __forceinline__ void horner_derivs(const double *__restrict__ c, double t, double &p0, double &p1,
                                              double &p2, double &p3) {
#pragma clang fp contract(off)
  double d0[NC], d1[NC], d2[NC], d3[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i) d0[i] = c[i];
#pragma unroll
  for (int i = 0; i < NC - 1; ++i) d1[i] = (double)(i + 1) * d0[i + 1];
#pragma unroll
  for (int i = 0; i < NC - 2; ++i) d2[i] = (double)(i + 1) * d1[i + 1];
#pragma unroll
  for (int i = 0; i < NC - 3; ++i) d3[i] = (double)(i + 1) * d2[i + 1];
  p0 = p1 = p2 = p3 = 0.0;
#pragma unroll
  for (int i = NC - 1; i >= 0; --i) p0 = p0 * t + d0[i];
#pragma unroll
  for (int i = NC - 2; i >= 0; --i) p1 = p1 * t + d1[i];
#pragma unroll
  for (int i = NC - 3; i >= 0; --i) p2 = p2 * t + d2[i];
#pragma unroll
  for (int i = NC - 4; i >= 0; --i) p3 = p3 * t + d3[i];
}

template <int NC>
__global__ void __launch_bounds__(256)
flat_eval_kernel(const double *__restrict__ coef, const double *__restrict__ dur, const double *__restrict__ ts,
                 int N, int M, int S, double *__restrict__ out) {
#pragma clang fp contract(off)
  // A workgroup's 256 (drone, instant) items own 256 * 13 CONSECUTIVE output doubles: they go through an LDS
  // image (stride 13 is odd: conflict-free) and leave as contiguous 8-byte-per-lane runs instead of 13 stores
  // at a 104-byte stride per lane.
  __shared__ double image[256 * 13];
  const size_t total = (size_t)N * S;
  const size_t span = (size_t)gridDim.x * blockDim.x;
  const size_t trips = (total + span - 1) / span;      // the same for every thread: the barriers below are uniform
  for (size_t trip = 0; trip < trips; ++trip) {
    const size_t block_base = trip * span + (size_t)blockIdx.x * blockDim.x;
    const size_t idx = block_base + threadIdx.x;
    double *o = image + threadIdx.x * 13;
    if (idx < total) {
    const int d = (int)(idx / S);
    const int s = (int)(idx - (size_t)d * S);
    const double t = ts[s];
    const double *dr = dur + (size_t)d * M;
    double acc_t = 0.0;
    int seg = -1;
    for (int i = 0; i < M; ++i) {
      const double Ti = dr[i];
      if (seg < 0) {
        if (t <= acc_t + Ti) seg = i;
        else acc_t = acc_t + Ti;
      }
    }
    if (!(t >= 0.0) || seg < 0) {
#pragma unroll
      for (int q = 0; q < 13; ++q) o[q] = __builtin_nan("");
    } else {
    const double tl = t - acc_t;
    const double *c = coef + ((size_t)d * M + seg) * 4 * NC;
    double px, vx, ax, jx, py, vy, ay, jy, pz, vz, az, jz, yaw, dyaw, q2, q3;
    horner_derivs<NC>(c + 0 * NC, tl, px, vx, ax, jx);
    horner_derivs<NC>(c + 1 * NC, tl, py, vy, ay, jy);
    horner_derivs<NC>(c + 2 * NC, tl, pz, vz, az, jz);
    horner_derivs<NC>(c + 3 * NC, tl, yaw, dyaw, q2, q3);
    const double thx = ax + 0.0, thy = ay + 0.0, thz = az + 9.81;
    const double tn = sqrt(thx * thx + thy * thy + thz * thz);
    const double zbx = thx / tn, zby = thy / tn, zbz = thz / tn;
    const double xwx = cos(yaw), xwy = sin(yaw), xwz = 0.0;
    // y_body = normalize(z_body x x_world)
    double ybx = zby * xwz - zbz * xwy, yby = zbz * xwx - zbx * xwz, ybz = zbx * xwy - zby * xwx;
    const double yn = sqrt(ybx * ybx + yby * yby + ybz * ybz);
    ybx = ybx / yn; yby = yby / yn; ybz = ybz / yn;
    // x_body = y_body x z_body
    const double xbx = yby * zbz - ybz * zby, xby = ybz * zbx - ybx * zbz, xbz = ybx * zby - yby * zbx;
    const double jd = jx * zbx + jy * zby + jz * zbz;
    const double hx = (jx - jd * zbx) / tn, hy = (jy - jd * zby) / tn, hz = (jz - jd * zbz) / tn;
    o[0] = px; o[1] = py; o[2] = pz;
    o[3] = vx; o[4] = vy; o[5] = vz;
    o[6] = ax; o[7] = ay; o[8] = az;
    o[9] = -(hx * ybx + hy * yby + hz * ybz);
    o[10] = hx * xbx + hy * xby + hz * xbz;
    o[11] = zbz * dyaw;
    o[12] = yaw;
    }
    }
    __syncthreads();
    const size_t ebase = block_base * 13, nelem = total * 13;
#pragma unroll
    for (int j = 0; j < 13; ++j) {
      const size_t e = (size_t)j * blockDim.x + threadIdx.x;
      if (ebase + e < nelem) out[ebase + e] = image[e];
    }
    __syncthreads();
  }
}

int launch_eval_flat(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur,
                     int n_samples, const double *ts, double *out) {
  const size_t total = (size_t)n_drones * n_samples;
  size_t blocks = (total + 255) / 256;
  if (blocks > (size_t)ctx->n_cu * 16) blocks = (size_t)ctx->n_cu * 16;
  if (ctx->order == 7)
    hipLaunchKernelGGL((flat_eval_kernel<8>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, coef, dur, ts,
                       n_drones, n_seg, n_samples, out);
  else
    hipLaunchKernelGGL((flat_eval_kernel<10>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, coef, dur, ts,
                       n_drones, n_seg, n_samples, out);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

// ------------------------------------------------------------------------------------
// Snap cost J = sum_seg int_0^T (p^(k)(t))^2 dt per (drone, axis), k = (order+1)/2: the quantity
// the trajectory minimises (the reference never evaluates it; it is the objective of the QP
// whose KKT system its collocation rows encode).  Monomial Hessian
//   Q[m][n] = m!/(m-k)! * n!/(n-k)! * T^(m+n-2k+1) / (m+n-2k+1),  m, n >= k.
// ------------------------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(256)
snap_cost_kernel(const double *__restrict__ coef, const double *__restrict__ dur, int N, int M,
                 double *__restrict__ cost) {
  constexpr int K = NC / 2;
  const int total = N * 4;
  uniform_for<int>(threadIdx.x, total, gridDim.x * blockDim.x, [&](int idx) {
    const int d = idx >> 2, a = idx & 3;
    double J = 0.0;
    for (int i = 0; i < M; ++i) {
      const double *c = coef + (((size_t)d * M + i) * 4 + a) * NC;
      const double T = dur[(size_t)d * M + i];
      double f[K];                      // f[q] = (k+q)!/q! * c[k+q]
#pragma unroll
      for (int q = 0; q < K; ++q) {
        double ff = 1.0;
#pragma unroll
        for (int r = q + 1; r <= K + q; ++r) ff *= (double)r;
        f[q] = ff * c[K + q];
      }
      double tp[2 * K];                 // T^e, e = 1 .. 2k-1
      tp[0] = 1.0;
#pragma unroll
      for (int e = 1; e < 2 * K; ++e) tp[e] = tp[e - 1] * T;
      double acc = 0.0;
#pragma unroll
      for (int p = 0; p < K; ++p)
#pragma unroll
        for (int q = 0; q < K; ++q) acc += f[p] * f[q] * (tp[p + q + 1] / (double)(p + q + 1));
      J += acc;
    }
    cost[idx] = J;
  }, blockIdx.x * blockDim.x);
}

int launch_snap_cost(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, const double *dur, double *cost) {
  const int total = n_drones * 4;
  int blocks = (total + 255) / 256;
  if (blocks > ctx->n_cu * 8) blocks = ctx->n_cu * 8;
  if (ctx->order == 7)
    hipLaunchKernelGGL((snap_cost_kernel<8>), dim3(blocks), dim3(256), 0, ctx->stream, coef, dur, n_drones, n_seg, cost);
  else
    hipLaunchKernelGGL((snap_cost_kernel<10>), dim3(blocks), dim3(256), 0, ctx->stream, coef, dur, n_drones, n_seg, cost);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

// -E per (drone, segment, axis), E the Ostrogradsky energy of the segment's polynomial at its start (msnap_sweep.h):
// the derivative of the optimal snap cost by the segment's duration when coef is the solve's result.  Streaming: one
// lane per (drone, segment, axis) reads its own coefficients.
template <int NC>
__global__ void __launch_bounds__(256)
snap_cost_grad_kernel(const double *__restrict__ coef, size_t total, double *__restrict__ grad) {
  uniform_for<size_t>(threadIdx.x, total, (size_t)gridDim.x * blockDim.x, [&](size_t idx) {
    double c[NC];
#pragma unroll
    for (int j = 0; j < NC; j += 2) {
      const double2 v = *reinterpret_cast<const double2 *>(coef + idx * NC + j);
      c[j] = v.x;
      c[j + 1] = v.y;
    }
    grad[idx] = -ostrogradsky_energy<NC / 2>(c);
  }, (size_t)blockIdx.x * blockDim.x);
}

int launch_snap_cost_grad(msnap_ctx *ctx, int n_drones, int n_seg, const double *coef, double *grad) {
  const size_t total = (size_t)n_drones * n_seg * 4;
  size_t blocks = (total + 255) / 256;
  if (blocks > (size_t)ctx->n_cu * 16) blocks = (size_t)ctx->n_cu * 16;
  if (ctx->order == 7)
    hipLaunchKernelGGL((snap_cost_grad_kernel<8>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, coef, total, grad);
  else
    hipLaunchKernelGGL((snap_cost_grad_kernel<10>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, coef, total, grad);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

// ------------------------------------------------------------------------------------
// Mesh sweep: min over samples and triangles of the point-triangle distance
// (closest-point regions, Ericson 5.1.5).  One workgroup per drone, one lane per
// sample; the triangle is wave-uniform (scalar loads).  Semantics are this
// repo's; the reference only has a boolean FCL mesh-mesh test in the
// planner (src/RigidBodyPlanners/fcl_checker.py:93-100).  The point-triangle functions are msnap_tri.h.
// ------------------------------------------------------------------------------------
// One workgroup per drone, one lane per sample (ceil(S / 64) waves, at most 16); the triangle under
// test is wave-uniform: its vertices are scalar loads and scalar operands.
// Exact culling per wave.  The squared distance between a triangle's bounding box and the bounding box
// of the wave's stretch of path is a lower bound of every point-triangle distance of that pair, so a
// triangle whose bound is not below the best distance found so far cannot lower the minimum.  Lane t
// of the wave holds the bound of triangle t (groups of 64 triangles); the wave repeatedly takes the
// triangle with the smallest bound, tests it against its 64 samples, and stops the group as soon as the
// smallest remaining bound is not below the best distance: a path far from the scene tests one or
// two triangles, a path through a wall all of the wall's.  min_dist stays the exact minimum over all
// samples and triangles -- a skipped test could only have returned something larger.
__global__ void __launch_bounds__(1024)
mesh_sweep_kernel(const double *__restrict__ pos, int N, int S, const double *__restrict__ tris, int n_tris,
                  double radius, double *__restrict__ min_dist, int32_t *__restrict__ hit,
                  unsigned long long *__restrict__ tests_done) {
  __shared__ double sBest[16];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave, nw = blockDim.x / kWave;
  unsigned long long done = 0;
  // one drone per workgroup, or ("mesh_waves_per_cu") a smaller grid whose workgroups walk the drones: a sweep that
  // runs beside another stream's kernels then leaves them wave slots and registers for as long as it runs
  for (int d = blockIdx.x; d < N; d += gridDim.x) {
  double best = INFINITY;
  for (int s0 = wv * kWave; s0 < S; s0 += nw * kWave) {      // one trip unless S > 1024
    const int s = s0 + lane;
    const double *p = pos + ((size_t)d * S + (s < S ? s : S - 1)) * 3;   // lanes past the end replay the last sample
    const double px = p[0], py = p[1], pz = p[2];
    // the box of the wave's FINITE samples, wave-uniform (non-finite samples never win a minimum, include/msnap.h:
    // they must not distort the cull of the finite ones either; a stretch without a finite coordinate gives a
    // NaN box, whose bound is 0 for every triangle: nothing is culled, nothing can win)
    double lo[3], hi[3];
    const double fx = __builtin_isfinite(px) ? px : __builtin_nan(""), fy = __builtin_isfinite(py) ? py : __builtin_nan(""),
                 fz = __builtin_isfinite(pz) ? pz : __builtin_nan("");
    lo[0] = uniform_f64(wave_minmax_num_f64<false>(fx)); lo[1] = uniform_f64(wave_minmax_num_f64<false>(fy));
    lo[2] = uniform_f64(wave_minmax_num_f64<false>(fz));
    hi[0] = uniform_f64(wave_minmax_num_f64<true>(fx)); hi[1] = uniform_f64(wave_minmax_num_f64<true>(fy));
    hi[2] = uniform_f64(wave_minmax_num_f64<true>(fz));
    double wbest = uniform_f64(wave_min_f64(best));            // wave-uniform bound: min over the lanes so far
    for (int t0 = 0; t0 < n_tris; t0 += kWave) {
      const int tl = t0 + lane;
      double lb = (tl < n_tris) ? box_tri_lb2(lo, hi, tris + (size_t)(tl < n_tris ? tl : 0) * 9) : INFINITY;
      // the triangle with the smallest bound first: it usually sets the distance the others have to beat
      const double m = uniform_f64(wave_min_f64(lb));
      if (!(m < wbest)) continue;                              // (also when the group has no triangle: every bound inf)
      // the group's zero-area triangles, one bit per lane: a scalar, so the choice below is a uniform branch
      const unsigned long long degen = __ballot(tl < n_tris && tri_degenerate(tris + (size_t)(tl < n_tris ? tl : 0) * 9));
      {
        const int sel = __builtin_ctzll(__ballot(lb == m));    // wave-uniform: the ballot is a scalar
        lb = (lane == sel) ? INFINITY : lb;
        const double *tri = tris + (size_t)(t0 + sel) * 9;
        const double v = ((degen >> sel) & 1ULL) ? pt_degenerate_tri_d2(px, py, pz, tri) : pt_tri_d2(px, py, pz, tri);
        best = (v < best) ? v : best;
        wbest = uniform_f64(wave_min_f64(best));
        done += 1;
      }
      // then every triangle whose bound is still below the best distance, in lane order; the best distance (two
      // cross-lane reductions: as long as a third of a triangle's evaluation) is refreshed every fourth triangle only --
      // a superset of what the one-by-one order evaluates, the same minimum
      unsigned long long cand = __ballot(lb < wbest);
      for (int k = 1; cand; ++k) {
        const int sel = __builtin_ctzll(cand);
        cand &= cand - 1;
        const double *tri = tris + (size_t)(t0 + sel) * 9;
        const double v = ((degen >> sel) & 1ULL) ? pt_degenerate_tri_d2(px, py, pz, tri) : pt_tri_d2(px, py, pz, tri);
        best = (v < best) ? v : best;
        done += 1;
        if ((k & 3) == 0 && cand) {
          wbest = uniform_f64(wave_min_f64(best));
          cand &= __ballot(lb < wbest);
        }
      }
      wbest = uniform_f64(wave_min_f64(best));
    }
  }
  best = wave_min_f64(best);
  if (lane == 0) sBest[wv] = best;
  lds_barrier();
  if (threadIdx.x == 0) {
    for (int k = 1; k < nw; ++k) best = (sBest[k] < best) ? sBest[k] : best;
    const double dist = sqrt(best);
    min_dist[d] = dist;
    hit[d] = (dist < radius) ? 1 : 0;
  }
  lds_barrier();      // (sBest is free for the next drone)
  }
  if (tests_done && lane == 0) atomicAdd(tests_done, done * kWave);
}

int launch_mesh_sweep(msnap_ctx *ctx, int n_drones, int n_samples, const double *pos, int n_tris,
                      const double *tris, double radius, double *min_dist, int32_t *hit) {
  int waves = (n_samples + kWave - 1) / kWave;
  if (waves > 16) waves = 16;
  int blocks = n_drones;
  if (ctx->mesh_waves_per_cu > 0) {      // msnap_set_option: room for other streams' workgroups beside the sweep
    const int cap = ctx->n_cu * ctx->mesh_waves_per_cu / waves;
    blocks = blocks < cap ? blocks : (cap > 0 ? cap : 1);
  }
  hipLaunchKernelGGL(mesh_sweep_kernel, dim3(blocks), dim3(waves * kWave), 0, ctx->stream, pos, n_drones,
                     n_samples, tris, n_tris, radius, min_dist, hit, (unsigned long long *)ctx->mesh_tests);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

// ------------------------------------------------------------------------------------
// f4: rigid-body state validity, batched -- the OMPL validity callback of the planner
// (reference src/RigidBodyPlanners/RB_planning_sep_coll_check.py:208-226: the robot mesh
// is placed at (x, y, z) with quaternion_from_euler(0, 0, yaw) and fcl.collide is asked
// whether it touches the environment mesh, src/RigidBodyPlanners/fcl_checker.py:93-100).
// FCL is not vendored in the reference (parity unpinned): the predicate here is "some
// robot triangle and some environment triangle intersect as closed sets", decided by the
// 23-axis separating-axis test (2 face normals, 9 edge x edge, 12 edge x normal for the
// coplanar case: each triangle's edges crossed with both normals, so that a triangle of zero
// area -- whose own normal is zero -- still meets the in-plane axes of its segment).  Complete
// in exact arithmetic for every pair in which at least one triangle has nonzero area; two zero-area triangles on
// one line or in one plane can be reported as touching when they are not (the safe side).
// One wavefront per state, lanes stride the triangle pairs.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ bool sat_separates(const double (&P)[3][3], const double (&Q)[3][3], double lx, double ly,
                                              double lz) {
#pragma clang fp contract(off)
  double p0 = P[0][0] * lx + P[0][1] * ly + P[0][2] * lz;
  double p1 = P[1][0] * lx + P[1][1] * ly + P[1][2] * lz;
  double p2 = P[2][0] * lx + P[2][1] * ly + P[2][2] * lz;
  double q0 = Q[0][0] * lx + Q[0][1] * ly + Q[0][2] * lz;
  double q1 = Q[1][0] * lx + Q[1][1] * ly + Q[1][2] * lz;
  double q2 = Q[2][0] * lx + Q[2][1] * ly + Q[2][2] * lz;
  const double pmin = fmin(p0, fmin(p1, p2)), pmax = fmax(p0, fmax(p1, p2));
  const double qmin = fmin(q0, fmin(q1, q2)), qmax = fmax(q0, fmax(q1, q2));
  return (pmin > qmax) || (pmax < qmin);
}

__device__ __forceinline__ bool tri_tri_intersect(const double (&P)[3][3], const double (&Q)[3][3]) {
#pragma clang fp contract(off)
  double e[3][3], f[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    e[0][c] = P[1][c] - P[0][c]; e[1][c] = P[2][c] - P[1][c]; e[2][c] = P[0][c] - P[2][c];
    f[0][c] = Q[1][c] - Q[0][c]; f[1][c] = Q[2][c] - Q[1][c]; f[2][c] = Q[0][c] - Q[2][c];
  }
  const double n1x = e[0][1] * e[1][2] - e[0][2] * e[1][1];
  const double n1y = e[0][2] * e[1][0] - e[0][0] * e[1][2];
  const double n1z = e[0][0] * e[1][1] - e[0][1] * e[1][0];
  if (sat_separates(P, Q, n1x, n1y, n1z)) return false;
  const double n2x = f[0][1] * f[1][2] - f[0][2] * f[1][1];
  const double n2y = f[0][2] * f[1][0] - f[0][0] * f[1][2];
  const double n2z = f[0][0] * f[1][1] - f[0][1] * f[1][0];
  if (sat_separates(P, Q, n2x, n2y, n2z)) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double lx = e[i][1] * f[j][2] - e[i][2] * f[j][1];
      const double ly = e[i][2] * f[j][0] - e[i][0] * f[j][2];
      const double lz = e[i][0] * f[j][1] - e[i][1] * f[j][0];
      if (sat_separates(P, Q, lx, ly, lz)) return false;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double lx = n1y * e[i][2] - n1z * e[i][1], ly = n1z * e[i][0] - n1x * e[i][2], lz = n1x * e[i][1] - n1y * e[i][0];
    if (sat_separates(P, Q, lx, ly, lz)) return false;
    lx = n2y * f[i][2] - n2z * f[i][1]; ly = n2z * f[i][0] - n2x * f[i][2]; lz = n2x * f[i][1] - n2y * f[i][0];
    if (sat_separates(P, Q, lx, ly, lz)) return false;
    // the other triangle's in-plane normals of these edges: the only in-plane axes left when n1 or n2 is zero
    lx = n2y * e[i][2] - n2z * e[i][1]; ly = n2z * e[i][0] - n2x * e[i][2]; lz = n2x * e[i][1] - n2y * e[i][0];
    if (sat_separates(P, Q, lx, ly, lz)) return false;
    lx = n1y * f[i][2] - n1z * f[i][1]; ly = n1z * f[i][0] - n1x * f[i][2]; lz = n1x * f[i][1] - n1y * f[i][0];
    if (sat_separates(P, Q, lx, ly, lz)) return false;
  }
  return true;
}

__global__ void __launch_bounds__(kWave)
mesh_validity_kernel(const double *__restrict__ states, int N, const double *__restrict__ rtris, int R,
                     const double *__restrict__ etris, int E, int32_t *__restrict__ valid) {
#pragma clang fp contract(off)
  const int sidx = blockIdx.x;
  const int lane = threadIdx.x;
  const double tx = states[(size_t)sidx * 4 + 0], ty = states[(size_t)sidx * 4 + 1], tz = states[(size_t)sidx * 4 + 2];
  const double yaw = states[(size_t)sidx * 4 + 3];
  // quaternion_from_euler(0, 0, yaw) = (0, 0, sin(yaw/2), cos(yaw/2)); its rotation matrix
  const double qz = sin(0.5 * yaw), qw = cos(0.5 * yaw);
  const double c = 1.0 - 2.0 * (qz * qz), s2 = 2.0 * (qz * qw);
  bool hit = false;
  const int pairs = R * E;
  for (int p0 = 0; p0 < pairs; p0 += kWave) {
    const int p = p0 + lane;
    if (p < pairs) {
      const int rt = p / E, et = p - rt * E;
      double P[3][3], Q[3][3];
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const double x = rtris[(size_t)rt * 9 + v * 3 + 0], y = rtris[(size_t)rt * 9 + v * 3 + 1];
        P[v][0] = (c * x - s2 * y) + tx;
        P[v][1] = (s2 * x + c * y) + ty;
        P[v][2] = rtris[(size_t)rt * 9 + v * 3 + 2] + tz;
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[v][k] = etris[(size_t)et * 9 + v * 3 + k];
      }
      hit = hit || tri_tri_intersect(P, Q);
    }
    if (__ballot(hit) != 0ULL) break;   // wave-uniform early exit
  }
  const unsigned long long any = __ballot(hit);
  if (lane == 0) valid[sidx] = (any == 0ULL) ? 1 : 0;
}

int launch_mesh_validity(msnap_ctx *ctx, int n_states, const double *states, int n_rtris, const double *rtris,
                         int n_etris, const double *etris, int32_t *valid) {
  hipLaunchKernelGGL(mesh_validity_kernel, dim3(n_states), dim3(kWave), 0, ctx->stream, states, n_states, rtris,
                     n_rtris, etris, n_etris, valid);
  MSNAP_HIP(ctx, hipGetLastError());
  return MSNAP_OK;
}

}  // namespace msnap
