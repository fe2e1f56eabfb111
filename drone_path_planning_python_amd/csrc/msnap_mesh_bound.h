// What a node of a walk against a triangle mesh computes, for the two lane kernels that walk one: K11's
// mesh_clearance_lane_kernel (msnap_mesh_clearance.hip: the minimum distance) and K19's mesh_conflict_lane_kernel
// (msnap_mesh_conflict.hip: the first and last time below a threshold).  Both compile this one text.
//
// node_points: the Bernstein control points of the three position polynomials on the node, their box, and the path's
// points at the node's start, middle and end.
// tri_node_bound: one triangle against one node -- the attained squared distances at those three points through the
// sweep's functions (msnap_tri.h), and a proven lower bound of the distance over the whole node.
//
// Bound.  For any vector n with |n| <= 1 and any point x, dist(x, triangle) >= n.x - max_j n.v_j (the triangle's
// support function).  On a sub-interval of a segment the control points b_k enclose the path, so
// min_k n.b_k - max_j n.v_j bounds the distance from below on the whole sub-interval, whatever n is.  Candidates: +N
// and -N (the face's unit normal: near the wall the direction below is rounding noise, and the support function charges
// a tilt eps with eps times the triangle's extent) and the unit direction from the triangle's closest point to whichever
// of the node's start, middle and end lies farthest from it (the tangent plane of a convex function: the bound
// converges quadratically with the node's width).  The largest of the three counts.  A triangle the sweep takes as the
// union of its edges (tri_degenerate) is bounded by its hull, which that union lies in: exact for a zero-area triangle,
// below the edge-union distance inside a sliver of non-zero area.
#pragma once

#include <math.h>

#include "msnap_tri.h"
#include "msnap_walk.h"

namespace msnap {
namespace {

// every vertex coordinate finite (wave-uniform: a triangle that is not never wins and is skipped)
__device__ __forceinline__ bool tri_finite(const double *__restrict__ t) {
  bool f = true;
#pragma unroll
  for (int j = 0; j < 9; ++j) f = f && isfinite(t[j]);
  return f;
}

// closest point of the closed segment ab to p (pt_seg_d2's parameter)
__device__ __forceinline__ void closest_on_seg(double px, double py, double pz, const double *__restrict__ a,
                                               const double *__restrict__ b, double &qx, double &qy, double &qz) {
#pragma clang fp contract(off)
  const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
  const double wx = px - a[0], wy = py - a[1], wz = pz - a[2];
  const double l2 = ux * ux + uy * uy + uz * uz;
  double u = 0.0;
  if (l2 > 0.0) {
    u = (wx * ux + wy * uy + wz * uz) / l2;
    u = (u > 0.0) ? u : 0.0;
    u = (u < 1.0) ? u : 1.0;
  }
  qx = a[0] + u * ux;
  qy = a[1] + u * uy;
  qz = a[2] + u * uz;
}

// The direction from the triangle's closest point to p, as a vector of length <= 1 (up to an ulp; zero when p lies on
// the triangle).  Only the QUALITY of the bound depends on it, not its validity: the closest point is found by
// projecting on the plane and, outside the face, on the three edges -- not by the sweep's region walk.
__device__ __forceinline__ void away_direction(double px, double py, double pz, const double *__restrict__ t,
                                               bool degenerate, double Nx, double Ny, double Nz, double &nx, double &ny,
                                               double &nz) {
#pragma clang fp contract(off)
  double qx, qy, qz, best;
  closest_on_seg(px, py, pz, t, t + 3, qx, qy, qz);
  best = (px - qx) * (px - qx) + (py - qy) * (py - qy) + (pz - qz) * (pz - qz);
  {
    double rx, ry, rz;
    closest_on_seg(px, py, pz, t + 3, t + 6, rx, ry, rz);
    const double d = (px - rx) * (px - rx) + (py - ry) * (py - ry) + (pz - rz) * (pz - rz);
    if (d < best) { best = d; qx = rx; qy = ry; qz = rz; }
    closest_on_seg(px, py, pz, t + 6, t, rx, ry, rz);
    const double e = (px - rx) * (px - rx) + (py - ry) * (py - ry) + (pz - rz) * (pz - rz);
    if (e < best) { best = e; qx = rx; qy = ry; qz = rz; }
  }
  if (!degenerate) {
    // the foot of the perpendicular, if it falls inside the face (same side of all three edges)
    const double h = (px - t[0]) * Nx + (py - t[1]) * Ny + (pz - t[2]) * Nz;
    const double fx = px - h * Nx, fy = py - h * Ny, fz = pz - h * Nz;
    bool inside = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const double *a = t + 3 * e, *b = t + 3 * ((e + 1) % 3);
      const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
      const double wx = fx - a[0], wy = fy - a[1], wz = fz - a[2];
      const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
      inside = inside && (cx * Nx + cy * Ny + cz * Nz >= 0.0);
    }
    if (inside && h * h < best) { qx = fx; qy = fy; qz = fz; }
  }
  const double dx = px - qx, dy = py - qy, dz = pz - qz;
  const double len = sqrt(dx * dx + dy * dy + dz * dz);
  const double inv = len > 0.0 ? 1.0 / len : 0.0;
  nx = dx * inv;
  ny = dy * inv;
  nz = dz * inv;
}

// the node [a, a + hh] of the segment e[s][.] (axis s in u): control points b[s][i] of axis s, the path's three points
// p[.][s] (x = 0, 1/2, 1) and the control points' box
template <int D>
__device__ __forceinline__ void node_points(const double (&e)[3][D + 1], double a, double hh, double (&b)[3][D + 1],
                                            double (&p)[3][3], double (&lo)[3], double (&hi)[3]) {
  constexpr BernsteinWeights<D> W{};
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    double f[D + 1], at[3];
    shift_scale<D>(e[s], a, hh, f);
    values_at_ends_and_middle<D>(f, at);
#pragma unroll
    for (int q = 0; q < 3; ++q) p[q][s] = at[q];
    b[s][0] = f[0];
    lo[s] = hi[s] = f[0];
#pragma unroll
    for (int i = 1; i <= D; ++i) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j <= i; ++j) v = fma(W.w[i][j], f[j], v);
      b[s][i] = v;
      lo[s] = fmin(lo[s], v);
      hi[s] = fmax(hi[s], v);
    }
  }
}

// One finite triangle against one node: d2[q] = the sweep's squared distance of p[q] to it; returns the largest of the
// three support-plane bounds of the distance over the node.  The triangle is wave-uniform: `degenerate` is a scalar
// branch.
template <int D>
__device__ __forceinline__ double tri_node_bound(const double *__restrict__ tri, const double (&b)[3][D + 1],
                                                 const double (&p)[3][3], double (&d2)[3]) {
  const double inf = __builtin_inf();
  const bool degenerate = tri_degenerate(tri);
#pragma unroll
  for (int q = 0; q < 3; ++q)
    d2[q] = degenerate ? pt_degenerate_tri_d2(p[q][0], p[q][1], p[q][2], tri)
                       : pt_tri_d2(p[q][0], p[q][1], p[q][2], tri);
  // the face's unit normal (zero for a triangle without area)
  const double abx = tri[3] - tri[0], aby = tri[4] - tri[1], abz = tri[5] - tri[2];
  const double acx = tri[6] - tri[0], acy = tri[7] - tri[1], acz = tri[8] - tri[2];
  double Nx = aby * acz - abz * acy, Ny = abz * acx - abx * acz, Nz = abx * acy - aby * acx;
  const double nn = sqrt(Nx * Nx + Ny * Ny + Nz * Nz);
  const double ninv = nn > 0.0 ? 1.0 / nn : 0.0;
  Nx *= ninv;
  Ny *= ninv;
  Nz *= ninv;
  // the node's point farthest from the triangle, and the direction away from the triangle there
  // (selects on the two comparisons, not on an index: an index into p can end as a load from scratch)
  const bool mid = d2[1] > d2[0];
  const bool end = d2[2] > (mid ? d2[1] : d2[0]);
  const double fx = end ? p[2][0] : (mid ? p[1][0] : p[0][0]);
  const double fy = end ? p[2][1] : (mid ? p[1][1] : p[0][1]);
  const double fz = end ? p[2][2] : (mid ? p[1][2] : p[0][2]);
  double ax, ay, az;
  away_direction(fx, fy, fz, tri, degenerate, Nx, Ny, Nz, ax, ay, az);
  // support-plane bounds of the three candidates
  double pn_min = inf, pn_max = -inf, pa_min = inf;
#pragma unroll
  for (int i = 0; i <= D; ++i) {
    const double pn = fma(Nz, b[2][i], fma(Ny, b[1][i], Nx * b[0][i]));
    const double pa = fma(az, b[2][i], fma(ay, b[1][i], ax * b[0][i]));
    pn_min = fmin(pn_min, pn);
    pn_max = fmax(pn_max, pn);
    pa_min = fmin(pa_min, pa);
  }
  double sn_min = inf, sn_max = -inf, sa_max = -inf;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double sn = fma(Nz, tri[3 * j + 2], fma(Ny, tri[3 * j + 1], Nx * tri[3 * j]));
    const double sa = fma(az, tri[3 * j + 2], fma(ay, tri[3 * j + 1], ax * tri[3 * j]));
    sn_min = fmin(sn_min, sn);
    sn_max = fmax(sn_max, sn);
    sa_max = fmax(sa_max, sa);
  }
  return fmax(fmax(pn_min - sn_max, sn_min - pn_max), pa_min - sa_max);
}

// the distance of the point (x, y, z) to the mesh as msnap_mesh_sweep takes it -- every finite triangle in index
// order, strict `<` -- and the lowest index that attains it (-1: no finite triangle, the distance is +inf)
__device__ __forceinline__ double mesh_distance_at(double x, double y, double z, int n_tris,
                                                   const double *__restrict__ tris, int &tw) {
  double d2 = __builtin_inf();
  tw = -1;
  for (int t = 0; t < n_tris; ++t) {
    const double *tri = tris + (size_t)t * 9;
    if (!tri_finite(tri)) continue;
    const double v = tri_degenerate(tri) ? pt_degenerate_tri_d2(x, y, z, tri) : pt_tri_d2(x, y, z, tri);
    if (v < d2) {
      d2 = v;
      tw = t;
    }
  }
  return sqrt(d2);
}

}  // namespace
}  // namespace msnap
