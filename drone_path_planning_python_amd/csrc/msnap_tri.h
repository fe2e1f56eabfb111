// Point-triangle geometry of the mesh sweep (msnap_aux.hip) and of the mesh clearance (msnap_mesh_clearance.hip): both
// kernels compile this one text, so a distance one of them reports is the other's bit for bit.  Closest-point regions
// after Ericson 5.1.5; every function is `fp contract(off)`.
#pragma once

#include <hip/hip_runtime.h>

namespace msnap {

__device__ __forceinline__ double pt_tri_d2(double px, double py, double pz, const double *__restrict__ t) {
#pragma clang fp contract(off)
  const double ax = t[0], ay = t[1], az = t[2];
  const double bx = t[3], by = t[4], bz = t[5];
  const double cx = t[6], cy = t[7], cz = t[8];
  const double abx = bx - ax, aby = by - ay, abz = bz - az;
  const double acx = cx - ax, acy = cy - ay, acz = cz - az;
  const double apx = px - ax, apy = py - ay, apz = pz - az;
  const double d1 = abx * apx + aby * apy + abz * apz;
  const double d2 = acx * apx + acy * apy + acz * apz;
  double qx, qy, qz;
  if (d1 <= 0.0 && d2 <= 0.0) {
    qx = ax; qy = ay; qz = az;
  } else {
    const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
    const double d3 = abx * bpx + aby * bpy + abz * bpz;
    const double d4 = acx * bpx + acy * bpy + acz * bpz;
    if (d3 >= 0.0 && d4 <= d3) {
      qx = bx; qy = by; qz = bz;
    } else {
      const double vc = d1 * d4 - d3 * d2;
      if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
        qx = ax + v * abx; qy = ay + v * aby; qz = az + v * abz;
      } else {
        const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
        const double d5 = abx * cpx + aby * cpy + abz * cpz;
        const double d6 = acx * cpx + acy * cpy + acz * cpz;
        if (d6 >= 0.0 && d5 <= d6) {
          qx = cx; qy = cy; qz = cz;
        } else {
          const double vb = d5 * d2 - d1 * d6;
          if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
            const double w = d2 / (d2 - d6);
            qx = ax + w * acx; qy = ay + w * acy; qz = az + w * acz;
          } else {
            const double va = d3 * d6 - d5 * d4;
            if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
              const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
              qx = bx + w * (cx - bx); qy = by + w * (cy - by); qz = bz + w * (cz - bz);
            } else {
              const double denom = 1.0 / (va + vb + vc);
              const double v = vb * denom, w = vc * denom;
              qx = ax + abx * v + acx * w;
              qy = ay + aby * v + acy * w;
              qz = az + abz * v + acz * w;
            }
          }
        }
      }
    }
  }
  const double ex = px - qx, ey = py - qy, ez = pz - qz;
  return ex * ex + ey * ey + ez * ez;
}

// Ericson's regions assume a triangle of nonzero area: with a repeated vertex they end in 0/0 (a NaN that never wins
// the minimum), with three collinear vertices sign noise in va/vb/vc can pick the face region and a far too large
// distance.  A triangle whose |ab x ac|^2 is below kTriDegenerate |ab|^2 |ac|^2 (sin^2 of the angle at a) is taken as
// the union of its three closed edges: a segment or a point, exactly, when the area is zero, and within the triangle's
// width (< 5e-6 x its longest edge) otherwise.  Both oracles restate this test and pt_degenerate_tri_d2.
constexpr double kTriDegenerate = 1e-10;

__device__ __forceinline__ bool tri_degenerate(const double *__restrict__ t) {
#pragma clang fp contract(off)
  const double abx = t[3] - t[0], aby = t[4] - t[1], abz = t[5] - t[2];
  const double acx = t[6] - t[0], acy = t[7] - t[1], acz = t[8] - t[2];
  const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
  const double nn = nx * nx + ny * ny + nz * nz;
  const double ab2 = abx * abx + aby * aby + abz * abz, ac2 = acx * acx + acy * acy + acz * acz;
  return nn <= kTriDegenerate * (ab2 * ac2);
}

// squared distance from p to the closed segment ab (a point when a == b)
__device__ __forceinline__ double pt_seg_d2(double px, double py, double pz, double ax, double ay, double az,
                                            double bx, double by, double bz) {
#pragma clang fp contract(off)
  const double ux = bx - ax, uy = by - ay, uz = bz - az;
  const double wx = px - ax, wy = py - ay, wz = pz - az;
  const double l2 = ux * ux + uy * uy + uz * uz;
  double u = 0.0;
  if (l2 > 0.0) {
    u = (wx * ux + wy * uy + wz * uz) / l2;
    u = (u > 0.0) ? u : 0.0;
    u = (u < 1.0) ? u : 1.0;
  }
  const double ex = px - (ax + u * ux), ey = py - (ay + u * uy), ez = pz - (az + u * uz);
  return ex * ex + ey * ey + ez * ez;
}

__device__ __forceinline__ double pt_degenerate_tri_d2(double px, double py, double pz, const double *__restrict__ t) {
  double d = pt_seg_d2(px, py, pz, t[0], t[1], t[2], t[3], t[4], t[5]);
  const double d_bc = pt_seg_d2(px, py, pz, t[3], t[4], t[5], t[6], t[7], t[8]);
  d = (d_bc < d) ? d_bc : d;
  const double d_ca = pt_seg_d2(px, py, pz, t[6], t[7], t[8], t[0], t[1], t[2]);
  return (d_ca < d) ? d_ca : d;
}

// squared distance between the box [lo, hi] and the bounding box of triangle t: a lower bound of every
// point-triangle distance between them
__device__ __forceinline__ double box_tri_lb2(const double (&lo)[3], const double (&hi)[3], const double *__restrict__ t) {
#pragma clang fp contract(off)
  double lb2 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double tmin = fmin(t[k], fmin(t[3 + k], t[6 + k])), tmax = fmax(t[k], fmax(t[3 + k], t[6 + k]));
    const double gap = fmax(0.0, fmax(lo[k] - tmax, tmin - hi[k]));
    lb2 = lb2 + gap * gap;
  }
  return lb2;
}

}  // namespace msnap
