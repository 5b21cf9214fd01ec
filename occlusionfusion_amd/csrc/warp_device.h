// Device code shared by integrate.hip and assoc.hip: the camera as kernels take it, the ED warp of a position
// and of a normal, and the f32 projection of ofx_visibility_f32. One definition, so that a point warped or
// projected by either translation unit has the same bits.
#pragma once
#include "ofx_common.h"

namespace ofx {

struct CamD {
  double fx, fy, cx, cy;
  float fxf, fyf, cxf, cyf;   // the same intrinsics as f32 (exact: ofx_camera is f32)
  int W, H;
};

inline CamD make_cam(const ofx_camera* cam) {
  CamD c;
  c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy;
  c.fxf = cam->fx; c.fyf = cam->fy; c.cxf = cam->cx; c.cyf = cam->cy;
  c.W = cam->width; c.H = cam->height;
  return c;
}

typedef float f2 __attribute__((ext_vector_type(2)));

// Warp one voxel position with its K anchors (f32, reference op order). Rows 0 and 1 of R(x-g)+g+t
// run as packed f32 pairs (v_pk_mul/add_f32; the same per-component rounding), row 2 scalar.
// Node record layout: see ofx_pack_nodes.
__device__ __forceinline__ void ed_warp(const float4* __restrict__ nodes, const int ids[4], const float w[4], int K,
                                        float& x, float& y, float& z) {
  f2 axy = {0.f, 0.f};
  float az = 0.f;
  const f2 xy = {x, y};
  for (int k = 0; k < K; ++k) {
    const float4* n = nodes + 4 * (int64_t)ids[k];
    const float4 a = n[0], b = n[1], c = n[2], d = n[3];
    const f2 P0 = {a.x, a.y}, P1 = {a.z, a.w}, P2 = {b.x, b.y}, G = {b.z, b.w}, T = {c.x, c.y};
    const f2 dxy = xy - G;
    const float dz = z - d.y;
    f2 r = P0 * dxy.x;
    r = r + P1 * dxy.y;
    r = r + P2 * dz;
    float rz = c.z * dxy.x;
    rz = rz + c.w * dxy.y;
    rz = rz + d.x * dz;
    const f2 yxy = ((r + G) + T) * w[k];
    const float yz = ((rz + d.y) + d.z) * w[k];
    if (k == 0) { axy = yxy; az = yz; }
    else { axy = axy + yxy; az = az + yz; }
  }
  x = axy.x; y = axy.y; z = az;
}

__device__ __forceinline__ float cdiv(float a, float b) { return (float)((double)a / (double)b); }

// Pixel p of a depth image in metres: f32 as it is, or u16 divided by the normalizer (correctly rounded)
template <bool U16>
__device__ __forceinline__ float depth_px(const void* __restrict__ depth, int64_t p, float normalizer) {
  if (U16) return cdiv((float)((const uint16_t*)depth)[p], normalizer);
  return ((const float*)depth)[p];
}

// The vertex of pixel (x, y) at depth d (image_proc.cpp:351-401): f32 d·(x − cx), the quotient by fx correctly rounded;
// z = d. One definition for ofx_backproject_depth and ofx_prepare_depth.
__device__ __forceinline__ void backproject_px(float d, int x, int y, float fx, float fy, float cx, float cy, float& X,
                                               float& Y) {
  X = cdiv(d * ((float)x - cx), fx);
  Y = cdiv(d * ((float)y - cy), fy);
}

// WarpField.deform_normals: deform_lbs with zero translation, weights==0 skipped (warpfield.py:208-231,312-345);
// the blend, not yet normalised
__device__ __forceinline__ void ed_warp_normal(const float4* __restrict__ nodes, const int ids[4], const float w[4],
                                               int K, float& x, float& y, float& z) {
  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int k = 0; k < K; ++k) {
    if (w[k] == 0.f) continue;
    const float4* nd = nodes + 4 * (int64_t)ids[k];
    const float4 a = nd[0], b = nd[1], c = nd[2], d = nd[3];   // record layout: ofx_pack_nodes
    float rx = a.x * x; rx = rx + a.z * y; rx = rx + b.x * z;
    float ry = a.y * x; ry = ry + a.w * y; ry = ry + b.y * z;
    float rz = c.z * x; rz = rz + c.w * y; rz = rz + d.x * z;
    ax = ax + w[k] * rx; ay = ay + w[k] * ry; az = az + w[k] * rz;
  }
  x = ax; y = ay; z = az;
}

// v / |v|: ((x² + y²) + z²), square root and divisions correctly rounded (f64, then rounded)
__device__ __forceinline__ void normalise3(float& x, float& y, float& z) {
  float nrm = (float)sqrt((double)((x * x + y * y) + z * z));
  x = cdiv(x, nrm); y = cdiv(y, nrm); z = cdiv(z, nrm);
}

// F32: the projection of f32 points as numba types cam2pix on an f32 array (tsdf.py:351-364 called from
// get_visible_nodes with the f32 deformed nodes, tsdf.py:614-638): (x·fx)/z + cx in f32 with the f32 intrinsics,
// np.round (half-even) in f32, int(); the depth lookup and the difference stay f64 as get_depth_from_image's
// np.zeros array makes them (tsdf.py:576-612). F32 = false: the f64 form of the integrate path (f64 cam_pts).
__device__ __forceinline__ int64_t project_f32(const CamD& c, float x, float y, float z) {
  const float su = cdiv(x * c.fxf, z) + c.cxf, sv = cdiv(y * c.fyf, z) + c.cyf;
  const float u = rintf(su), v = rintf(sv);
  if (!(u >= 0.0f && u < (float)c.W && v >= 0.0f && v < (float)c.H && z > 0.0f)) return -1;
  return (int64_t)v * c.W + (int64_t)u;
}

}  // namespace ofx
