// The skinned-point gate that assoc.hip, rigid.hip and splat.hip share: trip 1 (the load of a skinned point), trip 2 (its
// ED warp) and the projective gate against a vertex map, plus the host checks and the <VALID, NRM> dispatch of the three
// entry points. One definition, so that a point gated by any of the three kernels takes the same steps to the same bits;
// the kernels' file headers say what each does with the result. The gate's target normal (vertex_normal) is also what
// prepare.hip writes as a frame's normal map.
#pragma once
#include <type_traits>

#include "warp_device.h"

namespace ofx {

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

struct SkinPt {
  float x, y, z, nx, ny, nz;   // position and normal: as loaded, then as warped
  int ids[4];
  float w[4];
};

// Trip 1: point p, its normal (NRM; else (0, 0, nz0)), anchors, weights and valid flag (VALID; compile-time, so that the
// trip is branch-free) -> whether the point can be warped
template <bool VALID, bool NRM>
__device__ __forceinline__ bool skin_load(const float* __restrict__ pts, const float* __restrict__ nrm,
                                          const int4* __restrict__ anchors, const float4* __restrict__ weights,
                                          const uint8_t* __restrict__ valid, int n_nodes, int64_t p, float nz0,
                                          SkinPt& s) {
  s.x = pts[3 * p]; s.y = pts[3 * p + 1]; s.z = pts[3 * p + 2];
  const int4 a4 = anchors[p];
  const float4 w4 = weights[p];
  const bool ok = VALID ? valid[p] != 0 : true;
  s.nx = 0.f; s.ny = 0.f; s.nz = nz0;
  if (NRM) { s.nx = nrm[3 * p]; s.ny = nrm[3 * p + 1]; s.nz = nrm[3 * p + 2]; }
  s.ids[0] = a4.x; s.ids[1] = a4.y; s.ids[2] = a4.z; s.ids[3] = a4.w;
  s.w[0] = w4.x; s.w[1] = w4.y; s.w[2] = w4.z; s.w[3] = w4.w;
  // an anchor outside the graph cannot be gathered: such a point counts as invalid skin
  return ok && (unsigned)s.ids[0] < (unsigned)n_nodes && (unsigned)s.ids[1] < (unsigned)n_nodes &&
         (unsigned)s.ids[2] < (unsigned)n_nodes && (unsigned)s.ids[3] < (unsigned)n_nodes;
}

// Trip 2: the four 64-B node records (the normal's blend reads the same four)
template <bool NRM>
__device__ __forceinline__ void skin_warp(const float4* __restrict__ nodes, SkinPt& s) {
  ed_warp(nodes, s.ids, s.w, 4, s.x, s.y, s.z);
  if (NRM) {
    ed_warp_normal(nodes, s.ids, s.w, 4, s.nx, s.ny, s.nz);
    normalise3(s.nx, s.ny, s.nz);
  }
}

// the pixel of a camera-space point, -1: non-finite, behind the camera or off the image
__device__ __forceinline__ int64_t pixel_of(const CamD& c, float x, float y, float z) {
  return (isfinite(x) && isfinite(y) && isfinite(z)) ? project_f32(c, x, y, z) : -1;
}

struct GateHit {
  float qx, qy, qz;   // the target vertex
  float nx, ny, nz;   // its normal n_q, facing the camera
  float ex, ey, ez;   // q - point
};

// The target normal n_q of a vertex-map pixel from its vertex q and its left / right / upper / lower neighbours, all five
// already in registers (border: the pixel lies on the image border): code 3 (hole) or 4 (no normal), or 0 with the unit
// normal, facing the camera, in (nx, ny, nz). proj_gate's steps, and the normal map of prepare.hip.
__device__ __forceinline__ int vertex_normal(bool border, float qx, float qy, float qz, float lx, float ly, float lz,
                                             float rx, float ry, float rz, float ux, float uy, float uz, float dx,
                                             float dy, float dz, float edge_max, float& nx, float& ny, float& nz) {
  if (!(qz > 0.f)) return 3;
  if (border || !(lz > 0.f && rz > 0.f && uz > 0.f && dz > 0.f) || fabsf(lz - qz) > edge_max ||
      fabsf(rz - qz) > edge_max || fabsf(uz - qz) > edge_max || fabsf(dz - qz) > edge_max)
    return 4;
  const float ax = rx - lx, ay = ry - ly, az = rz - lz;
  const float bx = dx - ux, by = dy - uy, bz = dz - uz;
  float cx = ay * bz - az * by;
  float cy = az * bx - ax * bz;
  float cz = ax * by - ay * bx;
  const float l2 = (cx * cx + cy * cy) + cz * cz;
  if (!(l2 > 0.f && isfinite(l2))) return 4;
  const float len = (float)sqrt((double)l2);
  cx = cdiv(cx, len); cy = cdiv(cy, len); cz = cdiv(cz, len);
  if (dot3(cx, cy, cz, qx, qy, qz) > 0.f) { cx = -cx; cy = -cy; cz = -cz; }
  nx = cx; ny = cy; nz = cz;
  return 0;
}

// The projective gate of the camera-space point and normal in s against the vertex map vmap (3 planes of c.H x c.W):
// the first code of 2..6 that applies (assoc.hip's header), or 0 with the hit filled in. Trip 3: the five vertex-map
// pixels; neighbour coordinates are clamped into the image, so the fifteen loads are unconditional and issue together.
template <bool NRM>
__device__ __forceinline__ int proj_gate(const CamD& c, const float* __restrict__ vmap, const SkinPt& s, float dist_max,
                                         float cos_min, float edge_max, GateHit& h) {
  const int64_t pix = pixel_of(c, s.x, s.y, s.z);
  if (pix < 0) return 2;
  const int u = (int)(pix % c.W), v = (int)(pix / c.W);
  const int64_t hw = (int64_t)c.H * c.W;
  const int64_t il = (int64_t)v * c.W + max(u - 1, 0), ir = (int64_t)v * c.W + min(u + 1, c.W - 1);
  const int64_t iu = (int64_t)max(v - 1, 0) * c.W + u, id = (int64_t)min(v + 1, c.H - 1) * c.W + u;
  const float qx = vmap[pix], qy = vmap[hw + pix], qz = vmap[2 * hw + pix];
  const float lx = vmap[il], ly = vmap[hw + il], lz = vmap[2 * hw + il];
  const float rx = vmap[ir], ry = vmap[hw + ir], rz = vmap[2 * hw + ir];
  const float ux = vmap[iu], uy = vmap[hw + iu], uz = vmap[2 * hw + iu];
  const float dx = vmap[id], dy = vmap[hw + id], dz = vmap[2 * hw + id];
  // all fifteen values in registers here: the loads leave together instead of sinking into the gates below
  asm volatile("" :: "v"(qx), "v"(qy), "v"(qz), "v"(lx), "v"(ly), "v"(lz), "v"(rx), "v"(ry), "v"(rz), "v"(ux),
               "v"(uy), "v"(uz), "v"(dx), "v"(dy), "v"(dz));
  const bool border = u == 0 || v == 0 || u == c.W - 1 || v == c.H - 1;
  float cx, cy, cz;
  if (const int cd = vertex_normal(border, qx, qy, qz, lx, ly, lz, rx, ry, rz, ux, uy, uz, dx, dy, dz, edge_max, cx, cy,
                                   cz))
    return cd;
  const float ex = qx - s.x, ey = qy - s.y, ez = qz - s.z;
  const float d2 = (ex * ex + ey * ey) + ez * ez;
  if (d2 > dist_max * dist_max) return 5;
  if (NRM && dot3(s.nx, s.ny, s.nz, cx, cy, cz) < cos_min) return 6;
  h = {qx, qy, qz, cx, cy, cz, ex, ey, ez};
  return 0;
}

// The gate of one window tap of photo.hip against the warped point in s: the tap's vertex q, its normal n_q as
// ofx_prepare_depth wrote it (zeros where vertex_normal has none) and its colour difference (dr, dg, db) to the point ->
// the first code of 3..7 that applies, or 0; d2 = |q - point|² and c2 = |colour difference|² are filled in either way.
template <bool NRM>
__device__ __forceinline__ int tap_gate(const SkinPt& s, float qx, float qy, float qz, float nx, float ny, float nz,
                                        float dr, float dg, float db, float dist_max2, float cos_min, float color_max2,
                                        float& d2, float& c2) {
  const float ex = qx - s.x, ey = qy - s.y, ez = qz - s.z;
  d2 = (ex * ex + ey * ey) + ez * ez;
  c2 = (dr * dr + dg * dg) + db * db;
  if (!(qz > 0.f)) return 3;
  if (nx == 0.f && ny == 0.f && nz == 0.f) return 4;
  if (d2 > dist_max2) return 5;
  if (NRM && dot3(s.nx, s.ny, s.nz, nx, ny, nz) < cos_min) return 6;
  if (!(c2 <= color_max2)) return 7;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------- host part
// The argument checks the three entry points share, for n_points > 0. more: the entry point's further required buffers
// are all there; align16: its further pointers (or-ed) that must be 16-byte aligned.
inline int check_skinned(const void* points, const void* anchors, const void* weights, const void* packed_nodes,
                         int32_t n_nodes, bool more = true, uintptr_t align16 = 0) {
  OFX_CHECK_ARG(n_nodes >= 1, "bad n_nodes");
  OFX_CHECK_ARG(points && anchors && weights && packed_nodes && more, "null buffer");
  OFX_CHECK_ARG((((uintptr_t)anchors | (uintptr_t)weights | (uintptr_t)packed_nodes | align16) & 15) == 0,
                "anchors / weights / node records must be 16-byte aligned");
  return OFX_OK;
}

// f(VALID, NRM) with the two flags as compile-time constants (std::bool_constant): the caller's generic lambda names
// its kernel's instantiation by decltype(VALID)::value
template <class F>
inline void dispatch_valid_nrm(bool valid, bool nrm, F&& f) {
  if (valid) { if (nrm) f(std::true_type{}, std::true_type{}); else f(std::true_type{}, std::false_type{}); }
  else { if (nrm) f(std::false_type{}, std::true_type{}); else f(std::false_type{}, std::false_type{}); }
}

}  // namespace ofx
