// Projective data association: the data term of a depth frame without given matches.
//
// The reference takes its matches from learned front-ends (Lepard, the flow net); its geometric fallback for the target
// cloud is the truncated chamfer term (NonRigidICP/model/loss.py:275-292). The dense equivalent in a TSDF fusion system
// is projective association, which has no reference twin (parity unpinned; restated op for op in tests/assoc_ref.py):
//
//   x' = ED warp of the model point under the current estimate      (ed_warp: the bits of ofx_deform_points)
//   n' = ED warp of its normal, normalised                          (ed_warp_normal: ofx_deform_points, normals = 1)
//   (u, v) = pixel of x'                                            (project_f32: the pixel of ofx_visibility_f32)
//   q  = target vertex map at (u, v)                                (the planar image ofx_backproject_depth writes)
//   n_q = normalise((q[v,u+1] - q[v,u-1]) x (q[v+1,u] - q[v-1,u])), flipped to face the camera
//   gates, first that applies: 1 invalid skin, 2 behind the camera / non-finite / off the image, 3 hole, 4 no target
//   normal (image border, a 4-neighbour hole, a depth edge > edge_max, a zero cross product), 5 |q - x'|² > dist_max²,
//   6 n'·n_q < cos_min; 0 accepted
//   target: q (OFX_ASSOC_POINT) or the foot of x' on q's tangent plane, x' + n_q·((q - x')·n_q) (OFX_ASSOC_PLANE)
//
// One thread per point, a gather: trip 1 loads the point, its normal, anchors, weights and valid flag, trip 2 the four
// 64-B node records (L2-resident), trip 3 the five vertex-map pixels once the pixel is known (neighbour coordinates are
// clamped into the image, so the fifteen loads are unconditional and issue together); the three trips and the gates
// are gate_device.h's, shared with rigid.hip and splat.hip. No LDS, no atomics. The accepted
// points are ranked by scan_flags (ascending point index) and emitted in that order; more than max_matches of them are
// thinned evenly and deterministically (rank r is kept iff floor((r+1)·max/n) > floor(r·max/n), 64-bit), where the
// reference draws an unseeded randperm (model/model.py:319-334).
#include "ofx_common.h"
#include "assoc_handle.h"
#include "gate_device.h"
#include "scan_flags.h"

namespace ofx {

// VALID / NRM: valid / normals given (compile-time, so that trip 1 is branch-free)
template <bool VALID, bool NRM>
__global__ __launch_bounds__(256) void k_assoc_gate(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                     const int4* __restrict__ anchors,
                                                     const float4* __restrict__ weights,
                                                     const uint8_t* __restrict__ valid,
                                                     const float4* __restrict__ nodes, int n_nodes, CamD c,
                                                     const float* __restrict__ vmap, float dist_max, float cos_min,
                                                     float edge_max, int mode, int64_t n, uint8_t* __restrict__ code,
                                                     uint8_t* __restrict__ flag, float* __restrict__ tgt,
                                                     float* __restrict__ warped) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= n) return;
  SkinPt s;
  const bool ok = skin_load<VALID, NRM>(pts, nrm, anchors, weights, valid, n_nodes, p, 0.f, s);
  int cd = 1;
  float tx = 0.f, ty = 0.f, tz = 0.f;
  if (ok) {
    skin_warp<NRM>(nodes, s);
    GateHit h;
    cd = proj_gate<NRM>(c, vmap, s, dist_max, cos_min, edge_max, h);
    if (cd == 0) {
      if (mode == OFX_ASSOC_PLANE) {
        const float d = dot3(h.ex, h.ey, h.ez, h.nx, h.ny, h.nz);
        tx = s.x + h.nx * d; ty = s.y + h.ny * d; tz = s.z + h.nz * d;
      } else {
        tx = h.qx; ty = h.qy; tz = h.qz;
      }
    }
  }
  code[p] = (uint8_t)cd;
  flag[p] = cd == 0 ? 1 : 0;
  tgt[3 * p] = tx; tgt[3 * p + 1] = ty; tgt[3 * p + 2] = tz;
  if (warped) { warped[3 * p] = s.x; warped[3 * p + 1] = s.y; warped[3 * p + 2] = s.z; }
}

__global__ __launch_bounds__(256) void k_assoc_emit(const uint8_t* __restrict__ flag, const int32_t* __restrict__ rank,
                                                     int64_t n, int max_matches, const float* __restrict__ pts,
                                                     const float* __restrict__ tgt, const int4* __restrict__ anchors,
                                                     const float4* __restrict__ weights, int32_t* __restrict__ midx,
                                                     float* __restrict__ src_out, float* __restrict__ tgt_out,
                                                     int4* __restrict__ a_out, float4* __restrict__ w_out,
                                                     int32_t* __restrict__ count) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = rank[n], mm = max_matches;
  if (p == 0) { count[0] = (int32_t)total; count[1] = (int32_t)(total < mm ? total : mm); }
  if (p >= n || !flag[p]) return;
  const int64_t r = rank[p];
  int64_t slot = r;
  if (total > mm) {
    slot = r * mm / total;
    if (!((r + 1) * mm / total > slot)) return;
  }
  midx[slot] = (int32_t)p;
  src_out[3 * slot] = pts[3 * p]; src_out[3 * slot + 1] = pts[3 * p + 1]; src_out[3 * slot + 2] = pts[3 * p + 2];
  tgt_out[3 * slot] = tgt[3 * p]; tgt_out[3 * slot + 1] = tgt[3 * p + 1]; tgt_out[3 * slot + 2] = tgt[3 * p + 2];
  a_out[slot] = anchors[p];
  w_out[slot] = weights[p];
}

}  // namespace ofx

using namespace ofx;

extern "C" {

int ofx_assoc_create(int64_t max_points, void** handle) {
  OFX_CHECK_ARG(handle, "null handle");
  *handle = nullptr;
  OFX_CHECK_ARG(max_points >= 0, "bad max_points");
  if (max_points >= ((int64_t)1 << 31) - 1) {
    set_error("max_points %lld exceeds the int32 ranks", (long long)max_points);
    return OFX_ERR_RANGE;
  }
  Assoc* a = new Assoc();
  a->cap = max_points;
  if (hipMalloc((void**)&a->flag, (size_t)max_points + 16) != hipSuccess ||
      hipMalloc((void**)&a->rank, ((size_t)max_points + 1) * sizeof(int32_t)) != hipSuccess ||
      hipMalloc((void**)&a->tsum, ((size_t)scan_tiles(max_points) + 1) * sizeof(int32_t)) != hipSuccess) {
    for (void* p : {(void*)a->flag, (void*)a->rank, (void*)a->tsum})
      if (p) (void)hipFree(p);
    delete a;
    set_error("ofx_assoc_create: scratch for %lld points could not be allocated", (long long)max_points);
    return OFX_ERR_ALLOC;
  }
  *handle = a;
  return OFX_OK;
}

int ofx_assoc_destroy(void* handle) {
  if (!handle) return OFX_OK;
  Assoc* a = (Assoc*)handle;
  (void)hipDeviceSynchronize();
  for (void* p : {(void*)a->flag, (void*)a->rank, (void*)a->tsum})
    if (p) (void)hipFree(p);
  delete a;
  return OFX_OK;
}

int ofx_associate(void* handle, const float* points, const float* normals, const int32_t* anchors, const float* weights,
                  const uint8_t* valid, int64_t n_points, const float* packed_nodes, int32_t n_nodes,
                  const ofx_camera* cam, const float* point_image, int32_t height, int32_t width,
                  const ofx_assoc_params* prm, uint8_t* code, float* tgt, float* warped, int32_t* match_idx,
                  float* src_out, float* tgt_out, int32_t* anchors_out, float* weights_out, int32_t* count,
                  ofx_stream_t s) {
  Assoc* a = (Assoc*)handle;
  OFX_CHECK_ARG(a && cam && prm && count, "null handle / camera / params / count");
  OFX_CHECK_ARG(n_points >= 0 && n_points <= a->cap, "n_points %lld outside [0, %lld] (the handle's max_points)",
                (long long)n_points, (long long)a->cap);
  OFX_CHECK_ARG(prm->mode == OFX_ASSOC_POINT || prm->mode == OFX_ASSOC_PLANE, "bad mode %d", prm->mode);
  OFX_CHECK_ARG(prm->max_matches >= 0, "bad max_matches %d", prm->max_matches);
  OFX_CHECK_ARG(height > 0 && width > 0 && cam->width == width && cam->height == height,
                "the camera (%d x %d) and the point image (%d x %d) differ", cam->width, cam->height, width, height);
  hipStream_t hs = as_stream(s);
  if (n_points == 0) {
    OFX_HIP(hipMemsetAsync(count, 0, 2 * sizeof(int32_t), hs));
    return OFX_OK;
  }
  if (int st = check_skinned(points, anchors, weights, packed_nodes, n_nodes, point_image && code && tgt,
                             (uintptr_t)anchors_out | (uintptr_t)weights_out))
    return st;
  OFX_CHECK_ARG(prm->max_matches == 0 || (match_idx && src_out && tgt_out && anchors_out && weights_out),
                "null compacted output");
  const unsigned grid = grid_for(n_points, 256, 1 << 30);
  dispatch_valid_nrm(valid, normals, [&](auto V, auto N) {
    hipLaunchKernelGGL((k_assoc_gate<decltype(V)::value, decltype(N)::value>), dim3(grid), dim3(256), 0, hs, points,
                       normals, (const int4*)anchors, (const float4*)weights, valid, (const float4*)packed_nodes,
                       n_nodes, make_cam(cam), point_image, prm->dist_max, prm->cos_min, prm->edge_max, prm->mode,
                       n_points, code, a->flag, tgt, warped);
  });
  OFX_LAUNCH_CHECK();
  int st = scan_flags(a->flag, n_points, a->rank, a->tsum, hs);
  if (st) return st;
  hipLaunchKernelGGL(k_assoc_emit, dim3(grid), dim3(256), 0, hs, (const uint8_t*)a->flag, (const int32_t*)a->rank,
                     n_points, prm->max_matches, points, (const float*)tgt, (const int4*)anchors,
                     (const float4*)weights, match_idx, src_out, tgt_out, (int4*)anchors_out, (float4*)weights_out,
                     count);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

}  // extern "C"
