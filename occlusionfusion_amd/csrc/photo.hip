// Photometric correspondence search: the stand-in for the reference's flow network, as assoc.hip is for its landmark
// matcher. Each warped model point looks in a (2r + 1)² window around its own pixel for the live pixel whose colour
// matches the point's best, among the pixels that pass ofx_associate's geometric gates; that pixel's vertex is the
// point's 3-D target, so the solver's existing 3-D rows carry a tangential constraint. No reference twin (parity
// unpinned; restated op for op in tests/photo_ref.py).
//
//   x', n', (u, v)  = ofx_associate's (skin_load, skin_warp, pixel_of: gate_device.h); codes 1 and 2 are its codes
//   taps: dv = -r..r outer, du = -r..r inner, tap index t = (dv + r)·(2r + 1) + (du + r); a tap off the image is skipped
//   at a tap: q = point_image, n_q = normal_image (ofx_prepare_depth's: zeros where the gate has no normal), c =
//   color_image; tap code, first that applies: 3 !(q_z > 0), 4 n_q all zero, 5 d2 > dist_max² (d2 = (e_x² + e_y²) + e_z²,
//   e = q - x'), 6 normals given and n'·n_q < cos_min, 7 !(c2 <= color_max²) (c2 = (dr² + dg²) + db², a NaN lands here),
//   0 eligible with cost E = c2 + geo_weight·d2
//   point: code 0 with the eligible tap of the smallest E (ties: the first in tap order), else the largest tap code
//
// k_photo_gate<VALID, NRM, L>: L lanes per point (OFX_PHOTO_LANES: 8, eight points per wave; -DOFX_PHOTO_LANES=1 is the
// one-thread-per-point form; the A/B of 1 / 4 / 8 / 16 lanes is in profiles/photo_bench.json and DESIGN §6: one thread
// per point is competitive only while neighbouring points sit in neighbouring pixels). Every lane of a group runs
// trips 1 and 2 on the same addresses — one fetch per group, broadcast by the memory pipeline, and the same bits in
// every lane without a shuffle. Lane l then takes the taps t = l, l + L, ...: consecutive lanes read consecutive du of
// a window row, so the nine planar loads of a tap coalesce into row segments. Each lane keeps the minimum of the 64-bit
// key float_bits(E) << 32 | t over its eligible taps (E is a sum of non-negative terms, so its bits order as the float
// does: splat.hip's trick) and the maximum of its tap codes; both are reduced over the group by xor shuffles — no LDS,
// no atomics — and a minimum / maximum does not depend on which lane saw which tap. Lane 0 re-reads the winner's vertex
// and writes the point. Compaction is assoc.hip's: scan_flags over code == 0 and the rank-thinning emit, plus the match
// pixel.
#include <cmath>

#include "ofx_common.h"
#include "assoc_handle.h"
#include "gate_device.h"
#include "scan_flags.h"

#ifndef OFX_PHOTO_LANES
#define OFX_PHOTO_LANES 8
#endif

namespace ofx {

constexpr int kPhotoLanes = OFX_PHOTO_LANES;
static_assert(kPhotoLanes == 1 || kPhotoLanes == 2 || kPhotoLanes == 4 || kPhotoLanes == 8 || kPhotoLanes == 16 ||
              kPhotoLanes == 32 || kPhotoLanes == 64, "OFX_PHOTO_LANES must be a power of two up to the wave");
constexpr uint64_t kPhotoNone = ~(uint64_t)0;   // no eligible tap: above every key (t < 2^32 - 1)

template <bool VALID, bool NRM, int L>
__global__ __launch_bounds__(256) void k_photo_gate(
    const float* __restrict__ pts, const float* __restrict__ nrm, const float* __restrict__ col,
    const int4* __restrict__ anchors, const float4* __restrict__ weights, const uint8_t* __restrict__ valid,
    const float4* __restrict__ nodes, int n_nodes, CamD c, const float* __restrict__ vmap,
    const float* __restrict__ nmap, const float* __restrict__ cmap, float dist_max, float cos_min, float color_max,
    float geo_weight, int r, int64_t n, uint8_t* __restrict__ code, uint8_t* __restrict__ flag, float* __restrict__ tgt,
    float* __restrict__ warped, int32_t* __restrict__ pixel, float* __restrict__ cost) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t p = tid / L;
  const int lane = (int)(tid % L);
  // a group is whole or absent (256 and the wave are multiples of L), so the shuffles below see all of their lanes
  if (p >= n) return;
  SkinPt s;
  const bool ok = skin_load<VALID, NRM>(pts, nrm, anchors, weights, valid, n_nodes, p, 0.f, s);
  int cd = 1;
  uint64_t best = kPhotoNone;
  int u = 0, v = 0;
  const int w = 2 * r + 1;
  const int64_t hw = (int64_t)c.H * c.W;
  if (ok) {
    skin_warp<NRM>(nodes, s);
    const int64_t pix = pixel_of(c, s.x, s.y, s.z);
    cd = 2;
    if (pix >= 0) {
      u = (int)(pix % c.W); v = (int)(pix / c.W);
      const float cr = col[3 * p], cg = col[3 * p + 1], cb = col[3 * p + 2];
      const float dmax2 = dist_max * dist_max, cmax2 = color_max * color_max;
      int top = 0;
      // tap t = lane, lane + L, ...: (du, dv) stepped along, no division in the loop
      int dv = lane / w - r, du = lane % w - r;
      for (int t = lane; t < w * w; t += L, du += L) {
        while (du > r) { du -= w; ++dv; }
        const int uu = u + du, vv = v + dv;
        if (uu < 0 || uu >= c.W || vv < 0 || vv >= c.H) continue;
        const int64_t i = (int64_t)vv * c.W + uu;
        const float qx = vmap[i], qy = vmap[hw + i], qz = vmap[2 * hw + i];
        const float nx = nmap[i], ny = nmap[hw + i], nz = nmap[2 * hw + i];
        const float kr = cmap[i], kg = cmap[hw + i], kb = cmap[2 * hw + i];
        float d2, c2;
        const int tc = tap_gate<NRM>(s, qx, qy, qz, nx, ny, nz, kr - cr, kg - cg, kb - cb, dmax2, cos_min, cmax2, d2,
                                     c2);
        if (tc == 0) {
          const float gd = geo_weight * d2;
          const float E = c2 + gd;
          const uint64_t key = (uint64_t)__float_as_uint(E) << 32 | (uint32_t)t;
          best = key < best ? key : best;
        }
        top = tc > top ? tc : top;
      }
#pragma unroll
      for (int o = L / 2; o > 0; o >>= 1) {
        const uint64_t ob = __shfl_xor((unsigned long long)best, o, L);
        const int ot = __shfl_xor(top, o, L);
        best = ob < best ? ob : best;
        top = ot > top ? ot : top;
      }
      cd = best != kPhotoNone ? 0 : top;
    }
  }
  if (lane != 0) return;
  float tx = 0.f, ty = 0.f, tz = 0.f, E = 0.f;
  int pu = -1, pv = -1;
  if (cd == 0) {
    const int t = (int)(uint32_t)best;
    pu = u + (t % w - r); pv = v + (t / w - r);
    const int64_t i = (int64_t)pv * c.W + pu;
    tx = vmap[i]; ty = vmap[hw + i]; tz = vmap[2 * hw + i];
    E = __uint_as_float((uint32_t)(best >> 32));
  }
  code[p] = (uint8_t)cd;
  flag[p] = cd == 0 ? 1 : 0;
  tgt[3 * p] = tx; tgt[3 * p + 1] = ty; tgt[3 * p + 2] = tz;
  if (warped) { warped[3 * p] = s.x; warped[3 * p + 1] = s.y; warped[3 * p + 2] = s.z; }
  if (pixel) { pixel[2 * p] = pu; pixel[2 * p + 1] = pv; }
  if (cost) cost[p] = E;
}

// assoc.hip's k_assoc_emit (the same slot rule), with the match pixel as a further column
__global__ __launch_bounds__(256) void k_photo_emit(const uint8_t* __restrict__ flag, const int32_t* __restrict__ rank,
                                                     int64_t n, int max_matches, const float* __restrict__ pts,
                                                     const float* __restrict__ tgt, const int32_t* __restrict__ pixel,
                                                     const int4* __restrict__ anchors,
                                                     const float4* __restrict__ weights, int32_t* __restrict__ midx,
                                                     float* __restrict__ src_out, float* __restrict__ tgt_out,
                                                     int4* __restrict__ a_out, float4* __restrict__ w_out,
                                                     float* __restrict__ pixel_out, int32_t* __restrict__ count) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t total = rank[n], mm = max_matches;
  if (p == 0) { count[0] = (int32_t)total; count[1] = (int32_t)(total < mm ? total : mm); }
  if (p >= n || !flag[p]) return;
  const int64_t rk = rank[p];
  int64_t slot = rk;
  if (total > mm) {
    slot = rk * mm / total;
    if (!((rk + 1) * mm / total > slot)) return;
  }
  midx[slot] = (int32_t)p;
  src_out[3 * slot] = pts[3 * p]; src_out[3 * slot + 1] = pts[3 * p + 1]; src_out[3 * slot + 2] = pts[3 * p + 2];
  tgt_out[3 * slot] = tgt[3 * p]; tgt_out[3 * slot + 1] = tgt[3 * p + 1]; tgt_out[3 * slot + 2] = tgt[3 * p + 2];
  a_out[slot] = anchors[p];
  w_out[slot] = weights[p];
  if (pixel_out) { pixel_out[2 * slot] = (float)pixel[2 * p]; pixel_out[2 * slot + 1] = (float)pixel[2 * p + 1]; }
}

}  // namespace ofx

using namespace ofx;

extern "C" {

int ofx_photo_associate(void* handle, const float* points, const float* normals, const float* colors,
                        const int32_t* anchors, const float* weights, const uint8_t* valid, int64_t n_points,
                        const float* packed_nodes, int32_t n_nodes, const ofx_camera* cam, const float* point_image,
                        const float* normal_image, const float* color_image, int32_t height, int32_t width,
                        const ofx_photo_params* prm, uint8_t* code, float* tgt, float* warped, int32_t* pixel,
                        float* cost, int32_t* match_idx, float* src_out, float* tgt_out, int32_t* anchors_out,
                        float* weights_out, float* pixel_out, int32_t* count, ofx_stream_t s) {
  Assoc* a = (Assoc*)handle;
  OFX_CHECK_ARG(a && cam && prm && count, "null handle / camera / params / count");
  OFX_CHECK_ARG(n_points >= 0 && n_points <= a->cap, "n_points %lld outside [0, %lld] (the handle's max_points)",
                (long long)n_points, (long long)a->cap);
  OFX_CHECK_ARG(prm->radius >= 0 && prm->radius <= OFX_PHOTO_RMAX, "radius %d outside [0, %d]", prm->radius,
                OFX_PHOTO_RMAX);
  OFX_CHECK_ARG(prm->geo_weight >= 0.f && std::isfinite(prm->geo_weight), "geo_weight (%g) must be finite and >= 0",
                (double)prm->geo_weight);
  OFX_CHECK_ARG(!std::isnan(prm->color_max), "color_max is NaN");
  OFX_CHECK_ARG(prm->max_matches >= 0, "bad max_matches %d", prm->max_matches);
  OFX_CHECK_ARG(height > 0 && width > 0 && cam->width == width && cam->height == height,
                "the camera (%d x %d) and the images (%d x %d) differ", cam->width, cam->height, width, height);
  hipStream_t hs = as_stream(s);
  if (n_points == 0) {
    OFX_HIP(hipMemsetAsync(count, 0, 2 * sizeof(int32_t), hs));
    return OFX_OK;
  }
  if (int st = check_skinned(points, anchors, weights, packed_nodes, n_nodes,
                             colors && point_image && normal_image && color_image && code && tgt,
                             (uintptr_t)anchors_out | (uintptr_t)weights_out))
    return st;
  OFX_CHECK_ARG(prm->max_matches == 0 || (match_idx && src_out && tgt_out && anchors_out && weights_out),
                "null compacted output");
  OFX_CHECK_ARG(!pixel_out || pixel, "pixel_out needs the per-point pixel buffer");
  const unsigned grid = grid_for(n_points * kPhotoLanes, 256, 1 << 30);
  dispatch_valid_nrm(valid, normals, [&](auto V, auto N) {
    hipLaunchKernelGGL((k_photo_gate<decltype(V)::value, decltype(N)::value, kPhotoLanes>), dim3(grid), dim3(256), 0,
                       hs, points, normals, colors, (const int4*)anchors, (const float4*)weights, valid,
                       (const float4*)packed_nodes, n_nodes, make_cam(cam), point_image, normal_image, color_image,
                       prm->dist_max, prm->cos_min, prm->color_max, prm->geo_weight, prm->radius, n_points, code,
                       a->flag, tgt, warped, pixel, cost);
  });
  OFX_LAUNCH_CHECK();
  int st = scan_flags(a->flag, n_points, a->rank, a->tsum, hs);
  if (st) return st;
  hipLaunchKernelGGL(k_photo_emit, dim3(grid_for(n_points, 256, 1 << 30)), dim3(256), 0, hs, (const uint8_t*)a->flag,
                     (const int32_t*)a->rank, n_points, prm->max_matches, points, (const float*)tgt,
                     (const int32_t*)pixel, (const int4*)anchors, (const float4*)weights, match_idx, src_out, tgt_out,
                     (int4*)anchors_out, (float4*)weights_out, pixel_out, count);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

}  // extern "C"
