// Depth-frame preparation in front of the tracker: a bilateral filter of the depth image, the vertex map of the filtered
// depth and its normal map. KinectFusion and DynamicFusion track against such a map and integrate the raw depth; the
// reference has no twin (parity unpinned; restated op for op in tests/prepare_ref.py).
//
//   D   = the depth in metres (f32, or u16 / normalizer: ofx_backproject_depth's expression)
//   hole: !(D_c > 0) (NaN included) -> 0 in every output
//   taps: dv = -r..r outer, du = -r..r inner; a tap N is skipped when it lies outside the image, when !(N > 0), or when
//         |N - D_c| > range_cut (f32) — a skipped tap is a hole, so nothing bleeds across a depth edge
//   w   = ws·wr, ws = f32(exp(a_s·(du² + dv²))) (host table, f64 exp), wr = f32(exp(a_r·(f64(diff)·f64(diff)))), a = -0.5/σ²
//         in f64: the skinning weight's convention, f32 of the f64 exp
//   num += w·N, den += w in f32, in tap order; filtered depth = num / den, correctly rounded. The centre tap is always
//   taken with weight exactly 1 — what the formulas give for diff = 0, and held for a +inf centre too, whose own diff
//   would be inf - inf — so den >= 1 and radius 0 returns D_c exactly.
//   vertex = ofx_backproject_depth's of the filtered depth (backproject_px), zeros where it is not > 0
//   normal = the gate's n_q of that vertex map at the pixel (gate_device.h: vertex_normal), zeros where the gate would
//            return code 3 or 4
//
// k_prepare_filter: one workgroup per 32 x 8 pixel tile, the tile and its r-pixel halo of D staged in LDS ((32 + 2r)·(8 +
// 2r) floats, 2560 B at r = 4; pixels outside the image staged as holes). A wave is two tile rows of 32, so every tap
// is a ds_read_b32 of 32 consecutive words per half wave: no bank conflict at any row stride. One thread per pixel; a
// hole leaves at once; the f64 exp runs only for the taps that pass both tests. The spatial table rides in the kernel
// arguments and is indexed by the (uniform) tap counter.
// k_prepare_normals: one thread per pixel over the vertex map just written (L2-resident), proj_gate's five clamped
// pixels. The normals need the filtered neighbours across tile edges; a second small launch keeps the filter free of a
// redundantly filtered halo ring.
#include <cmath>

#include "ofx_common.h"
#include "gate_device.h"

namespace ofx {

constexpr int kPrepTW = 32, kPrepTH = 8;              // pixel tile of one workgroup
constexpr int kPrepTaps = (2 * OFX_PREPARE_RMAX + 1) * (2 * OFX_PREPARE_RMAX + 1);

struct PrepWs {
  float v[kPrepTaps];   // the first (2r + 1)² entries: ws in tap order
};

template <bool U16>
__global__ __launch_bounds__(256) void k_prepare_filter(const void* __restrict__ depth, float* __restrict__ depth_out,
                                                         float* __restrict__ pimg, int H, int W, int tiles_x, float fx,
                                                         float fy, float cx, float cy, float normalizer, int r,
                                                         float range_cut, double a_r, PrepWs ws) {
  __shared__ float tile[(kPrepTH + 2 * OFX_PREPARE_RMAX) * (kPrepTW + 2 * OFX_PREPARE_RMAX)];
  const int sw = kPrepTW + 2 * r, sh = kPrepTH + 2 * r;
  const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kPrepTW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kPrepTH;
  for (int i = threadIdx.x; i < sw * sh; i += 256) {
    const int ty = i / sw, tx = i - ty * sw;
    const int gx = x0 + tx - r, gy = y0 + ty - r;
    float d = 0.f;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) d = depth_px<U16>(depth, (int64_t)gy * W + gx, normalizer);
    tile[i] = d;
  }
  __syncthreads();
  const int lx = threadIdx.x & (kPrepTW - 1), ly = threadIdx.x / kPrepTW;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= W || y >= H) return;
  const int64_t hw = (int64_t)H * W, p = (int64_t)y * W + x;
  const float* centre = tile + (ly + r) * sw + (lx + r);
  const float dc = centre[0];
  float f = 0.f, X = 0.f, Y = 0.f, Z = 0.f;
  if (dc > 0.f) {
    float num = 0.f, den = 0.f;
    int k = 0;
#pragma unroll 1
    for (int dv = -r; dv <= r; ++dv) {
#pragma unroll 1
      for (int du = -r; du <= r; ++du, ++k) {
        const float n = centre[dv * sw + du];
        const float diff = n - dc;
        const bool own = (du | dv) == 0;   // the centre tap: always taken, wr = 1 (what diff = 0 gives; +inf too)
        if (!own && (!(n > 0.f) || fabsf(diff) > range_cut)) continue;
        const float wr = own ? 1.f : (float)exp(a_r * ((double)diff * (double)diff));
        const float w = ws.v[k] * wr;
        num = num + w * n;
        den = den + w;
      }
    }
    f = cdiv(num, den);
    if (f > 0.f) {
      backproject_px(f, x, y, fx, fy, cx, cy, X, Y);
      Z = f;
    }
  }
  depth_out[p] = f;
  pimg[p] = X;
  pimg[hw + p] = Y;
  pimg[2 * hw + p] = Z;
}

__global__ __launch_bounds__(256) void k_prepare_normals(const float* __restrict__ vmap, int H, int W, float edge_max,
                                                          float* __restrict__ nimg) {
  const int64_t hw = (int64_t)H * W;
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= hw) return;
  const int u = (int)(p % W), v = (int)(p / W);
  const int64_t il = (int64_t)v * W + max(u - 1, 0), ir = (int64_t)v * W + min(u + 1, W - 1);
  const int64_t iu = (int64_t)max(v - 1, 0) * W + u, id = (int64_t)min(v + 1, H - 1) * W + u;
  const float qx = vmap[p], qy = vmap[hw + p], qz = vmap[2 * hw + p];
  const float lx = vmap[il], ly = vmap[hw + il], lz = vmap[2 * hw + il];
  const float rx = vmap[ir], ry = vmap[hw + ir], rz = vmap[2 * hw + ir];
  const float ux = vmap[iu], uy = vmap[hw + iu], uz = vmap[2 * hw + iu];
  const float dx = vmap[id], dy = vmap[hw + id], dz = vmap[2 * hw + id];
  const bool border = u == 0 || v == 0 || u == W - 1 || v == H - 1;
  float nx, ny, nz;
  if (vertex_normal(border, qx, qy, qz, lx, ly, lz, rx, ry, rz, ux, uy, uz, dx, dy, dz, edge_max, nx, ny, nz) != 0) {
    nx = 0.f; ny = 0.f; nz = 0.f;
  }
  nimg[p] = nx;
  nimg[hw + p] = ny;
  nimg[2 * hw + p] = nz;
}

// Observation weights of the weighted integrate (ofx_observation_weights; ofx.h spells the arithmetic out): one thread per
// pixel over the vertex and normal maps just written (L2-resident), six coalesced planar loads and one store. COSP is
// the angle term's power (0, 1 or 2: no powf).
template <int COSP>
__global__ __launch_bounds__(256) void k_observation_weights(const float* __restrict__ pimg, const float* __restrict__ nimg,
                                                              int64_t hw, float z_ref, float w_floor, float edge_weight,
                                                              float* __restrict__ obs) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= hw) return;
  const float px = pimg[p], py = pimg[hw + p], pz = pimg[2 * hw + p];
  const float nx = nimg[p], ny = nimg[hw + p], nz = nimg[2 * hw + p];
  float w;
  if (!(pz > 0.f)) {
    w = 0.f;
  } else if (nx == 0.f && ny == 0.f && nz == 0.f) {
    w = edge_weight;
  } else {
    const float dot = (nx * px + ny * py) + nz * pz;
    const float ss = (px * px + py * py) + pz * pz;
    float c = cdiv(-dot, (float)sqrt((double)ss));
    if (!(c > 0.f)) c = 0.f;   // (a NaN too)
    if (c > 1.f) c = 1.f;
    const float a = COSP == 0 ? 1.f : COSP == 1 ? c : c * c;
    float sc = 1.f;
    if (z_ref != 0.f) {
      const float r = cdiv(z_ref, pz);
      sc = fminf(1.f, r * r);
    }
    w = fmaxf(w_floor, a * sc);
  }
  obs[p] = w;
}

}  // namespace ofx

using namespace ofx;

extern "C" {

int ofx_prepare_depth(const void* depth, int32_t is_u16, int32_t height, int32_t width, const ofx_camera* cam,
                      const ofx_prepare_params* prm, float* depth_out, float* point_image, float* normal_image,
                      ofx_stream_t s) {
  OFX_CHECK_ARG(cam && prm, "null camera / params");
  OFX_CHECK_ARG(prm->radius >= 0 && prm->radius <= OFX_PREPARE_RMAX, "radius %d outside [0, %d]", prm->radius,
                OFX_PREPARE_RMAX);
  OFX_CHECK_ARG(prm->sigma_s > 0.f && prm->sigma_r > 0.f, "sigma_s (%g) and sigma_r (%g) must be positive",
                (double)prm->sigma_s, (double)prm->sigma_r);
  OFX_CHECK_ARG(prm->range_cut > 0.f, "range_cut (%g) must be positive", (double)prm->range_cut);
  OFX_CHECK_ARG(height >= 1 && width >= 1 && cam->width == width && cam->height == height,
                "the camera (%d x %d) and the depth image (%d x %d) differ, or the image is empty", cam->width,
                cam->height, width, height);
  OFX_CHECK_ARG(depth && depth_out && point_image, "null buffer");
  const int64_t tiles_x = ((int64_t)width + kPrepTW - 1) / kPrepTW, tiles_y = ((int64_t)height + kPrepTH - 1) / kPrepTH;
  OFX_CHECK_ARG(tiles_x * tiles_y < ((int64_t)1 << 31), "depth image too large (%d x %d)", width, height);
  const int r = prm->radius;
  PrepWs ws{};
  const double a_s = -0.5 / ((double)prm->sigma_s * (double)prm->sigma_s);
  const double a_r = -0.5 / ((double)prm->sigma_r * (double)prm->sigma_r);
  int k = 0;
  for (int dv = -r; dv <= r; ++dv)
    for (int du = -r; du <= r; ++du) ws.v[k++] = (float)std::exp(a_s * (double)(du * du + dv * dv));
  hipStream_t hs = as_stream(s);
  const dim3 grid((unsigned)(tiles_x * tiles_y));
  if (is_u16)
    hipLaunchKernelGGL(k_prepare_filter<true>, grid, dim3(256), 0, hs, depth, depth_out, point_image, height, width,
                       (int)tiles_x, cam->fx, cam->fy, cam->cx, cam->cy, prm->normalizer, r, prm->range_cut, a_r, ws);
  else
    hipLaunchKernelGGL(k_prepare_filter<false>, grid, dim3(256), 0, hs, depth, depth_out, point_image, height, width,
                       (int)tiles_x, cam->fx, cam->fy, cam->cx, cam->cy, prm->normalizer, r, prm->range_cut, a_r, ws);
  if (normal_image)
    hipLaunchKernelGGL(k_prepare_normals, dim3(grid_for((int64_t)height * width, 256, 1 << 30)), dim3(256), 0, hs,
                       (const float*)point_image, height, width, prm->edge_max, normal_image);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

int ofx_observation_weights(const float* point_image, const float* normal_image, int32_t height, int32_t width,
                            const ofx_obs_params* prm, float* obs_im, ofx_stream_t s) {
  OFX_CHECK_ARG(prm, "null params");
  OFX_CHECK_ARG(prm->cos_power >= 0 && prm->cos_power <= 2, "cos_power %d outside {0, 1, 2}", prm->cos_power);
  OFX_CHECK_ARG(prm->z_ref >= 0.f && std::isfinite(prm->z_ref), "z_ref (%g) must be finite and >= 0", (double)prm->z_ref);
  OFX_CHECK_ARG(prm->w_floor >= 0.f && std::isfinite(prm->w_floor), "w_floor (%g) must be finite and >= 0",
                (double)prm->w_floor);
  OFX_CHECK_ARG(prm->edge_weight >= 0.f && std::isfinite(prm->edge_weight), "edge_weight (%g) must be finite and >= 0",
                (double)prm->edge_weight);
  OFX_CHECK_ARG(height >= 1 && width >= 1 && (int64_t)height * width < ((int64_t)1 << 31), "bad image size %d x %d", width,
                height);
  OFX_CHECK_ARG(point_image && normal_image && obs_im, "null buffer");
  OFX_CHECK_ARG(((reinterpret_cast<uintptr_t>(point_image) | reinterpret_cast<uintptr_t>(normal_image) |
                  reinterpret_cast<uintptr_t>(obs_im)) & 3) == 0, "buffers must be 4-byte aligned");
  const int64_t hw = (int64_t)height * width;
  const dim3 grid(grid_for(hw, 256, 1 << 30));
  hipStream_t hs = as_stream(s);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, hs, point_image, normal_image, hw, prm->z_ref, prm->w_floor,
                       prm->edge_weight, obs_im);
  };
  if (prm->cos_power == 0) go(k_observation_weights<0>);
  else if (prm->cos_power == 1) go(k_observation_weights<1>);
  else go(k_observation_weights<2>);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

}  // extern "C"
