// Sub-pixel refinement of the photometric matches: a translation-only, inverse compositional Lucas-Kanade step over a
// small colour patch. ofx_photo_associate picks a whole live pixel by the colour of one pixel; here the (2·half + 1)²
// patch around the point's place in a template image (the frame its colour came from) is aligned with the live frame,
// starting at that pixel, and the point's 3-D target becomes the vertex map interpolated at the refined place. It sits
// outside the solver: the refined target goes into the existing 3-D rows. No reference twin (parity unpinned; restated
// op for op in tests/refine_ref.py). The arithmetic is laid out in include/ofx.h.
//
// k_photo_refine<HALF, L>: L lanes per row (OFX_REFINE_LANES: 16, four rows per wave; the A/B of 4 / 8 / 16 lanes is in
// profiles/refine_bench.json and DESIGN §6: at half 4, 16 lanes hold 6 taps each where 8 hold 11 and leave the register
// file room for one wave per SIMD). Lane l takes the taps t = l, l + L, ... (t = (dy + half)·(2·half + 1) + (dx +
// half)): consecutive lanes read consecutive dx of a patch row. The
// template pass runs once: every lane keeps T and the two gradients of its taps, three channels each, in registers —
// K = ceil(taps / L) taps of 9 floats, the tap loops fully unrolled so that the arrays are indexed by constants (no
// scratch); HALF is a template parameter for that reason. H, b and the squared residual are f64 sums of exact f32·f32
// products: per lane over its taps in order, then over the group by xor shuffles (a + b in one lane is b + a in its
// partner: every lane of a group holds the same bits, so the group's control flow is uniform and a shuffle never reads
// a lane that has left). The order is fixed: two calls give the same bytes. Every load is behind the sample's own
// bounds check (bilin_ok); no address is formed from an unchecked pixel. Lane 0 writes the row.
#include <cmath>

#include "ofx_common.h"

#ifndef OFX_REFINE_LANES
#define OFX_REFINE_LANES 16
#endif

namespace ofx {

constexpr int kRefineLanes = OFX_REFINE_LANES;
static_assert(kRefineLanes == 4 || kRefineLanes == 8 || kRefineLanes == 16 || kRefineLanes == 32,
              "OFX_REFINE_LANES must be 4, 8, 16 or 32");

// the cell of a bilinear sample at (x, y): valid only if all four neighbours lie inside the image (NaN fails)
__device__ __forceinline__ bool bilin_ok(float x, float y, int H, int W, int& x0, int& y0, float& fx, float& fy) {
  const float xf = floorf(x), yf = floorf(y);
  if (!(xf >= 0.f && xf <= (float)(W - 2) && yf >= 0.f && yf <= (float)(H - 2))) return false;
  x0 = (int)xf; y0 = (int)yf;
  fx = x - xf; fy = y - yf;
  return true;
}

// one plane at a valid cell: ((1 - fx)·p00 + fx·p10)·(1 - fy) + ((1 - fx)·p01 + fx·p11)·fy, every step rounded
__device__ __forceinline__ float bilin(const float* __restrict__ p, int W, int x0, int y0, float fx, float fy) {
  const int64_t i = (int64_t)y0 * W + x0;
  const float p00 = p[i], p10 = p[i + 1], p01 = p[i + W], p11 = p[i + W + 1];
  const float wx = 1.f - fx, wy = 1.f - fy;
  const float a0 = wx * p00, a1 = fx * p10, top = a0 + a1;
  const float b0 = wx * p01, b1 = fx * p11, bot = b0 + b1;
  const float c0 = wy * top, c1 = fy * bot;
  return c0 + c1;
}

template <int L>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, L);
  return v;
}

template <int L>
__device__ __forceinline__ int group_or(int v) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, L);
  return v;
}

template <int HALF, int L>
__global__ __launch_bounds__(256) void k_photo_refine(
    const float* __restrict__ timg, const uint8_t* __restrict__ tmask, const float* __restrict__ cimg,
    const float* __restrict__ vmap, const float* __restrict__ tpx, const float* __restrict__ ipx,
    const float* __restrict__ tgt_in, const int32_t* __restrict__ count, int max_rows, int H, int W, int iters,
    float eps, float max_shift, float min_eig, float ssd_max, float edge_max, float* __restrict__ px_out,
    float* __restrict__ tgt_out, uint8_t* __restrict__ status, float* __restrict__ ssd_out) {
  constexpr int WP = 2 * HALF + 1, NT = WP * WP, K = (NT + L - 1) / L;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t row = tid / L;
  const int lane = (int)(tid % L);
  int n = count[1];
  n = n < 0 ? 0 : (n > max_rows ? max_rows : n);
  // a group is whole or absent (256 and the wave are multiples of L), so the shuffles below see all of their lanes
  if (row >= n) return;
  const int64_t hw = (int64_t)H * W;
  const float tx = tpx[2 * row], ty = tpx[2 * row + 1];
  const float ix = ipx[2 * row], iy = ipx[2 * row + 1];
  int st = 0;
  if (!(isfinite(tx) && isfinite(ty) && isfinite(ix) && isfinite(iy)) || (ix == -1.f && iy == -1.f)) st = 1;

  float T[K][3], GX[K][3], GY[K][3];
  double hxx = 0.0, hxy = 0.0, hyy = 0.0;
  if (st == 0) {
    int bad = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int t = lane + k * L;
#pragma unroll
      for (int c = 0; c < 3; ++c) { T[k][c] = 0.f; GX[k][c] = 0.f; GY[k][c] = 0.f; }
      if (t < NT) {
        const int dy = t / WP - HALF, dx = t % WP - HALF;
        // the five samples of a tap: the tap, its right, left, lower and upper neighbour
        float s[5][3];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          const int ox = dx + (j == 1) - (j == 2), oy = dy + (j == 3) - (j == 4);
          const float x = tx + (float)ox, y = ty + (float)oy;
          int x0, y0; float fx, fy;
          bool ok = bilin_ok(x, y, H, W, x0, y0, fx, fy);
          if (ok && tmask) {
            const int64_t i = (int64_t)y0 * W + x0;
            ok = tmask[i] && tmask[i + 1] && tmask[i + W] && tmask[i + W + 1];
          }
#pragma unroll
          for (int c = 0; c < 3; ++c) s[j][c] = ok ? bilin(timg + c * hw, W, x0, y0, fx, fy) : 0.f;
          bad |= !ok;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float gx = 0.5f * (s[1][c] - s[2][c]), gy = 0.5f * (s[3][c] - s[4][c]);
          T[k][c] = s[0][c]; GX[k][c] = gx; GY[k][c] = gy;
          hxx += (double)gx * (double)gx;
          hxy += (double)gx * (double)gy;
          hyy += (double)gy * (double)gy;
        }
      }
    }
    if (group_or<L>(bad)) st = 2;
  }
  double det = 1.0;
  if (st == 0) {
    hxx = group_sum<L>(hxx); hxy = group_sum<L>(hxy); hyy = group_sum<L>(hyy);
    det = hxx * hyy - hxy * hxy;
    const double df = hxx - hyy, tr = hxx + hyy;
    const double lmin = 0.5 * (tr - sqrt(df * df + 4.0 * (hxy * hxy)));
    if (!(det > 0.0) || !(lmin / (double)NT >= (double)min_eig)) st = 3;
  }
  float ux = ix, uy = iy;
  double msr = 0.0;
  if (st == 0) {
    // pass `it` < iters is an iteration; the pass after the last one (or after the freeze) only measures the residual
    bool frozen = false;
    for (int it = 0; st == 0; ++it) {
      const bool last = frozen || it >= iters;
      double bx = 0.0, by = 0.0, rr = 0.0;
      int bad = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int t = lane + k * L;
        if (t < NT) {
          const int dy = t / WP - HALF, dx = t % WP - HALF;
          const float x = ux + (float)dx, y = uy + (float)dy;
          int x0, y0; float fx, fy;
          const bool ok = bilin_ok(x, y, H, W, x0, y0, fx, fy);
          bad |= !ok;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float v = ok ? bilin(cimg + c * hw, W, x0, y0, fx, fy) : 0.f;
            const float r = v - T[k][c];
            bx += (double)GX[k][c] * (double)r;
            by += (double)GY[k][c] * (double)r;
            rr += (double)r * (double)r;
          }
        }
      }
      if (group_or<L>(bad)) { st = 4; break; }
      if (last) { msr = group_sum<L>(rr) / (double)(3 * NT); break; }
      bx = group_sum<L>(bx); by = group_sum<L>(by);
      const double ddx = (hyy * bx - hxy * by) / det, ddy = (hxx * by - hxy * bx) / det;
      ux = (float)((double)ux - ddx);
      uy = (float)((double)uy - ddy);
      const float sx = fabsf(ux - ix), sy = fabsf(uy - iy);
      if (fmaxf(sx, sy) > max_shift) { st = 5; break; }
      frozen = fabs(ddx) < (double)eps && fabs(ddy) < (double)eps;
    }
  }
  if (lane != 0) return;
  float ssd = 0.f, ox = ix, oy = iy;
  float g0 = tgt_in[3 * row], g1 = tgt_in[3 * row + 1], g2 = tgt_in[3 * row + 2];
  if (st == 0) {
    ssd = (float)msr;
    if (!(msr <= (double)ssd_max * (double)ssd_max)) st = 6;
  }
  if (st == 0) {
    int x0, y0; float fx, fy;
    // (the final pass sampled the live frame at (ux, uy) itself, the centre tap: the cell is inside the image)
    if (!bilin_ok(ux, uy, H, W, x0, y0, fx, fy)) {
      st = 4;
    } else {
      const float* zp = vmap + 2 * hw;
      const int64_t i = (int64_t)y0 * W + x0;
      const float z00 = zp[i], z10 = zp[i + 1], z01 = zp[i + W], z11 = zp[i + W + 1];
      const float lo = fminf(fminf(z00, z10), fminf(z01, z11)), hi = fmaxf(fmaxf(z00, z10), fmaxf(z01, z11));
      if (!(z00 > 0.f && z10 > 0.f && z01 > 0.f && z11 > 0.f) || !(hi - lo <= edge_max)) {
        st = 7;
      } else {
        ox = ux; oy = uy;
        g0 = bilin(vmap, W, x0, y0, fx, fy);
        g1 = bilin(vmap + hw, W, x0, y0, fx, fy);
        g2 = bilin(zp, W, x0, y0, fx, fy);
      }
    }
  }
  px_out[2 * row] = ox; px_out[2 * row + 1] = oy;
  tgt_out[3 * row] = g0; tgt_out[3 * row + 1] = g1; tgt_out[3 * row + 2] = g2;
  status[row] = (uint8_t)st;
  ssd_out[row] = ssd;
}

template <int HALF>
static void launch_refine(unsigned grid, hipStream_t hs, const float* timg, const uint8_t* tmask, const float* cimg,
                          const float* vmap, const float* tpx, const float* ipx, const float* tgt_in,
                          const int32_t* count, int max_rows, int H, int W, const ofx_refine_params* p, float* px_out,
                          float* tgt_out, uint8_t* status, float* ssd) {
  hipLaunchKernelGGL((k_photo_refine<HALF, kRefineLanes>), dim3(grid), dim3(256), 0, hs, timg, tmask, cimg, vmap, tpx,
                     ipx, tgt_in, count, max_rows, H, W, p->iters, p->eps, p->max_shift, p->min_eig, p->ssd_max,
                     p->edge_max, px_out, tgt_out, status, ssd);
}

}  // namespace ofx

using namespace ofx;

extern "C" {

int ofx_photo_refine(const float* template_image, const uint8_t* template_mask, const float* color_image,
                     const float* point_image, const float* template_px, const float* init_px, const float* tgt_in,
                     const int32_t* count, int32_t max_rows, int32_t height, int32_t width,
                     const ofx_refine_params* prm, float* px_out, float* tgt_out, uint8_t* status, float* ssd,
                     ofx_stream_t s) {
  OFX_CHECK_ARG(prm && count, "null params / count");
  OFX_CHECK_ARG(prm->half >= 1 && prm->half <= OFX_REFINE_HMAX, "half %d outside [1, %d]", prm->half, OFX_REFINE_HMAX);
  OFX_CHECK_ARG(prm->iters >= 1, "iters (%d) must be at least 1", prm->iters);
  OFX_CHECK_ARG(prm->eps >= 0.f && std::isfinite(prm->eps), "eps (%g) must be finite and >= 0", (double)prm->eps);
  OFX_CHECK_ARG(prm->max_shift >= 0.f && std::isfinite(prm->max_shift), "max_shift (%g) must be finite and >= 0",
                (double)prm->max_shift);
  OFX_CHECK_ARG(prm->min_eig >= 0.f && std::isfinite(prm->min_eig), "min_eig (%g) must be finite and >= 0",
                (double)prm->min_eig);
  OFX_CHECK_ARG(prm->edge_max >= 0.f && std::isfinite(prm->edge_max), "edge_max (%g) must be finite and >= 0",
                (double)prm->edge_max);
  OFX_CHECK_ARG(!std::isnan(prm->ssd_max), "ssd_max is NaN");
  OFX_CHECK_ARG(height >= 1 && width >= 1, "bad image size %d x %d", width, height);
  OFX_CHECK_ARG(max_rows >= 0, "bad max_rows %d", max_rows);
  OFX_CHECK_ARG(((uintptr_t)count & 3) == 0, "count must be 4-byte aligned");
  if (max_rows == 0) return OFX_OK;
  OFX_CHECK_ARG(template_image && color_image && point_image && template_px && init_px && tgt_in && px_out &&
                    tgt_out && status && ssd, "null buffer");
  OFX_CHECK_ARG((((uintptr_t)template_image | (uintptr_t)color_image | (uintptr_t)point_image |
                  (uintptr_t)template_px | (uintptr_t)init_px | (uintptr_t)tgt_in | (uintptr_t)px_out |
                  (uintptr_t)tgt_out | (uintptr_t)ssd) & 3) == 0, "float buffers must be 4-byte aligned");
  const unsigned grid = grid_for((int64_t)max_rows * kRefineLanes, 256, 1 << 30);
  hipStream_t hs = as_stream(s);
#define OFX_REFINE_CASE(h)                                                                                            \
  case h:                                                                                                             \
    launch_refine<h>(grid, hs, template_image, template_mask, color_image, point_image, template_px, init_px, tgt_in, \
                     count, max_rows, height, width, prm, px_out, tgt_out, status, ssd);                              \
    break;
  switch (prm->half) {
    OFX_REFINE_CASE(1)
    OFX_REFINE_CASE(2)
    OFX_REFINE_CASE(3)
    OFX_REFINE_CASE(4)
  }
#undef OFX_REFINE_CASE
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

}  // extern "C"
