// Model z-buffer: the warped model points splatted as oriented discs into a depth / index image of the live frame, and
// the occlusion code of every point against it.
//
// The reference sees the live model through marching cubes, a warp of the mesh and an external renderer
// (tsdf.get_deformed_model, NonRigidICP/model/point_render.py); nothing there is per point and nothing runs per ICP
// iteration. Here the model is already a set of skinned, oriented surface points (ofx_surface_points), so the live view
// is a z-buffer of their discs (no reference twin, parity unpinned; restated op for op in tests/splat_ref.py):
//
//   x', n' = ofx_associate's warped point and normalised warped normal     (gate_device.h: the same bits)
//   (u, v) = pixel of x'                                                   (gate_device.h: pixel_of)
//   codes, first that applies: 1 invalid skin, 2 non-finite / behind the camera / off the image, 3 back-facing
//   (!(s < 0), s = n'.x'); then 4 occluded ((z' - depth[v,u]) > occl_margin) or 0 visible, once the buffer is complete
//   footprint of a live point: |du| <= ru, |dv| <= rv, r = clamp(ceil(f*rho / z'), 0, OFX_SPLAT_RMAX); the centre pixel
//   takes z'; any other pixel the hit z_p = s / (n'.d) of its ray d = ((uu - cx)/fx, (vv - cy)/fy, 1) on the point's
//   tangent plane, kept if the hit lies within rho of x' (a true disc: an ellipse on the image)
//   write: 64-bit unsigned atomic minimum of (bits(z_p) << 32 | p) — z_p > 0 and finite, so the bits order as the
//   floats do; ties go to the lower index; a minimum does not depend on arrival order, so the buffer is a pure function
//   of the inputs
//
// Three launches: k_splat_clear (the library's own fill, no runtime memset: DESIGN §8), k_splat (one thread per point:
// trip 1 the point, its normal, anchors, weights and valid flag, trip 2 the four node records, then the footprint loop
// of no-return atomics) and k_splat_resolve (one grid over the pixels and then the points).
#include "ofx_common.h"
#include "gate_device.h"

namespace ofx {

constexpr unsigned long long kSplatEmpty = ~0ull;

struct Splat {
  int64_t cap_points = 0, cap_pixels = 0;
  unsigned long long* zbuf = nullptr;   // [cap_pixels] (bits(z) << 32 | point), kSplatEmpty = nothing written
  int32_t* ppix = nullptr;              // [cap_points] pixel of a live point, -code (-1, -2, -3) of a rejected one
  float* pz = nullptr;                  // [cap_points] z' of a live point
};

__global__ __launch_bounds__(256) void k_splat_clear(unsigned long long* __restrict__ zbuf, int64_t n) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) zbuf[i] = kSplatEmpty;
}

__device__ __forceinline__ int splat_extent(float f, float rho, float z) {
  const float r = ceilf(cdiv(f * rho, z));
  return r >= (float)OFX_SPLAT_RMAX ? OFX_SPLAT_RMAX : (r > 0.f ? (int)r : 0);
}

// VALID / NRM: valid / normals given (compile-time, as k_assoc_gate)
template <bool VALID, bool NRM>
__global__ __launch_bounds__(256) void k_splat(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                const int4* __restrict__ anchors, const float4* __restrict__ weights,
                                                const uint8_t* __restrict__ valid, const float4* __restrict__ nodes,
                                                int n_nodes, CamD c, float rho, int64_t n,
                                                unsigned long long* __restrict__ zbuf, int32_t* __restrict__ ppix,
                                                float* __restrict__ pz, float* __restrict__ warped,
                                                float* __restrict__ warped_n) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= n) return;
  SkinPt sk;
  const bool ok = skin_load<VALID, NRM>(pts, nrm, anchors, weights, valid, n_nodes, p, -1.f, sk);   // no normal: (0, 0, -1)
  float &x = sk.x, &y = sk.y, &z = sk.z, &nx = sk.nx, &ny = sk.ny, &nz = sk.nz;
  int32_t pix32 = -1;
  if (ok) {
    skin_warp<NRM>(nodes, sk);
    const int64_t pix = pixel_of(c, x, y, z);
    pix32 = -2;
    if (pix >= 0) {
      const float s = (nx * x + ny * y) + nz * z;
      pix32 = -3;
      if (s < 0.f) {
        pix32 = (int32_t)pix;
        const int u = (int)(pix % c.W), v = (int)(pix / c.W);
        const int ru = splat_extent(c.fxf, rho, z), rv = splat_extent(c.fyf, rho, z);
        const float rho2 = rho * rho;
        const unsigned long long lo = (unsigned long long)(uint32_t)p;
        const int v0 = max(v - rv, 0), v1 = min(v + rv, c.H - 1);
        const int u0 = max(u - ru, 0), u1 = min(u + ru, c.W - 1);
        for (int vv = v0; vv <= v1; ++vv) {
          const float dy = cdiv((float)vv - c.cyf, c.fyf);
          for (int uu = u0; uu <= u1; ++uu) {
            float zp = z;
            if (uu != u || vv != v) {
              const float dx = cdiv((float)uu - c.cxf, c.fxf);
              const float den = (nx * dx + ny * dy) + nz;
              zp = cdiv(s, den);
              const float ex = dx * zp - x, ey = dy * zp - y, ez = zp - z;
              const float d2 = (ex * ex + ey * ey) + ez * ez;
              if (!(den < 0.f && zp > 0.f && isfinite(zp) && d2 <= rho2)) continue;
            }
            const unsigned long long key = ((unsigned long long)__float_as_uint(zp) << 32) | lo;
            atomicMin(zbuf + ((int64_t)vv * c.W + uu), key);   // no-return
          }
        }
      }
    }
  }
  ppix[p] = pix32;
  pz[p] = z;
  if (warped) { warped[3 * p] = x; warped[3 * p + 1] = y; warped[3 * p + 2] = z; }
  if (NRM && warped_n) { warped_n[3 * p] = nx; warped_n[3 * p + 1] = ny; warped_n[3 * p + 2] = nz; }
}

// threads [0, n_pix): the pixel's depth and index; threads [n_pix, n_pix + n): the point's code
__global__ __launch_bounds__(256) void k_splat_resolve(const unsigned long long* __restrict__ zbuf, int64_t n_pix,
                                                        const int32_t* __restrict__ ppix, const float* __restrict__ pz,
                                                        int64_t n, float margin, float* __restrict__ depth,
                                                        int32_t* __restrict__ index, uint8_t* __restrict__ code) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n_pix) {
    const unsigned long long key = zbuf[i];
    const bool hit = key != kSplatEmpty;
    if (depth) depth[i] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
    if (index) index[i] = hit ? (int32_t)(uint32_t)key : -1;
    return;
  }
  const int64_t p = i - n_pix;
  if (p >= n || !code) return;
  const int32_t pix = ppix[p];
  int cd = -pix;
  if (pix >= 0) {
    // a live point wrote its own pixel, so the word is never empty here
    const float d = __uint_as_float((uint32_t)(zbuf[pix] >> 32));
    cd = (pz[p] - d) > margin ? 4 : 0;
  }
  code[p] = (uint8_t)cd;
}

}  // namespace ofx

using namespace ofx;

extern "C" {

int ofx_splat_create(int64_t max_points, int64_t max_pixels, void** handle) {
  OFX_CHECK_ARG(handle, "null handle");
  *handle = nullptr;
  OFX_CHECK_ARG(max_points >= 0 && max_pixels >= 0, "bad max_points / max_pixels");
  if (max_points >= ((int64_t)1 << 31) - 1 || max_pixels >= ((int64_t)1 << 31) - 1) {
    set_error("max_points %lld / max_pixels %lld exceed the 32-bit point and pixel indices", (long long)max_points,
              (long long)max_pixels);
    return OFX_ERR_RANGE;
  }
  Splat* h = new Splat();
  h->cap_points = max_points;
  h->cap_pixels = max_pixels;
  if (hipMalloc((void**)&h->zbuf, ((size_t)max_pixels + 1) * sizeof(unsigned long long)) != hipSuccess ||
      hipMalloc((void**)&h->ppix, ((size_t)max_points + 4) * sizeof(int32_t)) != hipSuccess ||
      hipMalloc((void**)&h->pz, ((size_t)max_points + 4) * sizeof(float)) != hipSuccess) {
    for (void* p : {(void*)h->zbuf, (void*)h->ppix, (void*)h->pz})
      if (p) (void)hipFree(p);
    delete h;
    set_error("ofx_splat_create: a z-buffer of %lld pixels and scratch for %lld points could not be allocated",
              (long long)max_pixels, (long long)max_points);
    return OFX_ERR_ALLOC;
  }
  *handle = h;
  return OFX_OK;
}

int ofx_splat_destroy(void* handle) {
  if (!handle) return OFX_OK;
  Splat* h = (Splat*)handle;
  (void)hipDeviceSynchronize();
  for (void* p : {(void*)h->zbuf, (void*)h->ppix, (void*)h->pz})
    if (p) (void)hipFree(p);
  delete h;
  return OFX_OK;
}

int ofx_splat_points(void* handle, const float* points, const float* normals, const int32_t* anchors,
                     const float* weights, const uint8_t* valid, int64_t n_points, const float* packed_nodes,
                     int32_t n_nodes, const ofx_camera* cam, const ofx_splat_params* prm, float* depth, int32_t* index,
                     uint8_t* code, float* warped, float* warped_normals, ofx_stream_t s) {
  Splat* h = (Splat*)handle;
  OFX_CHECK_ARG(h && cam && prm, "null handle / camera / params");
  OFX_CHECK_ARG(n_points >= 0 && n_points <= h->cap_points, "n_points %lld outside [0, %lld] (the handle's max_points)",
                (long long)n_points, (long long)h->cap_points);
  OFX_CHECK_ARG(cam->width > 0 && cam->height > 0, "bad image size %d x %d", cam->width, cam->height);
  const int64_t n_pix = (int64_t)cam->width * cam->height;
  OFX_CHECK_ARG(n_pix <= h->cap_pixels, "%d x %d pixels exceed the handle's max_pixels (%lld)", cam->width, cam->height,
                (long long)h->cap_pixels);
  OFX_CHECK_ARG(prm->splat_radius >= 0.f && prm->splat_radius <= 3.402823466e38f, "bad splat_radius %g",
                (double)prm->splat_radius);
  OFX_CHECK_ARG(prm->occl_margin == prm->occl_margin, "occl_margin is NaN");
  OFX_CHECK_ARG(!warped_normals || normals, "warped_normals without normals");
  hipStream_t hs = as_stream(s);
  hipLaunchKernelGGL(k_splat_clear, dim3(grid_for(n_pix, 256, 1 << 30)), dim3(256), 0, hs, h->zbuf, n_pix);
  OFX_LAUNCH_CHECK();
  if (n_points > 0) {
    if (int st = check_skinned(points, anchors, weights, packed_nodes, n_nodes)) return st;
    const unsigned grid = grid_for(n_points, 256, 1 << 30);
    dispatch_valid_nrm(valid, normals, [&](auto V, auto N) {
      hipLaunchKernelGGL((k_splat<decltype(V)::value, decltype(N)::value>), dim3(grid), dim3(256), 0, hs, points,
                         normals, (const int4*)anchors, (const float4*)weights, valid, (const float4*)packed_nodes,
                         n_nodes, make_cam(cam), prm->splat_radius, n_points, h->zbuf, h->ppix, h->pz, warped,
                         warped_normals);
    });
    OFX_LAUNCH_CHECK();
  }
  if (depth || index || (code && n_points > 0)) {
    hipLaunchKernelGGL(k_splat_resolve, dim3(grid_for(n_pix + n_points, 256, 1 << 30)), dim3(256), 0, hs,
                       (const unsigned long long*)h->zbuf, n_pix, (const int32_t*)h->ppix, (const float*)h->pz,
                       n_points, prm->occl_margin, depth, index, code);
    OFX_LAUNCH_CHECK();
  }
  return OFX_OK;
}

}  // extern "C"
