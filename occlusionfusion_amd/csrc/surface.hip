// Skinned surface points of the TSDF: the tracking model read off the bricked volume and the skin cache.
//
// The reference refreshes its model every frame by marching cubes plus a k-NN skin of the vertices (tsdf.get_deformed_model
// / optimizer.update in fusion_tests/lepard_nicp_test.py:471,537). Tracking needs no triangles: one pass over the skin
// cache's listed bricks takes, per voxel just in front of the zero level, the surface point below it (one Newton step
// along the central-difference gradient), the outward normal, and the voxel's own cached anchors and weights. The skin a
// point gets is the skin the integrate warps its voxel with, so the tracked and the fused model move identically. No
// reference twin (parity unpinned; restated op for op in tests/surface_ref.py). The contract is in include/ofx.h.
//
//   k_surface_classify  one 256-thread workgroup per listed brick, voxels l and l + 256 per thread. Trip 1: the brick's
//                       tsdf and weight (into LDS) and the codes 1-3. Most listed bricks are far from the surface: the
//                       workgroup-uniform "no voxel passed" leaves here with a zero count. Trip 2, surviving bricks only:
//                       the face layers of the six adjacent bricks into LDS (face neighbours only: no 10³ halo), codes
//                       4-6 from LDS. Trip 3, surviving lanes only: the cached anchors (code 7). Per wave the accepted
//                       lanes as a 64-bit ballot (8 words per brick), per brick their count.
//   k_surface_offsets   one workgroup of 1024: exclusive scan of the n_list counts (4096 a trip), count = [accepted,
//                       emitted].
//   k_surface_emit      one workgroup per listed brick (empty ones leave after one load): in-brick rank by popcounts of
//                       the ballots, row by the thinning rule, then the point from seven L2-resident gathers and the skin.
//   k_surface_pad       rows [emitted, max_points): the defined padding.
// Order comes from the counts and the scan, never from atomics: two runs give the same bytes.
#include "ofx_common.h"
#include "warp_device.h"

namespace ofx {

struct Surface {
  int32_t cap = 0;
  int32_t* cnt = nullptr;    // [cap] accepted voxels per listed brick
  int32_t* off = nullptr;    // [cap + 1] their exclusive scan, the total at [n_list]
  uint64_t* bits = nullptr;  // [cap * 8] accepted voxels of a brick, bit (l & 63) of word (l >> 6)
};

namespace {

__device__ __forceinline__ void brick_origin(const BrickGeom& g, int64_t b, int& i0, int& j0, int& k0) {
  const int64_t bz = b % g.nbz, r = b / g.nbz;
  const int64_t by = r % g.nby, bx = r / g.nby;   // whole volume: bx0 = 0
  i0 = (int)bx * kBrick; j0 = (int)by * kBrick; k0 = (int)bz * kBrick;
}

__device__ __forceinline__ int64_t vox_slot(const BrickGeom& g, int i, int j, int k) {
  const int64_t b = ((int64_t)(i >> 3) * g.nby + (j >> 3)) * g.nbz + (k >> 3);
  return b * kBrickVox + (((i & 7) * kBrick + (j & 7)) * kBrick + (k & 7));
}

// gradient of the seven values -> normal and surface point; false: degenerate (code 6)
__device__ __forceinline__ bool newton_point(float phi, const float nb[6], float two_h, float cx, float cy, float cz,
                                             float p[3], float n[3]) {
  const float gx = nb[1] - nb[0], gy = nb[3] - nb[2], gz = nb[5] - nb[4];
  const float l2 = (gx * gx + gy * gy) + gz * gz;
  if (!(l2 > 0.f) || !isfinite(l2)) return false;
  const float len = (float)sqrt((double)l2);
  if (phi > len) return false;
  n[0] = cdiv(gx, len); n[1] = cdiv(gy, len); n[2] = cdiv(gz, len);
  const float t = cdiv(phi * two_h, len);
  p[0] = cx - n[0] * t; p[1] = cy - n[1] * t; p[2] = cz - n[2] * t;
  return true;
}

constexpr int kFace = 64;   // voxels of one face layer

__global__ __launch_bounds__(256) void k_surface_classify(BrickGeom g, const float* __restrict__ tsdf,
                                                           const float* __restrict__ weight,
                                                           const int32_t* __restrict__ list,
                                                           const ushort4* __restrict__ anchors, float w_min, float two_h,
                                                           uint8_t* __restrict__ code, int32_t* __restrict__ cnt,
                                                           uint64_t* __restrict__ bits) {
  __shared__ float s_t[kBrickVox + 6 * kFace];   // the brick, then the faces -x +x -y +y -z +z
  __shared__ float s_w[kBrickVox + 6 * kFace];
  __shared__ int s_cnt[8];
  const int tid = threadIdx.x;
  const int64_t slot = blockIdx.x;
  const int64_t b = list[slot];
  if ((uint64_t)b >= (uint64_t)g.n_bricks) {   // (workgroup-uniform) not a brick of this volume: nothing is read
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (code) code[slot * kBrickVox + tid + 256 * h] = 1;
    if ((tid & 63) == 0) { bits[slot * 8 + (tid >> 6)] = 0; bits[slot * 8 + 4 + (tid >> 6)] = 0; }
    if (tid == 0) cnt[slot] = 0;
    return;
  }
  int i0, j0, k0;
  brick_origin(g, b, i0, j0, k0);
  const int ly = (tid >> 3) & 7, lz = tid & 7;
  const int j = j0 + ly, k = k0 + lz;
  // ---- trip 1
  float phi[2], wv[2];
  int cd[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int l = tid + 256 * h;
    phi[h] = tsdf[b * kBrickVox + l];
    wv[h] = weight[b * kBrickVox + l];
  }
  bool pass = false;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int l = tid + 256 * h;
    const int i = i0 + (tid >> 6) + 4 * h;
    s_t[l] = phi[h];
    s_w[l] = wv[h];
    const bool inner = i > 0 && j > 0 && k > 0 && i < g.Dx - 1 && j < g.Dy - 1 && k < g.Dz - 1;
    cd[h] = !inner ? 1 : !(wv[h] >= w_min) ? 2 : !(phi[h] >= 0.f && phi[h] < 1.f) ? 3 : 0;
    pass |= cd[h] == 0;
  }
  if (!__syncthreads_or(pass)) {   // (workgroup-uniform) far from the surface: nothing more is loaded
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (code) code[slot * kBrickVox + tid + 256 * h] = (uint8_t)cd[h];
    if ((tid & 63) == 0) { bits[slot * 8 + (tid >> 6)] = 0; bits[slot * 8 + 4 + (tid >> 6)] = 0; }
    if (tid == 0) cnt[slot] = 0;
    return;
  }
  // ---- trip 2: the six face layers (384 voxels, tsdf and weight); cells outside the volume are never read back
  for (int e = tid; e < 6 * kFace; e += 256) {
    const int f = e >> 6, a = (e >> 3) & 7, c = e & 7;
    const int ax = f >> 1, d = (f & 1) ? kBrick : -1;
    const int i = i0 + (ax == 0 ? d : a), jj = j0 + (ax == 1 ? d : ax == 0 ? a : c), kk = k0 + (ax == 2 ? d : c);
    const bool in = i >= 0 && jj >= 0 && kk >= 0 && i < g.Dx && jj < g.Dy && kk < g.Dz;
    float t = 0.f, w = 0.f;
    if (in) {
      const int64_t v = vox_slot(g, i, jj, kk);
      t = tsdf[v];
      w = weight[v];
    }
    s_t[kBrickVox + e] = t;
    s_w[kBrickVox + e] = w;
  }
  __syncthreads();
  // codes 4-6 straight-line from LDS (every index is valid whatever the lane's state: no nest of early exits), then
  // ---- trip 3, geometric survivors only: the cached anchors
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int lx = (tid >> 6) + 4 * h;
    const int l = tid + 256 * h;
    // LDS index of the six face neighbours: inside the brick, or on the adjacent brick's face layer
    // (face -x / +x indexed (ly, lz), -y / +y (lx, lz), -z / +z (lx, ly))
    int q[6];
    q[0] = lx > 0 ? l - 64 : kBrickVox + 0 * kFace + ly * 8 + lz;
    q[1] = lx < 7 ? l + 64 : kBrickVox + 1 * kFace + ly * 8 + lz;
    q[2] = ly > 0 ? l - 8 : kBrickVox + 2 * kFace + lx * 8 + lz;
    q[3] = ly < 7 ? l + 8 : kBrickVox + 3 * kFace + lx * 8 + lz;
    q[4] = lz > 0 ? l - 1 : kBrickVox + 4 * kFace + lx * 8 + ly;
    q[5] = lz < 7 ? l + 1 : kBrickVox + 5 * kFace + lx * 8 + ly;
    float nb[6], nw[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) { nb[m] = s_t[q[m]]; nw[m] = s_w[q[m]]; }
    int seen = 1, neg = 0;
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      seen &= (int)(nw[m] >= w_min);
      neg |= (int)(nb[m] < 0.f);
    }
    float p[3], n[3];
    const int ok = (int)newton_point(phi[h], nb, two_h, 0.f, 0.f, 0.f, p, n);
    const int geo = !seen ? 4 : !neg ? 5 : !ok ? 6 : 0;
    const int c13 = cd[h];
    int c = c13 != 0 ? c13 : geo;
    if (c == 0) {
      const ushort4 a4 = anchors[slot * kBrickVox + l];
      if (a4.x == kNoAnchor || a4.y == kNoAnchor || a4.z == kNoAnchor || a4.w == kNoAnchor) c = 7;
    }
    if (code) code[slot * kBrickVox + l] = (uint8_t)c;
    const uint64_t m = __ballot(c == 0);
    if ((tid & 63) == 0) {
      bits[slot * 8 + 4 * h + (tid >> 6)] = m;
      s_cnt[4 * h + (tid >> 6)] = __popcll(m);
    }
  }
  int n_acc = 0;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int m = 0; m < 8; ++m) n_acc += s_cnt[m];
    cnt[slot] = n_acc;
  }
}

// single workgroup of 1024: exclusive scan of the per-brick counts, four consecutive entries per thread (one 16-B load
// and store), 4096 per trip; count = [accepted, emitted]
__global__ __launch_bounds__(1024) void k_surface_offsets(const int32_t* __restrict__ cnt, int n_list, int max_points,
                                                           int32_t* __restrict__ off, int32_t* __restrict__ count) {
  __shared__ int s_wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int carry = 0;
  for (int b0 = 0; b0 < n_list; b0 += 4096) {
    const int i0 = b0 + 4 * tid;
    const bool whole = i0 + 4 <= n_list;
    int4 v = make_int4(0, 0, 0, 0);
    if (whole) {
      v = *(const int4*)(cnt + i0);
    } else {
      if (i0 < n_list) v.x = cnt[i0];
      if (i0 + 1 < n_list) v.y = cnt[i0 + 1];
      if (i0 + 2 < n_list) v.z = cnt[i0 + 2];
    }
    const int t = (v.x + v.y) + (v.z + v.w);
    int x = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) s_wsum[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int sq = s_wsum[q];
      base += q < w ? sq : 0;
      tot += sq;
    }
    __syncthreads();
    const int e = carry + base + x - t;
    if (whole) {
      *(int4*)(off + i0) = make_int4(e, e + v.x, e + v.x + v.y, e + v.x + v.y + v.z);
    } else {
      if (i0 < n_list) off[i0] = e;
      if (i0 + 1 < n_list) off[i0 + 1] = e + v.x;
      if (i0 + 2 < n_list) off[i0 + 2] = e + v.x + v.y;
    }
    carry += tot;
  }
  if (tid == 0) {
    off[n_list] = carry;
    count[0] = carry;
    count[1] = carry < max_points ? carry : max_points;
  }
}

__global__ __launch_bounds__(256) void k_surface_emit(BrickGeom g, const float* __restrict__ tsdf,
                                                       const int32_t* __restrict__ list,
                                                       const ushort4* __restrict__ anchors,
                                                       const float4* __restrict__ weights, float two_h,
                                                       const int32_t* __restrict__ cnt, const int32_t* __restrict__ off,
                                                       const uint64_t* __restrict__ bits, int n_list, int max_points,
                                                       float* __restrict__ points, float* __restrict__ normals,
                                                       int4* __restrict__ a_out, float4* __restrict__ w_out,
                                                       int32_t* __restrict__ voxel, uint8_t* __restrict__ valid) {
  const int64_t slot = blockIdx.x;
  if (cnt[slot] == 0) return;   // (workgroup-uniform)
  const int tid = threadIdx.x;
  const int64_t b = list[slot];
  const int64_t total = off[n_list], mm = max_points, base = off[slot];
  uint64_t word[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) word[m] = bits[slot * 8 + m];
  int i0, j0, k0;
  brick_origin(g, b, i0, j0, k0);
  const int wave = tid >> 6, lane = tid & 63;
  int before = 0;   // accepted voxels of the words in front of word m (word = l >> 6 = 4·h + wave)
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int h = m >> 2;
    if ((m & 3) == wave) {
      const uint64_t mine = word[m];
      if ((mine >> lane) & 1) {
        const int64_t r = base + before + __popcll(mine & (((uint64_t)1 << lane) - 1));
        int64_t row = r;
        bool emit = true;
        if (total > mm) {
          row = r * mm / total;
          emit = (r + 1) * mm / total > row;
        }
        if (emit) {
          const int l = tid + 256 * h;
          const int i = i0 + (l >> 6), j = j0 + ((l >> 3) & 7), k = k0 + (l & 7);
          const float phi = tsdf[b * kBrickVox + l];
          float nb[6];
          nb[0] = tsdf[vox_slot(g, i - 1, j, k)]; nb[1] = tsdf[vox_slot(g, i + 1, j, k)];
          nb[2] = tsdf[vox_slot(g, i, j - 1, k)]; nb[3] = tsdf[vox_slot(g, i, j + 1, k)];
          nb[4] = tsdf[vox_slot(g, i, j, k - 1)]; nb[5] = tsdf[vox_slot(g, i, j, k + 1)];
          const ushort4 a4 = anchors[slot * kBrickVox + l];
          const float4 w4 = weights[slot * kBrickVox + l];
          float p[3], n[3];
          (void)newton_point(phi, nb, two_h, vox2world(g.ox, g.vs, i), vox2world(g.oy, g.vs, j),
                             vox2world(g.oz, g.vs, k), p, n);   // (accepted: not degenerate)
          points[3 * row] = p[0]; points[3 * row + 1] = p[1]; points[3 * row + 2] = p[2];
          normals[3 * row] = n[0]; normals[3 * row + 1] = n[1]; normals[3 * row + 2] = n[2];
          a_out[row] = make_int4(a4.x, a4.y, a4.z, a4.w);
          w_out[row] = w4;
          voxel[row] = (int32_t)(((int64_t)i * g.Dy + j) * g.Dz + k);
          valid[row] = 1;
        }
      }
    }
    before += __popcll(word[m]);
  }
}

// rows [emitted, max_points): valid 0, voxel -1, zeros
__global__ __launch_bounds__(256) void k_surface_pad(const int32_t* __restrict__ count, int max_points,
                                                      float* __restrict__ points, float* __restrict__ normals,
                                                      int4* __restrict__ a_out, float4* __restrict__ w_out,
                                                      int32_t* __restrict__ voxel, uint8_t* __restrict__ valid) {
  const int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (row >= max_points || row < count[1]) return;
  points[3 * row] = 0.f; points[3 * row + 1] = 0.f; points[3 * row + 2] = 0.f;
  normals[3 * row] = 0.f; normals[3 * row + 1] = 0.f; normals[3 * row + 2] = 0.f;
  a_out[row] = make_int4(0, 0, 0, 0);
  w_out[row] = make_float4(0.f, 0.f, 0.f, 0.f);
  voxel[row] = -1;
  valid[row] = 0;
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" {

int ofx_surface_create(int32_t max_bricks, void** handle) {
  OFX_CHECK_ARG(handle, "null handle");
  *handle = nullptr;
  OFX_CHECK_ARG(max_bricks >= 0, "bad max_bricks %d", max_bricks);
  if (max_bricks > (1 << 22) - 1) {   // 512 voxels a brick: the ranks stay below 2^31
    set_error("max_bricks %d exceeds the int32 ranks", max_bricks);
    return OFX_ERR_RANGE;
  }
  Surface* sf = new Surface();
  sf->cap = max_bricks;
  const size_t n = (size_t)max_bricks;
  if (hipMalloc((void**)&sf->cnt, (n + 1) * sizeof(int32_t)) != hipSuccess ||
      hipMalloc((void**)&sf->off, (n + 1) * sizeof(int32_t)) != hipSuccess ||
      hipMalloc((void**)&sf->bits, (n + 1) * 8 * sizeof(uint64_t)) != hipSuccess) {
    for (void* p : {(void*)sf->cnt, (void*)sf->off, (void*)sf->bits})
      if (p) (void)hipFree(p);
    delete sf;
    set_error("ofx_surface_create: scratch for %d bricks could not be allocated", max_bricks);
    return OFX_ERR_ALLOC;
  }
  *handle = sf;
  return OFX_OK;
}

int ofx_surface_destroy(void* handle) {
  if (!handle) return OFX_OK;
  Surface* sf = (Surface*)handle;
  (void)hipDeviceSynchronize();
  for (void* p : {(void*)sf->cnt, (void*)sf->off, (void*)sf->bits})
    if (p) (void)hipFree(p);
  delete sf;
  return OFX_OK;
}

int ofx_surface_points(void* handle, const ofx_volume_desc* desc, const float* tsdf, const float* weight,
                       const int32_t* brick_list, int32_t n_list, const uint16_t* skin_anchors,
                       const float* skin_weights, int32_t k, float w_min, int32_t max_points, float* points,
                       float* normals, int32_t* anchors, float* weights, int32_t* voxel, uint8_t* valid, uint8_t* code,
                       int32_t* count, ofx_stream_t s) {
  Surface* sf = (Surface*)handle;
  OFX_CHECK_ARG(sf && desc && count, "null handle / volume desc / count");
  BrickGeom g;
  int st = make_geom(desc, &g);
  if (st) return st;
  OFX_CHECK_ARG(g.bx0 == 0 && g.bx1 == g.nbx, "ofx_surface_points needs the whole volume, not the shard [%d,%d) of %d",
                g.bx0, g.bx1, g.nbx);
  OFX_CHECK_ARG(k == 4, "ofx_surface_points serves K = 4 anchors, not %d", k);
  OFX_CHECK_ARG((int64_t)g.Dx * g.Dy * g.Dz < ((int64_t)1 << 31), "volume of %lld voxels: the voxel index is int32",
                (long long)((int64_t)g.Dx * g.Dy * g.Dz));
  OFX_CHECK_ARG(n_list >= 0 && n_list <= sf->cap, "n_list %d outside [0, %d] (the handle's max_bricks)", n_list, sf->cap);
  OFX_CHECK_ARG(max_points >= 0, "bad max_points %d", max_points);
  OFX_CHECK_ARG(max_points == 0 || (points && normals && anchors && weights && voxel && valid), "null output");
  OFX_CHECK_ARG((((uintptr_t)anchors | (uintptr_t)weights | (uintptr_t)skin_weights) & 15) == 0 &&
                    ((uintptr_t)skin_anchors & 7) == 0, "anchors / weights must be 16-byte aligned");
  hipStream_t hs = as_stream(s);
  const float two_h = (float)(2.0 * g.vs);
  if (n_list == 0) {
    OFX_HIP(hipMemsetAsync(count, 0, 2 * sizeof(int32_t), hs));
  } else {
    OFX_CHECK_ARG(tsdf && weight && brick_list && skin_anchors && skin_weights, "null buffer");
    hipLaunchKernelGGL(k_surface_classify, dim3((unsigned)n_list), dim3(256), 0, hs, g, tsdf, weight, brick_list,
                       (const ushort4*)skin_anchors, w_min, two_h, code, sf->cnt, sf->bits);
    hipLaunchKernelGGL(k_surface_offsets, dim3(1), dim3(1024), 0, hs, (const int32_t*)sf->cnt, n_list, max_points,
                       sf->off, count);
    OFX_LAUNCH_CHECK();
  }
  if (max_points > 0) {
    hipLaunchKernelGGL(k_surface_pad, dim3(grid_for(max_points, 256, 1 << 23)), dim3(256), 0, hs,
                       (const int32_t*)count, max_points, points, normals, (int4*)anchors, (float4*)weights, voxel,
                       valid);
    if (n_list > 0)
      hipLaunchKernelGGL(k_surface_emit, dim3((unsigned)n_list), dim3(256), 0, hs, g, tsdf, brick_list,
                         (const ushort4*)skin_anchors, (const float4*)skin_weights, two_h, (const int32_t*)sf->cnt,
                         (const int32_t*)sf->off, (const uint64_t*)sf->bits, n_list, max_points, points, normals,
                         (int4*)anchors, (float4*)weights, voxel, valid);
    OFX_LAUNCH_CHECK();
  }
  return OFX_OK;
}

}  // extern "C"
