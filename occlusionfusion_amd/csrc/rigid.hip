// Rigid pre-alignment: point-to-plane ICP of all model points against a depth frame, 6 unknowns, on the device.
//
// The cheap stage every TSDF fusion tracker puts in front of its non-rigid solve (KinectFusion's tracker, the first
// stage of DynamicFusion). It has no reference twin (parity unpinned; restated op for op in tests/rigid_ref.py). One
// iteration, per model point (f32, no contraction, every step fixed):
//
//   x', n' = ofx_associate's warped point and normalised warped normal (gate_device.h: skin_load, skin_warp)
//   y = Rf x' + tf, m = Rf n'      Rf, tf: the f32 roundings of the f64 pose; rows summed ((a0·x + a1·y) + a2·z) + t
//   pixel, q, n_q, codes 1-6       ofx_associate's (gate_device.h: proj_gate), with y and m in place of x' and n'
//   accepted: e = q - y, r = e·n_q, c = y x n_q (a·b - c·d per component), row J = [c, n_q]
//
// k_rigid_gate (one thread per point, ofx_associate's three-trip gather) forms the 28 exact f64 products of the row
// (21 of JᵀJ, 6 of Jᵀr, r²) and the accepted flag once the gate's registers are dead, and reduces them over the wave by
// a transposed halving of cross-lane shuffles (32 exchanges for all entries; one butterfly per entry took 6 each and
// made the kernel three times the association's gate), then over the workgroup's four waves through LDS in wave
// order: one 32-double record per workgroup, no atomics. k_rigid_solve (one workgroup of 1024) sums the records in a
// fixed order (32 strided chains per entry, then the chains in order), and its thread 0
// damps, factors (6x6 Cholesky, f64), solves, and left-multiplies the pose by exp of the twist. The grid is
// ceil(n / 256): the summation order depends on n_points alone. All iterations are enqueued at once; a device flag set
// by a failed or converged iteration makes every later launch leave after one load.
#include "ofx_common.h"
#include "gate_device.h"

namespace ofx {

constexpr int kRigidRec = 32;   // doubles per workgroup record and per systems row

struct Rigid {
  int64_t cap = 0;
  double* part = nullptr;    // [ceil(cap / 256)][kRigidRec] workgroup records
  int32_t* stop = nullptr;   // [1] non-zero: the remaining iterations drain
};

// One halving step of the wave's transposed reduction: lanes l and l ^ off pair up; the one with the bit clear keeps
// entries [0, N) and hands over [N, 2N), the other the reverse; each adds what it receives to what it keeps. N entries
// summed over twice as many lanes remain. (a + b is commutative bit for bit, so both lanes of a pair agree on the order.)
template <int N>
__device__ __forceinline__ void fold_half(double (&v)[32], int off, bool up) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double send = up ? v[i] : v[i + N];
    const double keep = up ? v[i + N] : v[i];
    v[i] = keep + __shfl_xor(send, off, 64);
  }
}

// 32 entries per lane -> entry (lane >> 1) & 31 summed over the 64 lanes, in v[0] of every lane: five halving steps
// (16 + 8 + 4 + 2 + 1 exchanges) and one last exchange between neighbours, 32 shuffles where a butterfly per entry
// takes 6 x 32. The order is a function of the lane layout alone.
__device__ __forceinline__ void wave_reduce32(double (&v)[32], int lane) {
  fold_half<16>(v, 32, (lane & 32) != 0);
  fold_half<8>(v, 16, (lane & 16) != 0);
  fold_half<4>(v, 8, (lane & 8) != 0);
  fold_half<2>(v, 4, (lane & 4) != 0);
  fold_half<1>(v, 2, (lane & 2) != 0);
  v[0] = v[0] + __shfl_xor(v[0], 1, 64);
}

// VALID / NRM: valid / normals given (compile-time, so that trip 1 is branch-free)
template <bool VALID, bool NRM>
__global__ __launch_bounds__(256) void k_rigid_gate(const float* __restrict__ pts, const float* __restrict__ nrm,
                                                     const int4* __restrict__ anchors,
                                                     const float4* __restrict__ weights,
                                                     const uint8_t* __restrict__ valid,
                                                     const float4* __restrict__ nodes, int n_nodes, CamD c,
                                                     const float* __restrict__ vmap, float dist_max, float cos_min,
                                                     float edge_max, int64_t n, const double* __restrict__ pose,
                                                     const int32_t* __restrict__ stop, uint8_t* __restrict__ code,
                                                     double* __restrict__ part) {
  __shared__ double red[4][kRigidRec];
  if (*stop) return;   // uniform over the grid
  const int64_t p0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool in = p0 < n;
  const int64_t p = in ? p0 : n - 1;   // a thread past the end reads the last point and contributes nothing
  float R[9], t[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (float)pose[4 * i + j];
    t[i] = (float)pose[4 * i + 3];
  }
  SkinPt s;
  const bool ok = skin_load<VALID, NRM>(pts, nrm, anchors, weights, valid, n_nodes, p, 0.f, s);
  int cd = 1;
  float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, r = 0.f;
  if (ok) {
    skin_warp<NRM>(nodes, s);
    {
      const float yx = ((R[0] * s.x + R[1] * s.y) + R[2] * s.z) + t[0];
      const float yy = ((R[3] * s.x + R[4] * s.y) + R[5] * s.z) + t[1];
      const float yz = ((R[6] * s.x + R[7] * s.y) + R[8] * s.z) + t[2];
      s.x = yx; s.y = yy; s.z = yz;
    }
    if (NRM) {
      const float mx = (R[0] * s.nx + R[1] * s.ny) + R[2] * s.nz;
      const float my = (R[3] * s.nx + R[4] * s.ny) + R[5] * s.nz;
      const float mz = (R[6] * s.nx + R[7] * s.ny) + R[8] * s.nz;
      s.nx = mx; s.ny = my; s.nz = mz;
    }
    GateHit h;
    cd = proj_gate<NRM>(c, vmap, s, dist_max, cos_min, edge_max, h);
    if (cd == 0) {
      r = dot3(h.ex, h.ey, h.ez, h.nx, h.ny, h.nz);
      J[0] = s.y * h.nz - s.z * h.ny;
      J[1] = s.z * h.nx - s.x * h.nz;
      J[2] = s.x * h.ny - s.y * h.nx;
      J[3] = h.nx; J[4] = h.ny; J[5] = h.nz;
    }
  }
  if (in && code) code[p] = (uint8_t)cd;
  const bool acc = in && cd == 0;
  if (!acc) {
    r = 0.f;
    for (int i = 0; i < 6; ++i) J[i] = 0.f;
  }
  // the reduction: every term a product of two f32 values, exact in f64; entry 28 counts the accepted points
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double v[32];
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++e) v[e] = (double)J[i] * (double)J[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[21 + i] = (double)J[i] * (double)r;
    v[27] = (double)r * (double)r;
    v[28] = acc ? 1.0 : 0.0;
    v[29] = v[30] = v[31] = 0.0;
  }
  wave_reduce32(v, lane);
  if ((lane & 1) == 0) red[wave][lane >> 1] = v[0];
  __syncthreads();
  if (threadIdx.x < 29) {
    const int k = threadIdx.x;
    part[(int64_t)blockIdx.x * kRigidRec + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// One workgroup: total of the n_part records (fixed order), then thread 0 solves and updates the pose.
__global__ __launch_bounds__(1024) void k_rigid_solve(const double* __restrict__ part, int64_t n_part, int min_matches,
                                                      double damping, double stop_twist, double* __restrict__ pose,
                                                      int32_t* __restrict__ stop, double* __restrict__ sys) {
  __shared__ double red[32][kRigidRec];
  __shared__ double tot[kRigidRec];
  if (*stop) {
    if (threadIdx.x < kRigidRec) sys[threadIdx.x] = threadIdx.x == 29 ? 3.0 : 0.0;
    return;
  }
  const int k = threadIdx.x & 31, chain = threadIdx.x >> 5;
  double s = 0.0;
  if (k < 29)
    for (int64_t b = chain; b < n_part; b += 32) s = s + part[b * kRigidRec + k];
  red[chain][k] = s;
  __syncthreads();
  if (threadIdx.x < kRigidRec) {
    double v = red[0][k];
    for (int ch = 1; ch < 32; ++ch) v = v + red[ch][k];
    tot[k] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int i = 0; i < 29; ++i) sys[i] = tot[i];
  double A[6][6], b[6], xi[6] = {0, 0, 0, 0, 0, 0};
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++e) A[i][j] = A[j][i] = tot[e];
#pragma unroll
    for (int i = 0; i < 6; ++i) b[i] = tot[21 + i];
  }
  int status = 0;
  double wn = 0.0, vn = 0.0;
  if (tot[28] < (double)min_matches) {
    status = 1;
  } else {
    const double tr = ((((A[0][0] + A[1][1]) + A[2][2]) + A[3][3]) + A[4][4]) + A[5][5];
    const double mu = damping * tr / 6.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + mu;
    // Cholesky, lower triangle in place; fully unrolled (register-resident), so a bad pivot is noted, not left early
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double d = A[j][j];
#pragma unroll
      for (int q = 0; q < j; ++q) d = d - A[j][q] * A[j][q];
      bad = bad || !(d > 0.0) || !isfinite(d);
      const double l = sqrt(d);
      A[j][j] = l;
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double v = A[i][j];
#pragma unroll
        for (int q = 0; q < j; ++q) v = v - A[i][q] * A[j][q];
        A[i][j] = v / l;
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double v = b[i];
#pragma unroll
      for (int q = 0; q < i; ++q) v = v - A[i][q] * xi[q];
      xi[i] = v / A[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double v = xi[i];
#pragma unroll
      for (int q = i + 1; q < 6; ++q) v = v - A[q][i] * xi[q];
      xi[i] = v / A[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) bad = bad || !isfinite(xi[i]);
    if (bad) status = 2;
    if (status == 0) {
      const double wx = xi[0], wy = xi[1], wz = xi[2];
      const double th2 = (wx * wx + wy * wy) + wz * wz;
      wn = sqrt(th2);
      vn = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
      double ca, cb;   // exp(w) = I + ca·K + cb·K²
      if (wn < 1e-8) {
        ca = 1.0 - th2 / 6.0;
        cb = 0.5 - th2 / 24.0;
      } else {
        ca = sin(wn) / wn;
        cb = (1.0 - cos(wn)) / th2;
      }
      const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
      double dR[3][3], P[3][4], out[3][4];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
          dR[i][j] = ((i == j ? 1.0 : 0.0) + ca * K[i][j]) + cb * k2;
        }
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) P[i][j] = pose[4 * i + j];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          double v = (dR[i][0] * P[0][j] + dR[i][1] * P[1][j]) + dR[i][2] * P[2][j];
          if (j == 3) v = v + xi[3 + i];
          out[i][j] = v;
        }
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) pose[4 * i + j] = out[i][j];
    }
  }
  sys[29] = (double)status;
  sys[30] = wn;
  sys[31] = vn;
  if (status != 0 || (wn < stop_twist && vn < stop_twist)) *stop = 1;
}

// n_points = 0: every row is "fewer than min_matches", nothing else happens
__global__ void k_rigid_empty(double* __restrict__ sys, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows * kRigidRec) sys[i] = (i % kRigidRec) == 29 ? 1.0 : 0.0;
}

}  // namespace ofx

using namespace ofx;

extern "C" {

int ofx_rigid_create(int64_t max_points, void** handle) {
  OFX_CHECK_ARG(handle, "null handle");
  *handle = nullptr;
  OFX_CHECK_ARG(max_points >= 0, "bad max_points");
  if (max_points >= ((int64_t)1 << 31) - 1) {
    set_error("max_points %lld exceeds the 32-bit grid", (long long)max_points);
    return OFX_ERR_RANGE;
  }
  Rigid* a = new Rigid();
  a->cap = max_points;
  const size_t recs = (size_t)((max_points + 255) / 256) + 1;
  if (hipMalloc((void**)&a->part, recs * kRigidRec * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&a->stop, 16) != hipSuccess) {
    for (void* p : {(void*)a->part, (void*)a->stop})
      if (p) (void)hipFree(p);
    delete a;
    set_error("ofx_rigid_create: scratch for %lld points could not be allocated", (long long)max_points);
    return OFX_ERR_ALLOC;
  }
  *handle = a;
  return OFX_OK;
}

int ofx_rigid_destroy(void* handle) {
  if (!handle) return OFX_OK;
  Rigid* a = (Rigid*)handle;
  (void)hipDeviceSynchronize();
  for (void* p : {(void*)a->part, (void*)a->stop})
    if (p) (void)hipFree(p);
  delete a;
  return OFX_OK;
}

int ofx_rigid_icp(void* handle, const float* points, const float* normals, const int32_t* anchors, const float* weights,
                  const uint8_t* valid, int64_t n_points, const float* packed_nodes, int32_t n_nodes,
                  const ofx_camera* cam, const float* point_image, int32_t height, int32_t width,
                  const ofx_rigid_params* prm, double* pose, uint8_t* code, double* systems, ofx_stream_t s) {
  Rigid* a = (Rigid*)handle;
  OFX_CHECK_ARG(a && cam && prm && pose && systems, "null handle / camera / params / pose / systems");
  OFX_CHECK_ARG(n_points >= 0 && n_points <= a->cap, "n_points %lld outside [0, %lld] (the handle's max_points)",
                (long long)n_points, (long long)a->cap);
  OFX_CHECK_ARG(prm->iters >= 1, "bad iters %d", prm->iters);
  OFX_CHECK_ARG(prm->min_matches >= 0, "bad min_matches %d", prm->min_matches);
  OFX_CHECK_ARG(prm->damping >= 0.0 && prm->stop_twist >= 0.0, "damping and stop_twist must not be negative");
  OFX_CHECK_ARG(height > 0 && width > 0 && cam->width == width && cam->height == height,
                "the camera (%d x %d) and the point image (%d x %d) differ", cam->width, cam->height, width, height);
  OFX_CHECK_ARG(((uintptr_t)pose & 7) == 0 && ((uintptr_t)systems & 7) == 0, "pose / systems must be 8-byte aligned");
  hipStream_t hs = as_stream(s);
  if (n_points == 0) {
    const int cells = prm->iters * kRigidRec;
    hipLaunchKernelGGL(k_rigid_empty, dim3((cells + 255) / 256), dim3(256), 0, hs, systems, prm->iters);
    OFX_LAUNCH_CHECK();
    return OFX_OK;
  }
  if (int st = check_skinned(points, anchors, weights, packed_nodes, n_nodes, point_image != nullptr)) return st;
  OFX_HIP(hipMemsetAsync(a->stop, 0, sizeof(int32_t), hs));
  const unsigned grid = (unsigned)((n_points + 255) / 256);
  for (int it = 0; it < prm->iters; ++it) {
    dispatch_valid_nrm(valid, normals, [&](auto V, auto N) {
      hipLaunchKernelGGL((k_rigid_gate<decltype(V)::value, decltype(N)::value>), dim3(grid), dim3(256), 0, hs, points,
                         normals, (const int4*)anchors, (const float4*)weights, valid, (const float4*)packed_nodes,
                         n_nodes, make_cam(cam), point_image, prm->dist_max, prm->cos_min, prm->edge_max, n_points,
                         (const double*)pose, (const int32_t*)a->stop, code, a->part);
    });
    OFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rigid_solve, dim3(1), dim3(1024), 0, hs, (const double*)a->part, (int64_t)grid,
                       prm->min_matches, prm->damping, prm->stop_twist, pose, a->stop,
                       systems + (size_t)it * kRigidRec);
    OFX_LAUNCH_CHECK();
  }
  return OFX_OK;
}

}  // extern "C"
