// Growing the deformation graph from the fused volume: new nodes where the sampled model leaves the graph's coverage.
//
// DynamicFusion adds nodes after every integrate at surface points that no node supports, a node spacing apart, with
// transforms blended from the neighbours. The reference's twin is the host loop of EDGraph.update
// (embedded_deformation_graph.py:496-609, greedy with `<`) behind WarpField.find_unreachable_nodes (warpfield.py:462-485,
// 2·coverage), which its drivers keep commented out. Here the model rows come from ofx_surface_points, so every point
// brings the four anchors and weights of its voxel. No reference twin for the transform blend and the edge rows (parity
// unpinned; restated op for op in tests/grow_ref.py). The contract is in include/ofx.h.
//
//   k_grow_candidates  kGP lanes per model row scan the nodes through 1024-node LDS tiles for the smallest squared
//                      distance (a minimum: the lanes' order cannot change it), then the row's candidate flag.
//   scan_flags         ranks of the flags; k_grow_compact writes the candidate rows in ascending order.
//   k_grow_select      ONE workgroup of 1024, a chunk of 1024 candidates a trip, one candidate per thread. A: every
//                      thread tests its candidate against the nodes selected in earlier chunks (LDS, broadcast reads).
//                      B: the lowest surviving thread is selected, the others test against it; repeated until the chunk
//                      has no survivor. That is the sequential loop's result: a candidate is selected iff no earlier
//                      selected one is closer than the spacing. Two barriers per selected node, one trip per chunk.
//   k_grow_nodes       one thread per selected row: position, warp translation (ed_warp: ofx_deform_points' bits) and
//                      the f64 quaternion blend of its anchors' rotations.
//   k_grow_edges       one wave per new node: the K_e nearest other nodes of the grown node set, register top-8 per lane
//                      and a butterfly merge, then the weights.
// Order comes from the scan and the single workgroup, never from atomics: two runs give the same bytes.
#include "ofx_common.h"
#include "scan_flags.h"
#include "warp_device.h"

namespace ofx {

constexpr int kGrowTile = 1024;      // nodes per LDS tile
constexpr int kGrowChunk = 1024;     // candidates per trip of k_grow_select = its workgroup size
constexpr int kGrowMaxNew = 4096;    // selected positions held in LDS (64 KiB)
constexpr int kGrowMaxPoints = 65536;
constexpr int kGrowMaxNodes = 65534;   // uint16 anchors of the skin cache

struct Grow {
  int32_t max_points = 0, max_new = 0;
  uint8_t* flag = nullptr;   // [max_points] candidate flags
  int32_t* rank = nullptr;   // [max_points + 1] their exclusive scan, the total at [n_points]
  int32_t* tsum = nullptr;   // scan tile sums
  int32_t* cand = nullptr;   // [max_points] candidate rows, ascending
  int32_t* sel = nullptr;    // [max_new] selected rows, in selection order
};

namespace {

__device__ __forceinline__ float sqdist3(float px, float py, float pz, float nx, float ny, float nz) {
  const float dx = px - nx, dy = py - ny, dz = pz - nz;
  const float a = dx * dx, b = dy * dy, c = dz * dz;
  return (a + b) + c;   // the ofx_knn_points / ofx_skin_points form
}
__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }
__device__ __forceinline__ float fexp(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float fdivr(float a, float b) { return (float)((double)a / (double)b); }

constexpr int kGP = 16;   // lanes per model row
static_assert(64 % kGP == 0, "a row's lanes within one wave");

__global__ __launch_bounds__(256) void k_grow_candidates(const float* __restrict__ pts, const int4* __restrict__ anchors,
                                                          const uint8_t* __restrict__ valid, int n_pts,
                                                          const float* __restrict__ nodes, int n_nodes, float min_dist,
                                                          uint8_t* __restrict__ flag) {
  __shared__ float4 sn[kGrowTile];
  const int part = threadIdx.x % kGP;
  const int64_t p = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kGP;
  const bool act = p < n_pts;
  float x = 0.f, y = 0.f, z = 0.f;
  if (act) { x = pts[3 * p]; y = pts[3 * p + 1]; z = pts[3 * p + 2]; }
  float best = __builtin_inff();
  for (int t0 = 0; t0 < n_nodes; t0 += kGrowTile) {
    const int nt = min(kGrowTile, n_nodes - t0);
    __syncthreads();
    for (int i = threadIdx.x; i < nt; i += blockDim.x) {
      const float* q = nodes + 3 * (int64_t)(t0 + i);
      sn[i] = make_float4(q[0], q[1], q[2], 0.f);
    }
    __syncthreads();
    if (act)
      for (int i = part; i < nt; i += kGP) {
        const float4 n = sn[i];
        best = fminf(best, sqdist3(x, y, z, n.x, n.y, n.z));
      }
  }
#pragma unroll
  for (int o = 1; o < kGP; o <<= 1) best = fminf(best, __shfl_xor(best, o, 64));   // (every lane takes part)
  if (!act || part != 0) return;
  bool c = valid[p] != 0 && isfinite(x) && isfinite(y) && isfinite(z);
  const int4 a = anchors[p];
  c = c && (uint32_t)a.x < (uint32_t)n_nodes && (uint32_t)a.y < (uint32_t)n_nodes && (uint32_t)a.z < (uint32_t)n_nodes &&
      (uint32_t)a.w < (uint32_t)n_nodes;
  const float dist = sqrt_rn(best);   // correctly rounded f32 square root, as finish_skin's
  flag[p] = (c && dist > min_dist) ? 1 : 0;   // (a NaN fails)
}

__global__ __launch_bounds__(256) void k_grow_compact(const uint8_t* __restrict__ flag, const int32_t* __restrict__ rank,
                                                       int n_pts, int32_t* __restrict__ cand) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_pts && flag[r]) cand[rank[r]] = r;
}

// the sequential greedy selection; count = [candidates, selected, capped]
__global__ __launch_bounds__(kGrowChunk) void k_grow_select(const float* __restrict__ pts, const int32_t* __restrict__ cand,
                                                             const int32_t* __restrict__ n_cand_p, float spacing,
                                                             int max_new, int32_t* __restrict__ sel,
                                                             int32_t* __restrict__ count) {
  __shared__ float4 s_pos[kGrowMaxNew];
  __shared__ int s_first[kGrowChunk / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_cand = *n_cand_p;
  int nsel = 0, capped = 0;
  for (int c0 = 0; c0 < n_cand && !capped; c0 += kGrowChunk) {
    const int ci = c0 + tid;
    bool alive = ci < n_cand;
    int row = 0;
    float x = 0.f, y = 0.f, z = 0.f;
    if (alive) {
      row = cand[ci];
      x = pts[3 * (int64_t)row]; y = pts[3 * (int64_t)row + 1]; z = pts[3 * (int64_t)row + 2];
    }
    // A: against the nodes of the earlier chunks (s_pos[0, nsel) is complete: the last trip ended on a barrier)
    if (alive)
      for (int t = 0; t < nsel; ++t) {
        const float4 q = s_pos[t];
        if (sqrt_rn(sqdist3(x, y, z, q.x, q.y, q.z)) < spacing) { alive = false; break; }
      }
    // B: the chunk's own order
    for (;;) {
      const uint64_t m = __ballot(alive);
      if (lane == 0) s_first[wave] = m ? wave * 64 + (__ffsll((unsigned long long)m) - 1) : kGrowChunk;
      __syncthreads();
      int first = kGrowChunk;
#pragma unroll
      for (int w = 0; w < kGrowChunk / 64; ++w) first = min(first, s_first[w]);
      if (first == kGrowChunk) break;                 // (workgroup-uniform) no survivor left in this chunk
      if (nsel == max_new) { capped = 1; break; }     // (workgroup-uniform) a survivor the cap leaves out
      if (tid == first) {
        s_pos[nsel] = make_float4(x, y, z, 0.f);
        sel[nsel] = row;
        alive = false;
      }
      __syncthreads();
      const float4 q = s_pos[nsel];
      ++nsel;
      if (alive && sqrt_rn(sqdist3(x, y, z, q.x, q.y, q.z)) < spacing) alive = false;
    }
    __syncthreads();   // s_first is rewritten by the next trip
  }
  if (tid == 0) {
    count[0] = n_cand;
    count[1] = nsel;
    count[2] = capped;
  }
}

// rotation matrix (row-major, f64) -> unit quaternion (w, x, y, z): Shepperd's form, the branch of the largest of the
// trace and the three diagonal entries (the first of equals, in that order)
__device__ __forceinline__ void quat_of(const double m[9], double q[4]) {
  const double tr = (m[0] + m[4]) + m[8];
  int br = 0;
  double big = tr;
  if (m[0] > big) { big = m[0]; br = 1; }
  if (m[4] > big) { big = m[4]; br = 2; }
  if (m[8] > big) { big = m[8]; br = 3; }
  if (br == 0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q[0] = 0.25 * s; q[1] = (m[7] - m[5]) / s; q[2] = (m[2] - m[6]) / s; q[3] = (m[3] - m[1]) / s;
  } else if (br == 1) {
    const double s = sqrt(((1.0 + m[0]) - m[4]) - m[8]) * 2.0;
    q[0] = (m[7] - m[5]) / s; q[1] = 0.25 * s; q[2] = (m[1] + m[3]) / s; q[3] = (m[2] + m[6]) / s;
  } else if (br == 2) {
    const double s = sqrt(((1.0 + m[4]) - m[0]) - m[8]) * 2.0;
    q[0] = (m[2] - m[6]) / s; q[1] = (m[1] + m[3]) / s; q[2] = 0.25 * s; q[3] = (m[5] + m[7]) / s;
  } else {
    const double s = sqrt(((1.0 + m[8]) - m[0]) - m[4]) * 2.0;
    q[0] = (m[3] - m[1]) / s; q[1] = (m[2] + m[6]) / s; q[2] = (m[5] + m[7]) / s; q[3] = 0.25 * s;
  }
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  if (n > 0.0 && isfinite(n)) { q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n; }
  else { q[0] = 1.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0; }   // no rotation to read: the identity
}

__global__ __launch_bounds__(64) void k_grow_nodes(const float* __restrict__ pts, const int4* __restrict__ anchors,
                                                    const float4* __restrict__ weights, const int32_t* __restrict__ sel,
                                                    const int32_t* __restrict__ count, int n_nodes,
                                                    float* __restrict__ nodes, float* __restrict__ R,
                                                    float* __restrict__ T) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count[1]) return;
  const int64_t row = sel[j];
  const float px = pts[3 * row], py = pts[3 * row + 1], pz = pts[3 * row + 2];
  const int4 a4 = anchors[row];
  const float4 w4 = weights[row];
  const int aid[4] = {a4.x, a4.y, a4.z, a4.w};   // candidates: all four in [0, n_nodes)
  const float w[4] = {w4.x, w4.y, w4.z, w4.w};
  // the anchors' records as ofx_pack_nodes lays them out, then the shared warp
  float4 rec[16];
  double acc[4] = {0.0, 0.0, 0.0, 0.0}, q0[4] = {1.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float* r = R + 9 * (int64_t)aid[k];
    const float* g = nodes + 3 * (int64_t)aid[k];
    const float* t = T + 3 * (int64_t)aid[k];
    rec[4 * k + 0] = make_float4(r[0], r[3], r[1], r[4]);
    rec[4 * k + 1] = make_float4(r[2], r[5], g[0], g[1]);
    rec[4 * k + 2] = make_float4(t[0], t[1], r[6], r[7]);
    rec[4 * k + 3] = make_float4(r[8], g[2], t[2], 0.f);
    double m[9], q[4];
#pragma unroll
    for (int e = 0; e < 9; ++e) m[e] = (double)r[e];
    quat_of(m, q);
    if (k == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { q0[e] = q[e]; acc[e] = (double)w[0] * q[e]; }
    } else {
      const double dot = ((q0[0] * q[0] + q0[1] * q[1]) + q0[2] * q[2]) + q0[3] * q[3];
      const double sg = dot < 0.0 ? -1.0 : 1.0;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = acc[e] + (double)w[k] * (sg * q[e]);
    }
  }
  const int ids[4] = {0, 1, 2, 3};
  float x = px, y = py, z = pz;
  ed_warp(rec, ids, w, 4, x, y, z);
  const int64_t o = (int64_t)n_nodes + j;
  nodes[3 * o] = px; nodes[3 * o + 1] = py; nodes[3 * o + 2] = pz;
  T[3 * o] = x - px; T[3 * o + 1] = y - py; T[3 * o + 2] = z - pz;
  const double n = sqrt(((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]) + acc[3] * acc[3]);
  double qw = 1.0, qx = 0.0, qy = 0.0, qz = 0.0;
  if (n > 0.0 && isfinite(n)) { qw = acc[0] / n; qx = acc[1] / n; qy = acc[2] / n; qz = acc[3] / n; }
  float* ro = R + 9 * o;
  ro[0] = (float)(1.0 - 2.0 * (qy * qy + qz * qz));
  ro[1] = (float)(2.0 * (qx * qy - qz * qw));
  ro[2] = (float)(2.0 * (qx * qz + qy * qw));
  ro[3] = (float)(2.0 * (qx * qy + qz * qw));
  ro[4] = (float)(1.0 - 2.0 * (qx * qx + qz * qz));
  ro[5] = (float)(2.0 * (qy * qz - qx * qw));
  ro[6] = (float)(2.0 * (qx * qz - qy * qw));
  ro[7] = (float)(2.0 * (qy * qz + qx * qw));
  ro[8] = (float)(1.0 - 2.0 * (qx * qx + qy * qy));
}

struct Top8 {
  float d[8];
  int id[8];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int s = 0; s < 8; ++s) { d[s] = __builtin_inff(); id[s] = 0x7fffffff; }
  }
  __device__ __forceinline__ static bool less(float da, int ia, float db, int ib) {
    return da < db || (da == db && ia < ib);
  }
  __device__ __forceinline__ void insert(float dn, int in) {
    if (!less(dn, in, d[7], id[7])) return;
    d[7] = dn; id[7] = in;
#pragma unroll
    for (int s = 7; s > 0; --s) {
      if (less(d[s], id[s], d[s - 1], id[s - 1])) {
        const float td = d[s]; d[s] = d[s - 1]; d[s - 1] = td;
        const int ti = id[s]; id[s] = id[s - 1]; id[s - 1] = ti;
      }
    }
  }
};

// one wave per new node, four to a workgroup; the node tiles are shared by the workgroup's waves
__global__ __launch_bounds__(256) void k_grow_edges(const float* __restrict__ nodes, int n_nodes,
                                                     const int32_t* __restrict__ count, int K, float two_c2,
                                                     int32_t* __restrict__ edges, float* __restrict__ ew) {
  __shared__ float4 sn[kGrowTile];
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n_sel = count[1];
  if (blockIdx.x * 4 >= n_sel) return;   // (workgroup-uniform)
  const int n_all = n_nodes + n_sel;
  const bool act = j < n_sel;
  const int me = n_nodes + j;
  float x = 0.f, y = 0.f, z = 0.f;
  if (act) { x = nodes[3 * (int64_t)me]; y = nodes[3 * (int64_t)me + 1]; z = nodes[3 * (int64_t)me + 2]; }
  Top8 tk;
  tk.init();
  for (int t0 = 0; t0 < n_all; t0 += kGrowTile) {
    const int nt = min(kGrowTile, n_all - t0);
    __syncthreads();
    for (int i = threadIdx.x; i < nt; i += blockDim.x) {
      const float* q = nodes + 3 * (int64_t)(t0 + i);
      sn[i] = make_float4(q[0], q[1], q[2], 0.f);
    }
    __syncthreads();
    if (act)
      for (int i = lane; i < nt; i += 64) {
        if (t0 + i == me) continue;
        const float4 n = sn[i];
        tk.insert(sqdist3(x, y, z, n.x, n.y, n.z), t0 + i);
      }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {   // (every lane takes part: the shuffles precede any exit)
    float od[8];
    int oi[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) { od[s] = __shfl_xor(tk.d[s], o, 64); oi[s] = __shfl_xor(tk.id[s], o, 64); }
#pragma unroll
    for (int s = 0; s < 8; ++s) tk.insert(od[s], oi[s]);
  }
  if (!act || lane != 0) return;
  // weights as k_geodesic's (graph.hip): exp(-(d·d)/(2c²)) in f32, f32 sum in order, w/sum or w/n
  float w[8];
  float sum = 0.f;
  int cnt = 0;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    w[s] = 0.f;
    if (s < K && tk.id[s] != 0x7fffffff) {
      const float d = sqrt_rn(tk.d[s]);
      w[s] = fexp(fdivr(-(d * d), two_c2));
      sum += w[s];
      ++cnt;
    }
  }
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    if (s >= K) continue;
    const int64_t o = (int64_t)me * K + s;
    const bool has = s < cnt;
    edges[o] = has ? tk.id[s] : -1;
    ew[o] = has ? (sum > 0.f ? fdivr(w[s], sum) : fdivr(w[s], (float)cnt)) : 0.f;
  }
}

void grow_free(Grow* gr) {
  for (void* p : {(void*)gr->flag, (void*)gr->rank, (void*)gr->tsum, (void*)gr->cand, (void*)gr->sel})
    if (p) (void)hipFree(p);
  delete gr;
}

}  // namespace
}  // namespace ofx

using namespace ofx;

extern "C" {

int ofx_grow_create(int32_t max_points, int32_t max_new, void** handle) {
  OFX_CHECK_ARG(handle, "null handle");
  *handle = nullptr;
  OFX_CHECK_ARG(max_points >= 0 && max_new >= 0, "bad max_points %d / max_new %d", max_points, max_new);
  if (max_points > kGrowMaxPoints || max_new > kGrowMaxNew) {
    set_error("ofx_grow_create: at most %d model rows and %d new nodes a call (got %d, %d)", kGrowMaxPoints,
              kGrowMaxNew, max_points, max_new);
    return OFX_ERR_RANGE;
  }
  Grow* gr = new Grow();
  gr->max_points = max_points;
  gr->max_new = max_new;
  const size_t n = (size_t)max_points;
  if (hipMalloc((void**)&gr->flag, n + 16) != hipSuccess ||
      hipMalloc((void**)&gr->rank, (n + 1) * sizeof(int32_t)) != hipSuccess ||
      hipMalloc((void**)&gr->tsum, ((size_t)scan_tiles(max_points) + 2) * sizeof(int32_t)) != hipSuccess ||
      hipMalloc((void**)&gr->cand, (n + 1) * sizeof(int32_t)) != hipSuccess ||
      hipMalloc((void**)&gr->sel, ((size_t)max_new + 1) * sizeof(int32_t)) != hipSuccess) {
    grow_free(gr);
    set_error("ofx_grow_create: scratch for %d rows could not be allocated", max_points);
    return OFX_ERR_ALLOC;
  }
  *handle = gr;
  return OFX_OK;
}

int ofx_grow_destroy(void* handle) {
  if (!handle) return OFX_OK;
  (void)hipDeviceSynchronize();
  grow_free((Grow*)handle);
  return OFX_OK;
}

int ofx_grow_nodes(void* handle, const float* points, const int32_t* anchors, const float* weights,
                   const uint8_t* valid, int32_t n_points, float* nodes, int32_t n_nodes, float* R, float* T,
                   int32_t* edges, float* edge_weights, int32_t k_e, float node_coverage, float min_dist, float spacing,
                   int32_t max_new, int32_t* count, ofx_stream_t s) {
  Grow* gr = (Grow*)handle;
  OFX_CHECK_ARG(gr && count, "null handle / count");
  OFX_CHECK_ARG(n_points >= 0 && n_points <= gr->max_points, "n_points %d outside [0, %d] (the handle's max_points)",
                n_points, gr->max_points);
  OFX_CHECK_ARG(max_new >= 0 && max_new <= gr->max_new, "max_new %d outside [0, %d] (the handle's max_new)", max_new,
                gr->max_new);
  OFX_CHECK_ARG(k_e >= 1 && k_e <= 8, "k_e %d outside [1, 8]", k_e);
  OFX_CHECK_ARG(n_nodes >= 1, "bad n_nodes %d", n_nodes);
  if ((int64_t)n_nodes + max_new > kGrowMaxNodes) {
    set_error("n_nodes %d + max_new %d exceeds %d (uint16 anchors)", n_nodes, max_new, kGrowMaxNodes);
    return OFX_ERR_RANGE;
  }
  OFX_CHECK_ARG(spacing > 0.f && spacing <= 3.402823466e38f, "spacing must be positive and finite");
  OFX_CHECK_ARG(node_coverage > 0.f && node_coverage <= 3.402823466e38f, "node_coverage must be positive and finite");
  OFX_CHECK_ARG(!(min_dist != min_dist), "min_dist is NaN");
  hipStream_t hs = as_stream(s);
  if (n_points == 0 || max_new == 0) {
    OFX_HIP(hipMemsetAsync(count, 0, 3 * sizeof(int32_t), hs));
    return OFX_OK;
  }
  OFX_CHECK_ARG(points && anchors && weights && valid && nodes && R && T && edges && edge_weights, "null buffer");
  OFX_CHECK_ARG((((uintptr_t)anchors | (uintptr_t)weights) & 15) == 0, "anchors / weights must be 16-byte aligned");
  hipLaunchKernelGGL(k_grow_candidates, dim3(grid_for((int64_t)n_points * kGP, 256, 1 << 30)), dim3(256), 0, hs, points,
                     (const int4*)anchors, valid, n_points, (const float*)nodes, n_nodes, min_dist, gr->flag);
  OFX_LAUNCH_CHECK();
  const int st = scan_flags(gr->flag, n_points, gr->rank, gr->tsum, hs);
  if (st) return st;
  hipLaunchKernelGGL(k_grow_compact, dim3(grid_for(n_points, 256)), dim3(256), 0, hs, (const uint8_t*)gr->flag,
                     (const int32_t*)gr->rank, n_points, gr->cand);
  hipLaunchKernelGGL(k_grow_select, dim3(1), dim3(kGrowChunk), 0, hs, points, (const int32_t*)gr->cand,
                     (const int32_t*)(gr->rank + n_points), spacing, max_new, gr->sel, count);
  hipLaunchKernelGGL(k_grow_nodes, dim3(grid_for(max_new, 64)), dim3(64), 0, hs, points, (const int4*)anchors,
                     (const float4*)weights, (const int32_t*)gr->sel, (const int32_t*)count, n_nodes, nodes, R, T);
  hipLaunchKernelGGL(k_grow_edges, dim3(grid_for(max_new, 4)), dim3(256), 0, hs, (const float*)nodes, n_nodes,
                     (const int32_t*)count, k_e, (2.f * node_coverage) * node_coverage, edges, edge_weights);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

}  // extern "C"
