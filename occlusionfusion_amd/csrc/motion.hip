// Motion completion network (OcclusionFusion's MotionCompleteNet, motion_model.py:7-98), inference only, f32, and the
// runner's pre- and post-processing (run_motion_model.py:45-196) in f64, all on the device.
//
// The graph layers (torch_geometric's TransformerConv and DeepGCNLayer 'res+') are restated from their published
// definition: they are unpinned against the reference (tests/motion_ref.py is the yardstick, in f64).
//
//   k_mo_seq     one launch: all T <= 16 steps of both LSTM layers, seq_linear and node_encoder. The 13.8k weight floats
//                sit in LDS (stored transposed, so thread j of a gate row reads consecutive words); a workgroup of 128
//                threads (one per gate row) carries 4 nodes, the cell states stay in registers.
//   k_mo_proj    per conv: LayerNorm + relu of the (gathered, concatenated) input, one wave per node, then the four
//                projections q | k | v | skip against the transposed weights (coalesced over the output channel).
//   k_mo_attn    per conv: one wave per target node over its incoming edges (CSR in edge-list order): scores, softmax
//                with the maximum subtracted, Σ α v + skip + residual. Lanes are channels; the sums over edges run in
//                list order, the sums over channels in a butterfly, so two runs are bitwise equal. No atomics.
//   k_mo_head    norm_out, relu, lin, softplus on channel 3.
// A forward is 1 + 15 * 2 + 1 = 32 launches. The level gathers and concatenations are folded into the loads of
// k_mo_proj / k_mo_attn (MoIn).
//
//   k_mo_indeg / k_mo_scan / k_mo_fill   the incoming-edge CSR of a level from its (N, K) neighbour lists: one wave per
//                target scans the flat list with ballots, so a target's sources come out ordered by (row, slot).
//   k_mo_fit     one workgroup: Kabsch fits of the current and of the previous frame (centroids, H, the orthogonal polar
//                factor of Hᵀ by scaled Newton steps), the normalising std; every reduction in a fixed order.
//   k_mo_apply   per node: curr_motion, centred position, the history update (cap, rescale, previous-frame row).
//   k_mo_post    per node: confidence and node motion.
#include "ofx_common.h"

#include <string.h>

#include <vector>

namespace ofx {

constexpr int kMoLayers = 15;
constexpr int kMoMaxK = 16;
constexpr int kMoMaxHist = 16;
constexpr int kMoMaxNodes = 16384;
constexpr uint32_t kMoTag = 0x4d4f5431u;   // 'MOT1': the layout below
constexpr int kMoTile = 4;                 // nodes per workgroup of k_mo_proj / k_mo_attn / k_mo_head (one wave each)
constexpr int kMoNB = 4;                   // nodes per workgroup of k_mo_seq

// the packed blob (floats), after the two header words (tag, total length):
//   lstm:  Wih0ᵀ (4,128) Whh0ᵀ (32,128) bih0 bhh0 | Wih1ᵀ (32,128) Whh1ᵀ (32,128) bih1 bhh1 | seq_linear Wᵀ (32,4) b (4)
//          node_encoder Wᵀ (11,32) b (32)
//   conv l (15 of them): Wᵀ (C, 4C) columns q | k | v | skip, bias (4C), norm weight (C), norm bias (C)
//   head:  norm_out weight (128) bias (128), lin Wᵀ (128,4), b (4)
constexpr int kSeqIh0 = 0, kSeqHh0 = 512, kSeqBi0 = 4608, kSeqBh0 = 4736, kSeqIh1 = 4864, kSeqHh1 = 8960,
              kSeqBi1 = 13056, kSeqBh1 = 13184, kSeqLinW = 13312, kSeqLinB = 13440, kSeqEncW = 13444, kSeqEncB = 13796,
              kSeqFloats = 13828;
constexpr int kHeadFloats = 128 + 128 + 512 + 4;

struct MoLayerDef { int C, level, norm; };
static const MoLayerDef kMoLayer[kMoLayers] = {
    {32, 0, 0},                                                                     // conv0
    {32, 0, 1}, {32, 0, 1}, {32, 1, 1}, {32, 1, 1}, {32, 2, 1}, {32, 2, 1}, {32, 3, 1}, {32, 3, 1},   // layer11 .. layer42
    {64, 2, 1}, {64, 2, 1}, {96, 1, 1}, {96, 1, 1}, {128, 0, 1}, {128, 0, 1}};     // layer51 .. layer72

inline int64_t mo_layer_floats(int C) { return (int64_t)4 * C * C + 4 * C + 2 * C; }
inline int64_t mo_blob_floats() {
  int64_t t = 2 + kSeqFloats + kHeadFloats;
  for (int l = 0; l < kMoLayers; ++l) t += mo_layer_floats(kMoLayer[l].C);
  return t;
}

struct MoLevel {
  int n = 0, k = 0;
  int32_t* nn = nullptr;       // [max_nodes * kMoMaxK] the level's lists (a copy)
  int32_t* deg = nullptr;      // [max_nodes]
  int32_t* rowptr = nullptr;   // [max_nodes + 1]
  int32_t* src = nullptr;      // [max_nodes * kMoMaxK]
};

struct Motion {
  int max_nodes = 0, max_hist = 0;
  float* w = nullptr;                 // the blob
  int64_t off_layer[kMoLayers];       // float offsets into w
  int64_t off_head = 0;
  MoLevel lv[4];
  int32_t* down[3] = {nullptr, nullptr, nullptr};   // [max_nodes]
  int32_t* up[3] = {nullptr, nullptr, nullptr};
  bool graph = false;
  float* x0 = nullptr;                // [max_nodes * 32]
  float* qkvs = nullptr;              // [max_nodes * 512]
  float* out[kMoLayers];              // [max_nodes * C]
  // the completer's state
  double* hist[2] = {nullptr, nullptr};   // [max_hist][max_nodes][4], ping-pong
  double* pprev = nullptr;                // [max_nodes * 3] last call's source positions
  uint8_t* vprev = nullptr;               // [max_nodes]
  double* rigid = nullptr;                // [max_nodes * 3] this call's rigid motion
  double* fit = nullptr;                  // [64] scalars of k_mo_fit; fit[40] is std_prev across calls
  int T = 0, n_prev = 0, cur = 0;
  int launches = 0;
  std::vector<void*> allocs;
};

// ------------------------------------------------------------------------------------------------ network
struct MoIn {
  const float* a;         // (na, ca), row amap[n] (or n)
  const int32_t* amap;
  int ca, na;
  const float* b;         // (n, cb) appended, or null
  int cb;
};

__device__ __forceinline__ float mo_load(const MoIn& in, int node, int c) {
  if (c < in.ca) {
    int r = node;
    if (in.amap) r = min(max(in.amap[node], 0), in.na - 1);
    return in.a[(int64_t)r * in.ca + c];
  }
  return in.b[(int64_t)node * in.cb + (c - in.ca)];
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

// LayerNorm (eps 1e-5, biased variance) + relu of a row held two channels per lane (lane, lane + 64)
__device__ __forceinline__ void mo_norm_relu(float& v0, float& v1, int lane, int C, const float* __restrict__ nw,
                                             const float* __restrict__ nb) {
  const bool in0 = lane < C, in1 = lane + 64 < C;
  const float mean = wave_sum(v0 + v1) / (float)C;
  const float d0 = in0 ? v0 - mean : 0.f, d1 = in1 ? v1 - mean : 0.f;
  const float var = wave_sum(fmaf(d0, d0, d1 * d1)) / (float)C;
  const float r = 1.0f / sqrtf(var + 1e-5f);
  v0 = in0 ? fmaxf(fmaf(d0 * r, nw[lane], nb[lane]), 0.f) : 0.f;
  v1 = in1 ? fmaxf(fmaf(d1 * r, nw[lane + 64], nb[lane + 64]), 0.f) : 0.f;
}

__global__ __launch_bounds__(128) void k_mo_seq(const float* __restrict__ wg, const float* __restrict__ pos,
                                                const float* __restrict__ cm, const float* __restrict__ hist, int T,
                                                int n, float* __restrict__ x0) {
  __shared__ float w[kSeqFloats];
  __shared__ float xin[kMoNB][4], h0[kMoNB][32], h1[kMoNB][32], g[kMoNB][128], sp[kMoNB][4];
  const int j = threadIdx.x, nl = j >> 5, u = j & 31;
  const int node0 = blockIdx.x * kMoNB, node = node0 + nl;
  for (int i = j; i < kSeqFloats; i += 128) w[i] = wg[i];
  h0[nl][u] = 0.f;
  h1[nl][u] = 0.f;
  float c0 = 0.f, c1 = 0.f;
  for (int t = 0; t < T; ++t) {
    if (j < 4 * kMoNB) {
      const int nd = node0 + (j >> 2);
      xin[j >> 2][j & 3] = nd < n ? hist[((int64_t)t * n + nd) * 4 + (j & 3)] : 0.f;
    }
    __syncthreads();
    float acc[kMoNB], hh[kMoNB];
#pragma unroll
    for (int b = 0; b < kMoNB; ++b) { acc[b] = 0.f; hh[b] = 0.f; }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float wv = w[kSeqIh0 + c * 128 + j];
#pragma unroll
      for (int b = 0; b < kMoNB; ++b) acc[b] = fmaf(xin[b][c], wv, acc[b]);
    }
#pragma unroll 8
    for (int c = 0; c < 32; ++c) {
      const float wv = w[kSeqHh0 + c * 128 + j];
#pragma unroll
      for (int b = 0; b < kMoNB; ++b) hh[b] = fmaf(h0[b][c], wv, hh[b]);
    }
#pragma unroll
    for (int b = 0; b < kMoNB; ++b) g[b][j] = (acc[b] + w[kSeqBi0 + j]) + (hh[b] + w[kSeqBh0 + j]);
    __syncthreads();
    {
      const float gi = 1.f / (1.f + expf(-g[nl][u])), gf = 1.f / (1.f + expf(-g[nl][32 + u]));
      const float gg = tanhf(g[nl][64 + u]), go = 1.f / (1.f + expf(-g[nl][96 + u]));
      c0 = fmaf(gf, c0, gi * gg);
      h0[nl][u] = go * tanhf(c0);
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < kMoNB; ++b) { acc[b] = 0.f; hh[b] = 0.f; }
#pragma unroll 8
    for (int c = 0; c < 32; ++c) {
      const float wi = w[kSeqIh1 + c * 128 + j], wh = w[kSeqHh1 + c * 128 + j];
#pragma unroll
      for (int b = 0; b < kMoNB; ++b) {
        acc[b] = fmaf(h0[b][c], wi, acc[b]);
        hh[b] = fmaf(h1[b][c], wh, hh[b]);
      }
    }
#pragma unroll
    for (int b = 0; b < kMoNB; ++b) g[b][j] = (acc[b] + w[kSeqBi1 + j]) + (hh[b] + w[kSeqBh1 + j]);
    __syncthreads();
    {
      const float gi = 1.f / (1.f + expf(-g[nl][u])), gf = 1.f / (1.f + expf(-g[nl][32 + u]));
      const float gg = tanhf(g[nl][64 + u]), go = 1.f / (1.f + expf(-g[nl][96 + u]));
      c1 = fmaf(gf, c1, gi * gg);
      h1[nl][u] = go * tanhf(c1);
    }
    __syncthreads();
  }
  if (j < 4 * kMoNB) {
    const int b = j >> 2, o = j & 3;
    float acc = 0.f;
    for (int c = 0; c < 32; ++c) acc = fmaf(h1[b][c], w[kSeqLinW + c * 4 + o], acc);
    sp[b][o] = acc + w[kSeqLinB + o];
  }
  __syncthreads();
  if (node < n) {
    float f[11];
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = pos[(int64_t)node * 3 + c];
#pragma unroll
    for (int c = 0; c < 4; ++c) f[3 + c] = sp[nl][c];
#pragma unroll
    for (int c = 0; c < 4; ++c) f[7 + c] = cm[(int64_t)node * 4 + c];
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 11; ++c) acc = fmaf(f[c], w[kSeqEncW + c * 32 + u], acc);
    x0[(int64_t)node * 32 + u] = acc + w[kSeqEncB + u];
  }
}

__global__ __launch_bounds__(256) void k_mo_proj(MoIn in, int n, int C, int norm, const float* __restrict__ Wt,
                                                 const float* __restrict__ bias, const float* __restrict__ nw,
                                                 const float* __restrict__ nb, float* __restrict__ qkvs) {
  __shared__ float xs[kMoTile][128];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int node0 = blockIdx.x * kMoTile, node = node0 + wave;
  float v0 = 0.f, v1 = 0.f;
  if (node < n) {
    if (lane < C) v0 = mo_load(in, node, lane);
    if (lane + 64 < C) v1 = mo_load(in, node, lane + 64);
  }
  if (norm) mo_norm_relu(v0, v1, lane, C, nw, nb);
  xs[wave][lane] = v0;
  xs[wave][lane + 64] = v1;
  __syncthreads();
  const int C4 = 4 * C;
  for (int o = threadIdx.x; o < C4; o += 256) {
    float acc[kMoTile];
#pragma unroll
    for (int t = 0; t < kMoTile; ++t) acc[t] = 0.f;
#pragma unroll 8
    for (int c = 0; c < C; ++c) {
      const float wv = Wt[(int64_t)c * C4 + o];
#pragma unroll
      for (int t = 0; t < kMoTile; ++t) acc[t] = fmaf(xs[t][c], wv, acc[t]);
    }
    const float bv = bias[o];
#pragma unroll
    for (int t = 0; t < kMoTile; ++t)
      if (node0 + t < n) qkvs[(int64_t)(node0 + t) * C4 + o] = acc[t] + bv;
  }
}

// the score of edge (s -> d): q_d · k_s / sqrt(C), the same value in every lane
__device__ __forceinline__ float mo_score(const float* __restrict__ qkvs, int C4, int C, int s, int lane, float q0,
                                          float q1, float scale) {
  const float* kr = qkvs + (int64_t)s * C4 + C;
  const float k0 = lane < C ? kr[lane] : 0.f, k1 = lane + 64 < C ? kr[lane + 64] : 0.f;
  return wave_sum(fmaf(q0, k0, q1 * k1)) * scale;
}

__global__ __launch_bounds__(256) void k_mo_attn(MoIn in, int n, int C, int res, const float* __restrict__ qkvs,
                                                 const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                                 float* __restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int d = blockIdx.x * kMoTile + wave;
  if (d >= n) return;   // uniform over the wave; no barrier below
  const int C4 = 4 * C;
  const bool in0 = lane < C, in1 = lane + 64 < C;
  const float* row = qkvs + (int64_t)d * C4;
  const float q0 = in0 ? row[lane] : 0.f, q1 = in1 ? row[lane + 64] : 0.f;
  const float scale = 1.0f / sqrtf((float)C);
  const int e0 = rowptr[d], e1 = rowptr[d + 1];
  float m = -INFINITY;
  for (int base = e0; base < e1; base += 64) {
    const int mine = base + lane < e1 ? src[base + lane] : 0;
    const int cnt = min(64, e1 - base);
    for (int i = 0; i < cnt; ++i) m = fmaxf(m, mo_score(qkvs, C4, C, __shfl(mine, i, 64), lane, q0, q1, scale));
  }
  float den = 0.f, a0 = 0.f, a1 = 0.f;
  for (int base = e0; base < e1; base += 64) {
    const int mine = base + lane < e1 ? src[base + lane] : 0;
    const int cnt = min(64, e1 - base);
    for (int i = 0; i < cnt; ++i) {
      const int s = __shfl(mine, i, 64);
      const float p = expf(mo_score(qkvs, C4, C, s, lane, q0, q1, scale) - m);
      const float* vr = qkvs + (int64_t)s * C4 + 2 * C;
      den = den + p;
      if (in0) a0 = fmaf(p, vr[lane], a0);
      if (in1) a1 = fmaf(p, vr[lane + 64], a1);
    }
  }
  const float inv = e1 > e0 ? 1.0f / (den + 1e-16f) : 0.f;
  if (in0) {
    float o = fmaf(a0, inv, row[3 * C + lane]);
    if (res) o = mo_load(in, d, lane) + o;
    out[(int64_t)d * C + lane] = o;
  }
  if (in1) {
    float o = fmaf(a1, inv, row[3 * C + lane + 64]);
    if (res) o = mo_load(in, d, lane + 64) + o;
    out[(int64_t)d * C + lane + 64] = o;
  }
}

__global__ __launch_bounds__(256) void k_mo_head(const float* __restrict__ x, int n, const float* __restrict__ hw,
                                                 float* __restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int node = blockIdx.x * kMoTile + wave;
  if (node >= n) return;
  float v0 = x[(int64_t)node * 128 + lane], v1 = x[(int64_t)node * 128 + lane + 64];
  mo_norm_relu(v0, v1, lane, 128, hw, hw + 128);
  const float* Wt = hw + 256;
  float r[4];
#pragma unroll
  for (int o = 0; o < 4; ++o) r[o] = wave_sum(fmaf(v0, Wt[lane * 4 + o], v1 * Wt[(lane + 64) * 4 + o])) + hw[768 + o];
  if (lane == 0) {
    const float s = r[3];
    r[3] = s > 20.f ? s : log1pf(expf(s));   // F.softplus, beta 1, threshold 20
    *(float4*)(out + (int64_t)node * 4) = make_float4(r[0], r[1], r[2], r[3]);
  }
}

// ------------------------------------------------------------------------------------------------ incoming-edge CSR
__global__ __launch_bounds__(256) void k_mo_indeg(const int32_t* __restrict__ nn, int n, int k,
                                                  int32_t* __restrict__ deg) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int d = blockIdx.x * 4 + wave;
  if (d >= n) return;
  const int E = n * k;
  int cnt = 0;
  for (int base = 0; base < E; base += 64) {
    const int i = base + lane;
    cnt += __popcll(__ballot(i < E && nn[i] == d));
  }
  if (lane == 0) deg[d] = cnt;
}

// one workgroup: rowptr = exclusive scan of deg (rowptr[n] = the number of edges)
__global__ __launch_bounds__(1024) void k_mo_scan(const int32_t* __restrict__ deg, int n, int32_t* __restrict__ rowptr) {
  __shared__ int part[1024];
  const int t = threadIdx.x, per = (n + 1023) / 1024;
  const int lo = min(t * per, n), hi = min(lo + per, n);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += deg[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int i = 0; i < 1024; ++i) {
      const int v = part[i];
      part[i] = run;
      run += v;
    }
    rowptr[n] = run;
  }
  __syncthreads();
  int run = part[t];
  for (int i = lo; i < hi; ++i) {
    rowptr[i] = run;
    run += deg[i];
  }
}

__global__ __launch_bounds__(256) void k_mo_fill(const int32_t* __restrict__ nn, int n, int k,
                                                 const int32_t* __restrict__ rowptr, int32_t* __restrict__ src) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int d = blockIdx.x * 4 + wave;
  if (d >= n) return;
  const int E = n * k;
  int off = rowptr[d];
  for (int base = 0; base < E; base += 64) {
    const int i = base + lane;
    const bool hit = i < E && nn[i] == d;
    const unsigned long long mask = __ballot(hit);
    if (hit) src[off + __popcll(mask & ((1ull << lane) - 1ull))] = i / k;
    off += __popcll(mask);
  }
}

// ------------------------------------------------------------------------------------------------ pre / post
// fit[]: 0-8 R, 9-11 t, 12-14 mean of all positions, 15 std, 16 std of the call before, 17 degenerate,
//        18-26 R of the previous-frame fit, 27-29 its t, 30 previous fit degenerate; 40 std carried to the next call
constexpr int kFitStdCarry = 40;

template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*red)[32]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();   // red may still be read from the reduction before
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const double s = wave_sum(v[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < K; ++i) {
    double s = red[0][i];
    for (int w = 1; w < 16; ++w) s = s + red[w][i];
    v[i] = s;
  }
}

__device__ __forceinline__ double fro3(const double (&X)[9]) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) s = s + X[i] * X[i];
  return sqrt(s);
}

// R = the orthogonal polar factor of Hᵀ (= V Uᵀ of H = U S Vᵀ, reflections kept), by scaled Newton steps
// X <- (γ X + X⁻ᵀ / γ) / 2. False: H is numerically singular (|det| <= 1e-12 |H|_F³).
__device__ bool polar3(const double (&H)[9], double (&R)[9]) {
  double X[9];
  const double nf = fro3(H);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) X[3 * i + j] = H[3 * j + i];
  const double det0 = X[0] * (X[4] * X[8] - X[5] * X[7]) - X[1] * (X[3] * X[8] - X[5] * X[6]) +
                      X[2] * (X[3] * X[7] - X[4] * X[6]);
  if (!(nf > 0.0) || !isfinite(nf) || !(fabs(det0) > 1e-12 * nf * nf * nf)) return false;
#pragma unroll
  for (int i = 0; i < 9; ++i) X[i] = X[i] / nf;
  for (int it = 0; it < 60; ++it) {
    double Y[9];   // X⁻ᵀ: the cofactors over the determinant
    Y[0] = X[4] * X[8] - X[5] * X[7];
    Y[1] = X[5] * X[6] - X[3] * X[8];
    Y[2] = X[3] * X[7] - X[4] * X[6];
    Y[3] = X[2] * X[7] - X[1] * X[8];
    Y[4] = X[0] * X[8] - X[2] * X[6];
    Y[5] = X[1] * X[6] - X[0] * X[7];
    Y[6] = X[1] * X[5] - X[2] * X[4];
    Y[7] = X[2] * X[3] - X[0] * X[5];
    Y[8] = X[0] * X[4] - X[1] * X[3];
    const double det = X[0] * Y[0] + X[1] * Y[1] + X[2] * Y[2];
#pragma unroll
    for (int i = 0; i < 9; ++i) Y[i] = Y[i] / det;
    const double gam = sqrt(fro3(Y) / fro3(X));
    double dl = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const double xn = 0.5 * (gam * X[i] + Y[i] / gam);
      dl = dl + (xn - X[i]) * (xn - X[i]);
      X[i] = xn;
    }
    if (dl < 1e-30) break;
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = X[i];
  return true;
}

__global__ __launch_bounds__(1024) void k_mo_fit(const double* __restrict__ src, const double* __restrict__ dst,
                                                 const uint8_t* __restrict__ vis, int n,
                                                 const double* __restrict__ pprev, const uint8_t* __restrict__ vprev,
                                                 int n_prev, double* __restrict__ fit) {
  __shared__ double red[16][32];
  const int tid = threadIdx.x;
  // phase 1: counts and centroids (current: visible src, visible dst, all src; previous: visible pprev, visible src)
  double a[17];
#pragma unroll
  for (int i = 0; i < 17; ++i) a[i] = 0.0;
  for (int i = tid; i < n; i += 1024) {
    const double p[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
    a[7] = a[7] + p[0]; a[8] = a[8] + p[1]; a[9] = a[9] + p[2];
    if (vis[i]) {
      a[0] = a[0] + 1.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        a[1 + c] = a[1 + c] + p[c];
        a[4 + c] = a[4 + c] + (p[c] + (dst[3 * i + c] - p[c]));
      }
    }
    if (i < n_prev && vprev[i]) {
      a[10] = a[10] + 1.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double q = pprev[3 * i + c];
        a[11 + c] = a[11 + c] + q;
        a[14 + c] = a[14 + c] + (q + (p[c] - q));
      }
    }
  }
  block_sum<17>(a, red);
  const double nv = a[0], npv = a[10];
  double c0[3], c1[3], call[3], d0[3], d1[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    c0[c] = nv > 0.0 ? a[1 + c] / nv : 0.0;
    c1[c] = nv > 0.0 ? a[4 + c] / nv : 0.0;
    call[c] = a[7 + c] / (double)n;
    d0[c] = npv > 0.0 ? a[11 + c] / npv : 0.0;
    d1[c] = npv > 0.0 ? a[14 + c] / npv : 0.0;
  }
  // phase 2: H = Σ (p0 - c0)ᵀ (p1 - c1) over the visible rows, for both fits
  double h[18];
#pragma unroll
  for (int i = 0; i < 18; ++i) h[i] = 0.0;
  for (int i = tid; i < n; i += 1024) {
    double p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = src[3 * i + c];
    if (vis[i]) {
      double x[3], y[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        x[c] = p[c] - c0[c];
        y[c] = (p[c] + (dst[3 * i + c] - p[c])) - c1[c];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) h[3 * r + c] = h[3 * r + c] + x[r] * y[c];
    }
    if (i < n_prev && vprev[i]) {
      double x[3], y[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double q = pprev[3 * i + c];
        x[c] = q - d0[c];
        y[c] = (q + (p[c] - q)) - d1[c];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) h[9 + 3 * r + c] = h[9 + 3 * r + c] + x[r] * y[c];
    }
  }
  block_sum<18>(h, red);
  // every thread solves the two 3x3 problems itself (the same arithmetic, the same result)
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tp[3] = {0, 0, 0};
  bool ok = false, okp = false;
  {
    double H[9], Q[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = h[i];
    ok = nv >= 3.0 && polar3(H, Q);
    if (ok) {
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = Q[i];
#pragma unroll
      for (int r = 0; r < 3; ++r) t[r] = c1[r] - ((R[3 * r] * c0[0] + R[3 * r + 1] * c0[1]) + R[3 * r + 2] * c0[2]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = h[9 + i];
    okp = npv >= 3.0 && polar3(H, Q);
    if (okp) {
#pragma unroll
      for (int i = 0; i < 9; ++i) Rp[i] = Q[i];
#pragma unroll
      for (int r = 0; r < 3; ++r) tp[r] = d1[r] - ((Rp[3 * r] * d0[0] + Rp[3 * r + 1] * d0[1]) + Rp[3 * r + 2] * d0[2]);
    }
  }
  // phases 3 and 4: the per-axis mean and (biased) variance of the visible rows' non-rigid motion in centimetres
  double s1[3] = {0, 0, 0};
  for (int i = tid; i < n; i += 1024) {
    if (!vis[i]) continue;
    double p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = src[3 * i + c];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double rm = (((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2]) + t[r]) - p[r];
      s1[r] = s1[r] + ((dst[3 * i + r] - p[r]) - rm) * 100.0;
    }
  }
  block_sum<3>(s1, red);
  double mu[3], s2[3] = {0, 0, 0};
#pragma unroll
  for (int c = 0; c < 3; ++c) mu[c] = nv > 0.0 ? s1[c] / nv : 0.0;
  for (int i = tid; i < n; i += 1024) {
    if (!vis[i]) continue;
    double p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = src[3 * i + c];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double rm = (((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2]) + t[r]) - p[r];
      const double e = ((dst[3 * i + r] - p[r]) - rm) * 100.0 - mu[r];
      s2[r] = s2[r] + e * e;
    }
  }
  block_sum<3>(s2, red);
  double sd = 0.0;
  if (nv > 0.0) sd = ((sqrt(s2[0] / nv) + sqrt(s2[1] / nv)) + sqrt(s2[2] / nv)) / 3.0;
  sd = sd + 0.1;
  if (tid == 0) {
    for (int i = 0; i < 9; ++i) { fit[i] = R[i]; fit[18 + i] = Rp[i]; }
    for (int i = 0; i < 3; ++i) { fit[9 + i] = t[i]; fit[12 + i] = call[i]; fit[27 + i] = tp[i]; }
    fit[15] = sd;
    fit[16] = fit[kFitStdCarry];
    fit[17] = ok ? 0.0 : 1.0;
    fit[30] = okp ? 0.0 : 1.0;
    fit[kFitStdCarry] = sd;
  }
}

// first: the handle's first call (the history is one row of zeros). T: rows of the new history; drop: the old one was
// full and loses its oldest row.
__global__ __launch_bounds__(256) void k_mo_apply(const double* __restrict__ src, const double* __restrict__ dst,
                                                  const uint8_t* __restrict__ vis, int n, double* __restrict__ pprev,
                                                  uint8_t* __restrict__ vprev, int n_prev, int first, int T, int drop,
                                                  int64_t stride, const double* __restrict__ fit,
                                                  const double* __restrict__ hold, double* __restrict__ hnew,
                                                  double* __restrict__ rigid, float* __restrict__ pos_c,
                                                  float* __restrict__ cm, float* __restrict__ hist_out,
                                                  int32_t* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *status = (fit[17] != 0.0 ? 1 : 0) | (!first && fit[30] != 0.0 ? 2 : 0);
  if (i >= n) return;
  const double sd = fit[15], sd_prev = fit[16];
  double p[3], rm[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) p[c] = src[3 * i + c];
  const bool v = vis[i] != 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    rm[r] = (((fit[3 * r] * p[0] + fit[3 * r + 1] * p[1]) + fit[3 * r + 2] * p[2]) + fit[9 + r]) - p[r];
    rigid[3 * i + r] = rm[r];
    pos_c[3 * i + r] = (float)(p[r] - fit[12 + r]);
    cm[4 * i + r] = v ? (float)((((dst[3 * i + r] - p[r]) - rm[r]) * 100.0) / sd) : 0.f;
  }
  cm[4 * i + 3] = v ? 1.f : 0.f;
  const bool old = !first && i < n_prev;
  for (int t = 0; t + 1 < T; ++t) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double hv = old ? hold[((int64_t)(t + drop) * stride + i) * 4 + c] * sd_prev / sd : 0.0;
      hnew[((int64_t)t * stride + i) * 4 + c] = hv;
      hist_out[((int64_t)t * n + i) * 4 + c] = (float)hv;
    }
  }
  double last[4] = {0.0, 0.0, 0.0, 0.0};
  if (old) {
    double q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = pprev[3 * i + c];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double rp = (((fit[18 + 3 * r] * q[0] + fit[19 + 3 * r] * q[1]) + fit[20 + 3 * r] * q[2]) + fit[27 + r]) - q[r];
      last[r] = fit[30] != 0.0 ? 0.0 : (((p[r] - q[r]) - rp) * 100.0) / sd;
    }
    last[3] = 1.0 / sd;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    hnew[((int64_t)(T - 1) * stride + i) * 4 + c] = last[c];
    hist_out[((int64_t)(T - 1) * n + i) * 4 + c] = (float)last[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) pprev[3 * i + c] = p[c];
  vprev[i] = v ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_mo_post(const float* __restrict__ raw, int n, const double* __restrict__ fit,
                                                 const double* __restrict__ rigid, double conf_scale,
                                                 double* __restrict__ node_motion, double* __restrict__ conf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (fit[17] != 0.0) {
    node_motion[3 * i] = node_motion[3 * i + 1] = node_motion[3 * i + 2] = 0.0;
    conf[i] = 0.0;
    return;
  }
  const double m0 = raw[4 * i], m1 = raw[4 * i + 1], m2 = raw[4 * i + 2], sg = raw[4 * i + 3];
  const double q = sg / (sqrt((m0 * m0 + m1 * m1) + m2 * m2) + 1.0);
  conf[i] = exp(-conf_scale * (q * q));
  const double sd = fit[15];
  node_motion[3 * i] = (m0 * sd) / 100.0 + rigid[3 * i];
  node_motion[3 * i + 1] = (m1 * sd) / 100.0 + rigid[3 * i + 1];
  node_motion[3 * i + 2] = (m2 * sd) / 100.0 + rigid[3 * i + 2];
}

// ------------------------------------------------------------------------------------------------ host
static void mo_free(Motion* a) {
  for (void* p : a->allocs)
    if (p) (void)hipFree(p);
  delete a;
}

template <typename T>
static bool mo_alloc(Motion* a, T** p, size_t count) {
  void* q = nullptr;
  if (hipMalloc(&q, (count ? count : 1) * sizeof(T)) != hipSuccess) return false;
  a->allocs.push_back(q);
  *p = (T*)q;
  return true;
}

static int mo_forward(Motion* a, const float* pos, const float* cm, const float* hist, int T, int n, float* out,
                      hipStream_t hs) {
  int launches = 0;
  hipLaunchKernelGGL(k_mo_seq, dim3((n + kMoNB - 1) / kMoNB), dim3(128), 0, hs, (const float*)a->w + 2, pos, cm, hist,
                     T, n, a->x0);
  OFX_LAUNCH_CHECK();
  ++launches;
  int nl[4];
  for (int l = 0; l < 4; ++l) nl[l] = a->lv[l].n;
  // the input of every conv: rows of `a` through a level map, with `b` appended
  MoIn in[kMoLayers];
  for (int l = 0; l < kMoLayers; ++l) in[l] = MoIn{l ? a->out[l - 1] : a->x0, nullptr, kMoLayer[l].C, nl[kMoLayer[l].level], nullptr, 0};
  in[3] = MoIn{a->out[2], a->down[0], 32, nl[0], nullptr, 0};
  in[5] = MoIn{a->out[4], a->down[1], 32, nl[1], nullptr, 0};
  in[7] = MoIn{a->out[6], a->down[2], 32, nl[2], nullptr, 0};
  in[9] = MoIn{a->out[8], a->up[2], 32, nl[3], a->out[6], 32};
  in[11] = MoIn{a->out[10], a->up[1], 64, nl[2], a->out[4], 32};
  in[13] = MoIn{a->out[12], a->up[0], 96, nl[1], a->out[2], 32};
  for (int l = 0; l < kMoLayers; ++l) {
    const MoLayerDef& d = kMoLayer[l];
    const MoLevel& lv = a->lv[d.level];
    const int C = d.C, nn = lv.n;
    const float* W = a->w + a->off_layer[l];
    const float* bias = W + (int64_t)4 * C * C;
    const unsigned grid = (unsigned)((nn + kMoTile - 1) / kMoTile);
    hipLaunchKernelGGL(k_mo_proj, dim3(grid), dim3(256), 0, hs, in[l], nn, C, d.norm, W, bias, bias + 4 * C,
                       bias + 5 * C, a->qkvs);
    OFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mo_attn, dim3(grid), dim3(256), 0, hs, in[l], nn, C, d.norm, (const float*)a->qkvs,
                       (const int32_t*)lv.rowptr, (const int32_t*)lv.src, a->out[l]);
    OFX_LAUNCH_CHECK();
    launches += 2;
  }
  hipLaunchKernelGGL(k_mo_head, dim3((n + kMoTile - 1) / kMoTile), dim3(256), 0, hs, (const float*)a->out[14], n,
                     (const float*)a->w + a->off_head, out);
  OFX_LAUNCH_CHECK();
  ++launches;
  a->launches = launches;
  return OFX_OK;
}

}  // namespace ofx

using namespace ofx;

extern "C" {

int ofx_motion_create(const float* weights, int64_t n_floats, int32_t max_nodes, int32_t max_hist, void** handle) {
  OFX_CHECK_ARG(handle, "null handle");
  *handle = nullptr;
  OFX_CHECK_ARG(weights, "null weights");
  OFX_CHECK_ARG(n_floats == mo_blob_floats(), "the weight blob has %lld floats, the layout has %lld",
                (long long)n_floats, (long long)mo_blob_floats());
  uint32_t head[2];
  memcpy(head, weights, sizeof(head));
  OFX_CHECK_ARG(head[0] == kMoTag && (int64_t)head[1] == n_floats, "the weight blob's layout tag %08x / length %u is not %08x / %lld",
                head[0], head[1], kMoTag, (long long)n_floats);
  OFX_CHECK_ARG(max_nodes >= 1 && max_hist >= 1 && max_hist <= kMoMaxHist, "bad max_nodes %d / max_hist %d (1..%d)",
                max_nodes, max_hist, kMoMaxHist);
  if (max_nodes > kMoMaxNodes) {
    set_error("max_nodes %d exceeds %d", max_nodes, kMoMaxNodes);
    return OFX_ERR_RANGE;
  }
  Motion* a = new Motion();
  a->max_nodes = max_nodes;
  a->max_hist = max_hist;
  const size_t mn = (size_t)max_nodes;
  bool ok = mo_alloc(a, &a->w, (size_t)n_floats);
  for (int l = 0; l < 4 && ok; ++l)
    ok = mo_alloc(a, &a->lv[l].nn, mn * kMoMaxK) && mo_alloc(a, &a->lv[l].deg, mn) &&
         mo_alloc(a, &a->lv[l].rowptr, mn + 1) && mo_alloc(a, &a->lv[l].src, mn * kMoMaxK);
  for (int l = 0; l < 3 && ok; ++l) ok = mo_alloc(a, &a->down[l], mn) && mo_alloc(a, &a->up[l], mn);
  ok = ok && mo_alloc(a, &a->x0, mn * 32) && mo_alloc(a, &a->qkvs, mn * 512);
  for (int l = 0; l < kMoLayers && ok; ++l) ok = mo_alloc(a, &a->out[l], mn * kMoLayer[l].C);
  for (int i = 0; i < 2 && ok; ++i) ok = mo_alloc(a, &a->hist[i], (size_t)max_hist * mn * 4);
  ok = ok && mo_alloc(a, &a->pprev, mn * 3) && mo_alloc(a, &a->vprev, mn) && mo_alloc(a, &a->rigid, mn * 3) &&
       mo_alloc(a, &a->fit, (size_t)64);
  if (!ok) {
    mo_free(a);
    set_error("ofx_motion_create: buffers for %d nodes could not be allocated", max_nodes);
    return OFX_ERR_ALLOC;
  }
  if (hipMemcpy(a->w, weights, (size_t)n_floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(a->fit, 0, 64 * sizeof(double)) != hipSuccess) {
    mo_free(a);
    set_error("ofx_motion_create: the weights could not be copied to the device");
    return OFX_ERR_HIP;
  }
  int64_t off = 2 + kSeqFloats;
  for (int l = 0; l < kMoLayers; ++l) {
    a->off_layer[l] = off;
    off += mo_layer_floats(kMoLayer[l].C);
  }
  a->off_head = off;
  *handle = a;
  return OFX_OK;
}

int ofx_motion_destroy(void* handle) {
  if (!handle) return OFX_OK;
  (void)hipDeviceSynchronize();
  mo_free((Motion*)handle);
  return OFX_OK;
}

int ofx_motion_set_graph(void* handle, const ofx_motion_graph* g, ofx_stream_t s) {
  Motion* a = (Motion*)handle;
  OFX_CHECK_ARG(a && g, "null handle / graph");
  for (int l = 0; l < 4; ++l) {
    OFX_CHECK_ARG(g->nn_index[l], "null nn_index of level %d", l);
    OFX_CHECK_ARG(g->n[l] >= 1 && g->n[l] <= a->max_nodes, "level %d has %d nodes, outside [1, %d] (the handle's max_nodes)",
                  l, g->n[l], a->max_nodes);
    OFX_CHECK_ARG(g->k[l] >= 1 && g->k[l] <= kMoMaxK, "level %d has %d neighbours per node, outside [1, %d]", l, g->k[l],
                  kMoMaxK);
  }
  for (int l = 0; l < 3; ++l) OFX_CHECK_ARG(g->down[l] && g->up[l], "null sample map of level %d", l);
  hipStream_t hs = as_stream(s);
  a->graph = false;
  for (int l = 0; l < 4; ++l) {
    MoLevel& lv = a->lv[l];
    lv.n = g->n[l];
    lv.k = g->k[l];
    OFX_HIP(hipMemcpyAsync(lv.nn, g->nn_index[l], (size_t)lv.n * lv.k * sizeof(int32_t), hipMemcpyDeviceToDevice, hs));
    const unsigned grid = (unsigned)((lv.n + 3) / 4);
    hipLaunchKernelGGL(k_mo_indeg, dim3(grid), dim3(256), 0, hs, (const int32_t*)lv.nn, lv.n, lv.k, lv.deg);
    OFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mo_scan, dim3(1), dim3(1024), 0, hs, (const int32_t*)lv.deg, lv.n, lv.rowptr);
    OFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mo_fill, dim3(grid), dim3(256), 0, hs, (const int32_t*)lv.nn, lv.n, lv.k,
                       (const int32_t*)lv.rowptr, lv.src);
    OFX_LAUNCH_CHECK();
  }
  for (int l = 0; l < 3; ++l) {
    OFX_HIP(hipMemcpyAsync(a->down[l], g->down[l], (size_t)g->n[l + 1] * sizeof(int32_t), hipMemcpyDeviceToDevice, hs));
    OFX_HIP(hipMemcpyAsync(a->up[l], g->up[l], (size_t)g->n[l] * sizeof(int32_t), hipMemcpyDeviceToDevice, hs));
  }
  a->graph = true;
  return OFX_OK;
}

int ofx_motion_forward(void* handle, const float* pos, const float* curr_motion, const float* hist, int32_t T,
                       int32_t n_nodes, float* out, ofx_stream_t s) {
  Motion* a = (Motion*)handle;
  OFX_CHECK_ARG(a && pos && curr_motion && hist && out, "null handle / pos / curr_motion / hist / out");
  if (!a->graph) {
    set_error("ofx_motion_forward before ofx_motion_set_graph");
    return OFX_ERR_STATE;
  }
  OFX_CHECK_ARG(n_nodes == a->lv[0].n, "n_nodes %d is not the graph's %d", n_nodes, a->lv[0].n);
  OFX_CHECK_ARG(T >= 1 && T <= kMoMaxHist, "T %d outside [1, %d]", T, kMoMaxHist);
  OFX_CHECK_ARG(((uintptr_t)out & 15) == 0, "out must be 16-byte aligned");
  return mo_forward(a, pos, curr_motion, hist, T, n_nodes, out, as_stream(s));
}

int ofx_motion_complete(void* handle, const double* src, const double* dst, const uint8_t* visible, int32_t n_nodes,
                        double conf_scale, double* node_motion, double* confidence, int32_t* status, float* pos_c,
                        float* curr_motion, float* hist, float* raw, ofx_stream_t s) {
  Motion* a = (Motion*)handle;
  OFX_CHECK_ARG(a && src && dst && visible && node_motion && confidence && status && pos_c && curr_motion && hist && raw,
                "null handle / input / output");
  if (!a->graph) {
    set_error("ofx_motion_complete before ofx_motion_set_graph");
    return OFX_ERR_STATE;
  }
  OFX_CHECK_ARG(n_nodes == a->lv[0].n, "n_nodes %d is not the graph's %d", n_nodes, a->lv[0].n);
  OFX_CHECK_ARG(n_nodes >= a->n_prev, "n_nodes %d is below the %d of the call before (nodes are only appended)", n_nodes,
                a->n_prev);
  OFX_CHECK_ARG(conf_scale >= 0.0 && conf_scale == conf_scale, "bad conf_scale");
  OFX_CHECK_ARG(((uintptr_t)raw & 15) == 0, "raw must be 16-byte aligned");
  hipStream_t hs = as_stream(s);
  const int first = a->T == 0;
  const int drop = a->T == a->max_hist ? 1 : 0;
  const int T = first ? 1 : (a->T + 1 < a->max_hist ? a->T + 1 : a->max_hist);
  hipLaunchKernelGGL(k_mo_fit, dim3(1), dim3(1024), 0, hs, src, dst, visible, n_nodes, (const double*)a->pprev,
                     (const uint8_t*)a->vprev, first ? 0 : a->n_prev, a->fit);
  OFX_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_mo_apply, dim3((n_nodes + 255) / 256), dim3(256), 0, hs, src, dst, visible, n_nodes, a->pprev,
                     a->vprev, a->n_prev, first, T, drop, (int64_t)a->max_nodes, (const double*)a->fit,
                     (const double*)a->hist[a->cur], a->hist[a->cur ^ 1], a->rigid, pos_c, curr_motion, hist, status);
  OFX_LAUNCH_CHECK();
  a->cur ^= 1;
  a->T = T;
  a->n_prev = n_nodes;
  if (int st = mo_forward(a, pos_c, curr_motion, hist, T, n_nodes, raw, hs)) return st;
  hipLaunchKernelGGL(k_mo_post, dim3((n_nodes + 255) / 256), dim3(256), 0, hs, (const float*)raw, n_nodes,
                     (const double*)a->fit, (const double*)a->rigid, conf_scale, node_motion, confidence);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

int ofx_motion_reset(void* handle) {
  Motion* a = (Motion*)handle;
  OFX_CHECK_ARG(a, "null handle");
  a->T = 0;
  a->n_prev = 0;
  return OFX_OK;
}

int ofx_motion_info(void* handle, int64_t* info) {
  Motion* a = (Motion*)handle;
  OFX_CHECK_ARG(a && info, "null handle / info");
  info[0] = a->launches;
  info[1] = a->T;
  info[2] = a->n_prev;
  info[3] = a->max_nodes;
  for (int l = 0; l < 4; ++l) info[4 + l] = a->graph ? a->lv[l].n : 0;
  info[8] = a->max_hist;
  info[9] = 0;
  return OFX_OK;
}

}  // extern "C"
