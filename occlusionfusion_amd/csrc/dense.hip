// Dense symmetric positive definite solve in f64 (ofx_spd_solve): the exact linear solver of the Gauss-Newton step for
// small graphs (ofx_gn_params.precond = OFX_PRECOND_DIRECT; the reference's LinearSolverLU, model/model.py:59-86).
//
// Right-looking blocked Cholesky with panel width kP, one launch per panel step and no communication between the
// workgroups of a launch: the only dependencies are the launch boundaries on the stream (no grid barrier, no flags, no
// atomics; every sum runs in a fixed order, so two runs are bit-identical). The right-hand side is carried as row n of
// the augmented lower triangle, so y = L⁻¹ b falls out of the same panel steps.
//
// Launch k (k = 0 .. panels + 1) runs three kinds of workgroups:
//   * tile (i, j), i >= j > k: loads the already-updated diagonal block A_kk and factors it in LDS (redundantly in every
//     workgroup), forms its two panel blocks L_ik = A_ik L_kk⁻ᵀ and L_jk by substitution, and subtracts L_ik L_jkᵀ from
//     its tile. It writes nothing but its own tile.
//   * write-back (i, k-1), i >= k-1: repeats that factorisation and substitution for panel k-1 and stores the rows of
//     L_{i,k-1} below the diagonal block (and b's) in place. The store is one launch late on purpose: within launch k-1
//     every tile workgroup still reads A_{i,k-1} to form its own copy of the panel, so a store in that launch would race
//     with them. In launch k the only readers of column block k-1 are these write-back workgroups: each reads its own rows,
//     which it alone stores, and the diagonal block A_{k-1,k-1}, which none of them stores.
//   * diagonal (k-2): one workgroup factors A_{k-2,k-2} once more and stores L_{k-2,k-2} over it — a launch later still,
//     when no workgroup reads that block any more (every write-back workgroup of launch k-1 needed it unfactored).
// So every address is either read by workgroups of a launch or written by exactly one that alone reads it, never both.
// Lᵀ x = y then runs as one small launch per panel from the right (k_chol_back_panel, the default) or as a single
// workgroup sweeping L once (k_chol_back); OFX_DENSE_BACK selects.
//
// A pivot <= 0 or non-finite sets status = [1, pivot index]; every workgroup factoring that block sees the same pivot,
// every later launch returns at its first load, and the backward solve leaves x = 0.
#include <float.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "ofx_common.h"

namespace ofx {

constexpr int kP = 64;            // panel width = tile edge
constexpr int kPL = kP + 1;       // LDS row stride of the row-major blocks (a lane per row: conflict-free)
constexpr int kW = 16;            // columns a lane keeps in registers at a time (factorisation and substitution)
static_assert(kP == 64 && kP % kW == 0, "a lane per row of a panel block");
constexpr int kDenseMax = 3072;   // unknowns (512 nodes)
constexpr bool kBackPanelDefault = true;   // the backward solve: one launch per panel (the faster form at n = 1626)
// LDS of k_chol_step, in doubles: LT (L_kk transposed, [c][r]), S (A_kk, row-major), Pi, Pj (the panel blocks), 1/diag
constexpr int kOffS = kP * kP, kOffPi = kOffS + kP * kPL, kOffPj = kOffPi + kP * kPL, kOffInv = kOffPj + kP * kPL,
              kOffBad = kOffInv + kP, kStepLds = (kOffBad + 2) * (int)sizeof(double);
static_assert(kStepLds <= 160 * 1024, "k_chol_step LDS");

__device__ __forceinline__ double dn_read_lane(double x, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}
// LDS hand-off inside one wave: wait for this wave's LDS operations (gfx9 s_waitcnt: lgkmcnt(0), others max)
__device__ __forceinline__ void dn_wave_lds_sync() {
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
}
// sd = sqrt(d) and inv = 1 / sqrt(d) for a positive normal d: v_rsq_f64, two Newton steps on the reciprocal root and one
// Heron correction of the root (each to within an ulp or two; a few dependent FMAs instead of the library sqrt and
// division, which sat on the factorisation's per-column critical path)
__device__ __forceinline__ void dn_sqrt_rsqrt(double d, double& sd, double& inv) {
  double y = __builtin_amdgcn_rsq(d);
  const double h = 0.5 * d;
  y = fma(y, fma(-h * y, y, 0.5), y);
  y = fma(y, fma(-h * y, y, 0.5), y);
  double r = d * y;
  r = fma(0.5 * y, fma(-r, r, d), r);
  sd = r;
  inv = y;
}
// row r of the augmented matrix: rows < n are A's, row n is b
__device__ __forceinline__ double* dn_row(double* A, int n, int lda, double* b, int r) {
  return r < n ? A + (int64_t)r * lda : b;
}

// One lane per row of a 64-row block P (row-major, stride kPL): P <- P L⁻ᵀ with L given transposed in LT and 1 / diag L
// in invd. Right-looking: x_c = a_c / L_cc, then a_q -= x_c L_qc for q > c.
__device__ __forceinline__ void dn_substitute(double* __restrict__ P, const double* __restrict__ LT,
                                              const double* __restrict__ invd, int lane) {
  double* row = P + lane * kPL;
  for (int b0 = 0; b0 < kP; b0 += kW) {   // kW columns at a time in registers
    double x[kW];
#pragma unroll
    for (int q = 0; q < kW; ++q) x[q] = row[b0 + q];
#pragma unroll 4
    for (int p = 0; p < b0; ++p) {   // the columns already final (left-looking; b0 is a multiple of kW)
      const double xp = row[p];
#pragma unroll
      for (int q = 0; q < kW; ++q) x[q] = fma(-xp, LT[p * kP + b0 + q], x[q]);
    }
#pragma unroll
    for (int c = 0; c < kW; ++c) {
      const double xc = x[c] * invd[b0 + c];
      x[c] = xc;
#pragma unroll
      for (int q = c + 1; q < kW; ++q) x[q] = fma(-xc, LT[(b0 + c) * kP + b0 + q], x[q]);
    }
#pragma unroll
    for (int q = 0; q < kW; ++q) row[b0 + q] = x[q];
  }
}

__global__ __launch_bounds__(256) void k_chol_step(double* A, int n, int lda, double* b, int32_t* status,
                                                   const int32_t* stop, int k, int ndg, int nwb) {
  if (stop && *stop) return;
  if (status[0]) return;
  extern __shared__ double4 dn_lds[];
  double* LT = reinterpret_cast<double*>(dn_lds);
  double* S = LT + kOffS;
  double* Pi = LT + kOffPi;
  double* Pj = LT + kOffPj;
  double* invd = LT + kOffInv;
  int* sbad = reinterpret_cast<int*>(LT + kOffBad);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nbr = (n + 1 + kP - 1) / kP;   // row blocks of the augmented matrix (b is row n)
  const bool dg = (int)blockIdx.x < ndg;           // stores the diagonal block of panel k - 2
  const bool wb = dg || (int)blockIdx.x < ndg + nwb;   // else: stores block (i, k - 1) below / beside the diagonal
  int kp, i, j;
  if (dg) {
    kp = k - 2;
    i = j = kp;
  } else if (wb) {
    kp = k - 1;
    i = kp + (int)blockIdx.x - ndg;
    j = i;
  } else {
    kp = k;
    int t = (int)blockIdx.x - ndg - nwb;
    j = k + 1;
    while (t >= nbr - j) { t -= nbr - j; ++j; }
    i = j + t;
  }
  const int c0 = kp * kP, pw = min(kP, n - c0);
  const bool two = !wb && i != j;
  if (tid == 0) *sbad = 0;
  // A_kk (lower triangle, identity beyond a ragged edge) and the panel blocks of row blocks i and j (zero beyond the edges)
  // (unrolled: all of a thread's loads are in flight before the first LDS store waits for one)
#pragma unroll
  for (int it = 0; it < kP * kP / 256; ++it) {
    const int idx = tid + 256 * it, r = idx >> 6, c = idx & 63;
    double d = r == c ? 1.0 : 0.0;
    if (r < pw && c <= r) d = A[(int64_t)(c0 + r) * lda + c0 + c];
    S[r * kPL + c] = d;
    const int gi = kP * i + r;
    double vi = 0.0;
    if (gi <= n && c < pw && c0 + c <= gi) vi = dn_row(A, n, lda, b, gi)[c0 + c];
    Pi[r * kPL + c] = vi;
    if (two) {
      const int gj = kP * j + r;
      double vj = 0.0;
      if (gj <= n && c < pw) vj = dn_row(A, n, lda, b, gj)[c0 + c];
      Pj[r * kPL + c] = vj;
    }
  }
  __syncthreads();
  if (wave == 0) {   // Cholesky of A_kk: a lane per row; left-looking over chunks of kW columns, right-looking inside one
    int badc = -1;
    for (int b0 = 0; b0 < kP; b0 += kW) {   // kW columns at a time in registers
      double a[kW];
#pragma unroll
      for (int q = 0; q < kW; ++q) a[q] = S[lane * kPL + b0 + q];
#pragma unroll 4
      for (int p = 0; p < b0; ++p) {   // the columns already final (left-looking): a_rq -= L_rp L_qp
        const double lp = LT[p * kP + lane];
#pragma unroll
        for (int q = 0; q < kW; ++q) a[q] = fma(-lp, LT[p * kP + b0 + q], a[q]);
      }
#pragma unroll
      for (int c = 0; c < kW; ++c) {
        const int gc = b0 + c;
        const double d = dn_read_lane(a[c], gc);
        const bool ok = d > 0.0 && d <= DBL_MAX;
        if (!ok && badc < 0) badc = gc;
        double sd, inv;
        dn_sqrt_rsqrt(ok ? d : 1.0, sd, inv);
        const double l = lane > gc ? a[c] * inv : (lane == gc ? sd : 0.0);
        LT[gc * kP + lane] = l;
        if (lane == gc) invd[gc] = inv;
#pragma unroll
        for (int q = c + 1; q < kW; ++q) a[q] = fma(-l, dn_read_lane(l, b0 + q), a[q]);
      }
      dn_wave_lds_sync();   // this chunk's columns of LT, before the next chunk reads them
    }
    if (badc >= 0 && lane == 0) {
      status[0] = 1;
      status[1] = c0 + badc;
      *sbad = 1;
    }
  }
  __syncthreads();
  if (*sbad) return;
  if (dg) {   // L_kk's lower triangle over A_kk: no workgroup of this launch reads panel k - 2
    for (int idx = tid; idx < kP * kP; idx += 256) {
      const int c = idx >> 6, r = idx & 63;
      if (r < pw && c <= r) A[(int64_t)(c0 + r) * lda + c0 + c] = LT[c * kP + r];
    }
    return;
  }
  if (wave == 0) dn_substitute(Pi, LT, invd, lane);
  else if (wave == 1 && two) dn_substitute(Pj, LT, invd, lane);
  __syncthreads();
  if (wb) {   // store the substituted rows of block (i, k - 1). Not the diagonal block's own rows: the other write-back
              // workgroups of this launch still read A_kk to factor it themselves (the next launch stores L_kk, above)
    for (int idx = tid; idx < kP * kP; idx += 256) {
      const int r = idx >> 6, c = idx & 63;
      const int gr = kP * i + r;
      if (c >= pw || gr > n || (i == kp && r < pw)) continue;
      dn_row(A, n, lda, b, gr)[c0 + c] = Pi[r * kPL + c];
    }
    return;
  }
  // tile (i, j) -= L_ik L_jkᵀ: 4 x 4 entries per thread, the sum over the panel in its fixed order
  const double* Lj = two ? Pj : Pi;
  const int tr = tid >> 4, tc = tid & 15;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[a][q] = 0.0;
#pragma unroll 4
  for (int p = 0; p < kP; ++p) {
    double va[4], vb[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) va[a] = Pi[(tr + 16 * a) * kPL + p];
#pragma unroll
    for (int q = 0; q < 4; ++q) vb[q] = Lj[(tc + 16 * q) * kPL + p];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[a][q] = fma(va[a], vb[q], acc[a][q]);
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int gr = kP * i + tr + 16 * a;
    if (gr > n) continue;
    double* rp = dn_row(A, n, lda, b, gr);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gc = kP * j + tc + 16 * q;
      if (gc < n && gc <= gr) rp[gc] = rp[gc] - acc[a][q];
    }
  }
}

// Lᵀ x = y, one workgroup sweeping L once from the right: per panel the 64 x 64 triangular solve by one wave (a lane per
// unknown), then y_q -= Σ_c L[c][q] x_c for the columns q to its left, a thread per column, in the fixed order of c.
__global__ __launch_bounds__(1024) void k_chol_back(const double* __restrict__ A, int n, int lda, double* __restrict__ b,
                                                    const int32_t* __restrict__ status, const int32_t* stop) {
  if (stop && *stop) return;
  __shared__ double ys[kDenseMax];
  __shared__ double Ld[kP * kPL];
  const int tid = threadIdx.x;
  if (status[0]) {   // not positive definite: x = 0
    for (int q = tid; q < n; q += 1024) b[q] = 0.0;
    return;
  }
  for (int q = tid; q < n; q += 1024) ys[q] = b[q];
  const int nbc = (n + kP - 1) / kP;
  for (int k = nbc - 1; k >= 0; --k) {
    const int c0 = k * kP, pw = min(kP, n - c0);
    for (int idx = tid; idx < kP * kP; idx += 1024) {
      const int r = idx >> 6, c = idx & 63;
      double d = r == c ? 1.0 : 0.0;
      if (r < pw && c <= r) d = A[(int64_t)(c0 + r) * lda + c0 + c];
      Ld[r * kPL + c] = d;
    }
    __syncthreads();
    if (tid < 64) {
      double yq = tid < pw ? ys[c0 + tid] : 0.0;
      const double rinv = 1.0 / Ld[tid * kPL + tid];
      for (int c = kP - 1; c >= 0; --c) {
        const double xc = dn_read_lane(yq * rinv, c);
        if (tid == c) yq = xc;
        else if (tid < c) yq = fma(-Ld[c * kPL + tid], xc, yq);
      }
      if (tid < pw) ys[c0 + tid] = yq;
    }
    __syncthreads();
    for (int q = tid; q < c0; q += 1024) {
      double acc = 0.0;
      const double* col = A + (int64_t)c0 * lda + q;
      int c = 0;
      for (; c + 16 <= pw; c += 16) {   // 16 loads in flight, the sum in the order of c
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = col[(int64_t)(c + u) * lda];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = fma(v[u], ys[c0 + c + u], acc);
      }
      for (; c < pw; ++c) acc = fma(col[(int64_t)c * lda], ys[c0 + c], acc);
      ys[q] -= acc;
    }
  }
  __syncthreads();
  for (int q = tid; q < n; q += 1024) b[q] = ys[q];
}

// Lᵀ x = y, one small launch per panel from the right (the other form of the backward solve). Launch k: a workgroup per
// column block j < k solves L_kkᵀ x_k = y_k itself (one wave, as above) and subtracts L_kjᵀ x_k from y_j, each quarter of
// the panel's rows summed by one wave and the four partial sums added in their fixed order. x_k is stored over y_k one
// launch later, by a workgroup of its own that repeats the solve: in launch k every workgroup still reads y_k. Launch 0
// has no reader of y_0 but the workgroup that solves for x_0, which stores it.
__global__ __launch_bounds__(256) void k_chol_back_panel(const double* __restrict__ A, int n, int lda, double* b,
                                                         const int32_t* __restrict__ status, const int32_t* stop, int k,
                                                         int nst) {
  if (stop && *stop) return;
  __shared__ double Ld[kP * kPL];
  __shared__ double xs[kP];
  __shared__ double part[4][kP];
  const int tid = threadIdx.x;
  const bool st = (int)blockIdx.x < nst;   // stores x_{k+1}
  if (status[0]) {   // not positive definite: x = 0 (the last launch's solving workgroup)
    if (k == 0 && !st)
      for (int q = tid; q < n; q += 256) b[q] = 0.0;
    return;
  }
  const int kp = st ? k + 1 : k;
  const int c0 = kp * kP, pw = min(kP, n - c0);
#pragma unroll
  for (int it = 0; it < kP * kP / 256; ++it) {
    const int idx = tid + 256 * it, r = idx >> 6, c = idx & 63;
    double d = r == c ? 1.0 : 0.0;
    if (r < pw && c <= r) d = A[(int64_t)(c0 + r) * lda + c0 + c];
    Ld[r * kPL + c] = d;
  }
  __syncthreads();
  if (tid < 64) {
    double yq = tid < pw ? b[c0 + tid] : 0.0;
    const double rinv = 1.0 / Ld[tid * kPL + tid];
    for (int c = kP - 1; c >= 0; --c) {
      const double xc = dn_read_lane(yq * rinv, c);
      if (tid == c) yq = xc;
      else if (tid < c) yq = fma(-Ld[c * kPL + tid], xc, yq);
    }
    xs[tid] = tid < pw ? yq : 0.0;
  }
  __syncthreads();
  if (st || k == 0) {
    if (tid < pw) b[c0 + tid] = xs[tid];
    return;
  }
  const int j = (int)blockIdx.x - nst, q = tid & 63, pt = tid >> 6;
  const double* col = A + (int64_t)c0 * lda + kP * j + q;
  double v[kP / 4];
#pragma unroll
  for (int u = 0; u < kP / 4; ++u) {
    const int c = (kP / 4) * pt + u;
    v[u] = c < pw ? col[(int64_t)c * lda] : 0.0;
  }
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < kP / 4; ++u) acc = fma(v[u], xs[(kP / 4) * pt + u], acc);
  part[pt][q] = acc;
  __syncthreads();
  if (pt == 0) b[kP * j + q] -= ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
}

// OFX_DENSE_BACK=panel|sweep (read per solve; A/B and tests): the backward solve's form
static bool dn_back_panel() {
  const char* e = getenv("OFX_DENSE_BACK");
  return e && e[0] ? strcmp(e, "panel") == 0 : kBackPanelDefault;
}

static void dn_step_grid(int n, int k, int* tiles, int* nwb, int* ndg) {
  const int nbr = (n + 1 + kP - 1) / kP, nbc = (n + kP - 1) / kP;
  int t = 0;
  for (int j = k + 1; j < nbc; ++j) t += nbr - j;
  *tiles = k < nbc ? t : 0;
  *nwb = (k >= 1 && k <= nbc) ? nbr - (k - 1) : 0;
  *ndg = (k >= 2 && k <= nbc + 1) ? 1 : 0;
}

int dense_spd_launches(int n) {
  const int nbc = (n + kP - 1) / kP;
  int c = dn_back_panel() ? nbc : 1;   // k_chol_back_panel per panel, or k_chol_back
  for (int k = 0; k <= nbc + 1; ++k) {
    int t, w, d;
    dn_step_grid(n, k, &t, &w, &d);
    if (t + w + d > 0) ++c;
  }
  return c;
}

int dense_panel_width() { return kP; }

// The solve's launches on hs; status (device int32[2]) must be zero when they run. stop (nullable): device word that
// makes every launch return at once when set.
int dense_spd_enqueue(double* A, int n, int lda, double* b, int32_t* status, const int32_t* stop, hipStream_t hs) {
  {   // k_chol_step's LDS is past the default limit: raised once per device
    static std::mutex mu;
    static bool done[64] = {};
    int dev = 0;
    OFX_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (dev < 0 || dev >= 64 || !done[dev]) {
      OFX_HIP(hipFuncSetAttribute((const void*)k_chol_step, hipFuncAttributeMaxDynamicSharedMemorySize, kStepLds));
      if (dev >= 0 && dev < 64) done[dev] = true;
    }
  }
  const int nbc = (n + kP - 1) / kP;
  for (int k = 0; k <= nbc + 1; ++k) {
    int t, w, d;
    dn_step_grid(n, k, &t, &w, &d);
    if (t + w + d == 0) continue;
    hipLaunchKernelGGL(k_chol_step, dim3(t + w + d), dim3(256), kStepLds, hs, A, n, lda, b, status, stop, k, d, w);
  }
  if (dn_back_panel()) {
    for (int k = nbc - 1; k >= 0; --k) {
      const int nst = k + 1 < nbc ? 1 : 0;
      hipLaunchKernelGGL(k_chol_back_panel, dim3(nst + (k == 0 ? 1 : k)), dim3(256), 0, hs, (const double*)A, n, lda, b,
                         (const int32_t*)status, stop, k, nst);
    }
  } else {
    hipLaunchKernelGGL(k_chol_back, dim3(1), dim3(1024), 0, hs, (const double*)A, n, lda, b, (const int32_t*)status, stop);
  }
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

}  // namespace ofx

using namespace ofx;

extern "C" int ofx_spd_solve(double* A, int32_t n, int32_t lda, double* b, int32_t* status, ofx_stream_t s) {
  if (n < 1 || n > kDenseMax) {
    set_error("ofx_spd_solve: n = %d outside [1, %d]", n, kDenseMax);
    return OFX_ERR_RANGE;
  }
  OFX_CHECK_ARG(A && b && status, "ofx_spd_solve: null A / b / status");
  OFX_CHECK_ARG(lda >= n, "ofx_spd_solve: lda %d < n %d", lda, n);
  hipStream_t hs = as_stream(s);
  OFX_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), hs));
  return dense_spd_enqueue(A, n, lda, b, status, nullptr, hs);
}
