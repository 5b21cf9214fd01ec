// Gauss-Newton solver, linearisation: the term records (k_terms) and the assembly of A = JᵀJ + λI and b = -Jᵀr from
// them (k_assemble), enqueued by gn_linearize for ofx_gn_linearize (gn.hip). Design: gn_internal.h.
#include "gn_device.h"

namespace ofx {

// ---------------------------------------------------------------------------- linearisation
struct DataCoef {
  double lf, ld, la, lm, fx, fy, cx, cy;
};

// Compact term records (kRec doubles per term at J + t·kRec; 160 B against the 576 B of four 3x6 blocks):
//   data  : [v_k w_k] for anchors k = 0..3 (v_k = w_k R_k(x - g_k)) at 4k, then [fx/z fy/z mfx mfy] at 16
//   ARAP  : [d0 d1 d2 s] at 0 (node i: d = R_i(g_j - g_i), s = la·w_e), node j's diagonal -s at 4
//   motion: the three diagonal entries at 0
// term_block() expands (record, slot) into the 3x6 block with the arithmetic the blocks were written with,
// operation for operation, so the assembled A and b are the same bits.
// (kRec = 20: gn_internal.h)

// Per-match weights and the robust kernel of the data rows (ofx_gn_set_robust), k_terms<true>'s own argument: mw the
// handle's copy of the weights (k_upload), c the Huber delta / Tukey c in metres, c2 = c² (Tukey's u = e² / c²)
struct RobustArg {
  const double* mw;
  double c, c2;
  int kernel;
};
// (k_terms' trailing argument pack holds exactly one RobustArg when kRobust, none otherwise)
__device__ __forceinline__ const RobustArg& only(const RobustArg& rb) { return rb; }

// The row scale of a match at geometric distance² e2 (metres²): mw · s_rob, with s_rob the square root of the IRLS weight
// ρ'(e)/e — Huber: 1 up to delta, sqrt(delta / e) beyond; Tukey: 1 - u below u = e²/c² = 1 (the root of the biweight
// (1 - u)², no sqrt), 0 from there on. A NaN distance gives NaN (Huber) or a zero scale on a NaN residual (Tukey): either
// way the term's loss partial is not finite and the solve is flagged.
__device__ __forceinline__ double robust_scale(const RobustArg& rb, double mw, double e2) {
  double s = 1.0;
  if (rb.kernel == OFX_ROBUST_TUKEY) {
    const double u = e2 / rb.c2;
    s = u < 1.0 ? 1.0 - u : 0.0;
  } else if (rb.kernel == OFX_ROBUST_HUBER) {
    const double e = sqrt(e2);
    s = e <= rb.c ? 1.0 : sqrt(rb.c / e);
  }
  return mw * s;
}

// slot k of data term m: its anchor's [v w]; slot 0 also the term's shared scalars. kRobust: w is w_k · s, the match's row
// scale (the blocks are linear in w_k: term_block then gives s times the unscaled rows; the tail scalars are not scaled)
template <bool kRobust>
__device__ __forceinline__ void data_record(const GnDev& g, const DataCoef& dc, int64_t m, int k, const double p[3],
                                            double zinv, double* __restrict__ rec, double s) {
  int a = g.anc[m * 4 + k];
  double w = g.wts[m * 4 + k];
  if (kRobust) w = w * s;
  const double* R = g.R + 9 * (int64_t)a;
  const double* gn = g.nodes + 3 * (int64_t)a;
  double d0 = g.src[3 * m] - gn[0], d1 = g.src[3 * m + 1] - gn[1], d2 = g.src[3 * m + 2] - gn[2];
  double2* o = reinterpret_cast<double2*>(rec + 4 * k);
  o[0] = make_double2(w * (R[0] * d0 + R[1] * d1 + R[2] * d2), w * (R[3] * d0 + R[4] * d1 + R[5] * d2));
  o[1] = make_double2(w * (R[6] * d0 + R[7] * d1 + R[8] * d2), w);
  if (k == 0) {
    double2* tl = reinterpret_cast<double2*>(rec + 16);
    tl[0] = make_double2(dc.fx * zinv, dc.fy * zinv);
    tl[1] = make_double2(-(dc.fx * p[0] * zinv) * zinv, -(dc.fy * p[1] * zinv) * zinv);
  }
}

enum TermKind { kData = 0, kEdge = 1, kMotion = 2 };
__device__ __forceinline__ int term_kind(const GnDev& g, int64_t t) {
  return t < g.M ? kData : (t < g.M + (int64_t)g.N * g.NB ? kEdge : kMotion);
}

// the 3x6 block of `slot` from the record's words x = rec[4·slot .. +3] and (data) tail = rec[16 .. 19]
__device__ __forceinline__ void term_block(int kind, int slot, const double x[4], const double tail[4],
                                           const DataCoef& dc, double J[18]) {
#pragma unroll
  for (int c = 0; c < 18; ++c) J[c] = 0.0;
  if (kind == kData) {
    const double v0 = x[0], v1 = x[1], v2 = x[2], w = x[3];
    const double fxdz = tail[0], fydz = tail[1], mfx = tail[2], mfy = tail[3];
    // S = -[v]x
    const double S[9] = {0.0, v2, -v1, -v2, 0.0, v0, v1, -v0, 0.0};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      J[0 + j] = dc.lf * fxdz * S[0 + j] + mfx * S[6 + j] + dc.ld * S[0 + j];
      J[6 + j] = dc.lf * fydz * S[3 + j] + mfy * S[6 + j] + dc.ld * S[3 + j];
      J[12 + j] = dc.ld * S[6 + j];
    }
    J[3] = dc.lf * w * fxdz + dc.ld * w; J[5] = dc.lf * w * mfx;
    J[10] = dc.lf * w * fydz + dc.ld * w; J[11] = dc.lf * w * mfy;
    J[17] = dc.ld * w;
  } else if (kind == kEdge && slot == 0) {   // node i: [-s[d]x | s I]
    const double d0 = x[0], d1 = x[1], d2 = x[2], s = x[3];
    J[1] = s * d2; J[2] = -s * d1; J[3] = s;
    J[6] = -s * d2; J[8] = s * d0; J[10] = s;
    J[12] = s * d1; J[13] = -s * d0; J[17] = s;
  } else if (kind == kEdge) {                 // node j: [0 | -s I]
    J[3] = x[0]; J[10] = x[0]; J[17] = x[0];
  } else {
    J[3] = x[0]; J[10] = x[1]; J[17] = x[2];
  }
}

// the record words of (t, slot): two 16-B loads, plus the two of a data term's tail — loaded for every kind (every
// record has them) and zeroed for the others: a load in a kind branch was waited for inside it, one term after another
__device__ __forceinline__ void load_record(const GnDev& g, int64_t t, int slot, int kind, double x[4], double tail[4]) {
  const double2* r = reinterpret_cast<const double2*>(g.J + t * kRec);
  const double2 a = r[2 * slot], b = r[2 * slot + 1];
  const double2 c = r[8], d = r[9];
  x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
  const bool dt = kind == kData;
  tail[0] = dt ? c.x : 0.0; tail[1] = dt ? c.y : 0.0; tail[2] = dt ? d.x : 0.0; tail[3] = dt ? d.y : 0.0;
}

// Anchor k's summand of the deformed point of match m: w_k (R_k (x - g_k) + g_k + t_k) (ED_warp, geometry.py:9-25)
__device__ __forceinline__ void anchor_term(const GnDev& g, int64_t m, int k, double c[3]) {
  int a = g.anc[m * 4 + k];
  double w = g.wts[m * 4 + k];
  const double* R = g.R + 9 * (int64_t)a;
  const double* gn = g.nodes + 3 * (int64_t)a;
  const double* tt = g.t + 3 * (int64_t)a;
  double d0 = g.src[3 * m] - gn[0], d1 = g.src[3 * m + 1] - gn[1], d2 = g.src[3 * m + 2] - gn[2];
  c[0] = w * ((R[0] * d0 + R[1] * d1 + R[2] * d2) + gn[0] + tt[0]);
  c[1] = w * ((R[3] * d0 + R[4] * d1 + R[5] * d2) + gn[1] + tt[1]);
  c[2] = w * ((R[6] * d0 + R[7] * d1 + R[8] * d2) + gn[2] + tt[2]);
}

// Four threads per term (t = id/4, slot k = id%4): slot k writes its node's words of the term record
// (kRec above); slot 0 also writes the residual triple and the loss partials. Terms outside this rank's
// share (data matches outside [m0,m1), regularisers when !add_reg) get all-zero records (exact zero
// blocks) so the fixed contribution lists stay valid.
// kRobust = false is the kernel without ofx_gn_set_robust (Rb empty: its arguments and code are what they were);
// kRobust = true takes one RobustArg more and scales each data term in [m0, m1) by s = mw[t] · s_rob(|p - tgt|),
// recomputed per linearisation (IRLS): w_k -> w_k · s in the record, r -> r · s, the loss partial from the scaled r.
// s = 0 zeroes every [v w] word of the record: exact zero blocks, which the contribution lists tolerate as they do a
// foreign match's.
template <bool kRobust, typename... Rb>
__global__ __launch_bounds__(kBlk) void k_terms(GnDev g, DataCoef dc, int m0, int m1, int add_reg, Rb... rb) {
  // every kernel-argument field in SGPRs up front, in one scalar trip (left to the compiler, each branch loaded its own
  // fields after the branch: four dependent scalar trips ahead of the first vector load)
  asm volatile("" :: "s"(g.J), "s"(g.anc), "s"(g.wts), "s"(g.R), "s"(g.nodes), "s"(g.src), "s"(g.t), "s"(g.tgt),
               "s"(g.tpx), "s"(g.tpy), "s"(g.edges), "s"(g.ew), "s"(g.res), "s"(g.T), "s"(g.M), "s"(g.N), "s"(g.NB),
               "s"(g.conf), "s"(g.tpos), "s"(g.prm.mode), "s"(g.part_loss), "s"(m0), "s"(m1), "s"(add_reg));
  asm volatile("" :: "s"(dc.lf), "s"(dc.ld), "s"(dc.la), "s"(dc.lm), "s"(dc.fx), "s"(dc.fy), "s"(dc.cx), "s"(dc.cy));
  if constexpr (kRobust)
    asm volatile("" :: "s"(only(rb...).mw), "s"(only(rb...).c), "s"(only(rb...).c2), "s"(only(rb...).kernel));
  const int64_t id = blockIdx.x * (int64_t)kBlk + threadIdx.x;
  const int64_t t = id >> 2;
  const int k = (int)(id & 3);
  double r[3] = {0.0, 0.0, 0.0};
  double l2[3] = {0.0, 0.0, 0.0};
  double bad = 0.0;
  if (t < g.T) {
    double* rec = g.J + t * kRec;
    if (t < g.M) {
      if (t >= m0 && t < m1) {
        // deformed point: slot k computes its anchor's summand, the four slots (adjacent lanes of one wave, all
        // in this branch together) exchange them and every slot adds them to 0 in the anchor order k = 0..3
        // (the oracle's sequence; each slot used to recompute all four summands itself: 13.2 -> 11.8 us)
        // the residual's target values are loaded by every slot up front (no trip behind the k == 0 branch)
        const double tpx = g.tpx[t], tpy = g.tpy[t];
        const double tg0 = g.tgt[3 * t], tg1 = g.tgt[3 * t + 1], tg2 = g.tgt[3 * t + 2];
        double mwt = 1.0;   // (kRobust) the match's weight, by every slot with the targets: each slot scales its own words
        if constexpr (kRobust) mwt = only(rb...).mw[t];
        double c[3];
        anchor_term(g, t, k, c);
        const int base = (int)(threadIdx.x & 63) & ~3;
        double p[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int d = 0; d < 3; ++d) p[d] += __shfl(c[d], base + kk, 64);
        double zinv = 1.0 / (p[2] + 1e-7);
        double s = 1.0;
        if constexpr (kRobust) {
          const double e0 = p[0] - tg0, e1 = p[1] - tg1, e2 = p[2] - tg2;
          s = robust_scale(only(rb...), mwt, e0 * e0 + e1 * e1 + e2 * e2);
        }
        data_record<kRobust>(g, dc, t, k, p, zinv, rec, s);
        if (k == 0) {
          r[0] = dc.lf * (dc.fx * p[0] * zinv + dc.cx - tpx) + dc.ld * (p[0] - tg0);
          r[1] = dc.lf * (dc.fy * p[1] * zinv + dc.cy - tpy) + dc.ld * (p[1] - tg1);
          r[2] = dc.ld * (p[2] - tg2);
          if constexpr (kRobust) { r[0] *= s; r[1] *= s; r[2] *= s; }
          l2[0] = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        }
      } else {
        double2* o = reinterpret_cast<double2*>(rec + 4 * k);
        o[0] = o[1] = make_double2(0.0, 0.0);
        if (k == 0) reinterpret_cast<double2*>(rec + 16)[0] = reinterpret_cast<double2*>(rec + 16)[1] = make_double2(0.0, 0.0);
      }
    } else if (t < g.M + (int64_t)g.N * g.NB) {
      const int64_t e = t - g.M;
      const int j = g.edges[e];
      // the edge's weight and node i's R, g, t leave with the edge's j (none depends on j; behind the j >= 0 test the
      // weight was a trip of its own, then i's and j's records another)
      const int i = (int)(e / g.NB);
      const double ewv = g.ew[e];
      double Ri[9], gi[3], ti[3];
#pragma unroll
      for (int q = 0; q < 9; ++q) Ri[q] = g.R[9 * (int64_t)i + q];
#pragma unroll
      for (int q = 0; q < 3; ++q) { gi[q] = g.nodes[3 * (int64_t)i + q]; ti[q] = g.t[3 * (int64_t)i + q]; }
      asm volatile("" ::: "memory");
      if (j >= 0 && k < 2) {
        if (add_reg) {
          const double s = dc.la * ewv;
          if (k == 0) {
            const double* gj = g.nodes + 3 * (int64_t)j;
            const double* tj = g.t + 3 * (int64_t)j;
            double e0 = gj[0] - gi[0], e1 = gj[1] - gi[1], e2 = gj[2] - gi[2];
            double d0 = Ri[0] * e0 + Ri[1] * e1 + Ri[2] * e2;
            double d1 = Ri[3] * e0 + Ri[4] * e1 + Ri[5] * e2;
            double d2 = Ri[6] * e0 + Ri[7] * e1 + Ri[8] * e2;
            r[0] = s * (d0 + gi[0] + ti[0] - (gj[0] + tj[0]));
            r[1] = s * (d1 + gi[1] + ti[1] - (gj[1] + tj[1]));
            r[2] = s * (d2 + gi[2] + ti[2] - (gj[2] + tj[2]));
            double2* o = reinterpret_cast<double2*>(rec);   // node i's [d s]
            o[0] = make_double2(d0, d1);
            o[1] = make_double2(d2, s);
            l2[1] = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
          } else {  // node j's diagonal
            rec[4] = -s;
          }
        } else if (k == 0) {
          reinterpret_cast<double2*>(rec)[0] = reinterpret_cast<double2*>(rec)[1] = make_double2(0.0, 0.0);
          rec[4] = 0.0;
        }
      }
    } else if (k == 0) {
      const int i = (int)(t - g.M - (int64_t)g.N * g.NB);
      double J3 = 0.0, J10 = 0.0, J17 = 0.0;
      if (add_reg && g.prm.mode == OFX_GN_ARAP) {
        // DeformNet.arap "flow" rows of the valid nodes (model.py:1766-1784): the Jacobian entry on
        // t_c is the residual itself, as the reference writes it
        const double c = dc.lf * g.conf[i];
        for (int q = 0; q < 3; ++q) r[q] = c * (g.t[3 * i + q] + g.nodes[3 * i + q] - g.tpos[3 * i + q]);
        J3 = r[0]; J10 = r[1]; J17 = r[2];
        l2[0] = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
      } else if (add_reg) {
        double c = dc.lm * g.conf[i];
        for (int q = 0; q < 3; ++q) r[q] = c * (g.t[3 * i + q] + g.nodes[3 * i + q] - g.tpos[3 * i + q]);
        J3 = c; J10 = c; J17 = c;
        l2[2] = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
      }
      rec[0] = J3; rec[1] = J10; rec[2] = J17;
    }
    if (k == 0) {
      g.res[3 * t] = r[0]; g.res[3 * t + 1] = r[1]; g.res[3 * t + 2] = r[2];
      bad = (isfinite(l2[0]) && isfinite(l2[1]) && isfinite(l2[2])) ? 0.0 : 1.0;
    }
  }
  double sv[4] = {l2[0], l2[1], l2[2], bad};
  block_sum4(sv);
  if (threadIdx.x == 0) {
    double* P = g.part_loss + 4 * (int64_t)blockIdx.x;
    P[0] = sv[0]; P[1] = sv[1]; P[2] = sv[2]; P[3] = sv[3];
  }
}

// b = -Jᵀr: one wave per node, entry-parallel (below). WG 0 also reduces the loss partials into the
// rhs tail.
__device__ __forceinline__ void rhs_body(const GnDev& g, const DataCoef& dc, double* __restrict__ rhs, int wg) {
  if (wg == 0 && threadIdx.x < 64) {   // the loss partials of k_terms, 4 streams in one pass, fixed order
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < g.nwg_terms; i += 64) {
      const double4 t = *reinterpret_cast<const double4*>(g.part_loss + 4 * (int64_t)i);
      a[0] += t.x; a[1] += t.y; a[2] += t.z; a[3] += t.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      for (int o = 32; o > 0; o >>= 1) a[k] += __shfl_xor(a[k], o, 64);
    if (threadIdx.x == 0) {
      double* tail = rhs + 6 * (int64_t)g.N;
      tail[0] = a[0]; tail[1] = a[1]; tail[2] = a[2]; tail[3] = a[3];
    }
  }
  const int n = wg * (kBlk / 64) + (threadIdx.x >> 6);
  if (n >= g.N) return;
  const int lane = threadIdx.x & 63;
  // one wave per node, one list entry per lane (two per lane per pass: a busy node's ~90 terms in one
  // pass of two dependent trips — code, then J + r — where 10 slots took ~10 serial passes); every load
  // unconditional (clamped index, masked value) so no branch splits a trip; fixed-order wave sums
  const int b = g.node_off[n], e = g.node_off[n + 1];
  int code[2];   // the first pass's codes come with the bounds (node_first), later passes' from the list
#pragma unroll
  for (int j = 0; j < 2; ++j) code[j] = g.node_first[(int64_t)n * 128 + lane + 64 * j];
  asm volatile("" ::: "memory");   // (issued with the bounds, not sunk into the loop behind its entry test)
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k0 = b; k0 < e; k0 += 128) {
    bool ok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + lane + 64 * j;
      ok[j] = k < e;
      if (k0 != b) code[j] = g.node_list[ok[j] ? k : e - 1];
    }
    // both entries' records and residuals first (one trip), then the blocks (left in the loop, the second entry's loads
    // issued after the first entry's kind branches: two trips)
    int kind[2];
    double x[2][4], tail[2][4], rv[2][3];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t t = code[j] >> 2;
      kind[j] = term_kind(g, t);
      load_record(g, t, code[j] & 3, kind[j], x[j], tail[j]);
      const double* rr = g.res + 3 * t;
      rv[j][0] = rr[0]; rv[j][1] = rr[1]; rv[j][2] = rr[2];
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      double P[18];
      term_block(kind[j], code[j] & 3, x[j], tail[j], dc, P);
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double t3 = P[c] * rv[j][0] + P[6 + c] * rv[j][1] + P[12 + c] * rv[j][2];
        v[c] += ok[j] ? t3 : 0.0;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) v[c] = wave_sum(v[c]);
  if (lane == 0)
#pragma unroll
    for (int c = 0; c < 6; ++c) rhs[6 * (int64_t)n + c] = -v[c];
}

// JᵀJ blocks, workgroup-cooperative: the workgroup's 16 blocks own one contiguous range of the sorted
// contribution list. Chunks of kCoop entries: one thread per entry loads its two Jacobian blocks (the next
// chunk's codes one chunk ahead) and writes the full 6×6 product to LDS ([output][entry], padded: conflict-
// free writes); then each (block, output) pair — 576 per workgroup, up to 3 per thread — adds its entries of
// the chunk in list order. A block's cost is its share of the workgroup's entries, not its own list length
// (the 16-lane form took ceil(len/16) dependent trips: ~6 for a busy node's diagonal block).
// (kCoop = OFX_KCOOP, tuning builds -DOFX_KCOOP=n: gn_internal.h)
__device__ __forceinline__ void blocks_coop(const GnDev& g, const DataCoef& dc, double* __restrict__ A, int64_t wg,
                                            double lm) {
  __shared__ double s_prod[36 * (kCoop + 1)];
  __shared__ int s_off[17];
  const int tid = threadIdx.x;
  const int64_t sb = wg * (kBlk / 16);   // upper blocks u in [sb, sb + 16); past the upper count up_slot is -1 and
                                         // the lists are empty (blk_off there = the total)
  constexpr int kPairs = (kBlk / 16) * 36;
  constexpr int kU = (kPairs + kBlk - 1) / kBlk;
  // first trip: the 17 list offsets and every pair's output slots (consumed at the end, in flight all along)
  // (every load unconditional, the list offsets first: a load inside the offsets' branch was waited for there, before
  // the other loads issued)
  const int offv = g.blk_off[min<int64_t>(sb + min(tid, kBlk / 16), g.nnzb)];
  int code_next = g.blk_first[wg * kCoop + min(tid, kCoop - 1)];   // the first chunk's codes (k_first_codes)
  int pb[kU], po[kU], os[kU], ot[kU];
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int p = tid + kBlk * u;
    pb[u] = p < kPairs ? p / 36 : kBlk / 16 - 1; po[u] = p % 36;
    os[u] = g.up_slot[sb + pb[u]];
    ot[u] = g.up_tr[sb + pb[u]];
  }
  if (tid <= kBlk / 16) s_off[tid] = offv;
  __syncthreads();
  const int E0 = s_off[0], E1 = s_off[kBlk / 16];
  if (E0 == E1) return;   // no upper block here (uniform over the workgroup)
  double acc[kU];
  int lo[kU], hi[kU];
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const bool ok = tid + kBlk * u < kPairs;
    lo[u] = ok ? s_off[pb[u]] : 0;
    hi[u] = ok ? s_off[pb[u] + 1] : 0;
    acc[u] = 0.0;
  }
  for (int c0 = E0; c0 < E1; c0 += kCoop) {
    if (tid < kCoop) {
      const int k = c0 + tid;
      const int code = code_next;
      code_next = k + kCoop < E1 ? g.blk_list[k + kCoop] : 0;
      if (k < E1) {
        const int64_t t = code >> 4;
        const int kind = term_kind(g, t), sp = (code >> 2) & 3, sq = code & 3;
        double xp[4], xq[4], tail[4], P[18], Q[18];
        load_record(g, t, sp, kind, xp, tail);
        const double2* r = reinterpret_cast<const double2*>(g.J + t * kRec + 4 * sq);
        const double2 a = r[0], b = r[1];
        xq[0] = a.x; xq[1] = a.y; xq[2] = b.x; xq[3] = b.y;
        term_block(kind, sp, xp, tail, dc, P);
        term_block(kind, sq, xq, tail, dc, Q);
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
          for (int j = 0; j < 6; ++j)
            s_prod[(6 * c + j) * (kCoop + 1) + tid] = P[c] * Q[j] + P[6 + c] * Q[6 + j] + P[12 + c] * Q[12 + j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int a = max(lo[u], c0), b = min(hi[u], c0 + kCoop);
      const double* sp = s_prod + po[u] * (kCoop + 1) - c0;
      double x = acc[u];
      // eight LDS reads in flight, then the eight adds in list order (a one-read-per-add loop waited out the LDS
      // latency per entry: a busy diagonal block's outputs cost ~90 serial round trips per chunk)
      int e = a;
      for (; e + 8 <= b; e += 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = sp[e + k];
#pragma unroll
        for (int k = 0; k < 8; ++k) x += v[k];
      }
      if (e + 4 <= b) {
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = sp[e + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) x += v[k];
        e += 4;
      }
      for (; e < b; ++e) x += sp[e];
      acc[u] = x;
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int p = tid + kBlk * u;
    if (p >= kPairs || os[u] < 0) continue;
    const int64_t s = os[u], st = ot[u];
    double v = acc[u];
    // LM damping of the diagonal blocks (model.py:641-662)
    if (lm != 0.0 && po[u] % 7 == 0 && s == st) v += lm;
    A[36 * s + po[u]] = v;
    if (st != s) A[36 * st + 6 * (po[u] % 6) + po[u] / 6] = v;   // the lower block: the transpose
  }
}

// JᵀJ blocks and -Jᵀr in one launch: the rhs workgroups first (their per-node loops are the longest
// chains), then nwb workgroups of blocks.
__global__ __launch_bounds__(kBlk) __attribute__((amdgpu_waves_per_eu(4))) void k_assemble(GnDev g, DataCoef dc, double* __restrict__ A, double* __restrict__ rhs,
                                                  int nrw, double lm) {
  // the kernel-argument fields in SGPRs up front (one scalar trip, see k_terms; nrw, the rhs workgroup count, is an
  // argument rather than gridDim.x - nwb: the grid size is one more scalar load)
  asm volatile("" :: "s"(g.N), "s"(g.M), "s"(g.NB), "s"(g.node_list), "s"(g.node_off), "s"(g.nwg_terms),
               "s"(g.part_loss), "s"(g.res), "s"(g.J), "s"(g.blk_list), "s"(g.blk_off), "s"(g.nnzb), "s"(g.up_slot),
               "s"(g.up_tr), "s"(A), "s"(rhs), "s"(nrw), "s"(lm));
  asm volatile("" :: "s"(dc.lf), "s"(dc.ld), "s"(dc.la), "s"(dc.lm), "s"(dc.fx), "s"(dc.fy), "s"(dc.cx), "s"(dc.cy));
  // XCD-aware order: workgroups b and b + 8 share an XCD, so each XCD takes a contiguous run of nodes / upper
  // blocks and the term records they share stay in one L2 (nrw is a multiple of 8, so both halves keep b % 8); a
  // relabelling of which workgroup computes what: A and b are unchanged. Fetch 20.2 -> 7.9 MB per launch, time
  // unchanged (the re-reads were served by the MALL): profiles/r05_ab.json
  const int hw = blockIdx.x, part = hw < nrw ? nrw : (int)gridDim.x - nrw, i = hw < nrw ? hw : hw - nrw;
  const int q = part >> 3, r = part & 7, x = i & 7;
  const int L = x * q + min(x, r) + (i >> 3);
  if (hw < nrw) rhs_body(g, dc, rhs, L);
  else blocks_coop(g, dc, A, L, lm);
}
#ifdef OFX_SPLIT_ASSEMBLE
__global__ __launch_bounds__(kBlk) void k_assemble_blocks(GnDev g, DataCoef dc, double* __restrict__ A, double lm) {
  blocks_coop(g, dc, A, blockIdx.x, lm);
}
__global__ __launch_bounds__(kBlk) void k_assemble_rhs(GnDev g, DataCoef dc, double* __restrict__ rhs) {
  rhs_body(g, dc, rhs, blockIdx.x);
}
#endif

int gn_linearize(Gn* g, int gn_iter, int m0, int m1, int add_reg, double* A, double* rhs, hipStream_t hs) {
  DataCoef dc;
  dc.lf = sqrt(g->prm.lambda_flow); dc.ld = sqrt(g->prm.lambda_depth);
  dc.la = sqrt(g->prm.lambda_arap); dc.lm = sqrt(g->prm.lambda_motion);
  dc.fx = g->fx; dc.fy = g->fy; dc.cx = g->cx; dc.cy = g->cy;
  const ofx_gn_robust& rs = g->rob_setup;   // the setting the setup was made under (its weights are in g->mw)
  if (robust_on(rs) && g->prm.mode == OFX_GN_OPTIMIZE) {
    RobustArg rb;
    rb.mw = g->mw;
    rb.kernel = rs.kernel;
    rb.c = rs.kernel != OFX_ROBUST_NONE ? rs.scale : 1.0;
    rb.c2 = rb.c * rb.c;
    hipLaunchKernelGGL((k_terms<true, RobustArg>), dim3(g->nwg_terms), dim3(kBlk), 0, hs, *g, dc, m0, m1, add_reg, rb);
  } else {
    hipLaunchKernelGGL((k_terms<false>), dim3(g->nwg_terms), dim3(kBlk), 0, hs, *g, dc, m0, m1, add_reg);
  }
#ifdef OFX_STAMPS
  if (gn_iter > 0 && g->t_seen.time_since_epoch().count()) {
    g->react_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - g->t_seen).count();
    ++g->react_n;
  }
#endif
  // the LM damping λ_k I (model.py:418-419,641-662) is added by the rank that adds the regularisers, so a
  // sum over ranks carries it once
  const double lm = add_reg ? lm_for_iter(g->prm.lm_factor, gn_iter) : 0.0;
  // upper blocks: (nnzb + diagonal blocks) / 2 <= (nnzb + rows) / 2 (the pattern is symmetric); workgroups past
  // the device-side count return at once
  const int nwb = g->nnzb > 0 ? (int)grid_for((g->nnzb + g->N) / 2 + 1, kBlk / 16, 1 << 30) : 0;
#ifdef OFX_SPLIT_ASSEMBLE   // tuning build: the two halves as separate kernels (rocprof times each)
  if (nwb) hipLaunchKernelGGL(k_assemble_blocks, dim3(nwb), dim3(kBlk), 0, hs, *g, dc, A, lm);
  hipLaunchKernelGGL(k_assemble_rhs, dim3(grid_for(g->N, kBlk / 64)), dim3(kBlk), 0, hs, *g, dc, rhs);
#else
  const int nrw = ((int)grid_for(g->N, kBlk / 64) + 7) & ~7;   // (a multiple of 8: see k_assemble)
  hipLaunchKernelGGL(k_assemble, dim3(nwb + nrw), dim3(kBlk), 0, hs, *g, dc, A, rhs, nrw, lm);
#endif
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

}  // namespace ofx
