// Gauss-Newton non-rigid registration solver: block-sparse JᵀJ / Jᵀr assembly + block-Jacobi PCG.
//
// Restates DeformNet.optimize (model/model.py:222-859) for one batch item:
//   unknowns per node i: [ω_i (3) | t_i (3)]  (reference orders all rotations, then all translations;
//                                              the dense oracle maps between the two orders)
//   data rows (3 per match, model.py:416-545): p = Σ_k w_k (R_k(x-g_k)+g_k+t_k)
//       r  = [lf(fx·px/z+cx-tpx) + ld(px-tx), lf(fy·py/z+cy-tpy) + ld(py-ty), ld(pz-tz)]
//       ∂/∂t_k = w_k·[[lf·fx/z+ld, 0, lf·(-fx·px/z²)], [0, lf·fy/z+ld, lf·(-fy·py/z²)], [0,0,ld]]
//       ∂/∂ω_k = S + [[-fx·px/z²·S₂ ], [-fy·py/z²·S₂], [0]] + lf·[[fx/z·S₀],[fy/z·S₁],[0]],  S = -[w_k R_k(x-g_k)]×
//       (the un-weighted -f·p/z² terms reproduce the operator-precedence quirk at model.py:505-510)
//   ARAP rows (3 per directed edge, model.py:554-601): r = la·w(R_i(g_j-g_i)+g_i+t_i-g_j-t_j)
//   motion rows (3 per node, model.py:604-612):       r = lm·c_i(t_i+g_i-target_i)
//   A = JᵀJ + λ_LM·I, b = -Jᵀr, λ_LM halved at gn_i ≡ 2 mod 3 (model.py:418-419, 641-662)
//   x = A⁻¹b (reference: dense LU, model.py:59-86,694-709 -> here: f64 block-Jacobi PCG)
//   early stop on loss increase > stop_diff or unchanged loss (model.py:726-732), then
//   R ← exp([x_ω]) R (kornia 0.7 angle_axis_to_rotation_matrix), t += x_t (model.py:744-748).
//
// MI355X design.
//  * Every residual row-triple is a "term" (data: 4 anchored nodes, ARAP edge: 2, motion: 1). Once per GN
//    iteration k_terms writes each term's compact record (kRec doubles: the per-anchor vectors and the
//    term's shared scalars, not its four 3x6 Jacobian blocks); the assembly expands a record into the
//    blocks it needs with the same arithmetic, so A and b are the bits the blocks themselves gave.
//  * JᵀJ lives as 6x6 f64 blocks in BSR over the node adjacency (diagonal, edges, co-anchored
//    pairs). Per solve, each block gets a sorted list of the (term, p, q) products that land on it,
//    so assembly is a deterministic gather: one wave per block, lane = block entry (k_blocks); the
//    rhs is the same per node entry (k_rhs). No atomics -> bitwise reproducible A and b.
//  * Node order: setup groups the nodes into clusters of <= kCS graph neighbours (host BFS over the
//    ED graph, first-fit packed into groups of exactly kCS rows, padded with decoupled dummy nodes),
//    and permutes every node-indexed array into that order; k_finish permutes the result back.
//  * PCG: pipelined (Ghysels-Vanroose) with a cluster block-Jacobi preconditioner (explicit inverse
//    of each damped 48x48 cluster diagonal block), ONE kernel per iteration: SpMV + all recurrences
//    + the cluster M⁻¹ (wave-local: one cluster = one wave's rows) + the three dot products. Scalars
//    never leave the device: each launch writes per-wave partial sums and every wave of the NEXT
//    launch re-derives the same scalars from them in a fixed order (kernel boundaries give
//    visibility; no fences, no tickets, no atomics). The host only polls convergence in chunks
//    sized from the previous frame's count for the same GN step.
//
// This header: what the solver's translation units share — the constants, the handle (GnDev / Gn), the as_tab layout,
// the flag, scalar and host-flag enums with host_flag, the scalar block's offsets, the iteration's argument structs
// and the host functions that cross files. gn_device.h: shared device helpers. gn_linearize.hip: term records and
// assembly. gn.hip: setup, PCG, Schwarz, the GN step, the prefetch worker and the C ABI.
#pragma once

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <array>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <utility>
#include <cstdlib>
#include <cstdio>
#include <vector>

#include "ofx_common.h"

namespace ofx {

// --------------------------------------------------------------------------------------------
constexpr int kBlk = 256;       // threads per WG
#ifndef OFX_KPROJ   // (tuning builds: -DOFX_KPROJ=<n>)
#define OFX_KPROJ 4
#endif
constexpr int kProj = OFX_KPROJ;   // warm start: Galerkin projection on the last kProj GN-step solutions
constexpr int kProjP = kProj * (kProj + 1) / 2 + kProj;   // projection partial streams (Gram upper triangle + Xᵀb)
constexpr int kCS = 8;        // nodes per preconditioner cluster (= PCG rows per wave)
constexpr int kMaxNodes = 8192;   // dense slot map of (2·max_nodes + kCS)² entries
constexpr int kDirectMaxNodes = 512;   // OFX_PRECOND_DIRECT: 3072 unknowns, a 75 MB dense f64 buffer (ofx_spd_solve's limit)
// Overlapping additive Schwarz (as_on): the ring of a cluster holds its kAsRing A-neighbours with the most coupling terms,
// and a row joins at most kAsX rings, so an output cluster has at most kAsSrc contributing subdomains and kAsRS row
// segments (a kAsD-entry inverse row each); kAsGat >= kAsSrc·kAsDN rounded up to whole passes of the apply's 192
#ifndef OFX_AS_RING   // (tuning builds: -DOFX_AS_RING=<n>; 12 -> 16: 198 -> 158 PCG iterations per bench frame, +10 %)
#define OFX_AS_RING 16
#endif
constexpr int kAsRing = OFX_AS_RING, kAsX = 3, kAsDN = kCS + kAsRing, kAsD = 6 * kAsDN, kAsK = kAsD / 8,
              kAsSrc = 1 + kCS * kAsX, kAsRS = 6 * kCS * (1 + kAsX),
              kAsGat = (kAsSrc * kAsDN + kAsRS - 1) / kAsRS * kAsRS, kAsMeta = 64 + kAsRS;
// One launch per Schwarz PCG iteration (k_as_iter, round 6): per subdomain a table of its rows' blocks (<= kAsDN rows of
// <= kRowMax blocks), the columns they touch (S2, <= kGS nodes) with the <= 1 + kAsX subdomain contributions that sum to m
// there, and the scaled inverse rows in subdomain order (the "tab" buffer, AsTab below)
constexpr int kGB = 512, kGS = 480, kGRow = 96;
constexpr int kAsIterT = 1024;   // k_as_iter's threads: blocks 0..511, S2 nodes from 512, the row waves 13..15
static_assert(kAsSrc * kAsDN <= kAsGat && kAsD % 8 == 0 && kAsD <= 144, "Schwarz tables");

// Everything the kernels read: trivially copyable, passed by value as the kernel argument (host-only
// members live in Gn below, so a launch copies these bytes and nothing else).
struct GnDev {
  int max_nodes = 0, max_matches = 0;
  int N = 0, M = 0, NB = 0;    // N: PCG rows (nodes in cluster order, padded to whole clusters)
  int N_real = 0;              // caller's node count
  int max_pad = 0;             // capacity of the node-indexed arrays (2·max_nodes + kCS)
  int32_t *perm = nullptr;     // row -> caller node (-1: padding), N entries
  int32_t *iperm = nullptr;    // caller node -> row, N_real entries
  int64_t T = 0;        // terms = M + N*NB + N
  ofx_gn_params prm{};
  float fx = 0, fy = 0, cx = 0, cy = 0;
  // problem (f64 device copies)
  double *nodes = nullptr, *tpos = nullptr, *conf = nullptr, *src = nullptr, *wts = nullptr, *tgt = nullptr,
         *tpx = nullptr, *tpy = nullptr, *ew = nullptr;
  int32_t *anc = nullptr, *edges = nullptr;
  // terms
  int32_t* term_node = nullptr;  // T*4, -1 = unused entry
  double* J = nullptr;           // T·kRec term records (k_terms)
  double* res = nullptr;         // T*3
  int64_t T_cap = 0;
  // pattern + contribution lists
  int32_t *map = nullptr, *row_ptr = nullptr, *col = nullptr, *row_cnt = nullptr;   // row_cnt[N]: max row length
  int2* wl = nullptr;            // per PCG wave: its first kWL blocks' columns and packed row bounds (k_wave_list)
  double* Aw = nullptr;          // per PCG wave: its kWL blocks of the operator, [wave][18][kWL] 16-B words (k_pcg_w0)
  int max_deg = 0;               // longest block row of the pattern
  int max_wave = 0;              // most blocks of one PCG wave (kCS rows)
  int32_t* stopw = nullptr;      // per PCG wave and lane: the epoch of the last converged (or stopped) PCG solve
  int32_t ep = 0;                // epoch of the current PCG solve (one per GN step, increasing per handle)
  uint64_t* stamps = nullptr;    // tuning builds (-DOFX_STAMPS): per iteration < 64 and wave, 8 clock stamps
  int32_t* blk_row = nullptr;    // block -> row (clears the slot map's pattern at the next setup)
  float* d_gnodes = nullptr;      // device copy of the graph the row order was built for (optimistic check)
  int32_t* d_gedges = nullptr;
  int32_t* d_gdiff = nullptr;
  int64_t gcap_n = 0, gcap_e = 0;
  int pat_N = 0;                 // N and block count of the pattern currently set in `map`
  int64_t pat_nnzb = 0;
  int64_t ne_cap = 0;            // capacity of edges / ew
  // contribution lists of the UPPER blocks only (col >= row, indexed u = up_of[slot]): the assembly computes each
  // upper block once and also stores its transpose at up_tr[u], so A is exactly symmetric. (A separate gather of the
  // lower block (j, i) would sum the same products in the same order only when no node repeats within a term; with
  // a repeated anchor its last bits could differ from the transpose.)
  int32_t *blk_off = nullptr, *blk_cnt = nullptr, *blk_list = nullptr, *blk_tmp = nullptr;
  int32_t *up_of = nullptr, *up_slot = nullptr, *up_tr = nullptr;   // slot -> u (+ total at [nnzb]), u -> slot, transpose
  int32_t *node_off = nullptr, *node_cnt = nullptr, *node_list = nullptr, *node_tmp = nullptr;
  // the first chunk of every assembly workgroup's list (kCoop codes) and of every node's rhs list (128), at fixed
  // offsets (k_first_codes): k_assemble's first memory trip carries them
  int32_t *blk_first = nullptr, *node_first = nullptr;
  int64_t nnzb = 0, nnzb_cap = 0;
  // state
  double *R = nullptr, *t = nullptr;
  double* racc = nullptr;        // per row: Σ|ω| of the GN steps since its cluster inverse was built (precond_rot_tol)
  int32_t gn_iter_now = 0;       // GN step of the current PCG solve
  double *A_own = nullptr, *rhs_own = nullptr;
  float* Mcl = nullptr;           // cluster inverses, f32, per cluster 48x48 in the lane-interleaved order of mcl_idx
  const double* Aop = nullptr;    // PCG operator (the damped A of the current step)
  double *st = nullptr;          // PCG recurrence state, 6N records of 8 (see the PCG layout note)
  double *m0 = nullptr, *m1 = nullptr;   // double-buffered m = M⁻¹w (gathered by the SpMV)
  double *pcg_alpha = nullptr, *pcg_gamma = nullptr;   // [-, -, 1/x of parity 0, 1] (+ alpha: [4 + par] = thr)
  // pcg_alpha, pcg_gamma, scal, sturm and flags live in ONE allocation at fixed offsets (kSc*), so the PCG iteration
  // reaches all of them through one preloaded pointer argument (no kernel-argument fetch ahead of their loads)
  double* pcs = nullptr;
  double2* sturm = nullptr;       // error-based PCG stop (k_pcg_iter): 64 shifted LDLᵀ pivots + counts
  double *part_p = nullptr, *part_b = nullptr, *part_loss = nullptr;
  int32_t nwg_row = 0, nwg_node = 0, nwg_terms = 0;   // nwg_row: PCG row waves (= workgroups)
  int32_t nw_pad = 0;            // stride of the iteration partial streams: 128·pcg_ku, zero beyond nwg_row
  int32_t pcg_w2 = 1;            // two waves per cluster in k_pcg_iter (OFX_PCG_W1=1: one)
  int32_t pcg_ku = 3;            // partial pairs per lane and stream in k_pcg_iter (pcg_ku_for)
  // overlapping additive Schwarz preconditioner (as_on): subdomain D_c = cluster c's kCS rows + up to kAsRing
  // ring rows; the setup's tables (k_as_choose .. k_as_segments) and the prep's inverses (k_as_invert), applied by
  // k_as_apply between two PCG iteration launches
  int32_t as_on = 0;
  int32_t *as_cand = nullptr, *as_csc = nullptr, *as_acc = nullptr;   // [cluster][kAsRing]: ring candidates, terms, kept
  int32_t* as_dom = nullptr;     // [cluster][kAsDN]: the subdomain's rows (own rows first, -1 = none)
  int32_t* as_meta = nullptr;    // [cluster][kAsMeta]: segment count, source count, row offsets, segment -> source slot
  int32_t* as_gat = nullptr;     // [cluster][kAsGat]: rows gathered into the apply's LDS image (source slot · kAsDN + l)
  int32_t* as_dst = nullptr;     // [cluster][kAsD]: subdomain row -> (output cluster · kAsRS + segment)
  uint16_t* as_slab = nullptr;   // [cluster][kAsK][kAsRS] x 8 fp16: the segments' scaled inverse rows, segment-minor
  int32_t* as_src = nullptr;     // [cluster][kAsSrc]: the apply's source subdomains
  float* as_dsc = nullptr;       // [cluster][kAsD]: the subdomain inverse's scales d = √diag(Z) (k_as_invert)
  float* as_rsc = nullptr;       // [cluster][kAsRS]: the segment rows' scales
  double* as_w = nullptr;        // 6N: the vector the next apply reads (w of the iteration, r0, ...)
  // one launch per iteration (k_as_iter, as_one): the per-subdomain tables, ghost (w, z) of the ring rows, the parity's
  // contributions y_c = Z_c w[D_c] and the subdomain-ordered inverse rows, in ONE buffer (offsets: AsTab)
  int32_t as_one = 0, as_tab_cap = 0;
  char* as_tab = nullptr;
  int32_t *as_mem = nullptr, *as_memn = nullptr;   // per row: its subdomain memberships (c·kAsD + 6·l, <= 1 + kAsX)
  double* scal = nullptr;
  int32_t* flags = nullptr;
  // DeformNet.arap mode with lambda_flow = 0: rows of each multi-node connected graph component
  // (comp_off[c]..comp_off[c+1] in comp_rows), whose common translation is the exact null space
  int32_t *comp_rows = nullptr, *comp_off = nullptr;
  int n_comp = 0, comp_cap = 0;
  double* loss_log = nullptr;
  double* stat = nullptr;         // kMaxLog x [pcg iterations, |b|², loss] of the last solve
  double* step_state = nullptr;   // (kMaxLog+1) x [previous loss, accepted steps] before each GN step
  // Galerkin warm start over the last kProj GN-step solutions of this solve (ring of kProj x 6N each;
  // the previous frame's solutions were measured not to help its first steps):
  // xh = previous solutions, th = A·xh
  double *xh = nullptr, *th = nullptr;
  struct StepArgs* step_args = nullptr;   // device copy (fused GN step in the converging PCG launch)
  bool step_fused = false;                // this step's k_step work was done by the PCG
  int n_prev = 0;                 // valid entries of the ring for the current step
  int warm_now = 0;               // this step starts from the projected x0
  int32_t* host_flags = nullptr;  // pinned, mapped: [H_DONE, H_PCG_IT, H_STOPPED] written by the kernels
  int32_t* hflags = nullptr;      // its device address (system-scope stores: no copy kernel per poll)
  int32_t* setup_stat = nullptr;  // pinned, mapped: the setup's one host read [nnz, max row, max wave, abort, graph diff]
  int32_t* d_setup_stat = nullptr;
  hipEvent_t poll_ev = nullptr;   // recorded after each chunk of PCG launches
  double host_enqueue_us = 0.0;   // tuning build: host time spent enqueuing PCG iterations
  int64_t host_enqueued = 0;
  bool setup_done = false;
  // optional timing of the PCG iteration loop (hipEvents on the caller's stream)
  bool timing = false;
  int64_t n_iter_launches = 0;
};
static_assert(std::is_trivially_copyable<GnDev>::value, "kernel argument");

// The as_tab buffer (k_as_iter), for a capacity of cap clusters: region by region, [cluster][...] each (16-B aligned)
//   blk  [kGB]  int2  the subdomain rows' blocks in row order (CSR order within a row): (A slot, S2 index << 5 | row)
//   con  [kGS]  int4  per S2 node the y indices (c'·kAsD + 6·l') of the subdomains holding it, ascending, -1 after
//   s2n  [kGS]  int   S2 node -> row (the first iteration gathers m from the warm start's m0)
//   row  [kGRow] int  row starts [0, kAsDN], then nd at 25, nb at 26, ns at 27; S2 index of each subdomain row at 32 + l,
//                     its node (row) at 64 + l
//   dsc  [kAsD] f32   the inverse's scales d = √diag Z (k_as_invert)
//   gh   [kAsRing·6] double2  ghost (w, z) of the ring rows (the owners' recurrences, repeated bit for bit)
//   y    [2][cap][kAsD] f64  per parity the contributions y_c = D Ẑ D w[D_c]
//   slab [kAsK][kAsD] uint4  Ẑ's rows (8 fp16 per word, its 32-bit pairs in the order 0, 2, 1, 3: a lane pair of the
//                     contribution dot takes 8-B halves), word k of every row contiguous
struct AsTabP {
  int2* blk; int4* con; int32_t* s2n; int32_t* row; float* dsc; double2* gh; double* y; uint4* slab;
};
__host__ __device__ __forceinline__ AsTabP as_tab_at(char* base, int64_t cap) {
  AsTabP p;
  char* q = base;
  p.blk = reinterpret_cast<int2*>(q); q += cap * kGB * 8;
  p.con = reinterpret_cast<int4*>(q); q += cap * kGS * 16;
  p.s2n = reinterpret_cast<int32_t*>(q); q += cap * kGS * 4;
  p.row = reinterpret_cast<int32_t*>(q); q += cap * kGRow * 4;
  p.dsc = reinterpret_cast<float*>(q); q += cap * kAsD * 4;
  p.gh = reinterpret_cast<double2*>(q); q += cap * kAsRing * 6 * 16;
  p.y = reinterpret_cast<double*>(q); q += 2 * cap * kAsD * 8;
  p.slab = reinterpret_cast<uint4*>(q);
  return p;
}
static inline int64_t as_tab_bytes(int64_t cap) {
  return cap * ((int64_t)kGB * 8 + (int64_t)kGS * 16 + (int64_t)kGS * 4 + kGRow * 4 + kAsD * 4 + kAsRing * 6 * 16 +
                2 * kAsD * 8 + (int64_t)kAsK * kAsD * 16);
}

// The solver handle: the kernel-visible state plus host-only members.
struct Gn : GnDev {
  std::vector<float> h_nodes;          // host copy of the graph the current order was built from
  std::vector<int32_t> h_edges, h_perm;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;   // timing events of the PCG loops
  // converged PCG iteration count of the previous solve, per GN step (sizes the first chunk of launches);
  // shared by the solver slots of one frame loop (ofx_gn_share_history)
  struct PcgHist {                  // per GN step the converged counts of the last 4 solves (ring), newest at n % 4
    int c[64][4] = {};
    int n[64] = {};
  };
  std::shared_ptr<PcgHist> last_pcg = std::make_shared<PcgHist>();
  // prefetched setup (ofx_gn_prepare): the next problem's setup runs on a host thread, on the handle's own
  // stream, while the caller's stream still works on the current problem (of another handle)
  std::thread worker;               // persistent (created by the first prefetch): no per-frame thread start
  std::mutex mu;
  std::condition_variable cv;
  bool job = false, quit = false;   // guarded by mu: a prefetch is queued / running; shut down
  // guarded by mu: a queued prefetch waits for its trigger (ofx_gn_prepare_after) — another handle's solve
  // reaching a GN step, that solve returning, or a wait on this handle
  bool gate = false;
  Gn* pf_peer = nullptr;            // (trigger side) the handle whose gated prefetch this handle's next solve opens
  int pf_step = 0;                  // ... at the start of this GN step (or on return)
  Gn* pf_trigger = nullptr;         // (prefetch side) the handle holding this one as pf_peer
  int prep_dev = 0;
  int prep_status = 0;
  bool prepared = false;            // the setup of prep_pb / prep_prm is (being) enqueued on `side`
  ofx_gn_problem prep_pb{};
  ofx_gn_params prep_prm{};
  hipStream_t side = nullptr;
  hipEvent_t ev_in = nullptr, ev_prep = nullptr;   // caller's stream at prepare -> side; side's setup done
  // side-stream work of a prefetch that no caller stream has been ordered after yet: the worker returns before
  // its last kernels (row assignment, contribution lists, ...) have run, and they write this handle's buffers
  bool side_dirty = false;
  hipEvent_t ev_side = nullptr;
  int64_t pf_used = 0, pf_missed = 0;   // solves that used / discarded a prefetched setup
  // per-match weights and robust data rows (ofx_gn_set_robust): rob is the caller's sticky setting; rob_setup the one
  // the last (or the prefetched, in-flight) setup was made under, which k_terms<true> then runs with — its
  // match_weights pointer is compared, never read again; mw holds the weights k_upload copied (max_matches doubles,
  // all 1 without a pointer). Host-only: the kernels get mw through Upload / RobustArg, GnDev stays as it is.
  ofx_gn_robust rob{}, rob_setup{};
  double* mw = nullptr;
  int32_t ep_next = 1;
  int as_env = -1;                  // OFX_PRECOND override of params.precond (-1: none; 3: direct)
  // exact dense solve (OFX_PRECOND_DIRECT, OFX_GN_OPTIMIZE): the dense lower triangle (dn_n x dn_n, row-major) and b / x
  // of the 6·N_real unknowns in caller node order, allocated at the first setup that asks for it and kept
  int direct = 0;                   // the last setup's solver: 1 = dense Cholesky instead of the PCG
  int dn_n = 0, dn_cap = 0;
  double *dn_A = nullptr, *dn_b = nullptr;
  int32_t* dn_status = nullptr;     // ofx_spd_solve's status of the current GN step
  void (*idle_fn)(void*) = nullptr; // ofx_gn_set_idle_hook: host work run once at the next solve's first PCG wait
  void* idle_arg = nullptr;
  int as_lanes = 2;                 // k_as_apply's lanes per segment (OFX_AS_LANES)
  int as_cap = 0;                   // clusters the Schwarz tables are allocated for
  // the PCG iteration's constant launch arguments (struct PcgIt) in device memory, and the bytes last copied there
  void* d_pcgit = nullptr;
  alignas(16) unsigned char pcgit_last[512] = {};
  bool pcgit_valid = false;
#ifdef OFX_STAMPS   // tuning build: stream idle between a PCG chunk's last launch and the next GN step's first kernel
  std::chrono::steady_clock::time_point t_seen{};   // host saw the step's convergence
  double react_us = 0.0, prologue_us = 0.0;         // -> k_terms enqueued; -> the first PCG chunk launch enqueued
  int64_t react_n = 0;
  hipEvent_t gap_end = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> gap_ev;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> entry_ev;   // solve entry -> pose done (the prefetched setup's wait)
  double prep_wait_us = 0.0;
#endif
};

// a setting that changes the data rows (else k_terms<false>, the solver as it is without ofx_gn_set_robust)
inline bool robust_on(const ofx_gn_robust& r) { return r.match_weights != nullptr || r.kernel != OFX_ROBUST_NONE; }

// Order stream hs after everything the prefetch worker enqueued on the handle's side stream (call after
// prep_wait: the worker has finished enqueuing). Every entry point that touches the handle's buffers on a
// caller stream does this first, whether or not the prefetched setup is used.
inline int fence_side(Gn* g, hipStream_t hs) {
  if (!g->side || !g->side_dirty) return OFX_OK;
  OFX_HIP(hipEventRecord(g->ev_side, g->side));
  OFX_HIP(hipStreamWaitEvent(hs, g->ev_side, 0));
  g->side_dirty = false;
  return OFX_OK;
}
// the same for host reads of device buffers (synchronous copies do not order after a non-blocking stream)
inline int sync_side(Gn* g) {
  if (!g->side || !g->side_dirty) return OFX_OK;
  OFX_HIP(hipStreamSynchronize(g->side));
  g->side_dirty = false;
  return OFX_OK;
}

// F_REFRESH: the GN step whose warm start rebuilds the cluster inverse (set by the previous step's update when a node's
// accumulated rotation passed precond_rot_tol; 0 = none); F_CAPPED: GN steps whose PCG ran into pcg_max_iter
enum { F_DONE = 0, F_STOPPED = 1, F_ILL = 2, F_ACCEPTED = 3, F_PCG_TOTAL = 4, F_APPLY = 5, F_RES_NONFINITE = 6,
       F_PCG_IT = 7, F_PCG_CNT = 8, F_REFRESH = 9, F_CAPPED = 10, F_COUNT = 11 };
// scalars: S_TH_CUR = the current solve's latest θ̂ (error-based stop), S_TH_PREV = the previous GN step's final θ̂
// (k_pcg_w0 moves it per solve; 1e300 = none)
enum { S_LOSS_PREV = 0, S_BB = 1, S_TH_PREV = 2, S_TH_CUR = 3, S_COUNT = 4 };
// host-mapped flags: H_DONE holds the epoch (GnDev::ep) of the last converged PCG solve (from the converging launch's
// lead lane);
// H_STOPPED the epoch of the solve whose GN step stopped the loop (0: running). k_upload clears them per setup.
enum { H_DONE = 0, H_PCG_IT = 1, H_STOPPED = 2, H_COUNT = 3 };
__device__ __forceinline__ void host_flag(const int32_t* hf, int k, int v) {
  __hip_atomic_store(const_cast<int32_t*>(hf) + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
constexpr int kMaxLog = 64;   // per-GN-step statistics slots
constexpr int32_t kEpochWrap = 1 << 30;   // GnDev::ep restarts at 1 from a setup once it reaches this (a solve adds <= 64)

// the scalar block (GnDev::pcs), in doubles: pcg_alpha [0, 6), pcg_gamma [6, 12), scal [12, 16), sturm (64 double2)
// [16, 144), flags (int32) from 144; written by k_pcg_w0 per solve: the PCG operator's address at 150, the stop tolerances
// (pcg_tol, pcg_err_tol) at 152, 153, the cluster inverses' address at 154, m0 / m1's at 156 / 157. The iteration gets
// the block's address with its parity in bit 3 (the block is 256-B aligned), so it needs no kernel-argument fetch for
// any of them.
constexpr int kPcgStreams = 4;   // k_pcg_iter's per-wave partial streams per parity: γ = r·u, δ = w·u, r·r, p·p
constexpr int kScAlpha = 0, kScGamma = 6, kScScal = 12, kScSturm = 16, kScFlags = 144, kScAop = 150, kScTol = 152,
              kScMcl = 154, kScM = 156, kScSize = 160;

// doubles per compact term record (layout: gn_linearize.hip; the setup sizes the record buffer by it)
constexpr int kRec = 20;

// entries per chunk of the assembly's workgroup-cooperative blocks (blocks_coop, gn_linearize.hip; the setup sizes
// blk_first by it)
#ifndef OFX_KCOOP
#define OFX_KCOOP 128   // (tuning builds: -DOFX_KCOOP=n, n <= kBlk)
#endif
constexpr int kCoop = OFX_KCOOP;
static_assert(kCoop <= kBlk, "one entry per thread per chunk");

// The iteration kernel's arguments: only what it reads (a ~200-B kernarg instead of the whole Gn:
// the host enqueues ~1000 of these per frame, so per-launch host work is on the critical path).
// What the converging PCG launch needs to also take the GN step (k_step's work, fused): fixed pointers in
// device memory (written once at create), per-step values in the kernel arguments.
struct StepArgs {
  double *R, *t, *xh, *stat, *loss_log, *step_state;
  const double* conf;
  double* racc;
};
struct PcgIt {
  const double* Aop;
  const float* Mcl;
  const int32_t *row_ptr, *col;
  const int2* wl;
  double *m0, *m1, *st, *part_p, *part_b, *pcg_alpha, *pcg_gamma, *scal;
  int32_t *flags, *hflags, *stopw;
  double2* sturm;               // error-based stop: per lead lane s the LDLᵀ pivot of T_k - σ_s I and its negative count
  uint64_t* stamps;
  int32_t nwg_row, nw_pad;
  struct { double pcg_tol, pcg_err_tol; } prm;
  // fused GN step (fuse = 0: k_step runs as its own launch)
  const StepArgs* sa;
  const double* tail;           // rhs + 6N: [loss² total, data, arap, motion, nonfinite]
  double stop_loss_diff;
  double rot_tol;               // precond_rot_tol
  int32_t fuse, gn_iter, N, mode, n_iter_log, warm;
  int32_t ep;                   // this solve's epoch (stop words, H_DONE)
};
inline PcgIt pcg_args(const Gn* g) {
  PcgIt a;
  memset(&a, 0, sizeof(a));   // (padding too: the host compares copies bytewise)
  a.Aop = g->Aop; a.Mcl = g->Mcl; a.row_ptr = g->row_ptr; a.col = g->col; a.wl = g->wl;
  a.m0 = g->m0; a.m1 = g->m1; a.st = g->st; a.part_p = g->part_p; a.part_b = g->part_b;
  a.pcg_alpha = g->pcg_alpha; a.pcg_gamma = g->pcg_gamma; a.scal = g->scal;
  a.flags = g->flags; a.hflags = g->hflags; a.stopw = g->stopw; a.stamps = g->stamps;
  a.nwg_row = g->nwg_row; a.nw_pad = g->nw_pad; a.prm.pcg_tol = g->prm.pcg_tol; a.prm.pcg_err_tol = g->prm.pcg_err_tol;
  a.sturm = g->sturm;
  a.sa = g->step_args; a.tail = nullptr; a.stop_loss_diff = g->prm.stop_loss_diff; a.rot_tol = g->prm.precond_rot_tol;
  a.fuse = 0; a.gn_iter = 0; a.N = g->N; a.mode = g->prm.mode; a.n_iter_log = 64; a.warm = g->prm.pcg_warm;
  a.ep = g->ep;
  return a;
}

inline double lm_for_iter(double lm0, int gn_iter) {
  double lm = lm0;
  for (int i = 0; i <= gn_iter; ++i)
    if (i % 3 == 2) lm /= 2;
  return lm;
}

// ---- host functions that cross files
// gn_linearize.hip: k_terms and the assembly of GN step gn_iter on hs (ofx_gn_linearize, gn.hip, checked the arguments)
int gn_linearize(Gn* g, int gn_iter, int m0, int m1, int add_reg, double* A, double* rhs, hipStream_t hs);

}  // namespace ofx
