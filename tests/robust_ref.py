"""Dense f64 Gauss-Newton with per-match weights and a robust kernel on the data rows: the reference of test_robust_ref.py
(CPU) and test_gpu_robust.py (device) for ofx_gn_set_robust / GaussNewtonSolver.optimize(match_weights=, robust=).

gn_optimize restates fo.gn_optimize's loop (oracle/fusion_oracle.py: the same rows, LM schedule, LU solve, stop rule and
update, operation for operation) with one addition: after the data rows and their residual are built, match m's three
rows and residuals are multiplied by

    s_m = match_weights[m] · s_rob(e_m),     e_m² = Σ_d (p_d - tgt_d)²  (metres², the deformed point against its target)
    Tukey c:  u = e²/c²,  s_rob = 1 - u for u < 1, else 0        (the square root of the biweight (1 - u)²)
    Huber δ:  s_rob = 1 for e <= δ, else sqrt(δ / e)

recomputed at every GN step (IRLS). Without weights and without a kernel s = 1.0 and the products are exact: the result
is fo.gn_optimize's bit for bit (test_robust_ref.py), and weights in {0, 1, 2} equal fo.gn_optimize on the problem with
each match repeated w² times — which ties the weight's meaning to the existing oracle.

The problems: gn_params_ref.base() (gn_small.npz, 257 nodes, 600 matches) with
* weights012(): seeded weights from {0, 1, 2}, and duplicated(): the match arrays with match m repeated w_m² times;
* outlier_targets(): 10 % of the targets displaced by seeded N(0, 0.05 m) per coordinate;
* isolated_targets(): every match anchored on node ISOLATED moved 0.5 m away (Tukey 0.03 rejects all of them at every step).
solve() caches the reference solves by name so that the GPU tests share them.
"""
import functools
import math

import numpy as np
from scipy.linalg import lu_factor, lu_solve

import gn_params_ref as P
from oracle import fusion_oracle as fo

F64 = np.float64
DEFAULTS = {"huber": 0.005, "tukey": 0.03}     # the package's ROBUST_DEFAULTS (test_robust_ops.py holds them equal)
OUTLIER_SHARE, OUTLIER_SIGMA = 0.10, 0.05
ISOLATED = 40                                  # a node with matches, for isolated_targets()


def row_scale(e2, kernel=None, scale=None):
    """s_rob of squared distances e2 (metres²)."""
    e2 = np.asarray(e2, F64)
    if kernel is None:
        return np.ones_like(e2)
    if kernel == "tukey":
        u = e2 / (scale * scale)
        return np.where(u < 1.0, 1.0 - u, 0.0)
    if kernel == "huber":
        e = np.sqrt(e2)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(e <= scale, 1.0, np.sqrt(scale / e))
    raise ValueError(kernel)


def gn_optimize(graph_nodes, graph_edges, graph_edges_weights, target_node_position, node_confidence, source_points,
                anchors, weights, target_points, intrinsics, target_px=None, target_py=None, prev_rot=None,
                prev_trans=None, match_weights=None, robust=None, **params):
    """fo.gn_optimize with the row scale above. robust: None or (kernel, scale). The result also carries "scales": per
    GN step that was linearised, the (M) row scales s."""
    p = dict(fo.GN_DEFAULTS)
    p.update(params)
    kernel, scale = robust if robust is not None else (None, None)
    g = np.asarray(graph_nodes, F64)
    N = g.shape[0]
    src = np.asarray(source_points, F64)
    M = src.shape[0]
    anc = np.asarray(anchors, np.int64)
    wts = np.asarray(weights, F64)
    tgt = np.asarray(target_points, F64)
    tpos = np.asarray(target_node_position, F64)
    conf = np.asarray(node_confidence, F64).reshape(-1)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    tpx = np.zeros(M) if target_px is None else np.asarray(target_px, F64).reshape(-1)
    tpy = np.zeros(M) if target_py is None else np.asarray(target_py, F64).reshape(-1)
    mw = np.ones(M) if match_weights is None else np.asarray(match_weights, F64).reshape(-1)
    edges, (ei, ek) = fo.gn_edges(graph_edges)
    E = edges.shape[0]
    n_nb = np.asarray(graph_edges).shape[1]
    ew = np.ones(E)
    if p['use_edge_weighting']:
        ew = float(n_nb) * np.asarray(graph_edges_weights, F64)[ei, ek]
    lf, ld = math.sqrt(p['lambda_flow']), math.sqrt(p['lambda_depth'])
    lm_, la = math.sqrt(p['lambda_motion']), math.sqrt(p['lambda_arap'])
    lm_factor = p['lm_factor']
    R = np.tile(np.eye(3), (N, 1, 1)) if prev_rot is None else np.asarray(prev_rot, F64).reshape(N, 3, 3).copy()
    t = np.zeros((N, 3)) if prev_trans is None else np.asarray(prev_trans, F64).reshape(N, 3).copy()
    conv = dict(total=[], data=[], arap=[], motion=[], errors=[])
    scales = []
    ill_posed = False
    rowsM = np.arange(M) * 3
    res = None
    for gn_i in range(p['num_iter']):
        if gn_i % 3 == 2:
            lm_factor /= 2
        J = np.zeros((M * 3, N * 6))
        defp = np.zeros((M, 3))
        for k in range(4):
            nk = anc[:, k]
            rot = np.einsum('mij,mj->mi', R[nk], src - g[nk])
            defp += wts[:, k:k + 1] * (rot + g[nk] + t[nk])
        zinv = 1.0 / (defp[:, 2] + 1e-7)
        fx_mul_x, fy_mul_y = fx * defp[:, 0], fy * defp[:, 1]
        fx_div_z, fy_div_z = fx * zinv, fy * zinv
        fx_mul_x_div_z, fy_mul_y_div_z = fx_mul_x * zinv, fy_mul_y * zinv
        mfx = -fx_mul_x_div_z * zinv
        mfy = -fy_mul_y_div_z * zinv
        for k in range(4):
            nk = anc[:, k]
            wk = wts[:, k]
            rot = np.einsum('mij,mj->mi', R[nk], src - g[nk])
            S = -fo.skew(wk[:, None] * rot)
            ct = 3 * N + 3 * nk
            J[rowsM, ct + 0] += lf * wk * fx_div_z
            J[rowsM, ct + 2] += lf * wk * mfx
            J[rowsM + 1, ct + 1] += lf * wk * fy_div_z
            J[rowsM + 1, ct + 2] += lf * wk * mfy
            J[rowsM, ct + 0] += ld * wk
            J[rowsM + 1, ct + 1] += ld * wk
            J[rowsM + 2, ct + 2] += ld * wk
            cr = 3 * nk
            for j in range(3):      # flow part with the reference's precedence quirk (model.py:505-510)
                J[rowsM, cr + j] += lf * fx_div_z * S[:, 0, j] + mfx * S[:, 2, j]
                J[rowsM + 1, cr + j] += lf * fy_div_z * S[:, 1, j] + mfy * S[:, 2, j]
            for i in range(3):
                for j in range(3):
                    J[rowsM + i, cr + j] += ld * S[:, i, j]
        rd = np.zeros(M * 3)
        rd[rowsM] = lf * (fx_mul_x_div_z + cx - tpx)
        rd[rowsM + 1] = lf * (fy_mul_y_div_z + cy - tpy)
        rd[rowsM] += ld * (defp[:, 0] - tgt[:, 0])
        rd[rowsM + 1] += ld * (defp[:, 1] - tgt[:, 1])
        rd[rowsM + 2] += ld * (defp[:, 2] - tgt[:, 2])
        # ---- the row scale: the one addition to fo.gn_optimize
        s = mw * row_scale(((defp - tgt) ** 2).sum(1), kernel, scale)
        scales.append(s)
        s3 = np.repeat(s, 3)
        J *= s3[:, None]
        rd *= s3
        # ----
        blocks_J, blocks_r = [J], [rd]
        ra = None
        if E > 0:
            Ja = np.zeros((E * 3, N * 6))
            i0, i1 = edges[:, 0], edges[:, 1]
            rowsE = np.arange(E) * 3
            delta = np.einsum('eij,ej->ei', R[i0], g[i1] - g[i0])
            ra = (la * ew[:, None] * (delta + g[i0] + t[i0] - (g[i1] + t[i1]))).reshape(-1)
            for c in range(3):
                Ja[rowsE + c, 3 * N + 3 * i0 + c] += la * ew
                Ja[rowsE + c, 3 * N + 3 * i1 + c] += -la * ew
            Sa = -la * ew[:, None, None] * fo.skew(delta)
            for i in range(3):
                for j in range(3):
                    Ja[rowsE + i, 3 * i0 + j] += Sa[:, i, j]
            blocks_J.append(Ja)
            blocks_r.append(ra)
        Jm = np.zeros((N * 3, N * 6))
        ids = np.arange(N)
        for c in range(3):
            Jm[ids * 3 + c, 3 * N + 3 * ids + c] += lm_ * conf
        rm = (lm_ * conf[:, None] * (t + g - tpos)).reshape(-1)
        blocks_J.append(Jm)
        blocks_r.append(rm)
        Jall = np.concatenate(blocks_J, 0)
        res = np.concatenate(blocks_r, 0)
        A = Jall.T @ Jall + np.eye(6 * N) * lm_factor
        b = -(Jall.T @ res)
        try:
            x = lu_solve(lu_factor(A), b)
        except Exception:
            ill_posed = True
            conv['errors'].append("Solver failed: Ill-posed system!")
            break
        if not np.all(np.isfinite(x)):
            ill_posed = True
            conv['errors'].append("Solver failed: Non-finite solution x!")
            break
        loss_total = float(np.linalg.norm(res))
        if len(conv['total']):
            if loss_total - conv['total'][-1] > p['stop_loss_diff']:
                break
            if loss_total == conv['total'][-1]:
                break
        conv['data'].append(float(np.linalg.norm(rd)))
        conv['total'].append(loss_total)
        R_inc = fo.angle_axis_to_rotation_matrix(x[:3 * N].reshape(N, 3))
        R = R_inc @ R
        t = t + x[3 * N:].reshape(N, 3)
        if ra is not None:
            conv['arap'].append(float(np.linalg.norm(ra)))
        conv['motion'].append(float(np.linalg.norm(rm)))
    valid = (not ill_posed) and res is not None and bool(np.all(np.isfinite(res)))
    if not valid:
        R = np.tile(np.eye(3), (N, 1, 1))
        t = np.zeros((N, 3))
    conv['valid'] = int(valid)
    return dict(node_rotations=R, node_translations=t, valid_solve=int(valid), convergence_info=conv, scales=scales)


# ---------------------------------------------------------------------------------------------- the problems
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def weights012():
    """(600) f32 weights from {0, 1, 2}, seeded."""
    M = P.base()["src"].shape[0]
    return _frozen(np.random.default_rng(20241020).integers(0, 3, M).astype(np.float32))


def duplicated(w):
    """Row indices of the problem with match m repeated w_m² times (0, 1 or 4 copies, kept in match order)."""
    return np.repeat(np.arange(len(w)), (np.asarray(w, np.int64) ** 2))


def with_matches(inputs, rows=None, tgt=None):
    """The ten positional arguments with the match arrays (src, anchors, weights, tgt) restricted to rows and / or the
    targets replaced."""
    i = list(inputs)
    if tgt is not None:
        i[8] = tgt
    if rows is not None:
        for k in (5, 6, 7, 8):
            i[k] = i[k][rows]
    return tuple(i)


@functools.lru_cache(maxsize=None)
def outlier_targets():
    """-> (tgt (600,3) f32 with 10 % of the rows displaced by N(0, 0.05 m), the displaced rows' mask)."""
    d = P.base()
    M = d["tgt"].shape[0]
    rng = np.random.default_rng(20241021)
    rows = rng.choice(M, int(round(OUTLIER_SHARE * M)), replace=False)
    tgt = d["tgt"].astype(np.float64)
    tgt[rows] += rng.normal(0.0, OUTLIER_SIGMA, (len(rows), 3))
    mask = np.zeros(M, bool)
    mask[rows] = True
    return _frozen(tgt.astype(np.float32)), _frozen(mask)


@functools.lru_cache(maxsize=None)
def isolated_targets():
    """-> (tgt with every match anchored on node ISOLATED moved 0.5 m along z, those matches' mask)."""
    d = P.base()
    mask = (d["anchors"] == ISOLATED).any(1)
    tgt = d["tgt"].copy()
    tgt[mask, 2] += np.float32(0.5)
    return _frozen(tgt), _frozen(mask)


def max_t_err(a, b):
    return float(np.abs(np.asarray(a["node_translations"]) - np.asarray(b["node_translations"])).max())


# name -> (tag, padded edges, targets, match rows, weights, robust, identity start)
def _cases():
    out_t = lambda: outlier_targets()[0]     # noqa: E731
    w = weights012
    return {
        "clean": ("default", False, None, None, None, None, True),
        "plain": ("default", False, out_t, None, None, None, True),
        "tukey": ("default", False, out_t, None, None, ("tukey", 0.03), True),
        "huber": ("default", False, out_t, None, None, ("huber", 0.005), True),
        "w_tukey": ("default", False, out_t, None, w, ("tukey", 0.03), True),
        "flow_tukey": ("flow_1e-3", False, out_t, None, None, ("tukey", 0.03), True),
        "w012": ("default", False, None, None, w, None, False),
        "zeros": ("default", False, None, None, lambda: np.zeros(600, np.float32), None, False),
        "isolated": ("default", False, lambda: isolated_targets()[0], None, None, ("tukey", 0.03), True),
        "pad_w_huber": ("default", True, out_t, None, w, ("huber", 0.005), True),
        "m597": ("default", False, out_t, np.arange(597), w, ("tukey", 0.03), True),
    }


CASES = tuple(_cases())


def problem(name):
    """-> (the ten positional arguments, keywords: flow targets, start pose, match_weights, robust as (kernel, scale))."""
    tag, pad, tgt, rows, w, robust, identity = _cases()[name]
    args = with_matches(P.inputs(tag, pad), rows, None if tgt is None else tgt())
    kw = dict(P.flow_targets(tag))
    if rows is not None:
        kw = {k: v[rows] for k, v in kw.items()}
    if not identity:
        d = P.base()
        kw.update(prev_rot=d["R0"], prev_trans=d["t0"])
    mw = None if w is None else w()
    if mw is not None and rows is not None:
        mw = mw[rows]
    return tag, args, kw, mw, robust


@functools.lru_cache(maxsize=None)
def solve(name):
    """The f64 reference solve of the named case."""
    tag, args, kw, mw, robust = problem(name)
    kw = {k: (np.asarray(v, F64) if k.startswith("prev_") else v) for k, v in kw.items()}
    return gn_optimize(*args, **kw, match_weights=mw, robust=robust, **P.params(tag))
