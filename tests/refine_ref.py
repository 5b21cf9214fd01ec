"""Op-for-op numpy restatement of ofx_photo_refine (occlusionfusion_amd/csrc/refine.hip; arithmetic in include/ofx.h).

The refinement has no reference twin, so this file is what the kernel is pinned to. Every per-tap term is one float32
operation in the kernel's order; every sum (H, b, the squared residual) is a float64 sum of exact float32·float32
products, accumulated here in tap order (dy outer, dx inner, channels innermost) where the kernel sums each lane's taps
and then the lanes of a group in an xor tree — the one place the two may differ, in the last bits of a float64 sum. The
2x2 solve is float64; u is kept as float32.
"""
import numpy as np

import photo_ref as pr

F32, F64 = np.float32, np.float64
HMAX = 4
DEFAULTS = dict(half=3, iters=8, eps=1e-3, max_shift=4.0, min_eig=1e-6, ssd_max=np.inf)


def _cell(x, y, H, W):
    """The bilinear cell of f32 (x, y): ok (all four neighbours inside the image; NaN fails), x0, y0 (0 where not ok),
    fx, fy."""
    with np.errstate(invalid="ignore"):
        xf, yf = np.floor(x), np.floor(y)
        ok = (xf >= 0) & (xf <= F32(W - 2)) & (yf >= 0) & (yf <= F32(H - 2))
        x0 = np.where(ok, xf, 0).astype(np.int64)
        y0 = np.where(ok, yf, 0).astype(np.int64)
        fx, fy = (x - xf).astype(F32), (y - yf).astype(F32)
    return ok, x0, y0, fx, fy


def _bilin(plane, x0, y0, fx, fy):
    """One plane at a valid cell, every step one f32 operation: (1 - fy)·((1 - fx)·p00 + fx·p10) + fy·(...)."""
    p00, p10, p01, p11 = plane[y0, x0], plane[y0, x0 + 1], plane[y0 + 1, x0], plane[y0 + 1, x0 + 1]
    one = F32(1)
    wx, wy = one - fx, one - fy
    top = wx * p00 + fx * p10
    bot = wx * p01 + fx * p11
    return (wy * top + fy * bot).astype(F32)


def _sample(img, x, y, mask=None):
    """S(img, x, y) of a (3,H,W) image at f32 coordinates -> (ok [R], values f32 [R,3]; 0 where not ok)."""
    _, H, W = img.shape
    ok, x0, y0, fx, fy = _cell(x, y, H, W)
    if mask is not None:
        ok = ok & (mask[y0, x0] != 0) & (mask[y0, x0 + 1] != 0) & (mask[y0 + 1, x0] != 0) & (mask[y0 + 1, x0 + 1] != 0)
    x0, y0 = np.where(ok, x0, 0), np.where(ok, y0, 0)
    with np.errstate(all="ignore"):
        v = np.stack([_bilin(img[c], x0, y0, fx, fy) for c in range(3)], 1)
    return ok, np.where(ok[:, None], v, F32(0)).astype(F32)


def refine(template_image, template_mask, color_image, point_image, template_px, init_px, tgt_in, count, edge_max,
           half=3, iters=8, eps=1e-3, max_shift=4.0, min_eig=1e-6, ssd_max=np.inf, outputs=None):
    """The whole call on the rows below min(max(count[1], 0), R). -> dict(px_out f32[R,2], tgt_out f32[R,3], status
    u8[R], ssd f32[R]) — rows past the count keep `outputs`' values (zeros without it) — plus, for the tests, margin
    f64[R]: the smallest relative distance of a row's deciding quantities to their thresholds (min_eig, max_shift,
    ssd_max, edge_max), inf where none was evaluated or the threshold is infinite."""
    assert 1 <= int(half) <= HMAX and int(iters) >= 1
    tim, cim, vm = (np.asarray(a, F32) for a in (template_image, color_image, point_image))
    _, H, W = cim.shape
    tpx, ipx, tin = (np.asarray(a, F32) for a in (template_px, init_px, tgt_in))
    R = ipx.shape[0]
    n = int(min(max(int(count[1]), 0), R))
    out = {k: (np.array(outputs[k], copy=True) if outputs is not None else np.zeros(s, d))
           for k, s, d in (("px_out", (R, 2), F32), ("tgt_out", (R, 3), F32), ("status", (R,), np.uint8),
                           ("ssd", (R,), F32))}
    out["margin"] = np.full(R, np.inf)
    if n == 0:
        return out
    tpx, ipx, tin = tpx[:n], ipx[:n], tin[:n]
    h, w = int(half), 2 * int(half) + 1
    nt = w * w
    eps, max_shift, min_eig, ssd_max, edge_max = (F32(v) for v in (eps, max_shift, min_eig, ssd_max, edge_max))
    st = np.zeros(n, np.uint8)
    margin = np.full(n, np.inf)

    def note(rows, value, thr):
        """relative margin of value (f64) to the threshold thr on the given rows"""
        if np.isfinite(thr) and thr != 0:
            with np.errstate(all="ignore"):
                m = np.abs(np.asarray(value, F64)[rows] - F64(thr)) / abs(F64(thr))
            margin[rows] = np.minimum(margin[rows], np.where(np.isnan(m), np.inf, m))

    with np.errstate(invalid="ignore"):
        fin = np.isfinite(tpx).all(1) & np.isfinite(ipx).all(1)
        st[~fin | ((ipx[:, 0] == -1) & (ipx[:, 1] == -1))] = 1
    tx, ty = tpx[:, 0], tpx[:, 1]
    taps = [(t // w - h, t % w - h) for t in range(nt)]     # (dy, dx), dy outer
    # ---- the template, once
    T, GX, GY = (np.zeros((nt, n, 3), F32) for _ in range(3))
    bad = np.zeros(n, bool)
    hxx, hxy, hyy = np.zeros(n), np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for t, (dy, dx) in enumerate(taps):
            s = []
            for ox, oy in ((dx, dy), (dx + 1, dy), (dx - 1, dy), (dx, dy + 1), (dx, dy - 1)):
                ok, v = _sample(tim, (tx + F32(ox)).astype(F32), (ty + F32(oy)).astype(F32), template_mask)
                bad |= ~ok
                s.append(v)
            gx = (F32(0.5) * (s[1] - s[2])).astype(F32)
            gy = (F32(0.5) * (s[3] - s[4])).astype(F32)
            T[t], GX[t], GY[t] = s[0], gx, gy
            for c in range(3):
                hxx += gx[:, c].astype(F64) * gx[:, c].astype(F64)
                hxy += gx[:, c].astype(F64) * gy[:, c].astype(F64)
                hyy += gy[:, c].astype(F64) * gy[:, c].astype(F64)
        st[(st == 0) & bad] = 2
        det = hxx * hyy - hxy * hxy
        df, tr = hxx - hyy, hxx + hyy
        lmin = 0.5 * (tr - np.sqrt(df * df + 4.0 * (hxy * hxy)))
        live = st == 0
        note(live, lmin / F64(nt), min_eig)
        st[live & (~(det > 0) | ~(lmin / F64(nt) >= F64(min_eig)))] = 3

        # ---- the iterations; a row's pass after its last iteration (or its freeze) measures the residual
        ux, uy = ipx[:, 0].copy(), ipx[:, 1].copy()
        msr = np.zeros(n)
        run = st == 0                      # rows still iterating
        done = np.zeros(n, bool)           # rows whose residual pass has run
        frozen = np.zeros(n, bool)
        for it in range(int(iters) + 1):
            act = run & ~done
            if not act.any():
                break
            last = frozen | (it >= int(iters))
            bx, by, rr = np.zeros(n), np.zeros(n), np.zeros(n)
            bad = np.zeros(n, bool)
            for t, (dy, dx) in enumerate(taps):
                ok, v = _sample(cim, (ux + F32(dx)).astype(F32), (uy + F32(dy)).astype(F32))
                bad |= ~ok
                r = (v - T[t]).astype(F32)
                for c in range(3):
                    r64 = r[:, c].astype(F64)
                    bx += GX[t][:, c].astype(F64) * r64
                    by += GY[t][:, c].astype(F64) * r64
                    rr += r64 * r64
            left = act & bad
            st[left] = 4
            run &= ~left
            act &= ~left
            fin_rows = act & last
            msr[fin_rows] = rr[fin_rows] / F64(3 * nt)
            done |= fin_rows
            upd = act & ~last
            ddx = (hyy * bx - hxy * by) / det
            ddy = (hxx * by - hxy * bx) / det
            nx = (ux.astype(F64) - ddx).astype(F32)
            ny = (uy.astype(F64) - ddy).astype(F32)
            ux, uy = np.where(upd, nx, ux), np.where(upd, ny, uy)
            shift = np.maximum(np.abs((ux - ipx[:, 0]).astype(F32)), np.abs((uy - ipx[:, 1]).astype(F32)))
            note(upd, shift, max_shift)
            far = upd & (shift > max_shift)
            st[far] = 5
            run &= ~far
            frozen |= upd & (np.abs(ddx) < F64(eps)) & (np.abs(ddy) < F64(eps))

        # ---- the gates at the final u and the target
        live = st == 0
        ssd = np.where(live, msr, 0.0).astype(F32)
        thr = F64(ssd_max) * F64(ssd_max)
        note(live, msr, thr)
        st[live & ~(msr <= thr)] = 6
        live = st == 0
        ok, x0, y0, fx, fy = _cell(ux, uy, H, W)
        assert ok[live].all()              # the residual pass sampled the centre tap there
        x0, y0 = np.where(live, x0, 0), np.where(live, y0, 0)
        z = np.stack([vm[2][y0, x0], vm[2][y0, x0 + 1], vm[2][y0 + 1, x0], vm[2][y0 + 1, x0 + 1]], 1)
        spread = (z.max(1) - z.min(1)).astype(F32)
        holes = ~(z > 0).all(1)
        note(live & ~holes, spread, edge_max)
        st[live & (holes | ~(spread <= edge_max))] = 7
        good = st == 0
        tgt = np.stack([_bilin(vm[c], x0, y0, fx, fy) for c in range(3)], 1)
    out["px_out"][:n] = np.where(good[:, None], np.stack([ux, uy], 1), ipx)
    out["tgt_out"][:n] = np.where(good[:, None], tgt, tin)
    out["status"][:n] = st
    out["ssd"][:n] = ssd
    out["margin"][:n] = margin
    return out


def small_case(half=3, seed=0, n_rows=300, count=291):
    """photo_ref.small_case's 40x32 frame (its vertex map with a hole, a depth step and a far patch; its colour image
    with a NaN pixel taken out) extended for the refinement: a template image that is the live texture warped by a
    smooth sub-pixel field, a template mask with a hole, and n_rows rows of which `count` (not a multiple of 8) are
    emitted. Most rows lie inside; the first rows are placed so that every status occurs: a (-1, -1) and a NaN pixel
    (1), template patches that touch each of the four borders and the mask's hole (2), a flat-texture patch (3), live
    patches that leave the image at each border (4), a start far from the answer (5), a brightened block of the
    template (6), the vertex map's hole and a refined pixel that straddles its depth step (7). -> dict of numpy arrays and `params`."""
    base = pr.small_case(300, 0)
    rng = np.random.default_rng(seed)
    vm = base["point_image"]
    _, H, W = vm.shape
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))

    def tex(x, y):
        return np.stack([0.5 + 0.4 * np.sin(0.9 * x + 0.3 * y), 0.5 + 0.4 * np.sin(0.5 * y - 0.2 * x + 1.0),
                         0.5 + 0.4 * np.cos(0.35 * (x + y))])
    live = tex(uu, vv)
    # the template shows the same texture displaced: template(x, y) = live texture at (x, y) + s(x, y)
    sx = 0.35 + 0.1 * np.sin(0.2 * vv)
    sy = -0.25 + 0.1 * np.cos(0.15 * uu)
    timg = tex(uu + sx, vv + sy)
    flat = (slice(19, 32), slice(11, 25))            # a flat patch in both images: no gradient
    live[:, flat[0], flat[1]] = 0.5
    timg[:, flat[0], flat[1]] = 0.5
    live += rng.normal(0, 0.003, live.shape)
    timg += rng.normal(0, 0.003, timg.shape)
    live[:, flat[0], flat[1]] = 0.5
    timg[:, flat[0], flat[1]] = 0.5
    timg[:, 1:14, 14:29] += 0.1                      # a brightness change the model does not know: a large residual
    mask = np.ones((H, W), np.uint8)
    mask[3:5, 30:33] = 0                             # the mask's hole
    R = int(n_rows)
    m = half + 2.5
    tpx = np.stack([rng.uniform(m, W - 1 - m, R), rng.uniform(m, H - 1 - m, R)], 1)
    # the whole-pixel match a search would give: the template pixel moved by the field, rounded, and a pixel of error
    ipx = np.rint(tpx + np.stack([np.full(R, 0.35), np.full(R, -0.25)], 1) + rng.uniform(-0.9, 0.9, (R, 2)))
    k = 0

    def put(t, i):
        nonlocal k
        tpx[k], ipx[k] = t, i
        k += 1
    put((15.2, 12.7), (-1, -1))                                       # 1: the search's "no match" pixel
    put((np.nan, 12.0), (15, 12))                                     # 1
    put((15.0, 12.0), (np.inf, 12))                                   # 1
    for t in ((half + 0.6, 14.3), (W - 1.4 - half, 14.3), (5.3 + half, half + 0.5), (5.3 + half, H - 1.4 - half)):
        put(t, np.rint(t))                                            # 2: the gradient samples touch each border
    put((half + 1.2, 14.3), (half + 1, 14))                           # (just inside at the left: not 2)
    put((31.0 + half, 6.0), (31 + half, 6))                           # 2: the mask's hole
    put((17.5, 25.5), (17, 25))                                       # 3: flat texture
    put((17.5, 25.5 - 2 * half), (17, 25 - 2 * half))                 # (half flat: one-sided gradients)
    for i in ((half - 1, 14), (W - 1 - half, 14), (20, half - 1), (20, H - 1 - half)):
        put((20.3, 14.6), i)                                          # 4: the live patch leaves each border
    put((20.3, 8.6), (26, 8))                                         # 5 (or 4): a start far from the answer
    put((24.3, 9.6), (24, 14))
    put((21.3, 7.4), (22, 7))                                         # 6: the brightened block
    put((11.3, 10.6), (11, 10))                                       # 7: the vertex map's hole (depth[10:12, 10:13])
    put((29.0, 18.4), (29, 18))                                       # 7: the refined pixel straddles the depth step
    put((29.3, 8.4), (30, 8))
    put((4.8 + half, 24.3), (5 + half, 24))                           # near the far patch's edge
    tin = vm[:, np.clip(ipx[:, 1], 0, H - 1).astype(int), np.clip(ipx[:, 0], 0, W - 1).astype(int)].T
    tin = np.where(np.isfinite(ipx).all(1)[:, None], tin, 0).astype(F32)
    return dict(template_image=timg.astype(F32), template_mask=mask, color_image=live.astype(F32), point_image=vm,
                template_px=tpx.astype(F32), init_px=ipx.astype(F32), tgt_in=np.ascontiguousarray(tin),
                count=np.array([count + 40, count], np.int32), edge_max=0.03, shift=(0.35, -0.25),
                params=dict(half=int(half), iters=8, eps=1e-3, max_shift=2.5, min_eig=1e-6, ssd_max=0.05))
