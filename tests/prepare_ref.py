"""Op-for-op float32 numpy restatement of ofx_prepare_depth (occlusionfusion_amd/csrc/prepare.hip).

Depth-frame preparation has no reference twin, so this file is what the kernels are pinned to, bit for bit: the taps run
in the kernel's order (dv outer, du inner), every product and sum is one f32 operation, the two exponentials are the f32
roundings of f64 exponentials and the final quotient is correctly rounded. The vertex map is fusion_oracle.
backproject_depth of the filtered depth and the normal map is assoc_ref.project_gate's n_q at every pixel's own ray, so
neither formula is repeated here. The loop is over taps and vectorised over pixels.
"""
import numpy as np

import assoc_ref as ar
from oracle import fusion_oracle as fo

F32, F64 = np.float32, np.float64
RMAX = 4
DEFAULTS = dict(radius=3, sigma_s=2.0, sigma_r=0.01, range_cut=None)


def depth_f32(depth, normalizer=1000.0):
    """The depth in metres as the kernel reads it: f32 as given, anything else as uint16 / f32(normalizer)."""
    d = np.asarray(depth)
    if d.dtype == F32:
        return d
    with np.errstate(all="ignore"):
        return (d.view(np.uint16) if d.dtype == np.int16 else d.astype(np.uint16)).astype(F32) / F32(normalizer)


def bilateral(depth, radius=3, sigma_s=2.0, sigma_r=0.01, range_cut=None, normalizer=1000.0):
    """The filtered depth f32 (H, W): zeros at the holes (!(D > 0)), else Σ w·N / Σ w over the taken taps."""
    D = depth_f32(depth, normalizer)
    H, W = D.shape
    r = int(radius)
    assert 0 <= r <= RMAX
    cut = F32(3.0 * float(sigma_r) if range_cut is None else range_cut)
    a_s = -0.5 / (F64(F32(sigma_s)) * F64(F32(sigma_s)))
    a_r = -0.5 / (F64(F32(sigma_r)) * F64(F32(sigma_r)))
    Dp = np.zeros((H + 2 * r, W + 2 * r), F32)                # a tap outside the image reads a hole
    Dp[r:r + H, r:r + W] = D
    num, den = np.zeros((H, W), F32), np.zeros((H, W), F32)
    with np.errstate(all="ignore"):
        valid = D > 0
        for dv in range(-r, r + 1):
            for du in range(-r, r + 1):
                N = Dp[r + dv:r + dv + H, r + du:r + du + W]
                diff = N - D
                own = du == 0 and dv == 0                     # the centre tap: always taken, wr = 1 (a +inf centre too)
                take = valid if own else valid & (N > 0) & ~(np.abs(diff) > cut)
                ws = F32(np.exp(a_s * F64(du * du + dv * dv)))
                wr = np.ones((H, W), F32) if own else np.exp(a_r * (diff.astype(F64) * diff.astype(F64))).astype(F32)
                w = ws * wr
                num = np.where(take, num + w * N, num)
                den = np.where(take, den + w, den)
        out = (num.astype(F64) / den.astype(F64)).astype(F32)
    return np.where(valid, out, F32(0)).astype(F32)


def pixel_rays(intr, H, W):
    """One camera-space point per pixel, row-major, that projects to exactly that pixel (checked): ((u - cx)/fx,
    (v - cy)/fy, 1) in f32."""
    fx, fy, cx, cy = (F32(v) for v in intr[:4])
    u, v = np.meshgrid(np.arange(W, dtype=F32), np.arange(H, dtype=F32))
    y = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones((H, W), F32)], -1).reshape(-1, 3).astype(F32)
    inside, uu, vv = ar.pixel_f32(y, intr, H, W)
    assert inside.all() and np.array_equal(uu.reshape(H, W), u) and np.array_equal(vv.reshape(H, W), v)
    return y


def normal_map(point_image, intr, edge_max=0.03):
    """The gate's n_q of the vertex map at every pixel (assoc_ref.project_gate with no distance and no cosine gate),
    zeros where it returns code 3 or 4 -> f32 (3, H, W)."""
    vm = np.asarray(point_image, F32)
    _, H, W = vm.shape
    y = pixel_rays(intr, H, W)
    code, live, q, nq, e = ar.project_gate(np.ones(H * W, bool), y, None, intr, vm, dist_max=np.inf, cos_min=0.0,
                                           edge_max=edge_max)
    assert set(np.unique(code)) <= {0, 3, 4}
    n = np.where(live[:, None], nq, F32(0)).astype(F32)
    return np.ascontiguousarray(n.T.reshape(3, H, W))


def prepare(depth, intr, radius=3, sigma_s=2.0, sigma_r=0.01, range_cut=None, edge_max=0.03, normals=True,
            normalizer=1000.0):
    """The whole call: dict(depth (H,W), point_image (3,H,W), normals (3,H,W) or None)."""
    f = bilateral(depth, radius, sigma_s, sigma_r, range_cut, normalizer)
    vm = fo.backproject_depth(f, *(float(v) for v in intr[:4]))
    return {"depth": f, "point_image": vm, "normals": normal_map(vm, intr, edge_max) if normals else None}


# ------------------------------------------------------------------------------------------------ denoising measures
def config1_frame(t=20):
    """Config 1's camera (320x224) and frame t: (intr, the sequence's own noisy depth, the noise-free render)."""
    from occlusionfusion_amd import synthetic as S
    scene, seed = S.config_scene(1)
    cam = S.bench_camera(S.BASELINE_CONFIGS[1]["cam_scale"])
    return (cam.fx, cam.fy, cam.cx, cam.cy), S.frame_depth(scene, cam, seed, t), scene.render(cam, t)


def clean_reference(clean, intr, edge_max=0.03):
    """What the measures compare against, computed once from the noise-free frame: its vertex map, its gate normals,
    and every 5th valid pixel of the vertex map as points on the clean surface."""
    vm = fo.backproject_depth(clean, *intr)
    pts = np.ascontiguousarray(vm.reshape(3, -1).T[clean.reshape(-1) > 0][::5])
    return {"depth": clean, "point_image": vm, "normals": normal_map(vm, intr, edge_max), "points": pts}


def measures(depth, point_image, normals, ref, intr):
    """dict(angle: mean / median / p95 degrees between this frame's gate normal and the clean frame's, over the pixels
    where both exist; depth_err: mean |depth - clean| over the pixels valid in both, metres; offset / offset_rms: the
    plane-mode target offset |tgt - x'| of the clean-surface points under the identity warp (assoc_ref.gate, default
    gates, no model normals), over the accepted ones; share: the accepted share of those points)."""
    both = (np.abs(normals).sum(0) > 0) & (np.abs(ref["normals"]).sum(0) > 0)
    c = (normals.astype(F64) * ref["normals"].astype(F64)).sum(0)[both]
    ang = np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))
    ok = (depth > 0) & (ref["depth"] > 0)
    derr = np.abs(depth.astype(F64) - ref["depth"].astype(F64))[ok].mean()
    pts = ref["points"]
    P = pts.shape[0]
    a = np.zeros((P, 4), np.int32)
    w = np.tile(np.array([1, 0, 0, 0], F32), (P, 1))
    code, tgt, warped = ar.gate(pts, None, a, w, None, np.eye(3, dtype=F32)[None], np.zeros((1, 3), F32),
                                np.zeros((1, 3), F32), intr, point_image)
    acc = code == 0
    off = np.linalg.norm(tgt[acc].astype(F64) - warped[acc].astype(F64), axis=1)
    return {"angle": (float(ang.mean()), float(np.median(ang)), float(np.percentile(ang, 95))),
            "depth_err": float(derr), "offset": float(off.mean()), "offset_rms": float(np.sqrt((off * off).mean())),
            "share": float(acc.mean()), "points": int(P)}


def check_denoising(raw, filt):
    """The four conditions on measures() of the raw and of the filtered frame; prints every figure first."""
    print(f"normal angle mean/median/p95: raw {raw['angle'][0]:.2f}/{raw['angle'][1]:.2f}/{raw['angle'][2]:.2f} deg, "
          f"filtered {filt['angle'][0]:.2f}/{filt['angle'][1]:.2f}/{filt['angle'][2]:.2f} deg, "
          f"ratio {filt['angle'][0] / raw['angle'][0]:.3f}")
    print(f"mean |depth - clean|: raw {1e3 * raw['depth_err']:.3f} mm, filtered {1e3 * filt['depth_err']:.3f} mm, "
          f"ratio {filt['depth_err'] / raw['depth_err']:.3f}")
    print(f"plane-mode target offset mean (rms): raw {1e3 * raw['offset']:.3f} ({1e3 * raw['offset_rms']:.3f}) mm, "
          f"filtered {1e3 * filt['offset']:.3f} ({1e3 * filt['offset_rms']:.3f}) mm, "
          f"ratio {filt['offset'] / raw['offset']:.3f}")
    print(f"accepted share of {raw['points']} points: raw {raw['share']:.4f}, filtered {filt['share']:.4f}")
    assert filt["angle"][0] <= 0.5 * raw["angle"][0]
    assert filt["depth_err"] <= 0.6 * raw["depth_err"]
    assert filt["offset"] <= 0.5 * raw["offset"]
    assert filt["share"] >= raw["share"] - 0.005
