"""CPU: the argument checks of the eight integrate entry points (ofx_integrate, _palette, _palette_cull, _points and
their _w forms) answer with a status code and a message before any launch, and a call with nothing to do returns OFX_OK
before any device call. Addresses are made up and never dereferenced. One table: every row is one call carrying at
most one fault, with the status and message the library gave before the entry points came to share their checks."""
import ctypes

import pytest

from occlusionfusion_amd import _lib

vp = ctypes.c_void_p
A = 64   # the made-up address
OK, ERR_ARG = 0, -1


def _call(entry, weighted, dim=(16, 16, 16), bricks=(0, 2), sem=0, cam=True, width=40, height=32, depth=A, color_im=None,
          color=None, tsdf=A, weight=A, nodes=A, n_nodes=8, k=4, brick_list=A, n_list=2, anchors=A, weights=A, pal_ids=A,
          pal_n=A, local=A, points=A, voxel_ids=A, n_points=10, generic=False):
    """One call of `entry` ("src" / "warp": ofx_integrate; "pal"; "cull"; "cull0": the cull entry point with null
    scratch; "points"), or of its _w form with valid observation weights -> (status, message)."""
    L, b = _lib.lib, ctypes.byref
    d = _lib.VolumeDesc()
    d.dim[:] = dim
    d.brick_x0, d.brick_x1, d.semantics = bricks[0], bricks[1], sem
    d.origin[:] = [0.0, 0.0, 1.0]
    d.voxel_size, d.trunc_margin = 0.004, 0.04
    c = b(_lib.Camera(525.0, 525.0, 20.0, 16.0, width, height)) if cam else None
    p = lambda v: None if v is None else vp(v)
    tail = ((b(_lib.ObsWeights(A, float("inf"), 0.0)),) if weighted else ()) + (None,)
    sfx = "_w" if weighted else ""
    out = (1.0, p(tsdf), p(weight), p(color), None)
    if entry in ("src", "warp"):
        warp = entry == "warp"
        st = getattr(L, "ofx_integrate" + sfx)(b(d), c, p(depth), p(color_im), int(warp), p(nodes) if warp else None,
                                               n_nodes if warp else 0, k if warp else 1, p(brick_list), n_list,
                                               p(anchors) if warp else None, p(weights) if warp else None, *out, *tail)
    elif entry == "points":
        st = getattr(L, "ofx_integrate_points" + sfx)(b(d), c, p(depth), p(color_im), p(points), p(voxel_ids), None,
                                                      n_points, *out, *tail)
    else:
        args = (b(d), c, p(depth), p(color_im), p(nodes), n_nodes, k, p(brick_list), n_list, p(anchors), p(weights),
                p(pal_ids), p(pal_n), p(local), *out)
        if entry == "pal":
            st = getattr(L, "ofx_integrate_palette" + sfx)(*args, *tail)
        else:
            scratch = (vp(A), vp(A)) if entry == "cull" else (None, None)
            st = getattr(L, "ofx_integrate_palette_cull" + sfx)(*args, *scratch, *tail)
    return st, L.ofx_last_error()


ALL = ("src", "warp", "pal", "cull", "cull0", "points")
WARPED = ("warp", "pal", "cull", "cull0")
PALETTE = ("pal", "cull", "cull0")
SRC = dict(brick_list=None, n_list=0)   # the source frame over all bricks of the shard

# (entries, the call's departure from a valid one, expected of the plain form, expected of the _w form): OK, or the
# message of an OFX_ERR_ARG
COLOR = b"color and color_im must both be set or both NULL"
ROWS = [
    (ALL, dict(dim=(16, 0, 16)), b"bad volume dims", b"bad volume dims"),
    (ALL, dict(bricks=(0, 3)), b"bad brick shard range [0,3) of 2", b"bad brick shard range [0,3) of 2"),
    (ALL, dict(bricks=(1, 1)), b"bad brick shard range [1,1) of 2", b"bad brick shard range [1,1) of 2"),
    (("src", "warp"), dict(cam=False), b"null buffer", b"null buffer"),
    (PALETTE, dict(cam=False), b"null camera/depth", b"null camera/depth"),
    (("points",), dict(cam=False), b"null buffer / bad size", b"null buffer / bad size"),
    (("src", "warp"), dict(depth=None), b"null buffer", b"null buffer"),
    (PALETTE, dict(depth=None), b"null camera/depth", b"null camera/depth"),
    (("points",), dict(depth=None), b"null buffer / bad size", b"null buffer / bad size"),
    (("src", "warp"), dict(tsdf=None), b"null buffer", b"null buffer"),
    (("points",), dict(tsdf=None), b"null buffer / bad size", b"null buffer / bad size"),
    (("src", "warp"), dict(weight=None), b"null buffer", b"null buffer"),
    (("points",), dict(weight=None), b"null buffer / bad size", b"null buffer / bad size"),
    (ALL, dict(width=0), b"bad camera size", b"bad camera size"),
    (ALL, dict(height=-1), b"bad camera size", b"bad camera size"),
    (ALL, dict(color_im=A), COLOR, COLOR),
    (ALL, dict(color=A), COLOR, COLOR),
    # semantics 7 with work to do: the _w forms of all but ofx_integrate look at the observation weights first
    (("src", "warp"), dict(sem=7), b"bad semantics 7", b"bad semantics 7"),
    (PALETTE + ("points",), dict(sem=7), b"bad semantics 7",
     b"the weighted integrate has CPU semantics only (semantics 7)"),
    (WARPED, dict(k=5), b"bad k/n_nodes", b"bad k/n_nodes"),
    (WARPED, dict(k=0), b"bad k/n_nodes", b"bad k/n_nodes"),
    (WARPED, dict(n_nodes=3), b"bad k/n_nodes", b"bad k/n_nodes"),
    (WARPED, dict(n_list=9), b"bad n_list", b"bad n_list"),           # the shard has 2 x 2 x 2 bricks
    (WARPED, dict(n_list=-1), b"bad n_list", b"bad n_list"),
    (("src",), dict(generic=True, brick_list=A, n_list=9), b"bad n_list", b"bad n_list"),
    (("src",), dict(generic=True, brick_list=A, n_list=-1), b"bad n_list", b"bad n_list"),
    (("warp",), dict(nodes=None), b"null warp buffer", b"null warp buffer"),
    (PALETTE, dict(nodes=None), b"null warp/palette buffer", b"null warp/palette buffer"),
    (("warp",), dict(brick_list=None), b"null warp buffer", b"null warp buffer"),
    (PALETTE, dict(brick_list=None), b"null warp/palette buffer", b"null warp/palette buffer"),
    (("warp",), dict(anchors=None), b"null warp buffer", b"null warp buffer"),
    (PALETTE, dict(anchors=None), b"null warp/palette buffer", b"null warp/palette buffer"),
    (("warp",), dict(weights=None), b"null warp buffer", b"null warp buffer"),
    (PALETTE, dict(weights=None), b"null warp/palette buffer", b"null warp/palette buffer"),
    (PALETTE, dict(pal_ids=None), b"null warp/palette buffer", b"null warp/palette buffer"),
    (PALETTE, dict(pal_n=None), b"null warp/palette buffer", b"null warp/palette buffer"),
    (PALETTE, dict(local=None), b"null warp/palette buffer", b"null warp/palette buffer"),
    (("points",), dict(n_points=-1), b"null buffer / bad size", b"null buffer / bad size"),
    (("points",), dict(points=None), b"null points / voxel ids", b"null points / voxel ids"),
    (("points",), dict(voxel_ids=None), b"null points / voxel ids", b"null points / voxel ids"),
    # nothing to do: OFX_OK before any device call (this runs where there is no device)
    (WARPED, dict(n_list=0), OK, OK),
    (WARPED, dict(n_list=0, generic=True), OK, OK),
    (("src",), dict(brick_list=A, n_list=0), OK, OK),
    (("src",), dict(brick_list=A, n_list=0, generic=True), OK, OK),
    (("points",), dict(n_points=0), OK, OK),
]


def _cases():
    for entries, kw, plain, w in ROWS:
        for e in entries:
            for weighted, want in ((False, plain), (True, w)):
                yield pytest.param(e, weighted, kw, want, id=f"{e}{'_w' if weighted else ''}-"
                                   + ",".join(f"{k}={v}" for k, v in kw.items()))


@pytest.mark.parametrize("entry,weighted,kw,want", _cases())
def test_integrate_argument_checks(entry, weighted, kw, want, monkeypatch):
    kw = dict(SRC, **kw) if entry == "src" and "brick_list" not in kw else dict(kw)
    if kw.get("generic"):
        monkeypatch.setenv("OFX_INT_GENERIC", "1")
    else:
        monkeypatch.delenv("OFX_INT_GENERIC", raising=False)
    st, msg = _call(entry, weighted, **kw)
    if want == OK:
        assert st == OK, (st, msg)
    else:
        assert st == ERR_ARG and msg == want, (st, msg)
