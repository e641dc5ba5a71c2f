"""The rasteriser's pixel rules in plain numpy, and the hand-built scenes that isolate each of them.

`render_rules` restates the conventions listed at the top of csrc/raster.hip -- 8-bit sub-pixel snapping, integer edge functions, the
top-left fill rule, the bounding box clamped to the frame, perspective-correct 1/z, z ties to the lower face id, per-fragment
[znear, zfar] discard, nearest / bilinear clamp-to-edge texel fetch with the flipped row -- for the identity pose, in int64 / float64
(texture coordinates in exact rationals, so that a pixel centre that lies exactly on a texel border or centre is decided by the rule and
not by rounding noise).  It is written from those conventions, not from oracle/raster.c, and knows nothing about near-plane clipping:
every vertex must lie at Z >= znear.

A scene is only a fair exact test if the f32 arithmetic of the kernel cannot move a vertex: `projection_is_exact` asserts that every
projected coordinate is the same multiple of 1/512 px in f32 and in f64 (and bit-equal where that multiple is odd, i.e. a snapping tie).
All exact scenes share K = RK, znear = 0.25 and zfar = 2.0, so that they can be the classes of one mesh table.

`near_cut` is apart: its expected answer is the analytic intersection of each pixel's ray with a flat patch, not `render_rules`.
"""
import collections
import functools
from fractions import Fraction

import numpy as np

RK = np.array([[64.0, 0, 18.5], [0, 64.0, 14.5], [0, 0, 1]], np.float32)
ZNEAR, ZFAR = 0.25, 2.0
FRAMES = ((30, 37), (32, 48))   # (H, W): W % 4 != 0 takes the one-pass resolve, 32x48 the two-pass one
COORD_LIM = 1.0e6               # a face with a projected coordinate at or beyond it is dropped whole
MASK_THR = 0.2

Rendered = collections.namedtuple("Rendered", "owner depth bgr mask bbox info")


# ---------------------------------------------------------------------------------------------------------------- the rules

def project(verts, K):
    """float64 pinhole projection of f32 vertices under the identity pose -> u, v (px), Z"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    return K[0, 0] * v[:, 0] / v[:, 2] + K[0, 2], K[1, 1] * v[:, 1] / v[:, 2] + K[1, 2], v[:, 2]


def projection_is_exact(verts, K):
    """the exactness guard: each projected coordinate, computed as the kernel does in f32 (x / z rounded, then one fused multiply-add),
    is a multiple of 1/512 px, the f64 projection rounds to the same multiple and lies within 1/100 of it, and where the multiple is
    odd (the snapping tie u * 256 + 0.5 = integer) the two are equal"""
    v32 = np.asarray(verts, np.float32)
    K32 = np.asarray(K, np.float32).reshape(3, 3)
    u64 = project(verts, K)[:2]
    for axis, (f, c) in enumerate(((K32[0, 0], K32[0, 2]), (K32[1, 1], K32[1, 2]))):
        q = (v32[:, axis] / v32[:, 2]).astype(np.float32)                                   # __fdiv_rn
        fma = (np.float64(f) * q.astype(np.float64) + np.float64(c)).astype(np.float32)     # product exact in f64, one rounding
        k32 = fma.astype(np.float64) * 512.0
        k64 = u64[axis] * 512.0
        assert np.all(k32 == np.round(k32)), "f32 projection off the 1/512 grid"
        assert np.all(np.round(k64) == k32) and np.all(np.abs(k64 - k32) < 0.01), "f64 and f32 projections name different grid points"
        odd = np.mod(k32, 2.0) == 1.0
        assert np.all(k64[odd] == k32[odd]), "a snapping tie that is not exact in f64"


def _ceil_div(a, b):
    return -((-a) // b)


def render_rules(verts, uvs, faces, tex, K, H, W, znear, zfar, tex_bilinear=False, mask_thr=MASK_THR, fill="top-left", tie="lower",
                 snap="nearest", flip_rows=True):
    """-> Rendered(owner (H,W) int64, -1 = background; depth (H,W) float64, 0 = background; bgr (H,W,3) float32; mask (H,W) float32 =
    depth > mask_thr; bbox [min x, max x, min y, max y] of the mask, [W, -1, H, -1] when it is empty; info).

    The switches select deliberately WRONG variants for the negative controls of tests/test_raster_rules_host.py:
    fill="bottom-right", tie="higher", snap="floor" (floor(u * 256) instead of floor(u * 256 + 0.5)), flip_rows=False.
    info: `edge_count` (H,W) = number of faces that hold the pixel centre exactly on an edge of their closed triangle (inside their
    bounding box and depth range), `edge_lo` / `edge_hi` = the lowest / highest id among those faces."""
    assert fill in ("top-left", "bottom-right") and tie in ("lower", "higher") and snap in ("nearest", "floor")
    verts = np.asarray(verts, np.float32)
    uvs = np.asarray(uvs, np.float32)
    faces = np.asarray(faces, np.int64)
    tex = np.asarray(tex, np.uint8)
    projection_is_exact(verts, K)
    u, v, Z = project(verts, K)
    assert np.all(Z >= max(znear, 1e-4)), "render_rules does not clip: every vertex must lie at Z >= znear"
    SX = np.floor(u * 256.0 + (0.5 if snap == "nearest" else 0.0)).astype(np.int64)
    SY = np.floor(v * 256.0 + (0.5 if snap == "nearest" else 0.0)).astype(np.int64)
    usable = (np.abs(u) < COORD_LIM) & (np.abs(v) < COORD_LIM)

    owner = np.full((H, W), -1, np.int64)
    depth = np.zeros((H, W), np.float64)
    edge_count = np.zeros((H, W), np.int64)
    edge_lo = np.full((H, W), -1, np.int64)
    edge_hi = np.full((H, W), -1, np.int64)
    for f, face in enumerate(faces):
        if not usable[face].all():
            continue
        X, Y = SX[face], SY[face]
        area = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
        if area == 0:
            continue
        s = 1 if area > 0 else -1          # orient so that the interior is where every edge function is positive
        x0, x1 = max(_ceil_div(X.min(), 256), 0), min(X.max() // 256, W - 1)
        y0, y1 = max(_ceil_div(Y.min(), 256), 0), min(Y.max() // 256, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        px, py = np.meshgrid(np.arange(x0, x1 + 1, dtype=np.int64) * 256, np.arange(y0, y1 + 1, dtype=np.int64) * 256)
        inside = np.ones(px.shape, bool)
        closed = np.ones(px.shape, bool)
        E = []
        for i in range(3):                 # edge i, opposite vertex i, runs from vertex a to vertex b
            a, b = (i + 1) % 3, (i + 2) % 3
            dx, dy = s * (X[b] - X[a]), s * (Y[b] - Y[a])
            Ei = dx * (py - Y[a]) - dy * (px - X[a])       # = cross(b - a, p - a) with y pointing down, > 0 inside
            # E grows by -dy per step to the right and by dx per step down: a LEFT edge has the interior on its right (-dy > 0),
            # a TOP edge is horizontal with the interior below it (dy == 0, dx > 0)
            top_left = (-dy > 0) or (dy == 0 and dx > 0)
            owns_edge = top_left if fill == "top-left" else not top_left
            inside &= (Ei > 0) | ((Ei == 0) & owns_edge)
            closed &= Ei >= 0
            E.append(Ei)
        A = float(abs(area))
        invz = sum((E[i].astype(np.float64) / A) / Z[face[i]] for i in range(3))
        with np.errstate(divide="ignore", invalid="ignore"):
            z = 1.0 / invz
        for plane in (znear, zfar):
            assert not np.any(closed & (np.abs(z - plane) <= 1e-5 * plane)), "a fragment within 1e-5 of a depth plane: move the scene"
        in_range = (z >= znear) & (z <= zfar)
        on_edge = closed & in_range & ((E[0] == 0) | (E[1] == 0) | (E[2] == 0))
        sub = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        edge_count[sub] += on_edge
        edge_lo[sub] = np.where(on_edge & (edge_lo[sub] < 0), f, edge_lo[sub])
        edge_hi[sub] = np.where(on_edge, f, edge_hi[sub])
        frag = inside & in_range
        best, have = depth[sub], owner[sub] >= 0
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(have & frag, (z - best) / best, -1.0)
        # two fragments of one pixel are either tied (the same depth up to f64 noise) or at least 5e-8 apart (an f32 ulp just below 1)
        assert not np.any((np.abs(rel) > 1e-12) & (np.abs(rel) < 5e-8)), "depths too close to call in f32"
        tied = np.abs(rel) <= 1e-12
        wins = frag & (~have | (rel < -1e-12) | (tied if tie == "higher" else False))   # faces come in ascending id
        owner[sub] = np.where(wins, f, owner[sub])
        depth[sub] = np.where(wins, z, best)

    bgr = np.zeros((H, W, 3), np.float32)
    Ht, Wt = tex.shape[:2]
    fr = lambda a: Fraction(float(a))
    clamp = lambda i, n: min(max(i, 0), n - 1)
    row = (lambda ty: Ht - 1 - ty) if flip_rows else (lambda ty: ty)
    for y, x in zip(*np.nonzero(owner >= 0)):
        face = faces[owner[y, x]]
        X, Y = [int(a) for a in SX[face]], [int(a) for a in SY[face]]
        w = []
        for i in range(3):
            a, b = (i + 1) % 3, (i + 2) % 3
            Ei = (X[b] - X[a]) * (256 * int(y) - Y[a]) - (Y[b] - Y[a]) * (256 * int(x) - X[a])
            w.append(Fraction(Ei) / fr(verts[face[i], 2]))        # the sign of the orientation cancels in the quotient below
        tu = sum(w[i] * fr(uvs[face[i], 0]) for i in range(3)) / sum(w)
        tv = sum(w[i] * fr(uvs[face[i], 1]) for i in range(3)) / sum(w)
        if not tex_bilinear:
            tx, ty = clamp(int(np.floor(tu * Wt)), Wt), clamp(int(np.floor(tv * Ht)), Ht)
            rgb = [int(c) for c in tex[row(ty), tx]]
        else:
            xf, yf = tu * Wt - Fraction(1, 2), tv * Ht - Fraction(1, 2)
            xi, yi = int(np.floor(xf)), int(np.floor(yf))
            ax, ay = xf - xi, yf - yi
            xa, xb, ya, yb = clamp(xi, Wt), clamp(xi + 1, Wt), clamp(yi, Ht), clamp(yi + 1, Ht)
            rgb = []
            for c in range(3):
                p00, p01, p10, p11 = int(tex[row(ya), xa, c]), int(tex[row(ya), xb, c]), int(tex[row(yb), xa, c]), int(tex[row(yb), xb, c])
                top, bot = p00 + ax * (p01 - p00), p10 + ax * (p11 - p10)
                rgb.append(int(np.floor(top + ay * (bot - top))))    # the unlit path truncates to whole grey levels
        bgr[y, x] = rgb[::-1]
    mask = (depth > mask_thr).astype(np.float32)
    ys, xs = np.nonzero(mask)
    bbox = [int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())] if len(xs) else [W, -1, H, -1]
    return Rendered(owner, depth, bgr, mask, bbox, dict(edge_count=edge_count, edge_lo=edge_lo, edge_hi=edge_hi))


# ------------------------------------------------------------------------------------------------- face identity by colour

def face_colour(f):
    """(r, g, b) of face f in the 1 x nf texture: never black, so background (0, 0, 0) names no face"""
    return (1 + f % 200, 1 + f // 200, 200)


def per_face_texels(verts, faces):
    """duplicate the vertices per face (keeping each face's vertex order), give face f texel f of a 1 x nf texture of distinct colours
    and put its three uvs on that texel's centre -> verts (3 nf, 3), uvs (3 nf, 2), faces (nf, 3), tex (1, nf, 3) uint8.  Under the
    nearest filter the rendered colour then names the face that won the pixel (`owner_from_bgr`)."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int64)
    nf = len(faces)
    assert nf <= 200 * 255
    v = verts[faces.reshape(-1)]
    uv = np.stack([np.repeat((np.arange(nf) + 0.5) / nf, 3), np.full(3 * nf, 0.5)], axis=1).astype(np.float32)
    tex = np.array([[face_colour(f) for f in range(nf)]], np.uint8)
    return v, uv, np.arange(3 * nf, dtype=np.int32).reshape(nf, 3), tex


def owner_from_bgr(bgr):
    """(..., 3) BGR of a nearest-filter render of a `per_face_texels` mesh -> face id, -1 where the pixel is background"""
    bgr = np.asarray(bgr)
    b, g, r = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    return np.where(b == 0, -1, (r - 1) + 200 * (g - 1)).astype(np.int64)


# -------------------------------------------------------------------------------------------------------------- the scenes

def _at(px, py, Z=1.0):
    """camera-frame points that project to pixel coordinates (px, py) under RK at depth Z"""
    px, py, Z = np.broadcast_arrays(np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(Z, np.float64))
    P = np.stack([(px - float(RK[0, 2])) / 64.0 * Z, (py - float(RK[1, 2])) / 64.0 * Z, Z], axis=-1)
    assert np.all(P.astype(np.float32).astype(np.float64) == P), "a scene vertex that f32 cannot hold"
    return P.astype(np.float32)


def _grid_faces(nx, ny, seed):
    """nx x ny quads over an (ny + 1) x (nx + 1) vertex grid (row-major), two triangles each: the diagonal alternates like a chess
    board, each triangle's winding is drawn at random and the face order is shuffled, all from `seed`"""
    rng = np.random.default_rng(seed)
    faces = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            pair = [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
            faces += [t if rng.random() < 0.5 else t[::-1] for t in pair]
    faces = np.asarray(faces, np.int32)
    assert len({tuple(np.roll(t, -np.argmin(t))) for t in faces.tolist()}) == len(faces)
    return faces[rng.permutation(len(faces))]


def _scene(name, verts, faces, uvs=None, tex=None):
    if uvs is None:
        verts, uvs, faces, tex = per_face_texels(verts, faces)
    return dict(name=name, verts=np.ascontiguousarray(verts, np.float32), uvs=np.ascontiguousarray(uvs, np.float32),
                faces=np.ascontiguousarray(faces, np.int32), tex=np.ascontiguousarray(tex, np.uint8), per_face=name != "texels")


def build_fill_rule():
    """9 x 8 quads at Z = 1.  Grid lines on whole pixels (centres exactly on an edge), on half pixels and on n + 1/512 (the snapping
    tie: floor(u * 256 + 0.5) puts the line 1/256 right of centre n, floor(u * 256) puts it on the centre); the first line of each
    axis is negative and the last lies beyond the right / bottom edge of both frames."""
    xs = [-2.5, 3.0, 7.5, 12 + 1 / 512, 17.0, 22.5, 27 + 1 / 512, 33.0, 40.5, 50.25]
    ys = [-1.5, 2.0, 6.5, 10 + 1 / 512, 15.0, 19.5, 24 + 1 / 512, 28.0, 34.25]
    gx, gy = np.meshgrid(xs, ys)
    sc = _scene("fill_rule", _at(gx.reshape(-1), gy.reshape(-1)), _grid_faces(len(xs) - 1, len(ys) - 1, seed=7))
    for H, W in FRAMES:
        assert xs[-1] > W - 1 and ys[-1] > H - 1
        r = render_rules(sc["verts"], sc["uvs"], sc["faces"], sc["tex"], RK, H, W, ZNEAR, ZFAR)
        n_edge = int((r.info["edge_count"] >= 1).sum())
        shared = (r.info["edge_count"] == 2) & (r.info["edge_hi"] > r.info["edge_lo"])
        n_higher = int((shared & (r.owner == r.info["edge_hi"])).sum())
        assert n_edge >= 20, n_edge            # pixel centres exactly on an edge
        assert n_higher >= 5, n_higher         # ... that belong to the higher-numbered of the two faces sharing it
        sc["edge_pixels_{}x{}".format(H, W)] = (n_edge, n_higher)
    return sc


TIE_IDS = (4, 1, 7)


def _x_under(m, Z):
    """an f32 X with X / Z == m in f32, for a Z one ulp off a power of two (m * Z itself is not an f32 then)"""
    m32, Z32 = np.float32(m), np.float32(Z)
    x = np.float32(np.float64(m32) * np.float64(Z32))
    for cand in (x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))):
        if np.float32(cand / Z32) == m32:
            return cand
    raise AssertionError("no f32 X projects to {} at Z = {}".format(m, Z))


def build_z_ties():
    """Three coincident right triangles (legs 16 px on whole pixels at Z = 1: twice the area is 2^24 sub-pixel units, so every
    barycentric and the interpolated depth are exact in f32 whatever the vertex order, and the tie is a tie of bits) under ids 4, 1 and
    7 with permuted vertex orders.  Face 8, the highest id, is the half-size triangle at the same corner one f32 ulp NEARER; face 0 is
    the full triangle one ulp FARTHER.  Faces 2, 3, 5, 6 are unrelated."""
    tri = [(6, 4), (22, 4), (6, 20)]
    half = [(6, 4), (14, 4), (6, 12)]
    z_near, z_far = float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2)))

    def at_ulp(p, Z):
        return [[_x_under((x - float(RK[0, 2])) / 64.0, Z), _x_under((y - float(RK[1, 2])) / 64.0, Z), np.float32(Z)] for x, y in p]

    def flat(p):
        return _at([q[0] for q in p], [q[1] for q in p]).tolist()

    other = [[(26, 2), (34, 2), (26, 10)], [(27, 12), (35, 12), (35, 20)], [(26, 21), (31, 21), (26, 27)], [(2, 22), (12, 22), (2, 28)]]
    order = {1: (0, 1, 2), 4: (1, 2, 0), 7: (2, 1, 0)}
    tris = {0: at_ulp(tri, z_far), 8: at_ulp(half, z_near), 2: flat(other[0]), 3: flat(other[1]), 5: flat(other[2]), 6: flat(other[3])}
    for i, o in order.items():
        tris[i] = [flat(tri)[k] for k in o]
    verts = np.asarray([p for i in range(9) for p in tris[i]], np.float32)
    sc = _scene("z_ties", verts, np.arange(27).reshape(9, 3))
    for H, W in FRAMES:
        r = render_rules(sc["verts"], sc["uvs"], sc["faces"], sc["tex"], RK, H, W, ZNEAR, ZFAR)
        ys, xs = np.mgrid[0:H, 0:W]
        in_tri = (xs >= 6) & (ys >= 4) & ((xs - 6) + (ys - 4) < 16)     # top-left rule: the hypotenuse is neither top nor left
        in_half = (xs >= 6) & (ys >= 4) & ((xs - 6) + (ys - 4) < 8)
        assert np.all(r.owner[in_half] == 8) and np.all(r.owner[in_tri & ~in_half] == 1)
        assert in_half.sum() == 36 and (in_tri & ~in_half).sum() == 100
        assert not np.isin(r.owner, (0, 4, 7)).any()
    return sc


def build_degenerate():
    """faces that must draw nothing (two coincident vertices; three collinear vertices; a sliver strictly between two pixel columns; a
    sub-pixel triangle that holds no centre) next to faces that draw little (a sliver whose left edge runs exactly through the centres
    of column 15; a sub-pixel triangle around one centre)"""
    tris = [[(3, 3), (3, 3), (9, 8)],                      # 0: coincident vertices
            [(2, 12), (6, 14), (10, 16)],                  # 1: collinear
            [(10.25, 2), (10.75, 2), (10.5, 12)],          # 2: between columns 10 and 11
            [(15, 2.5), (15.5, 7), (15, 11.5)],            # 3: left edge on column 15 -> rows 3 .. 11 of it
            [(19.75, 4.75), (20.5, 4.875), (19.875, 5.5)],   # 4: holds the centre (20, 5)
            [(24.25, 5.25), (24.75, 5.375), (24.375, 5.75)]]   # 5: holds none
    p = np.asarray(tris, np.float64).reshape(-1, 2)
    sc = _scene("degenerate", _at(p[:, 0], p[:, 1]), np.arange(18).reshape(6, 3))
    for H, W in FRAMES:
        r = render_rules(sc["verts"], sc["uvs"], sc["faces"], sc["tex"], RK, H, W, ZNEAR, ZFAR)
        assert 0 < (r.owner >= 0).sum() <= 40
        want = np.full((H, W), -1)
        want[3:12, 15] = 3
        want[5, 20] = 4
        assert np.array_equal(r.owner, want)
    return sc


def build_frame_clamp():
    """face 1 spans 1.8 million pixels around the frame (edge products of 1e17: the 64-bit edge functions), tilted (Z = 1, 4, 2 at its
    vertices), and covers every pixel; face 0 is nearer (Z = 0.5) and would cover every pixel too, but one of its vertices projects
    beyond 1e6 px, so it is dropped whole"""
    big = _at([-9e5, 9e5, 0], [-9e5, -9e5, 9e5], [1.0, 4.0, 2.0])
    lost = _at([-9e5, 1.2e6, 0], [-9e5, -9e5, 9e5], 0.5)
    sc = _scene("frame_clamp", np.concatenate([lost, big]), np.arange(6).reshape(2, 3))
    for H, W in FRAMES:
        r = render_rules(sc["verts"], sc["uvs"], sc["faces"], sc["tex"], RK, H, W, ZNEAR, ZFAR)
        assert np.all(r.owner == 1) and r.depth.max() - r.depth.min() > 1e-5
    return sc


def build_depth_range():
    """a tilted quad with vertex depths 0.25 (= znear exactly: still the screen-space path), 6, 5 and 0.5, so its fragments run from
    just behind the near plane to beyond zfar = 2 and the far ones are discarded per fragment.  (No fragment of a face whose vertices
    all lie at Z >= znear can be nearer than znear -- 1/z is a convex combination of the vertices' -- so only the far plane cuts.)
    `render_rules` asserts that no pixel comes within 1e-5 (relative) of either plane, so f32 rounding cannot move one across."""
    corners = _at([3.5, 28.0, 28.0, 3.5], [4.0, 4.0, 24.0, 24.0], [0.25, 6.0, 5.0, 0.5])
    sc = _scene("depth_range", corners, [[0, 1, 2], [2, 3, 0]])
    for H, W in FRAMES:
        r = render_rules(sc["verts"], sc["uvs"], sc["faces"], sc["tex"], RK, H, W, ZNEAR, 100.0)
        cut = render_rules(sc["verts"], sc["uvs"], sc["faces"], sc["tex"], RK, H, W, ZNEAR, ZFAR)
        lost = (r.owner >= 0) & (cut.owner < 0)
        assert lost.sum() >= 20 and (cut.owner >= 0).sum() >= 200 and np.all(r.depth[lost] > ZFAR)
        assert cut.depth[cut.owner >= 0].min() < 0.26 and cut.depth.max() > 1.9
    return sc


def build_texels():
    """an 8 x 6 texture of distinct colours (row 0 is the top of the picture) on two quads at Z = 1.
    Quad A (corners on half pixels) covers the pixels 4..11 x 3..8 one texel per pixel: every centre lies exactly on a texel centre, so both filters must return
    the texel.  (In f32 the texel coordinate of a centre is off by up to 3e-6; neighbouring texels differ by one grey level and all
    levels lie in [128, 256), where f32 steps by 1.5e-5, so the bilinear blend rounds back to the texel itself.)
    Quad B (16 x 8 px: twice its area is a power of two and its uvs are dyadic, so f32 is exact) maps u = -0.25 .. 0.75 at two pixels
    per texel -- centres alternate between texel centres and texel borders, where nearest takes the right-hand texel and bilinear
    floors the half-way blend -- and v = 1.25 .. 0.25 at 3/4 texel per pixel; a quarter of each axis is clamped to the edge texel."""
    r_, c_ = np.mgrid[0:6, 0:8]
    tex = np.stack([130 + c_, 140 + r_, 150 + c_ + r_], axis=-1).astype(np.uint8)
    assert len({tuple(t) for t in tex.reshape(-1, 3).tolist()}) == 48
    verts = _at([3.5, 11.5, 11.5, 3.5, 16, 32, 32, 16], [2.5, 2.5, 8.5, 8.5, 12, 12, 20, 20])
    uvs = np.array([[0, 1], [1, 1], [1, 0], [0, 0], [-0.25, 1.25], [0.75, 1.25], [0.75, 0.25], [-0.25, 0.25]], np.float32)
    sc = _scene("texels", verts, [[0, 1, 2], [0, 2, 3], [4, 5, 6], [6, 7, 4]], uvs=uvs, tex=tex)
    for H, W in FRAMES:
        for bil in (False, True):
            r = render_rules(sc["verts"], sc["uvs"], sc["faces"], sc["tex"], RK, H, W, ZNEAR, ZFAR, tex_bilinear=bil)
            assert np.array_equal(r.bgr[3:9, 4:12], tex[:, :, ::-1].astype(np.float32))     # quad A: the texture itself, row 0 on top
            assert (r.owner >= 0).sum() == 48 + 128
    return sc


def build_nothing():
    """a sample that draws nothing: a face beyond zfar, a face left of the frame and a face without area"""
    v = np.concatenate([_at([5, 25, 15], [5, 5, 25], 3.0), _at([-20, -4, -12], [3, 3, 20]), _at([8, 12, 16], [8, 12, 16])])
    sc = _scene("nothing", v, np.arange(9).reshape(3, 3))
    for H, W in FRAMES:
        assert render_rules(sc["verts"], sc["uvs"], sc["faces"], sc["tex"], RK, H, W, ZNEAR, ZFAR).bbox == [W, -1, H, -1]
    return sc


@functools.lru_cache(maxsize=None)
def exact_scenes():
    """the exact scenes in the order of their class ids in the GPU test's mesh table"""
    return tuple(b() for b in (build_fill_rule, build_z_ties, build_degenerate, build_frame_clamp, build_depth_range, build_texels,
                               build_nothing))


def scene(name):
    return {s["name"]: s for s in exact_scenes()}[name]


@functools.lru_cache(maxsize=None)
def expected(name, H, W, tex_bilinear=False, **wrong):
    """render_rules of a scene under the shared camera and depth range, computed once and shared; treat it as read-only"""
    s = scene(name)
    return render_rules(s["verts"], s["uvs"], s["faces"], s["tex"], RK, H, W, ZNEAR, ZFAR, tex_bilinear=tex_bilinear, **wrong)


# --------------------------------------------------------------------------------------------------------------- near plane

NEAR_H, NEAR_W = 48, 64
NEAR_K = np.array([[110.0, 0, 31.5], [0, 110.0, 23.5], [0, 0, 1]], np.float32)   # LK of tests/test_gpu_raster_dispatch.py
NEAR_ZNEAR, NEAR_ZFAR = 0.25, 6.0


def _rx(a):
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def _ry(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


@functools.lru_cache(maxsize=None)
def near_cut():
    """A flat square patch (9 x 9 vertices, side 0.5 m, model plane z = 0, split like fill_rule) under two poses that carry it across
    the near plane, the second one behind the eye.  The expected answer is analytic: pixel (x, y) sees the patch where its ray meets
    the patch's plane inside the square at 0.25 <= z <= 6.
    -> dict(verts, uvs, faces, tex, poses (2,3,4) f32, inside / interior / allowed (2,H,W) bool): `interior` = the whole 3x3
    neighbourhood of ray hits lies inside (every such pixel must be drawn), `allowed` = some hit of the 3x3 neighbourhood lies inside
    (no other pixel may be drawn)."""
    g = np.linspace(-0.25, 0.25, 9)
    gx, gy = np.meshgrid(g, g)
    verts = np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(81)], axis=1).astype(np.float32)
    v, uv, f, tex = per_face_texels(verts, _grid_faces(8, 8, seed=11))
    poses = np.stack([np.concatenate([_rx(1.2) @ _ry(0.3), [[0.01], [-0.005], [0.27]]], axis=1),
                      np.concatenate([_rx(0.4) @ _ry(1.3), [[0.01], [-0.005], [0.2]]], axis=1)]).astype(np.float32)
    K = NEAR_K.astype(np.float64)
    ys, xs = np.mgrid[-1:NEAR_H + 1, -1:NEAR_W + 1].astype(np.float64)      # one ring of rays around the frame
    d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], axis=-1)
    out = dict(verts=v, uvs=uv, faces=f, tex=tex, poses=poses, inside=[], interior=[], allowed=[])
    for P in poses.astype(np.float64):
        R, t = P[:, :3], P[:, 3]
        zc = verts.astype(np.float64) @ R[2] + t[2]
        assert zc.min() < NEAR_ZNEAR < zc.max()
        n = R[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (n @ t) / (d @ n)                      # the ray s * d meets the plane n . (p - t) = 0; its depth is s
        q = (s[..., None] * d - t) @ R                 # model coordinates of the hit
        hit = np.isfinite(s) & (s >= NEAR_ZNEAR) & (s <= NEAR_ZFAR) & (np.abs(q[..., 0]) <= 0.25) & (np.abs(q[..., 1]) <= 0.25)
        nb = np.stack([hit[1 + dy:1 + dy + NEAR_H, 1 + dx:1 + dx + NEAR_W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
        out["inside"].append(hit[1:-1, 1:-1])
        out["interior"].append(nb.all(axis=0))
        out["allowed"].append(nb.any(axis=0))
        assert out["interior"][-1].sum() >= 400
    for k in ("inside", "interior", "allowed"):
        out[k] = np.stack(out[k])
    return out


def near_cut_faults(depth, b):
    """(interior pixels left undrawn, pixels drawn where no neighbouring ray meets the patch) of sample b's depth plane"""
    nc = near_cut()
    drawn = np.asarray(depth) > 0
    return int((nc["interior"][b] & ~drawn).sum()), int((drawn & ~nc["allowed"][b]).sum())
