"""numpy restatement of the lightmaps (csrc/pt_lightmap.h), for tests/test_lightmap_host.py and tests/test_gpu_lightmap.py.

Coverage is integer arithmetic (int64) and exact.  Everything else is float32 in the order the header writes it (numpy's + - * / sqrt on float32 arrays are
correctly rounded; `_fma` of lens_reference.py is the single rounding).  pcg, seed_hash, path_key, rng_f and sincos2pi are lens_reference.py's: the header
calls csrc/pt_device.h's, as the lens and the probes do.

Also here: the float64 yardsticks of the closed-form tests (point-to-rectangle form factors) and the reference's own sampler for checking a test's size and
seed on the CPU."""
import numpy as np

from lens_reference import F32, F64, U64, _fma, path_key, rng_f, seed_hash, sincos2pi  # noqa: F401

NONE = np.uint32(0xFFFFFFFF)
PI32 = F32(3.1415927)
I64 = np.int64


# ---- coverage -------------------------------------------------------------------------------------------------------------------------------------
def fixed(u, side):
    """pt_lm_fixed: clamp to [0, 1], (int)rintf((u * side) * 256)."""
    c = np.minimum(np.maximum(np.asarray(u, F32), F32(0.0)), F32(1.0))
    return np.rint((c * F32(side)) * F32(256.0)).astype(I64)


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _tri(uv3, w, h):
    x, y = fixed(uv3[:, 0], w), fixed(uv3[:, 1], h)
    return x, y, _orient(x[0], y[0], x[1], y[1], x[2], y[2])


def _edges(x, y, area, px, py):
    """The oriented edge values (e0, e1, e2) at the points (px, py) (int64 arrays) and the covered mask."""
    e0 = _orient(x[1], y[1], x[2], y[2], px, py)
    e1 = _orient(x[2], y[2], x[0], y[0], px, py)
    e2 = _orient(x[0], y[0], x[1], y[1], px, py)
    if area < 0:
        e0, e1, e2 = -e0, -e1, -e2
    return e0, e1, e2, (area != 0) & (e0 >= 0) & (e1 >= 0) & (e2 >= 0)


def cover(indices, uv, w, h):
    """ptc_debug_lightmap_cover: the owner image (h, w) uint32.  Every triangle is tested at every centre of the atlas: no bounding box, so the box of the
    header is held to the exhaustive test."""
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    uv = np.asarray(uv, F32).reshape(-1, 2)
    px, py = np.meshgrid((2 * np.arange(w, dtype=I64) + 1) * 128, (2 * np.arange(h, dtype=I64) + 1) * 128)
    owner = np.full((h, w), NONE, np.uint32)
    for t in range(idx.shape[0] - 1, -1, -1):      # descending: the lowest index is written last
        x, y, area = _tri(uv[idx[t]], w, h)
        if area == 0:
            continue
        owner[_edges(x, y, area, px, py)[3]] = t
    return owner


# ---- texel records --------------------------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return _fma(a[..., 2], b[..., 2], _fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def cross3(a, b):
    return np.stack([_fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), _fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     _fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1).astype(F32)


def normalize3(a):
    with np.errstate(all="ignore"):
        inv = F32(1.0) / np.sqrt(dot3(a, a))
        return (a * inv[..., None]).astype(F32)


def _bary(a0, a1, a2, w0, w1, w2):
    return np.stack([_fma(a2[..., c], w2, _fma(a1[..., c], w1, a0[..., c] * w0)) for c in range(3)], -1).astype(F32)


def texels(indices, uv, positions, normals, w, h, ray_eps):
    """The texel list of pt_lightmap.h for an instance with the world `positions` / `normals` (n_verts, 3): dict(atlas_index, prim, origin, normal, dropped)."""
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    uv = np.asarray(uv, F32).reshape(-1, 2)
    P, Nn = np.asarray(positions, F32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3)
    owner = cover(idx, uv, w, h).reshape(-1)
    a = np.nonzero(owner != NONE)[0]
    tri = owner[a].astype(np.int64)
    p0, p1, p2 = P[idx[tri, 0]], P[idx[tri, 1]], P[idx[tri, 2]]
    ng = normalize3(cross3(p1 - p0, p2 - p0))
    keep = np.isfinite(ng).all(-1)
    dropped = int((~keep).sum())
    a, tri, p0, p1, p2, ng = a[keep], tri[keep], p0[keep], p1[keep], p2[keep], ng[keep]
    e = np.zeros((3, a.size), I64)
    px, py = (2 * (a % w).astype(I64) + 1) * 128, (2 * (a // w).astype(I64) + 1) * 128
    for t in np.unique(tri):
        m = tri == t
        x, y, area = _tri(uv[idx[t]], w, h)
        e[0, m], e[1, m], e[2, m], cov = _edges(x, y, area, px[m], py[m])
        assert cov.all()
    A = (e[0] + e[1] + e[2]).astype(F32)
    w0, w1 = e[0].astype(F32) / A, e[1].astype(F32) / A
    w2 = (F32(1.0) - w0) - w1
    Pt = _bary(p0, p1, p2, w0, w1, w2)
    ns = normalize3(_bary(Nn[idx[tri, 0]], Nn[idx[tri, 1]], Nn[idx[tri, 2]], w0, w1, w2))
    ns = np.where(np.isfinite(ns).all(-1)[:, None], ns, ng)
    ngo = np.where((dot3(ng, ns) < 0)[:, None], -ng, ng)
    origin = _fma(ngo, F32(ray_eps), Pt).astype(F32)
    return dict(atlas_index=a.astype(np.uint32), prim=tri.astype(np.uint32), origin=origin, normal=ns.astype(F32), dropped=dropped)


# ---- rays -----------------------------------------------------------------------------------------------------------------------------------------
def onb(n):
    sg = np.copysign(F32(1.0), n[..., 2])
    with np.errstate(all="ignore"):
        a = F32(-1.0) / (sg + n[..., 2])
        bb = n[..., 0] * n[..., 1] * a
        t = np.stack([_fma(sg * n[..., 0], n[..., 0] * a, F32(1.0)), sg * bb, -sg * n[..., 0]], -1)
        b = np.stack([bb, _fma(n[..., 1], n[..., 1] * a, sg), -n[..., 1]], -1)
    return t.astype(F32), b.astype(F32)


def dirs(seed, idx, sample, n):
    """(d (.., 3), key, u1) of pt_lm_dir for the texel indices idx (= base + atlas index), the samples and the unit normals n (broadcast)."""
    key = path_key(seed_hash(seed), np.asarray(idx, U64), np.asarray(sample, U64))
    u1, u2 = rng_f(key, 0, 0), rng_f(key, 0, 1)
    r, z = np.sqrt(u1), np.sqrt(np.maximum(F32(1.0) - u1, F32(0.0)))
    sn, co = sincos2pi(u2)
    n = np.broadcast_to(np.asarray(n, F32), key.shape + (3,))
    tx, ty = onb(n)
    v = _fma(tx, (r * co)[..., None], _fma(ty, (r * sn)[..., None], n * z[..., None]))
    inv = F32(1.0) / np.sqrt(_fma(v[..., 2], v[..., 2], _fma(v[..., 1], v[..., 1], v[..., 0] * v[..., 0])))
    return (v * inv[..., None]).astype(F32), key.astype(np.uint32), u1


def rays(tex, base, seed, first_sample, n_samples):
    """ptc_debug_lightmap_rays: (origins, dirs, keys) of n_samples * n rays in path order p = sample_local * n + entry, for the list `tex` of texels()."""
    n = tex["atlas_index"].size
    idx = np.tile(tex["atlas_index"].astype(U64) + U64(base), n_samples)
    smp = np.repeat(np.arange(n_samples, dtype=U64) + U64(first_sample), n)
    d, key, _ = dirs(seed, idx, smp, np.tile(tex["normal"], (n_samples, 1)))
    return np.tile(tex["origin"], (n_samples, 1)), d, key


# ---- resolve and dilation -----------------------------------------------------------------------------------------------------------------------------
def resolve(acc, n_samples):
    """E = sum * (pi / (float)N): the scale is rounded once, then the product."""
    return (np.asarray(acc, F32) * (PI32 / F32(n_samples))).astype(F32)


_NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def dilate(img, iters):
    """ptc_debug_lightmap_dilate: `iters` iterations over the (H, W, 4) image, each reading the previous one only."""
    a = np.array(img, F32)
    h, w = a.shape[:2]
    for _ in range(iters):
        pad = np.zeros((h + 2, w + 2, 4), F32)
        pad[1:-1, 1:-1] = a
        s = np.zeros((h, w, 3), F32)
        cnt = np.zeros((h, w), np.int32)
        for dx, dy in _NEIGHBOURS:
            q = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            m = q[..., 3] != 0
            s = np.where(m[..., None], s + q[..., :3], s).astype(F32)
            cnt += m
        fill = (a[..., 3] == 0) & (cnt > 0)
        with np.errstate(all="ignore"):
            mean = (s / cnt.astype(F32)[..., None]).astype(F32)
        b = a.copy()
        b[fill, :3] = mean[fill]
        b[fill, 3] = F32(0.5)
        a = b
    return a


# ---- float64 yardsticks -------------------------------------------------------------------------------------------------------------------------------
def rect_form_factor(p, n, corners):
    """The point-to-polygon form factor (the fraction of the cosine-weighted hemisphere of n at p that the planar polygon `corners` (k, 3) fills), float64, by the
    contour integral F = 1 / (2 pi) sum_i gamma_i (n . g_i): gamma_i the angle the edge i subtends at p, g_i the unit normal of the plane through p and the
    edge.  The polygon must lie wholly above the plane of n through p; the sign is that of the winding, so the absolute value is returned."""
    p, n, c = np.asarray(p, F64), np.asarray(n, F64), np.asarray(corners, F64)
    r = c - p[..., None, :]
    r = r / np.linalg.norm(r, axis=-1, keepdims=True)
    F = 0.0
    k = c.shape[0]
    for i in range(k):
        a, b = r[..., i, :], r[..., (i + 1) % k, :]
        g = np.cross(a, b)
        gl = np.linalg.norm(g, axis=-1)
        gamma = np.arctan2(gl, (a * b).sum(-1))
        F = F + gamma * (g * n).sum(-1) / np.where(gl > 0, gl, 1.0)
    return np.abs(F) / (2 * np.pi)


def sampled_fraction(tex, base, seed, n_samples, hits):
    """The reference's own sampler: per entry the fraction of its n_samples directions (samples 0 .. n_samples - 1) for which hits(origins, dirs) is true."""
    o, d, _ = rays(tex, base, seed, 0, n_samples)
    n = tex["atlas_index"].size
    return hits(o.astype(F64), d.astype(F64)).reshape(n_samples, n).mean(0)
