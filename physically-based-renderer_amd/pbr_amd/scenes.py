"""Procedural stand-ins for BASELINE.json's configs.

The reference's assets are stripped from the checkout (`.MISSING_LARGE_BLOBS:1-3`:
assets/models/test_scene.glb and two textures), so every benchmark scene is generated here,
deterministically, as float32 arrays that are handed unchanged to the C-ABI (and, in tests, to the
oracle).  All geometry is glTF-convention: y up, right-handed, CCW front faces.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np

from .scene import MESH_VERTEX, CameraDesc, InstanceDesc, Material, MeshDesc, SceneDesc

_ID_Q = (1.0, 0.0, 0.0, 0.0)


def _verts(pos, nrm, tan, uv) -> np.ndarray:
    n = len(pos)
    v = np.zeros(n, MESH_VERTEX)
    v["position"] = np.asarray(pos, np.float32)
    v["normal"] = np.asarray(nrm, np.float32)
    t = np.asarray(tan, np.float32)
    if t.shape[-1] == 3:
        t = np.concatenate([t, np.ones((n, 1), np.float32)], axis=1)
    v["tangent"] = t
    v["texCoords"] = np.asarray(uv, np.float32)
    return v


def grid_patch(origin, du, dv, nu: int, nv: int, displace=None) -> Tuple[np.ndarray, np.ndarray]:
    """(nu × nv)-cell parallelogram patch: origin + s·du + t·dv, normal = normalize(du × dv).
    `displace(P[n,3]) -> h[n]` moves vertices along the normal (normals recomputed by finite differences)."""
    o = np.asarray(origin, np.float64)
    du = np.asarray(du, np.float64)
    dv = np.asarray(dv, np.float64)
    s, t = np.meshgrid(np.linspace(0.0, 1.0, nu + 1), np.linspace(0.0, 1.0, nv + 1), indexing="xy")
    s = s.reshape(-1)
    t = t.reshape(-1)
    P = o[None, :] + s[:, None] * du[None, :] + t[:, None] * dv[None, :]
    n = np.cross(du, dv)
    n /= np.linalg.norm(n)
    N = np.repeat(n[None, :], P.shape[0], axis=0)
    tu = du / np.linalg.norm(du)
    if displace is not None:
        h = displace(P)
        eps = 1e-3
        hu = displace(P + eps * tu[None, :])
        tv = dv / np.linalg.norm(dv)
        hv = displace(P + eps * tv[None, :])
        P = P + h[:, None] * n[None, :]
        gu = (hu - h) / eps
        gv = (hv - h) / eps
        N = n[None, :] - gu[:, None] * tu[None, :] - gv[:, None] * tv[None, :]
        N /= np.linalg.norm(N, axis=1, keepdims=True)
    T = np.repeat(tu[None, :], P.shape[0], axis=0)
    uv = np.stack([s, t], axis=1)
    i0 = (np.arange(nv)[:, None] * (nu + 1) + np.arange(nu)[None, :]).reshape(-1)
    i1 = i0 + 1
    i2 = i0 + (nu + 1)
    i3 = i2 + 1
    idx = np.stack([i0, i1, i3, i0, i3, i2], axis=1).reshape(-1).astype(np.uint32)  # CCW seen from +n
    return _verts(P, N, T, uv), idx


def uv_sphere(nu: int, nv: int, radius: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """nu longitudinal × nv latitudinal segments; 2·nu·(nv−1) triangles (poles are fans)."""
    pos, nrm, tan, uv = [], [], [], []
    for j in range(nv + 1):
        th = math.pi * j / nv
        for i in range(nu + 1):
            ph = 2.0 * math.pi * i / nu
            n = (math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph))
            pos.append([radius * c for c in n])
            nrm.append(n)
            tan.append((-math.sin(ph), 0.0, math.cos(ph)))
            uv.append((i / nu, j / nv))
    idx = []
    for j in range(nv):
        for i in range(nu):
            a = j * (nu + 1) + i
            b = a + 1
            c = a + (nu + 1)
            d = c + 1
            if j != 0:
                idx += [a, b, c]
            if j != nv - 1:
                idx += [b, d, c]
    return _verts(pos, nrm, tan, uv), np.asarray(idx, np.uint32)


def cylinder(sides: int, segs: int, radius: float, height: float) -> Tuple[np.ndarray, np.ndarray]:
    """Open cylinder around +y from y=0 to y=height; 2·sides·segs triangles, outward normals."""
    ph = 2.0 * np.pi * np.arange(sides + 1) / sides
    y = height * np.arange(segs + 1) / segs
    PH, Y = np.meshgrid(ph, y, indexing="xy")
    PH = PH.reshape(-1)
    Y = Y.reshape(-1)
    N = np.stack([np.cos(PH), np.zeros_like(PH), np.sin(PH)], axis=1)
    P = N * radius
    P[:, 1] = Y
    T = np.stack([-np.sin(PH), np.zeros_like(PH), np.cos(PH)], axis=1)
    uv = np.stack([PH / (2.0 * np.pi), Y / height], axis=1)
    i0 = (np.arange(segs)[:, None] * (sides + 1) + np.arange(sides)[None, :]).reshape(-1)
    i1 = i0 + 1
    i2 = i0 + (sides + 1)
    i3 = i2 + 1
    idx = np.stack([i0, i2, i3, i0, i3, i1], axis=1).reshape(-1).astype(np.uint32)
    return _verts(P, N, T, uv), idx


def half_torus(major: float, minor: float, seg_major: int, seg_minor: int) -> Tuple[np.ndarray, np.ndarray]:
    """Arch: upper half of a torus in the xy-plane (spans x ∈ [−major, major], apex at y = major)."""
    a = np.pi * np.arange(seg_major + 1) / seg_major
    b = 2.0 * np.pi * np.arange(seg_minor + 1) / seg_minor
    A, B = np.meshgrid(a, b, indexing="xy")
    A = A.reshape(-1)
    B = B.reshape(-1)
    cx, cy = np.cos(A), np.sin(A)
    N = np.stack([np.cos(B) * cx, np.cos(B) * cy, np.sin(B)], axis=1)
    P = np.stack([major * cx, major * cy, np.zeros_like(A)], axis=1) + minor * N
    T = np.stack([-cy, cx, np.zeros_like(A)], axis=1)
    uv = np.stack([A / np.pi, B / (2.0 * np.pi)], axis=1)
    i0 = (np.arange(seg_minor)[:, None] * (seg_major + 1) + np.arange(seg_major)[None, :]).reshape(-1)
    i1 = i0 + 1
    i2 = i0 + (seg_major + 1)
    i3 = i2 + 1
    idx = np.stack([i0, i1, i3, i0, i3, i2], axis=1).reshape(-1).astype(np.uint32)
    return _verts(P, N, T, uv), idx


def _quad(a, b, c, d) -> Tuple[np.ndarray, np.ndarray]:
    """Quad a,b,c,d CCW seen from its front; 2 triangles (a,b,c),(a,c,d)."""
    a, b, c, d = (np.asarray(p, np.float64) for p in (a, b, c, d))
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    t = (b - a) / np.linalg.norm(b - a)
    v = _verts([a, b, c, d], [n] * 4, [t] * 4, [(0, 0), (1, 0), (1, 1), (0, 1)])
    return v, np.asarray([0, 1, 2, 0, 2, 3], np.uint32)


# ----------------------------------------------------------------------------------------------
def cornell_box() -> SceneDesc:
    """Config 1: 5 Lambert wall quads + 1 ceiling emitter quad = 12 triangles,
    box [−1,1]³ open towards +z, camera on +z looking down −z, fovY 40°."""
    mats = [
        Material((0.73, 0.73, 0.73, 1.0), 0.0, 1.0),
        Material((0.65, 0.05, 0.05, 1.0), 0.0, 1.0),
        Material((0.12, 0.45, 0.15, 1.0), 0.0, 1.0),
        Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (15.0, 15.0, 15.0)),
    ]
    q = []
    q.append((_quad((-1, -1, 1), (1, -1, 1), (1, -1, -1), (-1, -1, -1)), 0))  # floor, normal +y
    q.append((_quad((-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)), 0))  # ceiling, normal −y
    q.append((_quad((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)), 0))  # back, normal +z
    q.append((_quad((-1, -1, 1), (-1, -1, -1), (-1, 1, -1), (-1, 1, 1)), 1))  # left (x=−1), normal +x
    q.append((_quad((1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)), 2))  # right (x=+1), normal −x
    e = 0.25
    q.append((_quad((-e, 0.998, -e), (e, 0.998, -e), (e, 0.998, e), (-e, 0.998, e)), 3))  # light, normal −y
    meshes = [MeshDesc(v, i, m) for (v, i), m in q]
    inst = [InstanceDesc(k, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0)) for k in range(len(meshes))]
    d = 1.0 / math.tan(math.radians(20.0))
    cam = CameraDesc((0.0, 0.0, 1.0 + d), (0.0, 0.0, 0.0), math.radians(40.0), 1.0)
    return SceneDesc(mats, meshes, inst, cam, "cornell")


def sphere_scene(nu: int = 100, nv: int = 51) -> SceneDesc:
    """Config 2: one ~10 k-triangle UV sphere (metallic 1, roughness 0.3, base (0.9,0.6,0.2)) instanced
    with a rotation and a non-uniform scale (exercises R3's inverse-transpose), a diffuse ground quad
    grid and one emissive quad.  100×51 segments → 2·100·50 = 10 000 sphere triangles."""
    mats = [
        Material((0.9, 0.6, 0.2, 1.0), 1.0, 0.3),
        Material((0.6, 0.6, 0.6, 1.0), 0.0, 1.0),
        Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (12.0, 11.0, 10.0)),
        Material((0.2, 0.3, 0.8, 1.0), 0.0, 0.5),
    ]
    sv, si = uv_sphere(nu, nv, 1.0)
    gv, gi = grid_patch((-10.0, -1.0, 10.0), (20.0, 0.0, 0.0), (0.0, 0.0, -20.0), 8, 8)
    lv, li = _quad((-2.0, 4.0, -2.0), (2.0, 4.0, -2.0), (2.0, 4.0, 2.0), (-2.0, 4.0, 2.0))  # normal −y
    bv, bi = uv_sphere(24, 12, 0.4)
    meshes = [MeshDesc(sv, si, 0), MeshDesc(gv, gi, 1), MeshDesc(lv, li, 2), MeshDesc(bv, bi, 3)]
    a = math.radians(30.0)
    inst = [
        InstanceDesc(0, (0.0, -0.2, 0.0), (math.cos(a / 2), 0.0, math.sin(a / 2), 0.0), (1.0, 0.8, 1.0)),
        InstanceDesc(1, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0)),
        InstanceDesc(2, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0)),
        InstanceDesc(3, (1.6, -0.6, 0.8), _ID_Q, (1.0, 1.0, 1.0)),
        InstanceDesc(3, (-1.7, -0.6, 0.6), _ID_Q, (1.0, 1.0, 1.0)),
    ]
    cam = CameraDesc((0.0, 1.2, 4.5), (0.0, -0.1, 0.0), math.radians(45.0), 1.0)
    return SceneDesc(mats, meshes, inst, cam, "sphere10k")


def atrium(scale: float = 1.0) -> SceneDesc:
    """Config 3: Sponza-class procedural atrium, 250 000 ± 1 % triangles at scale=1 (tessellation
    counts scale with `scale` for small test versions).  40×12×20 m box shell (tessellated walls,
    ceiling), displaced floor, an 8×4 grid of 64-sided columns (two meshes, 32 instances), tube arches
    between columns along x, emissive ceiling panels.  6 material classes: Lambert, GGX dielectric at
    roughness 0.6 / 0.3 / 0.15, metal, emitter.  Every mesh has < 65 536 vertices (u16-expressible)."""
    sc = max(scale, 1e-3)

    def n_(x, lo=1):
        return max(lo, int(round(x * math.sqrt(sc))))

    mats = [
        Material((0.70, 0.68, 0.62, 1.0), 0.0, 1.0),  # 0 walls / ceiling: Lambert
        Material((0.50, 0.40, 0.35, 1.0), 0.0, 0.6),  # 1 floor: GGX rough 0.6
        Material((0.80, 0.80, 0.75, 1.0), 0.0, 0.3),  # 2 columns: GGX rough 0.3
        Material((0.60, 0.62, 0.70, 1.0), 0.0, 0.15),  # 3 arches: GGX rough 0.15
        Material((1.00, 0.78, 0.34, 1.0), 1.0, 0.2),  # 4 metal columns
        Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (20.0, 18.0, 15.0)),  # 5 emitter panels
    ]
    X, Y, Z = 20.0, 12.0, 10.0
    meshes: List[MeshDesc] = []
    inst: List[InstanceDesc] = []

    def add(vi, mat, t=(0.0, 0.0, 0.0), q=_ID_Q, s=(1.0, 1.0, 1.0)):
        meshes.append(MeshDesc(vi[0], vi[1], mat))
        inst.append(InstanceDesc(len(meshes) - 1, t, q, s))
        return len(meshes) - 1

    def bump(P):
        return 0.04 * np.sin(3.1 * P[:, 0]) * np.cos(2.3 * P[:, 2]) + 0.02 * np.sin(11.0 * P[:, 0] + 1.7 * P[:, 2])

    # floor (normal +y): du × dv = +y  →  du = +x, dv = −z
    add(grid_patch((-X, 0.0, Z), (2 * X, 0.0, 0.0), (0.0, 0.0, -2 * Z), n_(264), n_(132), bump), 1)
    # ceiling (normal −y)
    add(grid_patch((-X, Y, -Z), (2 * X, 0.0, 0.0), (0.0, 0.0, 2 * Z), n_(64), n_(32)), 0)
    # walls, normals pointing inside
    add(grid_patch((-X, 0.0, -Z), (2 * X, 0.0, 0.0), (0.0, Y, 0.0), n_(64), n_(24)), 0)  # back  z=−Z, n=+z
    add(grid_patch((X, 0.0, Z), (-2 * X, 0.0, 0.0), (0.0, Y, 0.0), n_(64), n_(24)), 0)  # front z=+Z, n=−z
    add(grid_patch((-X, 0.0, Z), (0.0, 0.0, -2 * Z), (0.0, Y, 0.0), n_(32), n_(24)), 0)  # left  x=−X, n=+x
    add(grid_patch((X, 0.0, -Z), (0.0, 0.0, 2 * Z), (0.0, Y, 0.0), n_(32), n_(24)), 0)  # right x=+X, n=−x
    # columns: 8 × 4 grid, two shared meshes (dielectric / metal), instanced with per-column yaw + scale
    col_h = 8.0
    col = cylinder(n_(64, 8), n_(32, 2), 0.45, col_h)
    meshes.append(MeshDesc(col[0], col[1], 2))
    m_col = len(meshes) - 1
    meshes.append(MeshDesc(col[0], col[1], 4))
    m_colm = len(meshes) - 1
    xs = [-17.5 + 5.0 * i for i in range(8)]
    zs = [-7.5 + 5.0 * k for k in range(4)]
    for k, z in enumerate(zs):
        for i, x in enumerate(xs):
            yaw = 0.37 * (i + 8 * k)
            q = (math.cos(yaw / 2), 0.0, math.sin(yaw / 2), 0.0)
            metal = (i + k) % 4 == 0
            sxz = 1.0 + 0.1 * ((i * 3 + k) % 3)
            inst.append(InstanceDesc(m_colm if metal else m_col, (x, 0.0, z), q, (sxz, 1.0, sxz)))
    # arches between neighbouring columns along x: one mesh, 7 × 4 instances
    arch = half_torus(2.5, 0.22, n_(40, 4), n_(16, 4))
    meshes.append(MeshDesc(arch[0], arch[1], 3))
    m_arch = len(meshes) - 1
    for z in zs:
        for i in range(7):
            inst.append(InstanceDesc(m_arch, (xs[i] + 2.5, col_h, z), _ID_Q, (1.0, 1.0, 1.0)))
    # emissive ceiling panels (normal −y), 2 × 4
    for k in range(2):
        for i in range(4):
            cx, cz = -15.0 + 10.0 * i, -5.0 + 10.0 * k
            add(_quad((cx - 1.5, Y - 0.02, cz - 1.0), (cx + 1.5, Y - 0.02, cz - 1.0), (cx + 1.5, Y - 0.02, cz + 1.0), (cx - 1.5, Y - 0.02, cz + 1.0)), 5)
    cam = CameraDesc((-18.5, 2.6, 1.2), (0.0, 3.4, -0.4), math.radians(60.0), 16.0 / 9.0)
    return SceneDesc(mats, meshes, inst, cam, "atrium")


def two_triangles_and_sphere() -> SceneDesc:
    """Raster-compat fixture scene (SURVEY §8c fixture 3): two triangles + a sphere in front of the
    reference's default camera (position 0, direction −z, fovY π/2 — CameraController.hpp:25-40)."""
    mats = [Material((0.8, 0.3, 0.2, 1.0), 0.0, 1.0), Material((0.2, 0.5, 0.9, 0.5), 0.0, 1.0)]
    qv, qi = _quad((-2.0, -1.5, -4.0), (2.0, -1.5, -4.0), (2.0, 1.5, -4.0), (-2.0, 1.5, -4.0))
    sv, si = uv_sphere(32, 16, 0.8)
    meshes = [MeshDesc(qv, qi, 0), MeshDesc(sv, si, 1)]
    inst = [
        InstanceDesc(0, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0)),
        InstanceDesc(1, (0.3, -0.2, -2.5), (math.cos(0.3), math.sin(0.3), 0.0, 0.0), (1.0, 1.2, 0.9)),
    ]
    cam = CameraDesc((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), math.pi / 2, 1.0)
    return SceneDesc(mats, meshes, inst, cam, "two_tris_sphere")




# ----------------------------------------------------------------------------------------------
# Config 5: textures + image-based environment light (all procedural and seeded: the reference's
# assets/textures/rusty_metal_grid_{diff,nor_gl}_1k.png are stripped from the checkout).
def _value_noise(size: int, seed: int, octaves: int = 4) -> np.ndarray:
    """Tileable value noise in [0,1], size × size (REPEAT-safe: lattice wraps)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((size, size), np.float64)
    amp, total = 1.0, 0.0
    for o in range(octaves):
        cells = 4 << o
        lat = rng.random((cells, cells))
        t = np.arange(size) * cells / size
        i0 = np.floor(t).astype(int) % cells
        i1 = (i0 + 1) % cells
        f = t - np.floor(t)
        f = f * f * (3 - 2 * f)
        a = lat[i0][:, i0] * (1 - f)[None, :] + lat[i0][:, i1] * f[None, :]
        b = lat[i1][:, i0] * (1 - f)[None, :] + lat[i1][:, i1] * f[None, :]
        out += amp * (a * (1 - f)[:, None] + b * f[:, None])
        total += amp
        amp *= 0.5
    return out / total


def texture_albedo(size: int = 256, seed: int = 5) -> np.ndarray:
    n1, n2 = _value_noise(size, seed), _value_noise(size, seed + 1)
    rgb = np.stack([0.55 + 0.4 * n1, 0.35 + 0.4 * n2, 0.25 + 0.3 * n1 * n2], -1)
    grid = ((np.arange(size) // max(1, size // 8)) % 2)[:, None] ^ ((np.arange(size) // max(1, size // 8)) % 2)[None, :]
    rgb *= (0.75 + 0.25 * grid)[..., None]
    return np.concatenate([np.clip(rgb * 255 + 0.5, 0, 255).astype(np.uint8), np.full((size, size, 1), 255, np.uint8)], -1)


def texture_normal(size: int = 256, seed: int = 6, strength: float = 2.0) -> np.ndarray:
    h = _value_noise(size, seed)
    dx = (np.roll(h, -1, 1) - np.roll(h, 1, 1)) * 0.5 * size / 64.0 * strength
    dy = (np.roll(h, -1, 0) - np.roll(h, 1, 0)) * 0.5 * size / 64.0 * strength
    n = np.stack([-dx, -dy, np.ones_like(h)], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    return np.concatenate([np.clip((n * 0.5 + 0.5) * 255 + 0.5, 0, 255).astype(np.uint8), np.full((size, size, 1), 255, np.uint8)], -1)


def texture_metal_rough(size: int = 256, seed: int = 7) -> np.ndarray:
    r = 0.15 + 0.75 * _value_noise(size, seed)
    m = (_value_noise(size, seed + 1, 2) > 0.55).astype(np.float64)
    z = np.zeros_like(r)
    return np.clip(np.stack([z, r, m, z + 1.0], -1) * 255 + 0.5, 0, 255).astype(np.uint8)   # glTF: G = roughness, B = metallic


def analytic_sky(w: int = 64, h: int = 32, sun_dir=(0.4, 0.7, 0.3), sun_radiance: float = 60.0) -> np.ndarray:
    """Lat-long RGB32F sky (row 0 = +y): horizon-to-zenith gradient, dark ground, and a small bright sun (which is what makes
    importance sampling necessary)."""
    v = (np.arange(h) + 0.5) / h
    u = (np.arange(w) + 0.5) / w
    th = np.pi * v[:, None]
    ph = 2 * np.pi * u[None, :] - np.pi
    d = np.stack([np.sin(th) * np.cos(ph), np.cos(th) * np.ones_like(ph), np.sin(th) * np.sin(ph)], -1)
    up = np.clip(d[..., 1], 0, 1)
    sky = np.stack([0.35 + 0.25 * (1 - up), 0.5 + 0.25 * (1 - up), 0.9 - 0.2 * (1 - up)], -1) * (0.6 + 0.8 * up[..., None])
    ground = np.array([0.12, 0.10, 0.08])
    img = np.where((d[..., 1] > 0)[..., None], sky, ground[None, None, :])
    s = np.asarray(sun_dir, np.float64)
    s /= np.linalg.norm(s)
    img = img + (np.einsum("ijk,k->ij", d, s) > np.cos(np.radians(6.0)))[..., None] * sun_radiance * np.array([1.0, 0.9, 0.7])
    return img.astype(np.float32)


def textured_atrium(scale: float = 1.0, tex_size: int = 1024, env_size=(2048, 1024), keep_panels: bool = True) -> SceneDesc:
    """Config 5: the atrium with albedo / normal / metallic-roughness textures on floor, columns and arches, its ceiling opened to an
    analytic-sky environment map (the emissive panels stay unless keep_panels=False: both light kinds are then sampled)."""
    d = atrium(scale)
    d.name = "textured_atrium"
    d.textures = [texture_albedo(tex_size, 5), texture_normal(tex_size, 6), texture_metal_rough(tex_size, 7)]
    for k in (1, 2, 3):                               # floor, columns, arches
        d.materials[k].tex_color, d.materials[k].tex_normal = 0, 1
    d.materials[3].tex_mr = 2
    d.materials[3].metallic, d.materials[3].roughness = 1.0, 1.0
    d.env = analytic_sky(env_size[0], env_size[1])
    # open the roof: drop the ceiling patch (mesh 1) and, optionally, the emissive panels
    drop = {1} | (set() if keep_panels else {i for i, m in enumerate(d.meshes) if m.material == 5})
    d.instances = [it for it in d.instances if it.mesh not in drop]
    return d


def textured_objects() -> SceneDesc:
    """Small textured + environment-lit test scene: a textured ground, a normal-mapped sphere with a metallic-roughness map and a
    plain diffuse sphere under the analytic sky; no emissive triangles (environment NEE only)."""
    d = sphere_scene(48, 25)
    d.name = "textured_objects"
    d.textures = [texture_albedo(64, 5), texture_normal(64, 6), texture_metal_rough(64, 7)]
    d.materials[0] = Material((1.0, 1.0, 1.0, 1.0), 1.0, 1.0, (0, 0, 0), 0, 1, 2)       # big sphere: all three maps
    d.materials[1] = Material((0.9, 0.9, 0.9, 1.0), 0.0, 1.0, (0, 0, 0), 0, -1, -1)     # ground: albedo map only (stays Lambert class)
    d.materials[3] = Material((0.2, 0.3, 0.8, 0.5), 0.0, 0.5, (0, 0, 0), -1, 1, -1)     # small spheres: normal map only
    d.instances = [it for it in d.instances if it.mesh != 2]                            # no emissive quad
    d.env = analytic_sky(64, 32)
    return d

def alpha_layers(n_mask: int = 3, n_blend: int = 2, texture_filter: str = "nearest", spacing: float = 0.25, mask_alpha=None, blend_alpha=None,
                 emitter: bool = True) -> SceneDesc:
    """The alpha-coverage test scene (csrc/pt_alpha.h): n_mask + n_blend parallel quads of two triangles each, `spacing` apart (thousands of ray epsilons in this
    unit-scale scene), above a Lambert floor, seen from far above through a narrow lens: the rays are within 5 degrees of the quads' normal and all of them cross
    every quad well inside its outline.  That is on purpose: a ray that passes a surface goes on from a point one ray epsilon off the surface ALONG ITS NORMAL, which moves
    a slanted ray sideways by epsilon x sin(angle); here that is under 1e-5 of a texture per layer, so which texel a later layer is met in does not depend on it.  Each quad has an 8x8 RGBA texture of its own: a MASK layer alpha 0 / 255 in a checker of 2x2-texel
    cells shifted by one texel per layer, a BLEND layer alpha in {0, 64, 128, 192, 255}; mask_alpha / blend_alpha (0..255) make a kind's alpha constant instead.
    The MASK layers lie below the BLEND layers.  The quads are added LAST, so the floor's (and the emitter's) primitive ids are those of the scene without them:
    floor 0-1, emitter 2-3 (a small quad above the layers, facing down, outside the camera's view; emitter=False leaves it out), layer k at 4 + 2k (2 + 2k without the emitter)."""
    mats = [Material((0.7, 0.7, 0.7, 1.0), 0.0, 1.0)]
    meshes = [MeshDesc(*_quad((-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)), 0)]                       # floor, normal +y
    if emitter:
        mats.append(Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (20.0, 20.0, 20.0)))
        meshes.append(MeshDesc(*_quad((1.6, 4.0, -0.2), (2.0, 4.0, -0.2), (2.0, 4.0, 0.2), (1.6, 4.0, 0.2)), 1))     # normal -y; beside the camera's view
    textures = []
    yy, xx = np.mgrid[0:8, 0:8]
    for k in range(n_mask + n_blend):
        mask = k < n_mask
        if mask:
            alpha = np.where((((xx + k) // 2 + yy // 2) % 2) == 0, 255, 0) if mask_alpha is None else np.full((8, 8), int(mask_alpha))
        else:
            alpha = np.asarray([0, 64, 128, 192, 255])[(xx + 2 * yy + k) % 5] if blend_alpha is None else np.full((8, 8), int(blend_alpha))
        rgb = np.stack([(37 * xx + 11 * k) % 200 + 40, (53 * yy + 29 * k) % 200 + 40, (17 * (xx + yy) + 71 * k) % 200 + 40], -1)
        textures.append(np.concatenate([rgb, alpha[..., None]], -1).astype(np.uint8))
        mats.append(Material((1.0, 1.0, 1.0, 1.0), 0.0, 1.0, (0, 0, 0), k, -1, -1, "mask" if mask else "blend", 0.5))
        y = 0.5 + spacing * k
        meshes.append(MeshDesc(*_quad((-2, y, 2), (2, y, 2), (2, y, -2), (-2, y, -2)), len(mats) - 1))   # normal +y
    inst = [InstanceDesc(k, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0)) for k in range(len(meshes))]
    cam = CameraDesc((1.2, 40.0, 1.0), (0.0, 0.0, 0.0), math.radians(2.9), 1.0)      # a square of side 2 of the quads, turned about y, corners within 1.55 of the axis: four texels across
    d = SceneDesc(mats, meshes, inst, cam, "alpha_layers")
    d.textures = textures
    d.texture_filter = texture_filter
    return d


def glass_slab(thin: bool = False, thickness: float = 0.5, transmission: float = 1.0, ior: float = 1.5, base=(1.0, 1.0, 1.0), metallic: float = 0.0,
               attenuation_color=(1.0, 1.0, 1.0), attenuation_distance: float = 0.0, sheet_alpha=None, emitter: bool = False, pane: bool = True,
               texture_filter: str = "nearest", textured: bool = False) -> SceneDesc:
    """The transmission test scene (csrc/pt_glass.h): a Lambert floor at y = 0 (primitives 0-1), an optional emissive quad facing down at y = 4 beside the view
    (emitter=True: primitives 2-3), then the glass over x, z in [-2, 2]: a box slab from y = 1 to y = 1 + thickness (solid, six quads, outward normals, top first then
    bottom) or a single pane at y = 1 (thin=True, normal +y); pane=False leaves the glass out.  sheet_alpha (0..1): a BLEND sheet of that constant alpha at y = 0.5,
    added last.  textured=True gives the glass a 4x4 base-colour texture, so that the tint depends on the texel and the filter.  Seen from above, slanted."""
    mats = [Material((0.7, 0.7, 0.7, 1.0), 0.0, 1.0)]
    meshes = [MeshDesc(*_quad((-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4)), 0)]
    if emitter:
        mats.append(Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (20.0, 20.0, 20.0)))
        meshes.append(MeshDesc(*_quad((-1.0, 4.0, -1.0), (1.0, 4.0, -1.0), (1.0, 4.0, 1.0), (-1.0, 4.0, 1.0)), len(mats) - 1))     # normal -y
    textures = []
    if pane:
        if textured:
            yy, xx = np.mgrid[0:4, 0:4]
            textures.append(np.stack([(37 * xx + 90) % 200 + 55, (53 * yy + 60) % 200 + 55, (17 * (xx + yy)) % 200 + 55, np.full((4, 4), 255)], -1).astype(np.uint8))
        mats.append(Material(tuple(base) + (1.0,), metallic, 0.2, (0, 0, 0), 0 if textured else -1, -1, -1, "opaque", 0.5, transmission, ior, thin,
                             tuple(attenuation_color), attenuation_distance))
        g = len(mats) - 1
        y0, y1, a = 1.0, 1.0 + thickness, 2.0
        if thin:
            meshes.append(MeshDesc(*_quad((-a, y0, a), (a, y0, a), (a, y0, -a), (-a, y0, -a)), g))
        else:
            meshes.append(MeshDesc(*_quad((-a, y1, a), (a, y1, a), (a, y1, -a), (-a, y1, -a)), g))        # top, +y
            meshes.append(MeshDesc(*_quad((-a, y0, -a), (a, y0, -a), (a, y0, a), (-a, y0, a)), g))        # bottom, -y
            meshes.append(MeshDesc(*_quad((-a, y0, a), (a, y0, a), (a, y1, a), (-a, y1, a)), g))          # +z
            meshes.append(MeshDesc(*_quad((a, y0, -a), (-a, y0, -a), (-a, y1, -a), (a, y1, -a)), g))      # -z
            meshes.append(MeshDesc(*_quad((a, y0, a), (a, y0, -a), (a, y1, -a), (a, y1, a)), g))          # +x
            meshes.append(MeshDesc(*_quad((-a, y0, -a), (-a, y0, a), (-a, y1, a), (-a, y1, -a)), g))      # -x
    if sheet_alpha is not None:
        mats.append(Material((0.9, 0.5, 0.3, float(sheet_alpha)), 0.0, 1.0, (0, 0, 0), -1, -1, -1, "blend", 0.5))
        meshes.append(MeshDesc(*_quad((-3, 0.5, 3), (3, 0.5, 3), (3, 0.5, -3), (-3, 0.5, -3)), len(mats) - 1))
    inst = [InstanceDesc(k, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0)) for k in range(len(meshes))]
    cam = CameraDesc((1.5, 6.0, 2.5), (0.0, 1.0, 0.0), math.radians(20.0), 1.0)
    d = SceneDesc(mats, meshes, inst, cam, "glass_slab")
    d.textures = textures
    d.texture_filter = texture_filter
    return d


def glass_panes(n: int = 3, spacing: float = 0.25, tilt: float = 0.0, transmission: float = 1.0, ior: float = 1.5, base=(0.9, 0.8, 0.7), metallic: float = 0.0,
                emitter: bool = False, sheets=(), texture_filter: str = "nearest", textured: bool = False) -> SceneDesc:
    """The transparent-shadow test scene (csrc/pt_glass_shadow.h): a Lambert floor at y = 0 (primitives 0-1), an optional emissive quad facing down at y = 4
    (emitter=True: primitives 2-3), then a stack of n thin-walled panes over x, z in [-2, 2] at y = 1 + spacing k (normal +y, one material; pane k is primitives
    first + 2k, first + 2k + 1).  tilt > 0 turns the four vertex normals of every pane away from +y by different amounts (tan of the angle up to `tilt`), so that the
    shading normal differs from the face normal and varies over the pane.  textured=True gives the panes a 4x4 base-colour texture.  sheets: alpha sheets below the
    panes, added last, from y = 0.75 downwards 0.25 apart: "blend" (8x8 texture, alpha in {0, 64, 128, 192, 255}) or "mask" (8x8 checker of 2x2-texel cells, cutoff 0.5).
    Seen from above, slanted, as glass_slab."""
    mats = [Material((0.7, 0.7, 0.7, 1.0), 0.0, 1.0)]
    meshes = [MeshDesc(*_quad((-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4)), 0)]
    if emitter:
        mats.append(Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (20.0, 20.0, 20.0)))
        meshes.append(MeshDesc(*_quad((-1.0, 4.0, -1.0), (1.0, 4.0, -1.0), (1.0, 4.0, 1.0), (-1.0, 4.0, 1.0)), len(mats) - 1))     # normal -y
    textures = []
    if textured:
        yy, xx = np.mgrid[0:4, 0:4]
        textures.append(np.stack([(37 * xx + 90) % 200 + 55, (53 * yy + 60) % 200 + 55, (17 * (xx + yy)) % 200 + 55, np.full((4, 4), 255)], -1).astype(np.uint8))
    mats.append(Material(tuple(base) + (1.0,), metallic, 0.2, (0, 0, 0), 0 if textured else -1, -1, -1, "opaque", 0.5, transmission, ior, True))
    g = len(mats) - 1
    a = 2.0
    lean = np.array([(1.0, 0.0, 0.3), (-0.4, 0.0, 1.0), (0.2, 0.0, -0.9), (-1.0, 0.0, -0.5)])
    for k in range(n):
        y = 1.0 + spacing * k
        v, i = _quad((-a, y, a), (a, y, a), (a, y, -a), (-a, y, -a))
        if tilt > 0.0:
            nrm = np.array([0.0, 1.0, 0.0]) + tilt * np.roll(lean, k, 0)
            v["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        meshes.append(MeshDesc(v, i, g))
    yy, xx = np.mgrid[0:8, 0:8]
    for k, kind in enumerate(sheets):
        if kind == "mask":
            alpha = np.where(((xx // 2 + yy // 2) % 2) == 0, 255, 0)
        else:
            alpha = np.asarray([0, 64, 128, 192, 255])[(xx + 2 * yy + k) % 5]
        rgb = np.stack([(37 * xx + 11 * k) % 200 + 40, (53 * yy + 29 * k) % 200 + 40, (17 * (xx + yy) + 71 * k) % 200 + 40], -1)
        textures.append(np.concatenate([rgb, alpha[..., None]], -1).astype(np.uint8))
        mats.append(Material((1.0, 1.0, 1.0, 1.0), 0.0, 1.0, (0, 0, 0), len(textures) - 1, -1, -1, kind, 0.5))
        y = 0.75 - 0.25 * k
        meshes.append(MeshDesc(*_quad((-3, y, 3), (3, y, 3), (3, y, -3), (-3, y, -3)), len(mats) - 1))
    inst = [InstanceDesc(k, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0)) for k in range(len(meshes))]
    cam = CameraDesc((1.5, 6.0, 2.5), (0.0, 1.0, 0.0), math.radians(20.0), 1.0)
    d = SceneDesc(mats, meshes, inst, cam, "glass_panes")
    d.textures = textures
    d.texture_filter = texture_filter
    return d


def glass_ball(nu: int = 24, nv: int = 12, ior: float = 1.5, transmission: float = 1.0, base=(1.0, 1.0, 1.0), env: float = 1.0, attenuation_color=(1.0, 1.0, 1.0),
               attenuation_distance: float = 0.0) -> SceneDesc:
    """A closed solid glass ball of radius 1 (smooth normals, 2 nu (nv - 1) triangles) in a constant environment of radiance `env`, and nothing else: with base 1
    and no attenuation a white furnace — every path that is not exhausted carries throughput 1 into the environment."""
    mats = [Material(tuple(base) + (1.0,), 0.0, 0.2, (0, 0, 0), -1, -1, -1, "opaque", 0.5, transmission, ior, False, tuple(attenuation_color), attenuation_distance)]
    meshes = [MeshDesc(*uv_sphere(nu, nv, 1.0), 0)]
    inst = [InstanceDesc(0, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0))]
    cam = CameraDesc((0.0, 0.6, 3.2), (0.0, 0.0, 0.0), math.radians(40.0), 1.0)
    d = SceneDesc(mats, meshes, inst, cam, "glass_ball")
    d.env = np.full((4, 8, 3), env, np.float32)
    return d


# ---- the scenes of the k_shade step tests (tests/shade_reference.py): a floor in the plane z = 0 seen from +z, so that the face normal is exactly (0, 0, 1) ----
SHADE_GRID = [(0.0, 1.0), (0.0, 0.0), (0.0, 0.05), (0.0, 0.5), (1.0, 0.0), (1.0, 0.05), (1.0, 0.5), (1.0, 1.0)]      # (metallic, roughness); (0, 1) is the Lambert class


def _shade_floor(nx: int, ny: int, half: float, material_of, uv_of=None, normal_of=None, tangent_w_of=None):
    """nx x ny square patches over [-half, half]^2 in the plane z = 0, front towards +z, one mesh of two triangles per patch: [(vertices, indices, material)]."""
    out = []
    sx, sy = 2.0 * half / nx, 2.0 * half / ny
    for j in range(ny):
        for i in range(nx):
            k = j * nx + i
            x0, y0 = -half + i * sx, -half + j * sy
            P = [(x0, y0, 0.0), (x0 + sx, y0, 0.0), (x0 + sx, y0 + sy, 0.0), (x0, y0 + sy, 0.0)]
            N = normal_of(k) if normal_of else [(0.0, 0.0, 1.0)] * 4
            N = [np.asarray(n, np.float64) / np.linalg.norm(n) for n in N]
            w = tangent_w_of(k) if tangent_w_of else 1.0
            T = [(1.0, 0.0, 0.0, w)] * 4
            (u0, v0), (u1, v1) = uv_of(k) if uv_of else ((0.0, 0.0), (1.0, 1.0))
            uv = [(u0, v0), (u1, v0), (u1, v1), (u0, v1)]
            out.append((_verts(P, N, T, uv), np.asarray([0, 1, 2, 0, 2, 3], np.uint32), material_of(k)))
    return out


def _shade_desc(parts, mats, name, fov=1.0) -> SceneDesc:
    meshes = [MeshDesc(v, i, m) for v, i, m in parts]
    inst = [InstanceDesc(k, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0)) for k in range(len(meshes))]
    return SceneDesc(mats, meshes, inst, CameraDesc((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), fov, 1.0), name)


def shade_lobes() -> SceneDesc:
    """3 x 3 floor patches over the material grid SHADE_GRID (the ninth: roughness 0.2 without metal), a tiny bright emitter above the floor and a large dim one standing at
    the floor's +x edge, which the floor next to that edge sees nearly edge-on.  The camera sees the floor and its surroundings, not the large emitter: a ray that
    hits an emitter samples that emitter's own plane half of the time, which no precision decides.  No environment.  21 triangles."""
    cols = [(0.8, 0.7, 0.6), (0.9, 0.5, 0.3), (0.4, 0.8, 0.5), (0.5, 0.5, 0.9), (0.95, 0.8, 0.4), (0.9, 0.9, 0.9), (0.7, 0.3, 0.3), (0.6, 0.6, 0.2)]
    mats = [Material(c + (1.0,), m, r) for c, (m, r) in zip(cols, SHADE_GRID)] + [Material((0.2, 0.3, 0.7, 1.0), 0.0, 0.2)]
    mats += [Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (4000.0, 3000.0, 2000.0)), Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (0.4, 0.5, 0.6))]
    parts = _shade_floor(3, 3, 1.5, lambda k: k)
    e = 0.01
    tiny = _verts([(0.3 - e, 0.2 - e, 2.0), (0.3 - e, 0.2 + e, 2.0), (0.3 + e, 0.2 - e, 2.0)], [(0, 0, -1)] * 3, [(1, 0, 0)] * 3, [(0, 0), (0, 1), (1, 0)])
    parts.append((tiny, np.asarray([0, 1, 2], np.uint32), 9))
    parts.append((*_quad((1.6, -1.5, 0.3), (1.6, -1.5, 1.8), (1.6, -0.5, 1.8), (1.6, -0.5, 0.3)), 10))      # faces -x; outside the camera's view
    return _shade_desc(parts, mats, "shade_lobes", fov=0.8)


def _shade_textures():
    """Six RGBA8 textures: colour, normal and metal-rough of 5 x 3 (one set), and a second normal map of 4 x 4, colour and metal-rough of 5 x 3 (sizes differ: no
    interleaved copy).  Normal texels stay within 45 degrees of +z."""
    rng = np.random.default_rng(41)

    def colour(w, h):
        return np.concatenate([rng.integers(30, 256, (h, w, 3)), np.full((h, w, 1), 255)], -1).astype(np.uint8)

    def normal(w, h):
        xy = rng.integers(128 - 60, 128 + 61, (h, w, 2))
        return np.concatenate([xy, rng.integers(215, 256, (h, w, 1)), np.full((h, w, 1), 255)], -1).astype(np.uint8)

    def metal_rough(w, h):
        t = rng.integers(0, 256, (h, w, 4))
        t[..., 2] = rng.integers(0, 2, (h, w)) * 255 * rng.integers(0, 2, (h, w)) + rng.integers(0, 256, (h, w)) * (1 - rng.integers(0, 2, (h, w)))
        return np.clip(t, 0, 255).astype(np.uint8)

    return [colour(5, 3), normal(5, 3), metal_rough(5, 3), colour(5, 3), normal(4, 4), metal_rough(5, 3)]


def shade_textured(texture_filter: str = "nearest") -> SceneDesc:
    """3 x 2 floor patches with colour, normal and metal-rough textures of 5 x 3 texels (one interleaved texture set, one material whose normal map has another size,
    one with a colour texture alone), texture coordinates from -0.7 to 1.9, tilted vertex normals, tangents of both handednesses; an 8 x 4 environment with zero
    texels and one emitter above the floor.  14 triangles."""
    mats = [Material((0.9, 0.8, 0.7, 1.0), 0.0, 1.0, (0, 0, 0), 0, -1, -1), Material((1.0, 0.9, 0.8, 1.0), 1.0, 0.9, (0, 0, 0), 0, 1, 2),
            Material((0.8, 0.9, 1.0, 1.0), 0.8, 1.0, (0, 0, 0), 3, 4, 5), Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (6.0, 5.0, 4.0))]
    uvs = [((-0.7, -0.4), (1.9, 1.3)), ((0.1, 0.2), (0.9, 0.8)), ((1.9, 1.6), (-0.6, -0.3))]
    tilt = np.random.default_rng(43).uniform(-0.25, 0.25, (6, 4, 2))
    parts = _shade_floor(3, 2, 1.5, lambda k: k % 3, uv_of=lambda k: uvs[(k + k // 3) % 3], normal_of=lambda k: [(tx, ty, 1.0) for tx, ty in tilt[k]],
                         tangent_w_of=lambda k: -1.0 if k in (1, 2, 3) else 1.0)
    parts.append((*_quad((1.2, -0.4, 2.5), (1.2, 0.4, 2.5), (2.0, 0.4, 2.5), (2.0, -0.4, 2.5)), 3))      # faces -z; outside the camera's view
    d = _shade_desc(parts, mats, "shade_textured", fov=1.1)
    d.textures = _shade_textures()
    d.texture_filter = texture_filter
    env = np.random.default_rng(47).uniform(0.0, 1.5, (4, 8, 3)).astype(np.float32)
    env[0, 2:5] = 0.0
    env[2, :] = 0.0
    env[3, 6] = 0.0
    d.env = env
    return d


def shade_sky() -> SceneDesc:
    """The floor of shade_lobes without emitters under a 64 x 32 environment whose two polar rows are the brightest.  18 triangles."""
    d = shade_lobes()
    d.meshes, d.instances, d.materials, d.name = d.meshes[:9], d.instances[:9], d.materials[:9], "shade_sky"
    env = np.random.default_rng(53).uniform(0.05, 1.0, (32, 64, 3)).astype(np.float32)
    env[0] *= 40.0
    env[31] *= 25.0
    env[10, 20:30] = 0.0
    d.env = env
    return d


def fog_box(sigma_t: float = 0.7, albedo=(0.9, 0.9, 0.9), g: float = 0.0, slit: float = 0.3, emitter: float = 8.0) -> SceneDesc:
    """A 4 x 4 floor at y = 0, a blocker at y = 1.5 with a slit of width `slit` along z, a small emissive quad under the blocker facing down, and fog between
    floor and blocker (the medium of the description; sigma_t 0: none).  A sun above the blocker — the tests and tools add one — draws a shaft through the slit.
    8 triangles."""
    mats = [Material((0.6, 0.6, 0.6, 1.0), 0.0, 1.0), Material((0.3, 0.3, 0.3, 1.0), 0.0, 1.0), Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (emitter,) * 3)]
    h, s = 1.5, 0.5 * slit
    q = [(_quad((-2, 0, 2), (2, 0, 2), (2, 0, -2), (-2, 0, -2)), 0),                    # floor, normal +y
         (_quad((-2, h, 2), (-s, h, 2), (-s, h, -2), (-2, h, -2)), 1),                  # blocker, x < -s, normal +y
         (_quad((s, h, 2), (2, h, 2), (2, h, -2), (s, h, -2)), 1),                      # blocker, x > s
         (_quad((1.0, h - 0.01, -0.3), (1.6, h - 0.01, -0.3), (1.6, h - 0.01, 0.3), (1.0, h - 0.01, 0.3)), 2)]      # emitter, normal -y
    meshes = [MeshDesc(v, i, m) for (v, i), m in q]
    inst = [InstanceDesc(k, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0)) for k in range(len(meshes))]
    cam = CameraDesc((0.0, 0.8, 5.0), (0.0, 0.6, 0.0), math.radians(45.0), 1.0)
    d = SceneDesc(mats, meshes, inst, cam, "fog_box")
    if sigma_t > 0.0:
        d.medium = dict(box_lo=(-2.0, 0.0, -2.0), box_hi=(2.0, h, 2.0), sigma_t=sigma_t, albedo=albedo, g=g)
    return d


def passes_surface(top: str = "normal") -> SceneDesc:
    """Everything that may share a frame with alpha and glass (tests/test_gpu_pass_policies.py), 30 triangles, seen from above through a camera that looks down:
    a Lambert floor at y = 0 (primitives 0-1), a plain emitter facing down at y = 2.4 (2-3), two floor patches at y = 0.01 with colour, normal and metal-rough
    textures — one interleaved set, one whose normal map has another size — (4-7), a quad with an emission texture facing down at y = 2.2 (8-9), a BLEND sheet at
    y = 0.6 (10-11), a solid glass slab from y = 1 to 1.3 (12-23) and a 4 x 8 environment.  Added LAST, so that every other primitive keeps its id without them, and
    ABOVE everything else: a clear thin pane at y = 2.8, a MASK sheet with a checkerboard alpha texture at y = 3 and a tinted thin pane at y = 3.2 (24-29).
    top = "invisible": the MASK sheet's alpha texture is all zero and both panes are the invisible pane (ior 1, white, transmission 1); top = "none": the three are
    left out.  A ray from below that passes them meets nothing afterwards, whose radiance depends on its direction and throughput alone, and the scene's largest
    extent — the floor's, which sets the ray epsilon — does not depend on them: a frame without a camera (probes, a lightmap) of the invisible variant computes
    the bits of the variant without."""
    assert top in ("normal", "invisible", "none")
    T = _shade_textures()
    yy, xx = np.mgrid[0:8, 0:8]
    rgb = np.stack([(37 * xx + 11) % 200 + 40, (53 * yy + 29) % 200 + 40, (17 * (xx + yy) + 71) % 200 + 40], -1)
    blend = np.concatenate([rgb, np.asarray([0, 64, 128, 192, 255])[(xx + 2 * yy) % 5][..., None]], -1).astype(np.uint8)
    check = np.where(((xx // 2 + yy // 2) % 2) == 0, 255, 0) if top != "invisible" else np.zeros((8, 8), np.int64)
    mask = np.concatenate([rgb[..., ::-1], check[..., None]], -1).astype(np.uint8)
    glow = np.array([[[0, 0, 0, 255], [255, 255, 255, 255], [255, 128, 64, 255]], [[64, 128, 255, 255], [0, 0, 0, 255], [200, 200, 200, 255]]], np.uint8)
    textures = T + [blend, mask, glow]
    invisible = top == "invisible"
    mats = [Material((0.7, 0.7, 0.7, 1.0), 0.0, 1.0),
            Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (15.0, 15.0, 15.0)),
            Material((1.0, 0.9, 0.8, 1.0), 1.0, 0.9, (0, 0, 0), 0, 1, 2),
            Material((0.8, 0.9, 1.0, 1.0), 0.8, 1.0, (0, 0, 0), 3, 4, 5),
            Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, emissive_texture=8, emissive_texture_factor=(6.0, 4.0, 2.0)),
            Material((1.0, 1.0, 1.0, 1.0), 0.0, 1.0, (0, 0, 0), 6, -1, -1, "blend", 0.5),
            Material((1.0, 1.0, 1.0, 1.0), 0.0, 0.2, (0, 0, 0), -1, -1, -1, "opaque", 0.5, 1.0, 1.5, False),
            Material((1.0, 1.0, 1.0, 1.0), 0.0, 1.0, (0, 0, 0), 7, -1, -1, "mask", 0.5),
            Material((1.0, 1.0, 1.0, 1.0), 0.0, 0.2, (0, 0, 0), -1, -1, -1, "opaque", 0.5, 1.0, 1.0 if invisible else 1.5, True),
            Material(((1.0, 1.0, 1.0) if invisible else (0.9, 0.7, 0.5)) + (1.0,), 0.0, 0.2, (0, 0, 0), -1, -1, -1, "opaque", 0.5, 1.0, 1.0 if invisible else 1.5, True)]

    def flat(x0, x1, z0, z1, y):      # normal +y
        return _quad((x0, y, z1), (x1, y, z1), (x1, y, z0), (x0, y, z0))

    def down(x0, x1, z0, z1, y):      # normal -y
        return _quad((x0, y, z0), (x1, y, z0), (x1, y, z1), (x0, y, z1))

    q = [(flat(-4, 4, -4, 4, 0.0), 0), (down(2.2, 3.2, -0.5, 0.5, 2.4), 1), (flat(-3.5, -2.0, 1.5, 3.5, 0.01), 2), (flat(2.0, 3.5, -3.5, -1.5, 0.01), 3),
         (down(-3.2, -2.0, -0.6, 0.6, 2.2), 4), (flat(-1.5, 1.5, -1.5, 1.5, 0.6), 5)]
    a, y0, y1 = 1.2, 1.0, 1.3
    q += [(flat(-a, a, -a, a, y1), 6), (down(-a, a, -a, a, y0), 6),
          (_quad((-a, y0, a), (a, y0, a), (a, y1, a), (-a, y1, a)), 6), (_quad((a, y0, -a), (-a, y0, -a), (-a, y1, -a), (a, y1, -a)), 6),
          (_quad((a, y0, a), (a, y0, -a), (a, y1, -a), (a, y1, a)), 6), (_quad((-a, y0, -a), (-a, y0, a), (-a, y1, a), (-a, y1, -a)), 6)]
    if top != "none":
        q += [(flat(-2, 2, -2, 2, 2.8), 8), (flat(-2, 2, -2, 2, 3.0), 7), (flat(-2, 2, -2, 2, 3.2), 9)]
    meshes = [MeshDesc(v, i, m) for (v, i), m in q]
    inst = [InstanceDesc(k, (0.0, 0.0, 0.0), _ID_Q, (1.0, 1.0, 1.0)) for k in range(len(meshes))]
    cam = CameraDesc((1.0, 9.0, 2.5), (0.0, 0.0, 0.0), math.radians(50.0), 1.5)
    d = SceneDesc(mats, meshes, inst, cam, "passes_surface")
    d.textures = textures
    d.env = np.random.default_rng(59).uniform(0.2, 1.0, (4, 8, 3)).astype(np.float32)
    return d


def passes_volume() -> SceneDesc:
    """The medium's side of the pass tests: fog_box with its emitter under a 4 x 8 environment.  The tests add a sun, a point light and a lens.  8 triangles."""
    d = fog_box()
    d.name = "passes_volume"
    d.env = np.random.default_rng(61).uniform(0.1, 0.6, (4, 8, 3)).astype(np.float32)
    return d


def by_name(name: str, **kw) -> SceneDesc:
    return {"passes_surface": passes_surface, "passes_volume": passes_volume, "cornell": cornell_box, "sphere10k": sphere_scene, "atrium": atrium, "two_tris_sphere": two_triangles_and_sphere,
            "textured_objects": textured_objects, "textured_atrium": textured_atrium, "alpha_layers": alpha_layers, "glass_slab": glass_slab, "glass_panes": glass_panes, "glass_ball": glass_ball,
            "shade_lobes": shade_lobes, "shade_textured": shade_textured, "shade_sky": shade_sky, "fog_box": fog_box}[name](**kw)
