"""Lightmaps without a GPU (include/ptc_lightmap.h: ptc_lightmap_begin, ptc_lightmap_texel_count, ptc_lightmap_read_texels, ptc_lightmap_read,
ptc_render_lightmap and the three ptc_debug_lightmap_* hooks): symbols and the binding's table, the host evaluation of csrc/pt_lightmap.h against its numpy
restatement (tests/lightmap_reference.py) bit for bit — coverage, texel records, rays, dilation — the statistics the definition promises (cosine-weighted
directions in the hemisphere of the normal), and the validation table.

A lightmap frame needs a device: tests/test_gpu_lightmap.py holds what needs one.  Here every call that would render validates its arguments first (PTC_E_ARG),
then its state (PTC_E_STATE), and then fails with PTC_E_DEVICE, as rendering does on a description-only context."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import c_header  # noqa: E402
import lightmap_reference as ref  # noqa: E402

NEW = ("ptc_lightmap_begin", "ptc_lightmap_texel_count", "ptc_lightmap_read_texels", "ptc_lightmap_read", "ptc_render_lightmap", "ptc_debug_lightmap_cover",
       "ptc_debug_lightmap_rays", "ptc_debug_lightmap_dilate")
E_ARG, E_STATE, E_DEVICE = -1, -2, -3
F32, F64 = np.float32, np.float64
NONE = 0xFFFFFFFF
SEEDS = (0, 1, 0x1234567890ABCDEF)      # both halves of the seed reach the hash
QUAD_UV = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], F32)
QUAD_IDX = np.array([(0, 1, 2), (0, 2, 3)], np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ctx(pbr):
    return pbr.PathTracer(pbr.ptc.DEVICE_NONE)


def patch_scene(pbr, nu=4, nv=3):
    """Instance 0: an emitter quad (so that the baked instance does not start at vertex 0 and primitive 0).  Instance 1: a displaced nu x nv grid patch — varying
    vertex normals — under a rotation and a non-uniform scale; its texcoord is the patch's (s, t) over the whole unit square."""
    S, sc = pbr.scene, pbr.scenes
    mats = [S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (4.0, 3.0, 2.0)), S.Material((0.6, 0.5, 0.4, 1.0), 0.0, 1.0)]
    lv, li = sc._quad((-1.0, 3.0, -1.0), (1.0, 3.0, -1.0), (1.0, 3.0, 1.0), (-1.0, 3.0, 1.0))
    gv, gi = sc.grid_patch((-1.0, 0.0, 1.0), (2.0, 0.0, 0.0), (0.0, 0.0, -2.0), nu, nv, lambda P: 0.2 * np.sin(2.1 * P[:, 0]) * np.cos(1.7 * P[:, 2]))
    a = math.radians(25.0)
    inst = [S.InstanceDesc(0), S.InstanceDesc(1, (0.3, -0.2, 0.1), (math.cos(a / 2), math.sin(a / 2) * 0.6, math.sin(a / 2) * 0.8, 0.0), (1.5, 0.7, 1.1))]
    return S.SceneDesc(mats, [S.MeshDesc(lv, li, 0), S.MeshDesc(gv, gi, 1)], inst, S.CameraDesc((0.0, 2.0, 4.0), (0.0, 0.0, 0.0), 1.0, 1.0), "lightmap_patch")


def instance_geometry(pt, desc, instance):
    """(local indices (n_tris, 3), world positions, world normals, texcoord) of one instance from the flat scene, and the scene's ray epsilon as
    ptc_refit_grid derives it: 1e-4 x the longest side of the scene box, float32."""
    verts, idx, _ = pt.flat_scene()
    vb = sum(len(desc.meshes[i.mesh].vertices) for i in desc.instances[:instance])
    tb = sum(desc.meshes[i.mesh].indices.size // 3 for i in desc.instances[:instance])
    m = desc.meshes[desc.instances[instance].mesh]
    nv, nt = len(m.vertices), m.indices.size // 3
    local = idx[tb:tb + nt].astype(np.int64) - vb
    assert np.array_equal(local.reshape(-1), m.indices.astype(np.int64))
    used = verts[np.unique(idx.reshape(-1))][:, :3]
    side = (used.max(0) - used.min(0)).astype(F32)
    eps = F32(1e-4) * max(side.max(), F32(1e-6))
    return local, verts[vb:vb + nv, 0:3].copy(), verts[vb:vb + nv, 3:6].copy(), verts[vb:vb + nv, 10:12].copy(), eps


# ---- symbols ----------------------------------------------------------------------------------------------------------------------------------------
def test_binding_table_matches_the_header(pbr, tmp_path):
    """include/ptc_lightmap.h against the binding's table, in the manner of test_shade_debug_table_matches_its_header: same functions in the same order, every
    one mapped to its ptcx_ name, the loaded library carrying the table; the core interface is what it was.  The header's one struct has a pointer member, which
    tests/c_header.py's struct reader does not know: the prototypes are read from a copy without the struct, and the struct is held to its mirror here."""
    path = os.path.join(ROOT, "include", "ptc_lightmap.h")
    text = open(path).read()
    body = re.search(r"typedef struct ptc_lightmap_desc \{(.*?)\} ptc_lightmap_desc;", text, flags=re.S)
    assert body
    stripped = tmp_path / "ptc_lightmap_prototypes.h"
    stripped.write_text(text.replace(body.group(0), ""))
    h = c_header.Header(str(stripped), "ptc_")
    table = pbr.ptc._LIGHTMAP_PROTOTYPES
    macros = dict(re.findall(r"^#define (ptc_\w+) (ptcx_\w+)$", text, flags=re.M))
    assert list(h.prototypes) == list(table) == list(macros) == list(NEW)
    assert all(macros[n] == "ptcx_" + n[4:] for n in macros)
    assert c_header.check_prototypes(h, table) == []
    fields = [tuple(d.replace("*", " * ").split()) for d in re.sub(r"/\*.*?\*/", " ", body.group(1), flags=re.S).replace(",", ";int").split(";") if d.strip()]
    want = [("int", "instance"), ("int", "width"), ("int", "height"), ("const", "float", "*", "uv"), ("uint32_t", "texel_index_base"), ("int", "spp_total"), ("uint64_t", "seed"),
            ("int", "max_bounces")]
    assert fields == want
    mirror = pbr.ptc.PtcLightmapDesc
    assert [k for k, _ in mirror._fields_] == [f[-1] for f in want]
    assert [t for _, t in mirror._fields_] == [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_uint32, C.c_int, C.c_uint64, C.c_int]
    L = pbr.load_library()
    for name, (restype, argtypes) in table.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert L.ptc_abi_version() == 4 and not set(table) & set(pbr.ptc.ABI_SYMBOLS)
    assert '#include "ptc_lightmap.h"' in open(os.path.join(ROOT, "include", "ptc.h")).read()
    for m in ("lightmap_begin", "read_lightmap", "render_lightmap", "lightmap_texels", "lightmap_texel_count", "debug_lightmap_cover", "debug_lightmap_rays", "debug_lightmap_dilate"):
        assert callable(getattr(pbr.PathTracer, m)), m


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------------
def _cover(pt, idx, uv, w, h):
    got = pt.debug_lightmap_cover(idx, uv, w, h)
    want = ref.cover(idx, uv, w, h)
    assert got.shape == (h, w) and got.dtype == np.uint32 and np.array_equal(got, want), (w, h)
    return got


def test_coverage_one_triangle(pbr):
    pt = _ctx(pbr)
    uv = np.array([(0.1, 0.1), (0.9, 0.2), (0.3, 0.8)], F32)
    for w, h in ((1, 1), (8, 8), (17, 5), (64, 64)):
        for order in ((0, 1, 2), (0, 2, 1)):      # either winding covers the same texels
            o = _cover(pt, [order], uv, w, h)
            assert set(np.unique(o)) <= {0, NONE}
        assert np.array_equal(pt.debug_lightmap_cover([(0, 1, 2)], uv, w, h), pt.debug_lightmap_cover([(0, 2, 1)], uv, w, h))
    o = pt.debug_lightmap_cover([(0, 1, 2)], uv, 64, 64)
    a, b = (uv[1] - uv[0]).astype(F64), (uv[2] - uv[0]).astype(F64)
    assert abs(int((o == 0).sum()) - 0.5 * abs(a[0] * b[1] - a[1] * b[0]) * 64 * 64) < 64      # the area, up to the boundary


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (7, 5), (64, 64)])
def test_coverage_unit_quad_owns_every_texel_once(pbr, w, h):
    o = _cover(_ctx(pbr), QUAD_IDX, QUAD_UV, w, h)
    assert (o != NONE).sum() == w * h and set(np.unique(o)) <= {0, 1}
    ys, xs = np.nonzero(np.ones((h, w), bool))
    on_diagonal = (2 * xs + 1) * h == (2 * ys + 1) * w      # the centre lies on the shared edge u = v
    assert (o[ys[on_diagonal], xs[on_diagonal]] == 0).all()      # both triangles cover it: the lower primitive owns it
    if w == h:
        assert on_diagonal.sum() == w
    strictly = (2 * xs + 1) * h > (2 * ys + 1) * w      # u > v: inside triangle (0, 1, 2) only
    assert (o[ys[strictly], xs[strictly]] == 0).all() and (o[ys[~strictly & ~on_diagonal], xs[~strictly & ~on_diagonal]] == 1).all()


def test_coverage_vertex_grid_leaves_no_crack(pbr):
    """A 9 x 9 vertex grid (128 triangles) unwrapped over the whole square: every interior edge is shared, many texel centres lie exactly on one."""
    gv, gi = pbr.scenes.grid_patch((0, 0, 0), (1, 0, 0), (0, 0, -1), 8, 8)
    for w, h in ((64, 64), (7, 5), (16, 24), (1, 1)):
        o = _cover(_ctx(pbr), gi.reshape(-1, 3), gv["texCoords"], w, h)
        assert (o != NONE).sum() == w * h


def test_coverage_special_cases(pbr):
    pt = _ctx(pbr)
    # overlapping triangles: the lowest primitive wins, whatever the order of the larger one
    uv = np.array([(0, 0), (1, 0), (0, 1), (0, 0), (0.6, 0), (0, 0.6)], F32)
    a = _cover(pt, [(0, 1, 2), (3, 4, 5)], uv, 16, 16)
    b = _cover(pt, [(3, 4, 5), (0, 1, 2)], uv, 16, 16)
    assert (a[a != NONE] == 0).all() and (b == 0).sum() > 0 and (b == 1).sum() > 0 and np.array_equal(a != NONE, b != NONE)
    # zero UV area: collinear, and two equal corners
    for tri in ([(0.1, 0.1), (0.5, 0.5), (0.9, 0.9)], [(0.2, 0.3), (0.2, 0.3), (0.8, 0.1)]):
        assert (_cover(pt, [(0, 1, 2)], np.array(tri, F32), 32, 32) == NONE).all()
    # a triangle between the centres misses every one of them
    assert (_cover(pt, [(0, 1, 2)], np.array([(0.51, 0.51), (0.74, 0.52), (0.52, 0.74)], F32), 2, 2) == NONE).all()
    # UVs at exactly 0 and 1, and beyond: clamped to the atlas
    assert (_cover(pt, QUAD_IDX, QUAD_UV * 3 - 1, 5, 9) != NONE).all()
    o = _cover(pt, [(0, 1, 2)], np.array([(0, 0), (1, 0), (0, 1)], F32), 4, 4)
    assert o[0, 0] == 0 and o[3, 3] == NONE and o[0, 3] == 0 and o[3, 0] == 0 and o[1, 2] == 0      # the hypotenuse passes through the centres of the anti-diagonal


@pytest.mark.parametrize("seed", range(5))
def test_coverage_random_triangles(pbr, seed):
    """40 triangles per seed; a third of the corners snapped to the half-texel lattice, where centres and edges meet exactly; some corners outside [0, 1]."""
    rng = np.random.default_rng(seed)
    w, h = (37, 29) if seed % 2 else (16, 48)
    uv = rng.uniform(-0.1, 1.1, (120, 2)).astype(F32)
    snap = rng.random(120) < 1 / 3
    uv[snap] = (np.rint(uv[snap] * [2 * w, 2 * h]) / [2 * w, 2 * h]).astype(F32)
    idx = rng.permutation(120).reshape(40, 3)
    o = _cover(_ctx(pbr), idx, uv, w, h)
    assert (o != NONE).sum() > 0.5 * w * h
    for t in (0, 17, 39):      # a triangle alone covers a superset of what it owns among others
        alone = _ctx(pbr).debug_lightmap_cover([idx[t]], uv, w, h)
        assert (alone[o == t] == 0).all()


# ---- texel records and rays ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (9, 7), (13, 5)], ids=["n1", "n63", "n65"])
def test_texel_records_and_rays_equal_reference_bit_for_bit(pbr, w, h):
    desc = patch_scene(pbr)
    pt = _ctx(pbr).load_scene(desc)
    idx, P, N, uv, eps = instance_geometry(pt, desc, 1)
    want = ref.texels(idx, uv, P, N, w, h, eps)
    n = w * h
    assert want["atlas_index"].size == n and want["dropped"] == 0
    for seed in SEEDS:
        for base in (0, 1000):
            for first, ns in ((0, 1), (3, 5), (0xFFFFFFF0, 4)):
                got = pt.debug_lightmap_rays(1, w, h, seed, first, ns, index_base=base)
                assert got["covered"] == n and got["dropped"] == 0
                assert np.array_equal(got["atlas_index"], want["atlas_index"]) and np.array_equal(got["prim"], want["prim"])
                assert _same_bits(got["origin"], want["origin"]) and _same_bits(got["normal"], want["normal"])
                ro, rd, rkey = ref.rays(want, base, seed, first, ns)
                assert got["ray_o"].shape == (ns * n, 3) and got["key"].dtype == np.uint32
                assert _same_bits(got["ray_o"], ro) and _same_bits(got["ray_d"], rd) and np.array_equal(got["key"], rkey), (seed, base, first, ns)
    assert np.abs(np.linalg.norm(want["normal"].astype(F64), axis=1) - 1).max() < 1e-6
    # an explicit uv array equal to the texcoord gives the same list; the key goes by atlas index: a one-triangle "shard" of the same atlas draws what the whole draws
    a = pt.debug_lightmap_rays(1, w, h, 7, 2, 3, uv=uv, index_base=1000)
    b = pt.debug_lightmap_rays(1, w, h, 7, 2, 3, index_base=1000)
    assert all(np.array_equal(a[k], b[k]) for k in ("atlas_index", "prim", "key")) and _same_bits(a["ray_d"], b["ray_d"])
    shard = uv.copy()
    shard[np.setdiff1d(np.arange(len(uv)), idx[0])] = 0      # every triangle but 0 collapses (a corner it shares with 0 keeps its place)
    s = pt.debug_lightmap_rays(1, w, h, 7, 2, 3, uv=shard, index_base=1000)
    mine = s["prim"] == 0
    if mine.any():
        where = np.searchsorted(b["atlas_index"], s["atlas_index"][mine])
        assert np.array_equal(b["atlas_index"][where], s["atlas_index"][mine])
        nb, nsd = b["covered"], s["covered"]
        assert np.array_equal(s["key"].reshape(3, nsd)[:, mine], b["key"].reshape(3, nb)[:, where])


def test_degenerate_world_triangles_are_dropped(pbr):
    """A triangle with a UV area and no area in the world has no normal: its texels are counted, not listed."""
    S, sc = pbr.scene, pbr.scenes
    v = sc._verts([(0, 0, 0), (1, 0, 0), (1, 0, -1), (0.5, 0, 0)], [(0, 1, 0)] * 4, [(1, 0, 0)] * 4, [(0, 0), (1, 0), (1, 1), (0, 1)])
    desc = S.SceneDesc([S.Material()], [S.MeshDesc(v, np.array([0, 1, 2, 0, 3, 1], np.uint32), 0)], [S.InstanceDesc(0)], S.CameraDesc((0, 2, 2), (0, 0, 0), 1.0, 1.0), "degenerate")
    pt = _ctx(pbr).load_scene(desc)
    got = pt.debug_lightmap_rays(0, 8, 8, 1, 0, 1)
    idx, P, N, uv, eps = instance_geometry(pt, desc, 0)
    want = ref.texels(idx, uv, P, N, 8, 8, eps)
    owner = ref.cover(idx, uv, 8, 8)
    assert want["dropped"] == (owner == 1).sum() > 0 and got["dropped"] == want["dropped"] and got["covered"] == (owner == 0).sum()
    assert (got["prim"] == 0).all() and np.array_equal(got["atlas_index"], want["atlas_index"]) and _same_bits(got["origin"], want["origin"])


def test_directions_follow_the_cosine_law(pbr):
    """65,536 directions (256 texels x 256 samples) from ptc_debug_lightmap_rays.  Every one lies in the hemisphere of its normal.  Under the cosine law cos(theta) has
    mean 2/3 and variance 1/18, and cos^2(theta) = 1 - u1 is uniform: the mean within 5 standard errors, and the chi-square statistic of 16 equal bands of
    cos^2(theta) — 15 degrees of freedom: mean 15, variance 30 — within 5 standard deviations of its mean.  The azimuth about the normal is uniform: the mean of
    the tangential part is 0 within 5 standard errors.  | |d| - 1 | <= 2^-22."""
    desc = patch_scene(pbr)
    pt = _ctx(pbr).load_scene(desc)
    got = pt.debug_lightmap_rays(1, 16, 16, 0x1234567890ABCDEF, 0, 256)
    n = got["covered"]
    assert n == 256
    d = got["ray_d"].astype(F64)
    nrm = np.tile(got["normal"].astype(F64), (256, 1))
    N = d.shape[0]
    assert N == 65536
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 2.0 ** -22
    c = (d * nrm).sum(1)
    assert (c > 0).all()
    assert ((got["ray_d"] * np.tile(got["normal"], (256, 1))).sum(1, dtype=F32) > 0).all()
    se = math.sqrt((1 / 18) / N)
    assert abs(c.mean() - 2 / 3) <= 5 * se, (c.mean(), se)
    bands = np.bincount(np.minimum((c * c * 16).astype(int), 15), minlength=16)
    chi2 = ((bands - N / 16) ** 2 / (N / 16)).sum()
    print(f"mean cos(theta) - 2/3 = {c.mean() - 2 / 3:+.2e} (standard error {se:.2e}); chi-square over 16 bands of cos^2 = {chi2:.1f} (15 +- {math.sqrt(30):.1f})")
    assert chi2 <= 15 + 5 * math.sqrt(30)
    t = d - c[:, None] * nrm
    for k in range(3):
        assert abs(t[:, k].mean()) <= 5 * t[:, k].std(ddof=1) / math.sqrt(N), k


# ---- dilation -----------------------------------------------------------------------------------------------------------------------------------------
def test_dilation_equals_reference_bit_for_bit(pbr):
    pt = _ctx(pbr)
    rng = np.random.default_rng(11)
    for w, h in ((1, 1), (7, 5), (33, 18)):
        img = np.zeros((h, w, 4), F32)
        baked = rng.random((h, w)) < 0.15
        img[baked, :3] = rng.normal(0, 3, (int(baked.sum()), 3)).astype(F32) * F32(1e3) ** rng.integers(-1, 2, (int(baked.sum()), 1)).astype(F32)
        img[baked, 3] = 1
        for k in (0, 1, 2, 5):
            got = pt.debug_lightmap_dilate(img, k)
            assert got.shape == img.shape and _same_bits(got, ref.dilate(img, k)), (w, h, k)
            assert _same_bits(got[baked], img[baked])      # baked texels never change
            assert set(np.unique(got[..., 3])) <= {0.0, 0.5, 1.0}
    # one baked texel grows to (2k + 1)^2 after k iterations, every filled texel carrying its colour (a mean of equal values, exact here)
    one = np.zeros((15, 15, 4), F32)
    one[7, 7] = (2.0, 1.0, 0.5, 1.0)
    for k in range(0, 5):
        got = pt.debug_lightmap_dilate(one, k)
        assert (got[..., 3] != 0).sum() == (2 * k + 1) ** 2 and (got[..., 3] == 1).sum() == 1
        filled = got[..., 3] == 0.5
        assert (got[filled][:, :3] == (2.0, 1.0, 0.5)).all()
        assert (got[7 - k:8 + k, 7 - k:8 + k, 3] != 0).all()
    # an iteration reads the previous image only: a texel two steps from the source stays empty after one iteration
    assert pt.debug_lightmap_dilate(one, 1)[7, 9, 3] == 0
    # an all-empty atlas stays empty
    assert not pt.debug_lightmap_dilate(np.zeros((6, 9, 4), F32), 64).any()


# ---- validation -----------------------------------------------------------------------------------------------------------------------------------------
def test_validation_state_and_device_errors(pbr):
    """Every PTC_E_ARG case; PTC_E_STATE without a committed scene and outside a lightmap frame; a valid begin then fails with PTC_E_DEVICE on a description-only
    context; nothing of the context changes and no refused call writes its output."""
    L = pbr.load_library()
    D = pbr.ptc.PtcLightmapDesc
    fpt, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)

    def desc(**kw):
        d = D()
        d.instance, d.width, d.height, d.texel_index_base, d.spp_total, d.seed, d.max_bounces = 0, 8, 8, 0, 4, 1, 2
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    out = np.zeros((8, 8, 4), F32)
    op = out.ctypes.data_as(fpt)
    fresh = _ctx(pbr)
    assert L.ptc_lightmap_begin(fresh._h, C.byref(desc())) == E_ARG      # no instance at all: unknown
    pt = _ctx(pbr).load_scene(pbr.scenes.cornell_box())
    h = pt._h
    before = (pt.get_camera_lens(), L.ptc_light_count(h))
    begin = lambda **kw: L.ptc_lightmap_begin(h, C.byref(desc(**kw)))
    render = lambda it, th, o=op, **kw: L.ptc_render_lightmap(h, C.byref(desc(**kw)), it, th, o)
    assert L.ptc_lightmap_begin(h, None) == E_ARG and b"lightmap_begin" in L.ptc_last_error(h)
    assert L.ptc_lightmap_begin(None, C.byref(desc())) == E_ARG and L.ptc_render_lightmap(None, C.byref(desc()), 0, 0.1, op) == E_ARG
    for kw in (dict(instance=-1), dict(instance=6), dict(width=0), dict(width=8193), dict(height=0), dict(height=8193), dict(spp_total=0), dict(max_bounces=-1),
               dict(texel_index_base=0xFFFFFFC1), dict(width=8192, height=8192, texel_index_base=0xFC000001)):
        assert begin(**kw) == E_ARG, kw
        assert render(0, 0.1, **kw) == E_ARG, kw
    inf, nan = float("inf"), float("nan")
    for bad in (inf, -inf, nan):
        uv = QUAD_UV.copy()
        uv[2, 1] = bad
        assert begin(uv=uv.ctypes.data_as(fpt)) == E_ARG, bad
    for it, th in ((-1, 0.1), (65, 0.1), (0, -0.5), (0, nan), (0, inf)):
        assert render(it, th) == E_ARG, (it, th)
        assert L.ptc_lightmap_read(h, it, th, op, None) == E_ARG, (it, th)
    assert render(0, 0.1, o=None) == E_ARG and L.ptc_lightmap_read(h, 0, 0.1, None, None) == E_ARG and L.ptc_lightmap_read(None, 0, 0.1, op, None) == E_ARG
    # valid arguments: the last texel index is 2^32 - 1
    assert begin() == E_DEVICE and begin(texel_index_base=0xFFFFFFC0) == E_DEVICE and begin(uv=QUAD_UV.ctypes.data_as(fpt)) == E_DEVICE
    assert render(2, 0.0) == E_DEVICE and render(64, 1e30) == E_DEVICE
    with pytest.raises(pbr.PtcError, match="ptc error -3"):
        pt.render_lightmap(0, 8, 8, 4)
    with pytest.raises(pbr.PtcError, match="ptc error -1"):
        pt.render_lightmap(0, 8, 8, 0)
    with pytest.raises(pbr.PtcError):
        pt.render_lightmap(0, 8, 8, 4, uv=np.zeros((4, 3), F32))
    # outside a lightmap frame
    n = C.c_uint32(7)
    assert L.ptc_lightmap_texel_count(h, C.byref(n), None) == E_STATE and n.value == 7 and L.ptc_lightmap_texel_count(None, None, None) == E_ARG
    assert L.ptc_lightmap_read_texels(h, None, None, op, op) == E_STATE and L.ptc_lightmap_read_texels(None, None, None, None, None) == E_ARG
    assert L.ptc_lightmap_read(h, 2, 0.1, op, None) == E_STATE and b"lightmap_read" in L.ptc_last_error(h)
    assert (pt.get_camera_lens(), L.ptc_light_count(h)) == before and not out.any()
    # the hooks
    owner = np.zeros((4, 4), np.uint32)
    idx = QUAD_IDX.copy()
    ip, up, wp = idx.ctypes.data_as(u32p), QUAD_UV.ctypes.data_as(fpt), owner.ctypes.data_as(u32p)
    cover = L.ptc_debug_lightmap_cover
    assert cover(h, None, 2, up, 4, 4, 4, wp) == E_ARG and cover(h, ip, 2, None, 4, 4, 4, wp) == E_ARG and cover(h, ip, 2, up, 4, 4, 4, None) == E_ARG
    assert cover(h, ip, 0, up, 4, 4, 4, wp) == E_ARG and cover(h, ip, 2, up, 3, 4, 4, wp) == E_ARG      # an index >= n_verts
    assert cover(h, ip, 2, up, 4, 0, 4, wp) == E_ARG and cover(h, ip, 2, up, 4, 4, 8193, wp) == E_ARG and cover(None, ip, 2, up, 4, 4, 4, wp) == E_ARG
    assert not owner.any() and cover(h, ip, 2, up, 4, 4, 4, wp) == 0 and (owner != NONE).all()
    counts = np.zeros(2, np.uint32)
    cp = counts.ctypes.data_as(u32p)
    rays = L.ptc_debug_lightmap_rays
    assert rays(h, C.byref(desc()), 0, 1, None, None, None, None, None, None, None) == E_ARG and rays(h, None, 0, 1, cp, None, None, None, None, None, None) == E_ARG
    assert rays(h, C.byref(desc()), 0, 0, cp, None, None, None, None, None, None) == E_ARG and rays(h, C.byref(desc()), 0xFFFFFFFF, 2, cp, None, None, None, None, None, None) == E_ARG
    assert rays(h, C.byref(desc(instance=9)), 0, 1, cp, None, None, None, None, None, None) == E_ARG and rays(None, C.byref(desc()), 0, 1, cp, None, None, None, None, None, None) == E_ARG
    assert rays(h, C.byref(desc(width=8192, height=8192)), 0, 32, cp, None, None, None, None, None, None) == E_ARG      # 2^31 paths
    assert not counts.any()
    assert rays(h, C.byref(desc(spp_total=0, max_bounces=-1)), 0, 1, cp, None, None, None, None, None, None) == 0 and counts[0] == 64      # the budget is not read; the floor fills its atlas
    dil = L.ptc_debug_lightmap_dilate
    assert dil(h, 8, 8, 1, None) == E_ARG and dil(h, 0, 8, 1, op) == E_ARG and dil(h, 8, 8, -1, op) == E_ARG and dil(h, 8, 8, 65, op) == E_ARG and dil(None, 8, 8, 1, op) == E_ARG
    assert dil(h, 8, 8, 64, op) == 0 and not out.any()


def test_begin_before_commit_is_a_state_error(pbr):
    """The arguments are valid for the description (instance 0 exists), the scene is not committed: PTC_E_STATE, from the hook too."""
    L = pbr.load_library()
    pt = _ctx(pbr).load_scene(pbr.scenes.cornell_box())
    d = pbr.ptc.PtcLightmapDesc()
    d.instance, d.width, d.height, d.spp_total, d.max_bounces = 0, 4, 4, 1, 0
    assert L.ptc_lightmap_begin(pt._h, C.byref(d)) == E_DEVICE
    assert L.ptc_scene_begin(pt._h) == 0      # the description is gone, and the commit with it
    assert L.ptc_lightmap_begin(pt._h, C.byref(d)) == E_ARG      # no instance: unknown
    v = pbr.scenes.cornell_box().meshes[0]
    assert L.ptc_add_material(pt._h, (C.c_float * 4)(1, 1, 1, 1), C.c_float(0), C.c_float(1), (C.c_float * 3)(0, 0, 0), -1, -1, -1) >= 0
    assert L.ptc_add_mesh(pt._h, C.c_void_p(v.vertices.ctypes.data), len(v.vertices), v.indices.ctypes.data_as(C.POINTER(C.c_uint32)), v.indices.size, 0) >= 0
    assert L.ptc_add_instance(pt._h, 0, (C.c_float * 3)(0, 0, 0), (C.c_float * 4)(1, 0, 0, 0), (C.c_float * 3)(1, 1, 1)) >= 0
    counts = np.zeros(2, np.uint32)
    assert L.ptc_lightmap_begin(pt._h, C.byref(d)) == E_STATE and b"not committed" in L.ptc_last_error(pt._h)
    assert L.ptc_debug_lightmap_rays(pt._h, C.byref(d), 0, 1, counts.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None, None, None, None) == E_STATE


def test_cli_refuses_bad_lightmap_arguments_before_any_device_work(pbr):
    """ptc_render --lightmap / --lightmap-out: exit code 1 and the reason, on a machine without a GPU too."""
    import subprocess

    exe = os.path.join(os.path.dirname(pbr.ptc.LIB_PATH), "ptc_render")
    ok = ["--lightmap", "0:8x8", "--lightmap-out", "x.pfm"]
    for args, text in ((["--lightmap", "0:8x8"], "--lightmap-out"), (["--lightmap-out", "x.pfm"], "--lightmap INSTANCE:WxH"), (["--lightmap", "0:8", "--lightmap-out", "x.pfm"], "1..8192"),
                       (["--lightmap", "0:0x8", "--lightmap-out", "x.pfm"], "1..8192"), (["--lightmap", "-1:8x8", "--lightmap-out", "x.pfm"], "instance index"),
                       (["--lightmap", "0:8x8193", "--lightmap-out", "x.pfm"], "1..8192"), (ok + ["--raster"], "path integrator"), (ok + ["--spp", "0"], "--spp"),
                       (ok + ["--lightmap-dilate", "65"], "0..64"), (ok + ["--lightmap-backface", "-0.1"], "fraction"), (ok + ["--probe-grid", "2,2,2", "--probes-out", "s.pfm"], "probes")):
        r = subprocess.run([exe, "--scene", "cornell"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and text in r.stderr and "ptc_create" not in r.stderr, (args, r.stderr)
