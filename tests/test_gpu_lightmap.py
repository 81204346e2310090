"""Lightmaps on a real MI355X (include/ptc_lightmap.h; csrc/pt_lightmap.hip).

1. The kernels against the definition: k_lm_cover, the compaction, k_lm_texels, k_raygen_texel and k_lm_dilate through the debug hooks against the host evaluation
   of a description-only context (which tests/test_lightmap_host.py holds to tests/lightmap_reference.py), bit for bit.
2. However the samples are cut — calls, batches, lanes, texel shards, sample-range shards — the atlas is bit for bit the same.
3. Closed forms: a constant environment exactly; a wall and an emitter against float64 form factors within 5 binomial standard errors; a furnace.
4. Validity: a box standing through the floor, the dilation of what it hides.
5. Neighbours: a refit on the device, camera frames around a lightmap frame, the refusals of a lightmap frame, the kernel hash, the command-line tool."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lightmap_reference as ref  # noqa: E402
from test_lightmap_host import instance_geometry, patch_scene  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
E_ARG, E_STATE = -1, -2
SEED = 0x5EED0FC0FFEE1234
NONE = 0xFFFFFFFF
PI32 = float(F32(3.1415927))


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _host(pbr):
    return pbr.PathTracer(pbr.ptc.DEVICE_NONE)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------------
def _flat(pbr, meshes, env=None, name="lightmap", transforms=None):
    """meshes: [(vertices, indices, material)] one instance each, materials: 0 black, 1 grey, 2 emitter (4, 2, 1)."""
    S = pbr.scene
    mats = [S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0), S.Material((0.5, 0.5, 0.5, 1.0), 0.0, 1.0), S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (4.0, 2.0, 1.0))]
    md = [S.MeshDesc(v, i, m) for v, i, m in meshes]
    inst = [S.InstanceDesc(k, **((transforms or {}).get(k, {}))) for k in range(len(md))]
    d = S.SceneDesc(mats, md, inst, S.CameraDesc((0.0, 3.0, 3.0), (0.0, 0.0, 0.0), 1.0, 1.0), name)
    if env is not None:
        d.env = np.broadcast_to(np.asarray(env, F32), (2, 4, 3)).copy()      # a constant lat-long map
    return d


def _floor(pbr, half=1.0, mat=0):
    """[-half, half]^2 at y = 0, normal +y; uv (0, 0) at (-half, +half) and (1, 1) at (+half, -half): x = (2u - 1) half, z = (1 - 2v) half."""
    v, i = pbr.scenes._quad((-half, 0, half), (half, 0, half), (half, 0, -half), (-half, 0, -half))
    return v, i, mat


def _texel_xz(w, h, half=1.0):
    u, v = (np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h
    return np.meshgrid((2 * u - 1) * half, (1 - 2 * v) * half)      # (h, w) each


L_ENV = np.array([1.0, 0.5, 0.25])
WALL = np.array([(1.0, 0.25, -1.0), (1.0, 0.25, 1.0), (1.0, 1.5, 1.0), (1.0, 1.5, -1.0)])          # at x = 1, front towards -x, floating above the floor's plane
PANEL = np.array([(-0.5, 1.0, -0.25), (0.5, 1.0, -0.25), (0.5, 1.0, 0.75), (-0.5, 1.0, 0.75)])      # at y = 1, front towards -y


def _wall_scene(pbr):
    return _flat(pbr, [_floor(pbr), pbr.scenes._quad(*WALL) + (0,)], env=L_ENV, name="lightmap_wall")


def _panel_scene(pbr, flipped=False):
    t = {0: dict(q_wxyz=(0.0, 1.0, 0.0, 0.0))} if flipped else None      # half a turn about x: the floor looks down
    return _flat(pbr, [_floor(pbr), pbr.scenes._quad(*PANEL) + (2,)], name="lightmap_panel", transforms=t)


def _hits_rect(corners):
    """hits(o, d) for the rectangle `corners` (a, b, c, d in order), float64, either side."""
    a, e1, e2 = corners[0], corners[1] - corners[0], corners[3] - corners[0]
    n = np.cross(e1, e2)

    def hits(o, d):
        den = d @ n
        with np.errstate(all="ignore"):
            t = ((a - o) @ n) / den
        p = o + t[:, None] * d - a
        s, r = (p @ e1) / (e1 @ e1), (p @ e2) / (e2 @ e2)
        return (den != 0) & (t > 0) & (s >= 0) & (s <= 1) & (r >= 0) & (r <= 1)
    return hits


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------------------------------
def _kernel_scene(pbr):
    """Instances of 2 (an emitter), 1, 2 and 130 triangles: a lone triangle, a quad, a displaced 13 x 5 grid patch under a rotation and a non-uniform scale."""
    S, sc = pbr.scene, pbr.scenes
    d = patch_scene(pbr, 13, 5)
    tri = sc._verts([(-2.0, 0.5, 0.0), (-1.0, 0.5, 0.3), (-1.6, 1.4, -0.2)], [(0.1, 0.2, 1.0), (-0.2, 0.1, 1.0), (0.0, -0.3, 1.0)], [(1, 0, 0)] * 3, [(0.05, 0.1), (0.95, 0.2), (0.4, 0.9)])
    qv, qi = sc._quad((1.5, 0.0, 0.5), (2.5, 0.2, 0.5), (2.5, 0.4, -0.5), (1.5, 0.2, -0.5))
    patch, patch_inst = d.meshes[1], d.instances[1]
    d.meshes = [d.meshes[0], S.MeshDesc(tri, np.array([0, 1, 2], np.uint32), 1), S.MeshDesc(qv, qi, 1), patch]
    d.instances = [d.instances[0], S.InstanceDesc(1), S.InstanceDesc(2), S.InstanceDesc(3, patch_inst.t, patch_inst.q_wxyz, patch_inst.s)]
    return d


@pytest.fixture(scope="module")
def kernel_ctx(gpu):
    d = _kernel_scene(gpu)
    pt, host = gpu.PathTracer(0).load_scene(d), _host(gpu).load_scene(d)
    yield pt, host, d
    pt.close()


@pytest.mark.parametrize("w,h", [(1, 1), (63, 65), (256, 256)])
@pytest.mark.parametrize("instance", [1, 2, 3], ids=["1_triangle", "2_triangles", "130_triangles"])
def test_kernels_equal_host_evaluation_bit_for_bit(kernel_ctx, instance, w, h):
    """One wave per triangle (130 triangles: 33 blocks of four waves, the last half empty), one thread per texel and per entry (63 x 65 and the lists it gives are no
    multiples of 64 or 256; 256 x 256 is 256 blocks for the compaction's scan), one thread per path.  The sample range starts above 0 and the index base is not 0."""
    pt, host, d = kernel_ctx
    m = d.meshes[d.instances[instance].mesh]
    idx, uv = m.indices.reshape(-1, 3), m.vertices["texCoords"]
    assert len(idx) == (1, 2, 130)[instance - 1]
    owner = pt.debug_lightmap_cover(idx, uv, w, h)
    assert np.array_equal(owner, host.debug_lightmap_cover(idx, uv, w, h))
    ns = 2 if w * h > 10000 else 5
    got = pt.debug_lightmap_rays(instance, w, h, SEED, 7, ns, index_base=1000)
    want = host.debug_lightmap_rays(instance, w, h, SEED, 7, ns, index_base=1000)
    assert got["covered"] == want["covered"] == int((owner != NONE).sum()) and got["dropped"] == want["dropped"] == 0
    if (w, h) != (1, 1) or instance == 3:
        assert got["covered"] > 0
    for k in ("atlas_index", "prim", "key"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("origin", "normal", "ray_o", "ray_d"):
        assert _bits_equal(got[k], want[k]), k
    assert np.array_equal(got["prim"], owner.reshape(-1)[got["atlas_index"]]) and (np.diff(got["atlas_index"].astype(np.int64)) > 0).all()
    if w * h <= 10000:      # and the numpy restatement itself, where it is quick
        _, P, N, _, eps = instance_geometry(host, d, instance)
        r = ref.texels(idx, uv, P, N, w, h, eps)
        assert np.array_equal(r["atlas_index"], got["atlas_index"]) and _bits_equal(r["origin"], got["origin"]) and _bits_equal(r["normal"], got["normal"])
        if got["covered"]:
            assert _bits_equal(ref.rays(r, 1000, SEED, 7, ns)[1], got["ray_d"])


@pytest.mark.parametrize("w,h", [(1, 1), (63, 65), (256, 256)])
def test_dilate_kernel_equals_host_evaluation(kernel_ctx, w, h):
    pt, host, _ = kernel_ctx
    rng = np.random.default_rng(w)
    img = np.zeros((h, w, 4), F32)
    baked = rng.random((h, w)) < 0.1
    img[baked, :3] = rng.normal(0, 3, (int(baked.sum()), 3)).astype(F32)
    img[baked, 3] = 1
    for k in (1, 3):
        assert _bits_equal(pt.debug_lightmap_dilate(img, k), host.debug_lightmap_dilate(img, k)), k


# ---- 2. however the samples are cut -------------------------------------------------------------------------------------------------------------------------
LM = dict(instance=0, width=24, height=20, seed=SEED, max_bounces=3)      # the Cornell box's floor


@pytest.fixture(scope="module")
def cornell(gpu):
    pt = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    yield pt
    pt.close()


def _bake(pt, spp=16, steps=None, sync=False, dilate=0, **kw):
    a = dict(LM, **kw)
    pt.lightmap_begin(a["instance"], a["width"], a["height"], spp, uv=a.get("uv"), seed=a["seed"], max_bounces=a["max_bounces"], index_base=a.get("index_base", 0))
    for k in steps or [spp]:
        pt.frame_add_samples(k)
        if sync:
            pt.sync()
    return pt.read_lightmap(dilate=dilate, with_backface=True)


@pytest.fixture(scope="module")
def whole(cornell):
    """The floor of the Cornell box, 24 x 20 texels, 16 samples, 3 bounces, in one call: the result everything in 2 must reproduce.  Computed once, never written to."""
    atlas, back = _bake(cornell)
    atlas.setflags(write=False)
    back.setflags(write=False)
    assert atlas.shape == (20, 24, 4) and (atlas[..., 3] == 1).all() and (atlas[..., :3] > 0).all() and np.isfinite(atlas).all() and not back.any()
    return atlas, back


def test_render_lightmap_is_begin_add_read(cornell, whole):
    assert _bits_equal(cornell.render_lightmap(0, 24, 20, 16, seed=SEED, max_bounces=3, dilate=0), whole[0])
    assert cornell.lightmap_texel_count() == (480, 0)
    t = cornell.lightmap_texels()
    assert np.array_equal(t["atlas_index"], np.arange(480)) and set(np.unique(t["prim"])) == {0, 1} and _bits_equal(t["normal"], np.tile(F32([0, 1, 0]), (480, 1)))
    assert (t["origin"][:, 1] > -1).all() and (t["origin"][:, 1] < -0.999).all()      # lifted off the floor at y = -1 by the ray epsilon


def test_sample_splits_leave_the_result_unchanged(cornell, whole):
    assert _bits_equal(_bake(cornell, steps=[5, 11])[0], whole[0])             # a held-back remainder merges with the next call
    assert _bits_equal(_bake(cornell, steps=[1] * 16, sync=True)[0], whole[0])  # sixteen batches of one sample
    cornell.lightmap_begin(0, 24, 20, 16, seed=SEED, max_bounces=3)
    cornell.frame_add_samples(4)
    part = cornell.read_lightmap(dilate=0)
    cornell.frame_add_samples(12)
    assert _bits_equal(cornell.read_lightmap(dilate=0), whole[0]) and not _bits_equal(part, whole[0])      # N is the samples accumulated
    # sample-range shards: partial sums with the whole frame's divisor; pi / 16 is half of pi / 8, exactly
    cornell.lightmap_begin(0, 24, 20, 8, seed=SEED, max_bounces=3)
    cornell.frame_set_sample_range(0, 16)
    cornell.frame_add_samples(8)
    lo = cornell.read_lightmap(dilate=0)
    cornell.lightmap_begin(0, 24, 20, 8, seed=SEED, max_bounces=3)
    cornell.frame_set_sample_range(8, 16)
    cornell.frame_add_samples(8)
    hi = cornell.read_lightmap(dilate=0)
    cornell.lightmap_begin(0, 24, 20, 8, seed=SEED, max_bounces=3)
    cornell.frame_add_samples(8)
    first8 = cornell.read_lightmap(dilate=0)
    assert _bits_equal(lo[..., :3], (first8[..., :3] * F32(0.5)).astype(F32))
    assert np.abs((lo[..., :3].astype(F64) + hi[..., :3]) - whole[0][..., :3]).max() <= 2.0 ** -22 * whole[0][..., :3].max()      # the two halves add up to the whole, up to the order of the sum


@pytest.mark.parametrize("env", [dict(PTC_BATCH_PATHS="1024"), dict(PTC_LANES="2"), dict(PTC_LANES="2", PTC_BATCH_PATHS="1024")], ids=["small_batches", "two_lanes", "two_lanes_small_batches"])
def test_batches_and_lanes_leave_the_result_unchanged(gpu, whole, env):
    """PTC_BATCH_PATHS=1024: 2 samples of 480 texels per batch on one lane, 1 on each of two — the frame spans 8 or 16 batches, which alternate between the lanes;
    the back-face counts are integer sums."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pt = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    atlas, back = _bake(pt)
    pt.close()
    assert _bits_equal(atlas, whole[0]) and _bits_equal(back, whole[1])


def test_texel_shards_merge_to_the_whole(cornell, whole):
    """The key goes by atlas index: the floor baked one triangle at a time (the other's UVs collapsed) gives, texel by texel, what the whole bake gives; on the
    shared edge the lower primitive's shard has the whole's owner.  An index base shifts every key."""
    uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], F32)
    a_uv, b_uv = uv.copy(), uv.copy()
    a_uv[3] = a_uv[0]      # triangle 1 = (0, 2, 3) collapses to an edge
    b_uv[1] = b_uv[0]      # triangle 0 = (0, 1, 2) likewise
    a, _ = _bake(cornell, uv=a_uv)
    ta = cornell.lightmap_texels()
    b, _ = _bake(cornell, uv=b_uv)
    tb = cornell.lightmap_texels()
    assert (ta["prim"] == 0).all() and (tb["prim"] == 1).all() and 0 < ta["prim"].size < 480 and ta["prim"].size + tb["prim"].size >= 480
    merged = np.where(a[..., 3:] == 1, a, b)
    assert (a[..., 3] + b[..., 3] >= 1).all() and _bits_equal(merged, whole[0])
    assert not _bits_equal(_bake(cornell, index_base=480)[0], whole[0])


# ---- 3. closed forms ----------------------------------------------------------------------------------------------------------------------------------------
def test_constant_environment_is_exact(gpu):
    """A lone floor under a constant sky: every path misses, the sum of 64 equal powers of two is exact, and so is the product with pi / 64."""
    pt = gpu.PathTracer(0).load_scene(_flat(gpu, [_floor(gpu)], env=L_ENV, name="lightmap_sky"))
    pt.lightmap_begin(0, 13, 7, 64, seed=SEED, max_bounces=2)
    pt.frame_add_samples(64)
    atlas, back = pt.read_lightmap(dilate=0, with_backface=True)
    pt.close()
    assert atlas.shape == (7, 13, 4) and (atlas[..., 3] == 1).all() and back.shape == (91,) and not back.any()
    assert _bits_equal(atlas[..., :3], np.broadcast_to((F32(3.1415927) * L_ENV.astype(F32)).astype(F32), (7, 13, 3)))


def _binomial_check(E, scale, frac_want, N, what):
    """E (h, w, 3) against scale[c] * frac_want (h, w) with the binomial standard error scale sqrt(F (1 - F) / N) per texel: at most 1 % of the texels beyond 5."""
    F = frac_want[..., None]
    se = scale * np.sqrt(np.maximum(F * (1 - F), 0) / N)
    with np.errstate(all="ignore"):
        z = np.where(se > 0, np.abs(E.astype(F64) - scale * F) / se, np.where(np.abs(E - scale * F) <= 1e-6 * scale, 0.0, np.inf))
    out = (z > 5).any(-1).mean()
    print(f"{what}: largest |error| / standard error {z.max():.2f}, texels beyond 5: {100 * out:.2f} % (bound 1 %)")
    assert out <= 0.01


def test_wall_shadows_the_sky_by_its_form_factor(gpu):
    """The floor beside a black wall under a constant sky, max_bounces = 0: a path that meets the wall returns nothing, one that misses it returns L, so
    E = pi L (1 - F) with F the wall's form factor at the texel.  N = 256, 16 x 16 texels.  The size and the seed are first checked here on the CPU with the
    reference's own sampler; the device must then count what that sampler counts, up to rays that graze the wall's outline."""
    d, w, h, N = _wall_scene(gpu), 16, 16, 256
    host = _host(gpu).load_scene(d)
    tex = host.debug_lightmap_rays(0, w, h, SEED, 0, 1, rays=False)
    assert tex["covered"] == w * h
    F = ref.rect_form_factor(tex["origin"].astype(F64), tex["normal"].astype(F64), WALL).reshape(h, w)
    assert 0.05 < F.max() < 0.5 and F.min() > 1e-3 and F[:, 8:].mean() > 2 * F[:, :8].mean()      # larger on the half towards the wall at u = 1
    seen = 1 - ref.sampled_fraction(tex, 0, SEED, N, _hits_rect(WALL)).reshape(h, w)
    _binomial_check(np.pi * L_ENV * seen[..., None], np.pi * L_ENV, 1 - F, N, "reference sampler, wall")
    pt = gpu.PathTracer(0).load_scene(d)
    pt.lightmap_begin(0, w, h, N, seed=SEED, max_bounces=0)
    pt.frame_add_samples(N)
    E, back = pt.read_lightmap(dilate=0, with_backface=True)
    pt.close()
    assert (E[..., 3] == 1).all() and not back.any()      # the wall is met from its front
    _binomial_check(E[..., :3], np.pi * L_ENV, 1 - F, N, "device, wall")
    same = np.abs(E[..., 0] / PI32 - seen) <= 1e-6
    print(f"texels where the device counted what the reference sampler counted: {100 * same.mean():.1f} %")
    assert same.mean() >= 0.99


def test_emitter_lights_the_floor_by_its_form_factor(gpu):
    """A one-sided emissive panel above the floor, no sky, max_bounces = 0: E = pi Le F.  The same floor turned upside-down looks away from everything: 0."""
    d, w, h, N = _panel_scene(gpu), 16, 16, 256
    Le = np.array([4.0, 2.0, 1.0])
    host = _host(gpu).load_scene(d)
    tex = host.debug_lightmap_rays(0, w, h, SEED, 0, 1, rays=False)
    F = ref.rect_form_factor(tex["origin"].astype(F64), tex["normal"].astype(F64), PANEL).reshape(h, w)
    assert 0.1 < F.max() < 0.5 and F.min() > 1e-3
    seen = ref.sampled_fraction(tex, 0, SEED, N, _hits_rect(PANEL)).reshape(h, w)
    _binomial_check(np.pi * Le * seen[..., None], np.pi * Le, F, N, "reference sampler, panel")
    pt = gpu.PathTracer(0).load_scene(d)
    pt.lightmap_begin(0, w, h, N, seed=SEED, max_bounces=0)
    pt.frame_add_samples(N)
    E, back = pt.read_lightmap(dilate=0, with_backface=True)
    pt.close()
    assert (E[..., 3] == 1).all() and not back.any()      # the panel is met from its front
    _binomial_check(E[..., :3], np.pi * Le, F, N, "device, panel")
    pt = gpu.PathTracer(0).load_scene(_panel_scene(gpu, flipped=True))
    E = pt.render_lightmap(0, w, h, 64, seed=SEED, max_bounces=0, dilate=0)
    t = pt.lightmap_texels()
    pt.close()
    assert (t["normal"][:, 1] < -0.999).all() and (t["origin"][:, 1] < 0).all()
    assert (E[..., 3] == 1).all() and not E[..., :3].any()


def test_furnace(gpu):
    """The floor (the face -y) of tests/test_gpu_probes.py's furnace — a closed cube whose faces all emit Le, albedo 0 — at that test's bounce depth, 0: every
    sample's radiance is Le, so E / pi is Le, that test's expected radiance.  16 seeds estimate the standard error of the mean, which is 0 here up to rounding:
    what remains is float32 — the running sum of N equal terms and the resolve, (N + 2) 2^-24 relative as in that test, and the float32 constant pi, which the
    comparison divides by."""
    from test_gpu_probes import ALL_FACES, _cube

    Le, N = np.array([2.0, 1.0, 0.5]), 64
    pt = gpu.PathTracer(0).load_scene(_cube(gpu, ALL_FACES, Le))
    floor = 2 * 1 + 1      # instances in the order (+x, -x, +y, -y, +z, -z)
    means = []
    for seed in range(16):
        E = pt.render_lightmap(floor, 8, 8, N, seed=seed, max_bounces=0, dilate=0)
        assert (E[..., 3] == 1).all()
        means.append(E[..., :3].astype(F64).mean((0, 1)) / PI32)
    t = pt.lightmap_texels()
    pt.close()
    assert (t["normal"][:, 1] > 0.999).all()      # the floor's front looks at the centre
    means = np.array(means)
    se = means.std(0, ddof=1) / math.sqrt(16)
    err = np.abs(means.mean(0) - Le)
    print(f"furnace: |E / pi - Le| / Le = {err / Le}, standard error over 16 seeds {se}, float32 allowance {(N + 2) * 2.0 ** -24:.3e}")
    assert (err <= 5 * se + Le * (N + 2) * 2.0 ** -24).all()


# ---- 4. validity ----------------------------------------------------------------------------------------------------------------------------------------------
def _box(pbr, lo, hi):
    """A closed box, outward fronts: 6 quads in one mesh."""
    S = pbr.scenes
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    faces = [((x1, y0, z1), (x1, y0, z0), (x1, y1, z0), (x1, y1, z1)), ((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)),
             ((x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0)), ((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)),
             ((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)), ((x1, y0, z0), (x0, y0, z0), (x0, y1, z0), (x1, y1, z0))]
    vs, is_ = [], []
    for k, f in enumerate(faces):
        v, i = S._quad(*f)
        centre = np.mean(f, 0) - (np.array(lo) + hi) / 2
        assert v["normal"][0] @ centre > 0      # outward
        vs.append(v)
        is_.append(i + 4 * k)
    return np.concatenate(vs), np.concatenate(is_).astype(np.uint32), 1


def test_texels_inside_geometry_are_invalid_and_dilated(gpu):
    """A closed box [-0.5, 0.5] x [-0.5, 1] x [-0.5, 0.5] standing through a floor of [-2, 2]^2 under a constant sky, 16 x 16 texels of 0.25: the box's outline runs
    between texel centres.  From inside, every ray meets the box's faces from behind; from outside, none does."""
    d = _flat(gpu, [_floor(gpu, 2.0, mat=1), _box(gpu, (-0.5, -0.5, -0.5), (0.5, 1.0, 0.5))], env=L_ENV, name="lightmap_box")
    pt = gpu.PathTracer(0).load_scene(d)
    pt.lightmap_begin(0, 16, 16, 32, seed=SEED, max_bounces=1)
    pt.frame_add_samples(32)
    raw, back = pt.read_lightmap(dilate=0, backface_threshold=1.0, with_backface=True)
    cut = pt.read_lightmap(dilate=0, backface_threshold=0.1)
    filled = pt.read_lightmap(dilate=2, backface_threshold=0.1)
    half = pt.read_lightmap(dilate=0, backface_threshold=0.999)      # 1 > 0.999: still invalid
    pt.close()
    X, Z = _texel_xz(16, 16, 2.0)
    inside = (np.abs(X) < 0.5) & (np.abs(Z) < 0.5)
    assert inside.sum() == 16
    back = back.reshape(16, 16)
    assert (back[inside] == 1).all() and (back[~inside] == 0).all()
    assert (raw[..., 3] == 1).all()                                           # threshold 1: nothing is invalid
    assert np.array_equal(cut[..., 3] == 0, inside) and _bits_equal(cut[~inside], raw[~inside]) and not cut[inside].any()      # exactly the inside entries
    assert _bits_equal(half, cut)
    assert _bits_equal(filled, ref.dilate(cut, 2))
    assert (filled[inside][:, 3] == 0.5).all() and (filled[inside][:, :3] > 0).all() and _bits_equal(filled[~inside], raw[~inside])
    ring = inside & ~((np.abs(X) < 0.25) & (np.abs(Z) < 0.25))               # the 12 texels next to the outline: filled by the first iteration from baked neighbours
    one = ref.dilate(cut, 1)
    assert (one[ring][:, 3] == 0.5).all() and (one[inside & ~ring][:, 3] == 0).all() and _bits_equal(filled[ring], one[ring])


# ---- 5. neighbours ------------------------------------------------------------------------------------------------------------------------------------------
def test_bake_follows_a_refit_on_the_device(gpu):
    """update_instance + scene_refit: the world vertices the bake reads are the ones the refit left in HBM — the host evaluation on the moved vertices, bit for bit."""
    d = _kernel_scene(gpu)
    pt, host = gpu.PathTracer(0).load_scene(d), _host(gpu).load_scene(d)
    before = pt.debug_lightmap_rays(3, 20, 12, 1, 0, 1, rays=False)
    a = math.radians(40.0)
    for c in (pt, host):
        c.update_instance(3, t=(0.5, 0.3, -0.2), q_wxyz=(math.cos(a / 2), 0.0, math.sin(a / 2), 0.0), s=(1.2, 1.0, 0.8))
        c.scene_refit()
    L = gpu.load_library()
    out = (C.c_uint64 * 8)()
    assert L.ptc_debug_get_internals(pt._h, out) == 0 and out[7] & 1      # the refit ran on the device
    pt.lightmap_begin(3, 20, 12, 4, seed=1, max_bounces=1)
    got = pt.lightmap_texels()
    pt.frame_add_samples(4)
    atlas = pt.read_lightmap(dilate=0, backface_threshold=1.0)      # an open, bumpy patch: a ray below the geometric plane may meet its own back
    want = host.debug_lightmap_rays(3, 20, 12, 1, 0, 1, rays=False)
    pt.close()
    assert got["atlas_index"].size == want["covered"] == 240 and np.array_equal(got["atlas_index"], want["atlas_index"]) and np.array_equal(got["prim"], want["prim"])
    assert _bits_equal(got["origin"], want["origin"]) and _bits_equal(got["normal"], want["normal"])
    assert not _bits_equal(got["origin"], before["origin"]) and np.isfinite(atlas).all() and (atlas[..., 3] == 1).all()


def test_camera_frames_around_a_lightmap_frame(gpu, cornell, whole):
    before = cornell.render(48, 32, 4, seed=9, max_bounces=3)
    assert _bits_equal(_bake(cornell)[0], whole[0])
    after = cornell.render(48, 32, 4, seed=9, max_bounces=3)
    assert after.shape == (32, 48, 4) and _bits_equal(before, after)
    fresh = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())             # a context that never baked
    assert _bits_equal(fresh.render(48, 32, 4, seed=9, max_bounces=3), after)
    fresh.close()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):                    # the camera frame left lightmap mode
        cornell.read_lightmap()


def test_refusals_in_a_lightmap_frame(gpu, cornell, whole):
    """PTC_E_STATE, and the frame goes on as if nothing had been called."""
    L, pt = gpu.load_library(), cornell
    h = pt._h
    out = np.zeros((20, 24, 4), F32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    pt.render(16, 16, 1, seed=1, max_bounces=1)
    assert L.ptc_lightmap_read(h, 0, 0.1, fp, None) == E_STATE and b"lightmap_read" in L.ptc_last_error(h)      # outside a lightmap frame
    assert L.ptc_lightmap_texel_count(h, None, None) == E_STATE and L.ptc_lightmap_read_texels(h, None, None, None, None) == E_STATE
    d = gpu.ptc.PtcLightmapDesc()
    d.instance, d.width, d.height, d.spp_total, d.seed, d.max_bounces = 0, 0, 20, 16, SEED, 3
    assert L.ptc_lightmap_begin(h, C.byref(d)) == E_ARG
    pt.frame_resolve()                                                         # PTC_E_ARG changed nothing: the camera frame is still the frame
    pt.probes_begin(np.zeros((3, 3), F32), 4, seed=1, max_bounces=1)
    assert L.ptc_lightmap_read(h, 0, 0.1, fp, None) == E_STATE                # a probe frame is no lightmap frame
    pt.lightmap_begin(0, 24, 20, 16, seed=SEED, max_bounces=3)
    pt.frame_add_samples(5)
    n64, u32, f1 = C.c_uint64(0), C.c_uint32(0), C.c_float(0)
    px = np.zeros(1, np.uint32)
    calls = {
        "probes_read_sh": lambda: L.ptc_probes_read_sh(h, fp),
        "frame_guides": lambda: L.ptc_frame_guides(h),
        "set_sample_covariance": lambda: L.ptc_set_sample_covariance(h, 1),
        "frame_set_adaptive": lambda: L.ptc_frame_set_adaptive(h, None),
        "frame_adapt": lambda: L.ptc_frame_adapt(h, C.byref(n64)),
        "denoise": lambda: L.ptc_denoise(h, None),
        "denoise_sampled": lambda: L.ptc_denoise_sampled(h, None),
        "denoise_accumulated": lambda: L.ptc_denoise_accumulated(h, None),
        "temporal_accumulate": lambda: L.ptc_temporal_accumulate(h, None),
        "frame_checkpoint": lambda: L.ptc_frame_checkpoint(h, None, C.byref(n64), C.byref(u32)),
        "frame_restore": lambda: L.ptc_frame_restore(h, fp, 480, 0),
        "comm_reduce_radiance": lambda: L.ptc_comm_reduce_radiance(h, 0),
        "focus_distance_at_pixel": lambda: L.ptc_focus_distance_at_pixel(h, 0, 0, C.byref(f1)),
        "debug_camera_rays": lambda: L.ptc_debug_camera_rays(h, 4, 4, 1, 0, 1, px.ctypes.data_as(C.POINTER(C.c_uint32)), 1, fp, fp),
    }
    for name, call in calls.items():
        assert call() == E_STATE, name
    assert L.ptc_set_sample_covariance(h, 0) == 0                              # switching it off is no request for statistics
    assert L.ptc_lightmap_read(h, 65, 0.1, fp, None) == E_ARG and L.ptc_lightmap_read(h, 0, -1.0, fp, None) == E_ARG
    pt.frame_add_samples(11)
    assert not out.any()
    assert _bits_equal(pt.read_lightmap(dilate=0), whole[0])
    assert L.ptc_frame_add_samples(h, 1) == E_ARG                              # the budget of ptc_lightmap_begin holds, as in any frame
    assert pt.stats()["paths"] == 480 * 16
    pt.frame_resolve()                                                         # the frame's n x 1 image: the mean radiance per entry, E / pi up to rounding
    img = pt.read_radiance()
    assert img.shape == (1, 480, 4) and np.allclose(img[0, :, :3] * PI32, whole[0][..., :3].reshape(480, 3), rtol=1e-6)


def test_an_atlas_nothing_covers_is_empty(cornell):
    uv = np.full((4, 2), 0.25, F32)      # every triangle collapses
    cornell.lightmap_begin(0, 8, 8, 4, uv=uv, seed=1, max_bounces=1)
    assert cornell.lightmap_texel_count() == (0, 0)
    cornell.frame_add_samples(4)
    atlas, back = cornell.read_lightmap(dilate=3, with_backface=True)
    assert atlas.shape == (8, 8, 4) and not atlas.any() and back.size == 0
    assert cornell.lightmap_texels()["atlas_index"].size == 0


def test_kernel_hash_is_the_profiled_one(gpu):
    """The hashed kernel sources are untouched: ptc_build_info reports the hash the committed kernel models were measured on."""
    sha = gpu.load_library().ptc_build_info().decode().split()[-1]
    for f in ("r04_kernel_model.json", "r04_textured_kernel_model.json"):      # the two models bench.py uses (tests/test_profiles.py)
        assert json.load(open(os.path.join(ROOT, "profiles", f)))["kernel_source_sha256"] == sha, f


def test_cli_bakes_a_lightmap(gpu, tmp_path, whole):
    """ptc_render --lightmap 0:24x20 on the Cornell box: an RGB PFM of the irradiance and one of the coverage — the bytes of the Python bake."""
    import subprocess

    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    out, alpha = str(tmp_path / "lm.pfm"), str(tmp_path / "a.pfm")
    r = subprocess.run([exe, "--scene", "cornell", "--lightmap", "0:24x20", "--lightmap-out", out, "--lightmap-alpha", alpha, "--lightmap-dilate", "0", "--spp", "16", "--seed", str(SEED),
                        "--bounces", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    head = json.loads(r.stdout.splitlines()[-1])
    assert head["lightmap"] == [0, 24, 20] and head["texels"] == 480 and head["dropped"] == 0 and head["paths"] == 480 * 16
    for path, want in ((out, whole[0][..., :3]), (alpha, np.repeat(whole[0][..., 3:], 3, -1))):
        magic, size, scale, body = open(path, "rb").read().split(b"\n", 3)
        assert magic == b"PF" and size == b"24 20" and float(scale) < 0 and len(body) == 24 * 20 * 12
        assert _bits_equal(np.frombuffer(body, "<f4").reshape(20, 24, 3)[::-1], want)      # PFM stores the bottom row first
