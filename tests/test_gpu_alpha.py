"""Alpha coverage on a real MI355X (include/ptc_alpha.h: ptc_set_material_alpha ..., ptc_debug_alpha_closest / _any; csrc/pt_alpha.hip).

 5. The closest-hit resolution against the independent float64 walk of all triangles (tests/alpha_reference.py), on and around a wave and over two segments.
 6. The resolutions against their float32 restatement, bit for bit, fed from ptc_debug_trace_closest layer by layer.
 7. Exhaustion: max_layers = 2 on five fully transparent layers.
 8. All-covering alpha renders the bits of the opaque scene.
 9. A scene without alpha materials queues what it always queued.
10. Shadow transmittance is deterministic: (1 - a) x the unshadowed pixel.
11. Stochastic coverage is unbiased.
12. The guides see the first covering surface.
13. Invariance: tile shards, adaptive frames, refit and rebuild."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alpha_reference as ref  # noqa: E402
import lights_reference as lref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SEED = ref.SEED


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _hold_to_the_walk(pt, desc, tag):
    """ptc_debug_alpha_closest on the ray sets against walk_closest on the context's own flat scene: primitive and layers exact, t within t_bound, on every decided ray."""
    verts, idx, tri_mat = pt.flat_scene()
    eps = lref.scene_ray_eps(verts[:, 0:3])
    linear = desc.texture_filter == "linear"
    total = und = passed = 0
    for n, o, d, keys in ref.ray_sets(pt):
        t, prim, uv, layers = pt.alpha_closest(o, d, keys, 0)
        rt, rp, rl, undecided = ref.walk_closest(verts, idx, tri_mat, desc.materials, desc.textures, linear, o, d, keys, 0, 8)
        ok = ~undecided
        what = f"{tag} n {n}"
        bad = np.flatnonzero(ok & ((prim != rp) | (layers != rl)))
        assert len(bad) == 0, f"{what}: rays {bad[:8].tolist()}: prim {prim[bad[:8]].tolist()} want {rp[bad[:8]].tolist()}, layers {layers[bad[:8]].tolist()} want {rl[bad[:8]].tolist()}"
        h = ok & (rp >= 0)
        err = np.abs(t[h].astype(F64) - rt[h])
        assert (err <= ref.t_bound(rt[h], rl[h], eps)).all(), f"{what}: t off by up to {err.max():.3e}"
        assert (t[ok & (rp < 0)] == -1.0).all(), what
        total += n; und += int(undecided.sum()); passed += int((layers[ok] > 0).sum())
    print(f"{tag}: {total} rays, {und} left out ({100.0 * und / total:.2f} %), {passed} passed at least one layer")
    assert und <= ref.MAX_UNDECIDED * total and passed > 0.2 * total


@pytest.mark.parametrize("filt", ["nearest", "linear"])
def test_resolution_equals_the_float64_walk(gpu, filt):
    desc = gpu.scenes.alpha_layers(3, 2, filt)
    pt = gpu.PathTracer(0).load_scene(desc)
    _hold_to_the_walk(pt, desc, f"alpha_layers {filt}")
    pt.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["nearest", "linear"])
def test_resolution_equals_the_restatement_bit_for_bit(gpu, filt):
    desc = gpu.scenes.alpha_layers(3, 2, filt)
    pt = gpu.PathTracer(0).load_scene(desc)
    sc = ref.Scene32(pt, desc)
    _, _, _, n_prims, _ = pt.alpha_tables()
    assert np.array_equal(pt.alpha_tables()[0], sc.bits) and n_prims == 14
    seen_pass = seen_partial = 0
    for n, o, d, keys in ref.ray_sets(pt):
        for det in (False, True):
            for bounce in (0, 2):
                got = pt.alpha_closest(o, d, keys, bounce, det)
                want = ref.resolve_closest(sc, pt.trace_closest, o, d, keys, bounce, 8, det)
                what = f"{filt} n {n} deterministic {det} bounce {bounce}"
                assert _bits_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and _bits_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what
                seen_pass += int((got[3] > 0).sum())
        # shadow rays along the same rays: tmax short of the first surface, between the layers, beyond everything
        t0, p0, _ = pt.trace_closest(o, d)
        first = np.where(p0 >= 0, t0, F32(1.0))
        for tmax in (first * F32(0.5), first + F32(0.6), np.full(n, 1e3, F32)):
            got = pt.alpha_any(o, d, tmax)
            want = ref.resolve_any(sc, pt.trace_closest, pt.trace_any, o, d, tmax, 8)
            assert _bits_equal(got, want), f"{filt} n {n} shadow"
            seen_partial += int(((got > 0) & (got < 1)).sum())
    assert seen_pass > 500 and seen_partial > 50
    assert pt.alpha_tables()[4]                                      # the scene has alpha materials: the lane has its alpha queue
    pt.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_exhaustion(gpu):
    desc = gpu.scenes.alpha_layers(5, 0, mask_alpha=0)                    # five fully transparent MASK layers: prims 4 + 2k, 5 + 2k of layer k, the camera above the top one
    pt = gpu.PathTracer(0).load_scene(desc)
    o, d = pt.debug_camera_rays(24, 24, SEED, 0, 1)
    assert np.isin(pt.trace_closest(o, d)[1], (12, 13)).all()             # every ray crosses all five layers; the plain trace stops at the top one
    n = len(o)
    assert n > 100
    keys = np.arange(n, dtype=np.uint32)
    far = np.full(n, 1e3, F32)
    pt.set_alpha_max_layers(2)
    t, prim, _, layers = pt.alpha_closest(o, d, keys)
    assert np.isin(prim, (8, 9)).all() and (layers == 2).all()            # the third layer from the top stands
    st = pt.alpha_stats()
    assert st["exhausted"] == n and st["closest_passes"] == 2 * n
    assert (pt.alpha_any(o, d, far) == 0).all()
    st = pt.alpha_stats()
    assert st["exhausted"] == n and st["shadow_walked"] == n and st["shadow_passes"] == 2 * n
    pt.set_alpha_max_layers(8)
    t, prim, _, layers = pt.alpha_closest(o, d, keys)
    assert np.isin(prim, (0, 1)).all() and (layers == 5).all()            # the floor
    assert pt.alpha_stats()["exhausted"] == 0
    assert (pt.alpha_any(o, d, t * F32(0.999)) == 1).all()                # short of the floor: free, and bit for bit 1
    st = pt.alpha_stats()
    assert st["exhausted"] == 0 and st["shadow_passes"] == 5 * n and st["seconds_alpha"] > 0
    assert (pt.alpha_any(o, d, far) == 0).all()                           # the floor is opaque
    pt.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _textured_scene_with_emitter(pbr):
    """scenes.textured_objects with sphere_scene's emissive quad left in: textures (every texel alpha 255), an environment, one emitter."""
    M = pbr.scene.Material
    d = pbr.scenes.sphere_scene(48, 25)
    d.textures = [pbr.scenes.texture_albedo(64, 5), pbr.scenes.texture_normal(64, 6), pbr.scenes.texture_metal_rough(64, 7)]
    d.materials[0] = M((1.0, 1.0, 1.0, 1.0), 1.0, 1.0, (0, 0, 0), 0, 1, 2)
    d.materials[1] = M((0.9, 0.9, 0.9, 1.0), 0.0, 1.0, (0, 0, 0), 0, -1, -1)
    d.materials[3] = M((0.2, 0.3, 0.8, 0.5), 0.0, 0.5, (0, 0, 0), -1, 1, -1)
    d.env = pbr.scenes.analytic_sky(64, 32)
    assert all((t[..., 3] == 255).all() for t in d.textures)
    return d


COUNTERS = ("paths", "segments", "shadow_rays", "hits", "node_visits_closest", "tri_tests_closest", "node_visits_any", "tri_tests_any", "algorithmic_bytes",
            "launches_trace_closest", "launches_trace_any", "n_triangles", "n_bvh_nodes", "n_emitters", "bvh_max_depth")


def test_all_covering_alpha_is_opaque_bit_for_bit(gpu):
    light = dict(type="point", position=(-1.5, 2.5, 1.5), intensity=(30.0, 28.0, 25.0))
    imgs, stats = [], []
    for masked in (False, True):
        d = _textured_scene_with_emitter(gpu)
        if masked:
            for m in d.materials:
                if not any(m.emissive):
                    m.alpha_mode, m.alpha_cutoff = "mask", 0.5               # base alpha 1 or 0.5, texel alpha 1: every hit is covered
        pt = gpu.PathTracer(0).load_scene(d)
        pt.add_light(light)
        imgs.append(pt.render(32, 32, 8, seed=SEED, max_bounces=3))
        stats.append(pt.stats())
        if masked:
            st = pt.alpha_stats()
            assert pt.alpha_tables()[4] and st["closest_passes"] == 0 and st["shadow_passes"] == 0 and st["exhausted"] == 0
            assert st["shadow_walked"] > 0                                   # occluded shadow records were walked — and found their opaque occluder again
        pt.close()
    assert stats[0]["n_emitters"] > 0 and (imgs[0][..., :3] > 0).any()
    assert _bits_equal(imgs[0], imgs[1])
    assert stats[0]["paths"] == stats[1]["paths"] and stats[0]["hits"] == stats[1]["hits"]


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_scene_without_alpha_queues_what_it_always_queued(gpu):
    pt = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    a = pt.render(48, 48, 8, seed=SEED, max_bounces=4)
    sa = pt.stats()
    # every alpha call a scene without alpha materials can make
    pt.set_alpha_max_layers(3)
    assert pt.alpha_stats()["closest_passes"] == 0
    bits, mode, _, _, queue = pt.alpha_tables()
    assert not bits.any() and not mode.any() and not queue
    o, d = pt.debug_camera_rays(8, 8, SEED, 0, 1)
    t, prim, uv, layers = pt.alpha_closest(o, d, np.arange(64, dtype=np.uint32))
    t0, prim0, uv0 = pt.trace_closest(o, d)
    assert _bits_equal(t, t0) and np.array_equal(prim, prim0) and _bits_equal(uv, uv0) and not layers.any()
    assert np.array_equal(pt.alpha_any(o, d, np.full(64, 1e3, F32)) == 0, pt.trace_any(o, d, np.full(64, 1e3, F32)) != 0)
    b = pt.render(48, 48, 8, seed=SEED, max_bounces=4)
    sb = pt.stats()
    assert _bits_equal(a, b)
    for k in COUNTERS:
        assert sa[k] == sb[k], k
    assert sa["launches_trace_closest"] == 5 and not pt.alpha_tables()[4]      # no alpha queue was ever allocated
    pt.close()


# ---- 10 --------------------------------------------------------------------------------------------------------------------------------------------------
def _shadow_scene(pbr, a):
    """A point light at height 3 above a 1 x 1 BLEND quad of constant alpha a at height 1 above the floor; the camera lies below the quad and sees only floor.
    The quad's shadow on the floor is the square |x|, |z| < 0.75; a = None: no quad."""
    S = pbr.scene
    mats = [S.Material((0.8, 0.7, 0.6, 1.0), 0.0, 1.0)]
    meshes = [S.MeshDesc(*pbr.scenes._quad((-3, 0, 3), (3, 0, 3), (3, 0, -3), (-3, 0, -3)), 0)]
    if a is not None:
        mats.append(S.Material((0.5, 0.5, 0.5, a), 0.0, 1.0, alpha_mode="blend"))
        meshes.append(S.MeshDesc(*pbr.scenes._quad((-0.5, 1, 0.5), (0.5, 1, 0.5), (0.5, 1, -0.5), (-0.5, 1, -0.5)), 1))
    cam = S.CameraDesc((0.0, 0.9, 0.3), (0.0, 0.0, 0.0), math.radians(100.0), 1.0)
    d = S.SceneDesc(mats, meshes, [S.InstanceDesc(k) for k in range(len(meshes))], cam, "alpha_shadow")
    d.lights = [dict(type="point", position=(0.0, 3.0, 0.0), intensity=(20.0, 18.0, 16.0))]
    return d


@pytest.mark.parametrize("a", [0.25, 0.5])
def test_shadow_transmittance_is_deterministic(gpu, a):
    w = h = 32
    spp = 4
    pt = gpu.PathTracer(0).load_scene(_shadow_scene(gpu, None))
    plain = pt.render(w, h, spp, seed=SEED, max_bounces=1)[..., :3]
    o, d = pt.debug_camera_rays(w, h, SEED, 0, spp)
    pt.close()
    # where every sample of a pixel meets the floor: at least 2 pixels (0.15 on the floor; a pixel is < 0.07 wide there) inside or outside the shadow's edge
    with np.errstate(divide="ignore", invalid="ignore"):
        tf = -o[:, 1] / d[:, 1]
    P = o + tf[:, None] * d
    r = np.maximum(np.abs(P[:, 0]), np.abs(P[:, 2])).reshape(spp, h, w)
    down = (d[:, 1] < 0).reshape(spp, h, w).all(0)
    inside, outside = down & (r < 0.75 - 0.15).all(0), down & (r > 0.75 + 0.15).all(0) & (r < 2.9).all(0)
    assert inside.sum() > 100 and outside.sum() > 50
    pt = gpu.PathTracer(0).load_scene(_shadow_scene(gpu, a))
    img = pt.render(w, h, spp, seed=SEED, max_bounces=1)[..., :3]
    st = pt.alpha_stats()
    pt.close()
    assert (plain[inside] > 0).all() and st["shadow_walked"] > 0 and st["shadow_passes"] == st["shadow_walked"] and st["exhausted"] == 0
    assert _bits_equal(img[outside], plain[outside])
    want = F64(1.0 - a) * plain[inside].astype(F64)
    rel = np.abs(img[inside].astype(F64) - want) / want
    print(f"a = {a}: {int(inside.sum())} pixels in the shadow, worst relative error {rel.max():.3e} (bound {4 * 2.0 ** -23:.3e})")
    assert (rel <= 4 * 2.0 ** -23).all()


# ---- 11 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_stochastic_coverage_is_unbiased(gpu):
    S = gpu.scene
    a, E, N = 0.5, 2.0, 1024
    mats = [S.Material((0.0, 0.0, 0.0, a), 0.0, 1.0, alpha_mode="blend")]
    meshes = [S.MeshDesc(*gpu.scenes._quad((-2, -2, 0), (2, -2, 0), (2, 2, 0), (-2, 2, 0)), 0)]
    d = S.SceneDesc(mats, meshes, [S.InstanceDesc(0)], S.CameraDesc((0.0, 0.0, 2.0), (0.0, 0.0, 0.0), math.radians(40.0), 1.0), "alpha_blend_quad")
    d.env = np.full((4, 8, 3), E, F32)
    pt = gpu.PathTracer(0).load_scene(d)
    img = pt.render(16, 16, N, seed=SEED, max_bounces=0)[..., :3].astype(F64)
    st = pt.alpha_stats()
    pt.close()
    assert st["closest_passes"] > 0.4 * 256 * N and st["exhausted"] == 0
    sd = E * math.sqrt(a * (1 - a) / N)
    assert (np.abs(img - (1 - a) * E) <= 5 * sd).all(), f"worst pixel off by {np.abs(img - (1 - a) * E).max() / sd:.2f} sd"
    assert abs(img[..., 0].mean() - (1 - a) * E) <= 5 * sd / 16.0


# ---- 12 --------------------------------------------------------------------------------------------------------------------------------------------------
def _guides(pt, w, h):
    pt.frame_begin(w, h, 1, seed=SEED, max_bounces=1)
    pt.frame_guides()
    prim, uv = pt.read_guide_hit()
    return prim, uv, pt.read_guide(0)[..., 3], pt.read_guide(1)[..., 3]      # primitive, barycentrics, class, depth


def test_guides_see_the_first_covering_surface(gpu):
    w = h = 24
    make = lambda **kw: gpu.scenes.alpha_layers(emitter=False, **kw)            # floor 0-1, the one layer 2-3
    desc = make(n_mask=1, n_blend=0)
    pt = gpu.PathTracer(0).load_scene(make(n_mask=0, n_blend=0))
    floor = _guides(pt, w, h)
    opaque_desc = make(n_mask=1, n_blend=0)
    opaque_desc.materials[1].alpha_mode = "opaque"
    pt.load_scene(opaque_desc)
    quad = _guides(pt, w, h)
    verts, idx, _ = pt.flat_scene()
    eps = lref.scene_ray_eps(verts[:, 0:3])
    pt.load_scene(desc)
    got = _guides(pt, w, h)
    # the texel under every pixel that sees the quad, from the opaque scene's hit: decided unless within 1e-4 of a texel edge
    on = quad[0] >= 2
    T = verts[:, 10:12].astype(F64)[idx.astype(np.int64)]                        # (tri, corner, uv)
    pr = np.where(on, quad[0], 2)
    hu, hv = quad[1][..., 0].astype(F64), quad[1][..., 1].astype(F64)
    tuv = T[pr, 0] * (1 - hu - hv)[..., None] + T[pr, 1] * hu[..., None] + T[pr, 2] * hv[..., None]
    f = (tuv - np.floor(tuv)) * 8.0
    decided = (np.abs(f - np.round(f)) > 8 * 1e-4).all(-1)
    tex = desc.textures[0]
    covered = tex[np.minimum(f[..., 1].astype(int), 7), np.minimum(f[..., 0].astype(int), 7), 3] == 255
    hole, solid = on & decided & ~covered, on & decided & covered
    assert hole.sum() > 50 and solid.sum() > 50 and (on & ~decided).sum() <= 0.02 * w * h
    # covered texels: the quad, bit for bit the opaque scene's guides; holes: the floor's primitive and class, its depth through one layer; beside the quad: the floor
    for k in range(4):
        assert _bits_equal(got[k][solid], quad[k][solid]) and _bits_equal(got[k][~on], floor[k][~on]), k
    assert np.array_equal(got[0][hole], floor[0][hole]) and np.isin(got[0][hole], (0, 1)).all() and _bits_equal(got[2][hole], floor[2][hole])
    assert (np.abs(got[3][hole].astype(F64) - floor[3][hole]) <= ref.t_bound(floor[3][hole], 1, eps)).all()
    # a BLEND layer of alpha 128 / 255 counts as covered: 128 / 255 >= 0.5
    pt.load_scene(make(n_mask=0, n_blend=1, blend_alpha=128))
    blend = _guides(pt, w, h)
    for k in range(4):
        assert _bits_equal(blend[k], quad[k]), k
    pt.load_scene(make(n_mask=0, n_blend=1, blend_alpha=127))                   # and one of 127 / 255 does not
    blend = _guides(pt, w, h)
    assert np.array_equal(blend[0], floor[0]) and _bits_equal(blend[2], floor[2])
    pt.close()


# ---- 13 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_tile_shards_merge_to_the_unsharded_frame(gpu):
    w = h = 48
    desc = gpu.scenes.alpha_layers(3, 2, "linear")
    desc.lights = [dict(type="point", position=(0.5, 2.5, -0.5), intensity=(8.0, 8.0, 6.0))]
    pt = gpu.PathTracer(0).load_scene(desc)
    whole = pt.render(w, h, 8, seed=SEED, max_bounces=3)
    st = pt.alpha_stats()
    assert st["closest_passes"] > 0 and st["shadow_passes"] > 0
    merged = np.zeros_like(whole)
    for rank in range(2):
        pt.frame_begin(w, h, 8, seed=SEED, max_bounces=3, tile_rank=rank, tile_count=2)
        pt.frame_add_samples(8)
        pt.frame_resolve()
        part = pt.read_radiance()
        assert (part[merged[..., 3] > 0] == 0).all()
        merged += part
    assert _bits_equal(merged, whole) and (whole[..., :3] > 0).any()
    pt.close()


def test_adaptive_pixels_hold_the_uniform_frames_bits(gpu):
    w = h = 32
    pt = gpu.PathTracer(0).load_scene(gpu.scenes.alpha_layers(3, 2))
    img = pt.render_adaptive(w, h, 32, seed=SEED, max_bounces=2, threshold=0.05, radius=1, min_samples=8, step_samples=8)
    counts = pt.read_sample_counts()
    seen = np.unique(counts)
    print("adaptive counts:", {int(n): int((counts == n).sum()) for n in seen})
    assert set(seen.tolist()) <= {8, 16, 24, 32}, seen
    for n in seen:
        uniform = pt.render(w, h, int(n), seed=SEED, max_bounces=2)
        assert _bits_equal(img[counts == n], uniform[counts == n]), int(n)
    pt.close()


def test_tables_follow_primitive_ids_through_refit_and_rebuild(gpu):
    desc = gpu.scenes.alpha_layers(3, 2)
    pt = gpu.PathTracer(0).load_scene(desc)
    before = pt.alpha_tables()[0].copy()
    for k, step in enumerate(("refit", "rebuild")):
        for inst in range(len(desc.instances)):                                # the floor stays; emitter and layers shift, the layers each a little more
            if inst:
                pt.update_instance(inst, (0.03 * inst * (k + 1), 0.01 * inst, -0.02 * inst * (k + 1)), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        pt.scene_refit() if step == "refit" else pt.scene_rebuild()
        assert np.array_equal(pt.alpha_tables()[0], before)
        _hold_to_the_walk(pt, desc, f"alpha_layers after {step}")
    pt.close()
