"""Dielectric transmission on a real MI355X (include/ptc_glass.h: ptc_set_material_transmission ..., ptc_debug_glass_closest; csrc/pt_glass.hip).

 1. The resolution against its float32 restatement, bit for bit, fed from ptc_debug_trace_closest segment by segment: on and around a wave and over two segments,
    NEAREST and LINEAR, thin and solid, bounces 0 and 2.
 2. The slab against float64: the resolution against the float64 walk of glass_reference.py on every ray the walk decides; the exit direction is the entry
    direction, the floor hit is displaced by the analytic offset; Beer through the slab.
 3. Total internal reflection inside the slab: exhausted, counted, contributes nothing.
 4. The white furnace: radiance = paths - exhausted, exactly.
 5. The Fresnel split and the p_t split over 4096 keys.
 6. An ior-1 pane between a diffuse floor and an emissive quad changes nothing: the MIS weight behind a delta event is 1.
 7. A BLEND sheet under a thin pane: bit for bit, and the floor's arrival rate.
 8. tau = 0 set explicitly launches and renders what a context that never called the feature does.
 9. The guides of a glass scene are those of its tau = 0 twin.
10. Invariance: tile shards, adaptive frames, refit and rebuild; a probe inside the furnace solid."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glass_reference as ref  # noqa: E402
import lights_reference as lref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SEED = ref.SEED
COUNTERS = ("paths", "segments", "shadow_rays", "hits", "node_visits_closest", "tri_tests_closest", "node_visits_any", "tri_tests_any", "algorithmic_bytes",
            "launches_trace_closest", "launches_trace_any", "n_triangles", "n_bvh_nodes", "n_emitters", "bvh_max_depth")


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same_resolution(got, want, what):
    """ptc_debug_glass_closest's eight arrays against resolve_closest's."""
    names = ("t", "prim", "uv", "o", "d", "T", "pdf", "j")
    for k, name in enumerate(names):
        same = np.array_equal(got[k], want[k]) if name in ("prim", "j") else _bits_equal(got[k], want[k])
        if not same:
            bad = np.flatnonzero((np.asarray(got[k]) != np.asarray(want[k])).reshape(len(got[k]), -1).any(1))
            raise AssertionError(f"{what}: {name} differs at rays {bad[:8].tolist()}: {np.asarray(got[k])[bad[:4]].tolist()} want {np.asarray(want[k])[bad[:4]].tolist()}")


def _slab(gpu, **kw):
    kw.setdefault("base", (0.9, 0.8, 0.7))
    return gpu.scenes.glass_slab(**kw)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thin", [False, True], ids=["solid", "thin"])
@pytest.mark.parametrize("filt", ["nearest", "linear"])
def test_resolution_equals_the_restatement_bit_for_bit(gpu, filt, thin):
    desc = _slab(gpu, thin=thin, transmission=0.8, textured=True, texture_filter=filt, attenuation_color=(0.5, 0.8, 0.95), attenuation_distance=0.7)
    pt = gpu.PathTracer(0).load_scene(desc)
    sc = ref.Scene(pt, desc)
    bits, mats, n_prims, _ = pt.glass_tables()
    assert np.array_equal(bits, sc.bits) and _bits_equal(mats, sc.mats) and n_prims == (4 if thin else 14)
    events = stood = beer = 0
    for n, o, d, keys in ref.ray_sets(pt):
        for bounce in (0, 2):
            got = pt.glass_closest(o, d, keys, bounce)
            want = ref.resolve_closest(sc, pt.trace_closest, o, d, keys, bounce, 8)
            _same_resolution(got, want[:8], f"{filt} thin {thin} n {n} bounce {bounce}")
            st = pt.glass_stats()
            assert {k: st[k] for k in want[8]} == want[8], (n, bounce, st, want[8])
            j, pdf = got[7], got[6]
            assert (pdf[j >= 1] == ref.DELTA_PDF).all() and (pdf[j == 0] == 1.0).all()
            events += int(j.sum()); stood += int(((j >= 1) & (got[1] >= 0)).sum()); beer += int(((got[5] != 1.0).any(1) & (j >= 2)).sum())
    assert events > 700 and stood > 300 and (thin or beer > 100) and pt.glass_tables()[3]      # the scene has glass: the lane has its glass queue
    pt.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thin", [False, True], ids=["solid", "thin"])
def test_resolution_agrees_with_the_float64_walk(gpu, thin):
    """ptc_debug_glass_closest against `walk64` — float64 throughout, its own search of all triangles, the same random numbers — on the scene and the ray sets
    test_glass_host.py runs the walk on.  On every ray the walk decides (all but at most 2 %): the same final primitive, the same number of events, exhausted
    alike, t, o, d and T within the bounds the walk carries per ray (glass_reference.check_against_walk64)."""
    desc = _slab(gpu, thin=thin, ior=1.5, attenuation_color=(0.5, 0.8, 0.95), attenuation_distance=0.7)
    pt = gpu.PathTracer(0).load_scene(desc)
    sc = ref.Scene(pt, desc)
    total = compared = 0
    for n, o, d, keys in ref.ray_sets(pt, (65, 513)):
        w = ref.walk64(sc, o, d, keys, 0, 8)
        got = pt.glass_closest(o, d, keys, 0)
        m, worst = ref.check_against_walk64(got, w, f"thin {thin} n {n}")
        print(f"thin={thin} n={n}: {m} rays compared with the float64 walk, error / bound at most {worst}")
        total += n; compared += m
        assert (got[7] > 0).sum() > 0.5 * n
    assert compared >= (1.0 - ref.MAX_UNDECIDED) * total
    pt.close()


def test_slab_against_float64(gpu):
    n_ior, thick, col, dist = 1.5, 0.5, (0.5, 0.8, 0.95), 0.7
    desc = _slab(gpu, thin=False, transmission=1.0, ior=n_ior, thickness=thick, attenuation_color=col, attenuation_distance=dist)
    pt = gpu.PathTracer(0).load_scene(desc)
    sc = ref.Scene(pt, desc)
    o, d = pt.debug_camera_rays(24, 24, SEED, 0, 1)
    keys = np.arange(len(o), dtype=np.uint32)
    t, prim, uv, of, df, T, pdf, j = pt.glass_closest(o, d, keys, 0)
    through = (j == 2) & np.isin(prim, (0, 1))                                    # in through the top, out through the bottom, down to the floor
    assert through.sum() > 0.7 * len(o)
    o64, d64 = o[through].astype(F64), d[through].astype(F64)
    # the exit direction is the entry direction: two refractions, each within the direction bound
    assert (np.abs(df[through].astype(F64) - d64) <= 2 * ref.DIR_BOUND).all(), np.abs(df[through] - d64).max()
    # the analytic path: down to the top face, Snell inside, out of the bottom face, down to the floor
    y1, y0 = 1.0 + thick, 1.0
    t0 = (y1 - o64[:, 1]) / d64[:, 1]
    E = o64 + t0[:, None] * d64
    sin_i = np.hypot(d64[:, 0], d64[:, 2])
    sin_t = sin_i / n_ior
    cos_t = np.sqrt(1.0 - sin_t * sin_t)
    lat = d64[:, [0, 2]] / sin_i[:, None]
    d_in = np.stack([lat[:, 0] * sin_t, -cos_t, lat[:, 1] * sin_t], 1)
    t_in = thick / cos_t
    X = E + t_in[:, None] * d_in
    t2 = y0 / -d64[:, 1]
    Fl = X + t2[:, None] * d64
    straight = o64 + (o64[:, 1] / -d64[:, 1])[:, None] * d64
    offset = np.linalg.norm(Fl - straight, axis=1)
    assert offset.min() > 0.02                                                    # the displacement is there to be seen: hundreds of ray epsilons
    got = of[through].astype(F64) + t[through].astype(F64)[:, None] * df[through].astype(F64)
    total = t0 + t_in + t2
    bound = 3 * (8 * 2.0 ** -23 * total + float(sc.eps)) + 2 * ref.DIR_BOUND * total
    err = np.abs(got - Fl).max(1)
    print(f"slab: {int(through.sum())} rays, floor hit off by up to {err.max():.3e} (bound {bound.min():.3e}), displacement {offset.min():.3f} .. {offset.max():.3f}")
    assert (err <= bound).all()
    # Beer: base on the way in, 2^(-sigma2 t) inside, nothing on the way out
    s2 = ref.sigma2(col, dist).astype(F64)
    want = np.asarray(desc.materials[-1].base_color[:3], F64)[None] * np.exp2(-s2[None] * t_in[:, None])
    rel = np.abs(T[through].astype(F64) / want - 1.0)
    rb = ref.BEER_BOUND + 2.0 ** -22 + math.log(2.0) * s2.max() * (8 * 2.0 ** -23 * t_in + 2 * float(sc.eps)) + math.log(2.0) * s2.max() * t_in * 2 * ref.DIR_BOUND / cos_t
    print(f"Beer: relative error up to {rel.max():.3e} (bound {rb.min():.3e})")
    assert (rel <= rb[:, None]).all()
    pt.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_total_internal_reflection_exhausts(gpu):
    desc = _slab(gpu, thin=False, transmission=1.0, ior=1.5, thickness=0.5)
    pt = gpu.PathTracer(0).load_scene(desc)
    # from inside the slab along the box's diagonals: the cosine to every face is 0.577, under cos(asin(1 / 1.5)) = 0.745: trapped for good
    rng = np.random.default_rng(9)
    n = 200
    o = np.stack([rng.uniform(-1, 1, n), rng.uniform(1.1, 1.4, n), rng.uniform(-1, 1, n)], 1).astype(F32)
    d = rng.choice([-1.0, 1.0], (n, 3)) + rng.normal(size=(n, 3)) * 0.03
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    keys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    for maxi in (1, 5):
        pt.set_glass_max_interactions(maxi)
        t, prim, uv, of, df, T, pdf, j = pt.glass_closest(o, d, keys, 1)
        st = pt.glass_stats()
        assert (prim == -1).all() and (t == -1.0).all() and not uv.any() and not T.any() and (j == maxi).all() and (pdf == ref.DELTA_PDF).all()
        assert st["exhausted"] == n and st["reflections"] == n * maxi and st["refractions"] == 0 and st["standing"] == 0 and st["seconds_glass"] > 0
    # rendered from inside, every path is trapped: a black image, all paths counted
    pt.set_glass_max_interactions(4)
    S = gpu.scene
    desc.camera = S.CameraDesc((0.0, 1.25, 0.0), (1.0, 2.25, 1.0), math.radians(8.0), 1.0)
    desc.env = np.full((4, 8, 3), 1.0, F32)
    pt.load_scene(desc)
    img = pt.render(16, 16, 4, seed=SEED, max_bounces=2)
    assert not img[..., :3].any() and pt.glass_stats()["exhausted"] == 16 * 16 * 4
    pt.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_white_furnace(gpu):
    w = h = 32
    spp = 16
    pt = gpu.PathTracer(0).load_scene(gpu.scenes.glass_ball())
    pt.set_glass_max_interactions(16)
    img = pt.render(w, h, spp, seed=SEED, max_bounces=0)[..., :3].astype(F64)
    st, gs = pt.stats(), pt.glass_stats()
    paths = w * h * spp
    assert st["paths"] == paths and gs["refractions"] > 0.5 * paths and gs["reflections"] > 0
    print(f"furnace: {paths} paths, {gs['exhausted']} exhausted, {gs['refractions']} refractions, {gs['reflections']} reflections")
    for c in range(3):
        assert img[..., c].sum() * spp == paths - gs["exhausted"]
    assert gs["exhausted"] <= ref.MAX_EXHAUSTED * paths
    # a probe inside the solid: every direction carries 1, as in the same ball with the ior of air
    pos = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1]], F32)
    sh = pt.render_probes(pos, 256, seed=5, max_bounces=0)
    gp = pt.glass_stats()
    assert gp["exhausted"] == 0 and gp["refractions"] == 2 * 256
    pt.load_scene(gpu.scenes.glass_ball(ior=1.0))
    sh1 = pt.render_probes(pos, 256, seed=5, max_bounces=0)
    assert pt.glass_stats() == dict(gp, reflections=0, seconds_glass=pt.glass_stats()["seconds_glass"])
    assert _bits_equal(sh, sh1) and (sh[:, 0] > 0).all()
    pt.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _fresnel_thin64(cos_i, n):
    F = float(ref.event(np.array([[0.0, 0.0, 1.0]]), np.array([[math.sqrt(1 - cos_i * cos_i), 0.0, -cos_i]]), np.array([[-math.sqrt(1 - cos_i * cos_i), 0.0, cos_i]]),
                        [1.0 / n], [True], [2.0], F64)[2][0])
    return F


def test_fresnel_and_choice_splits(gpu):
    tau, n_ior, N = 0.6, 1.5, 4096
    desc = _slab(gpu, thin=True, transmission=tau, ior=n_ior)
    pt = gpu.PathTracer(0).load_scene(desc)
    cos_i = 0.5                                                                   # 60 degrees: F = 0.089 per face, 0.164 for the pane
    d1 = np.array([math.sqrt(1 - cos_i * cos_i), -cos_i, 0.0])
    o = np.repeat(np.array([[0.3, 1.0, 0.5]]) - 2.0 * d1[None], N, 0).astype(F32)      # meets the pane, the sheet and the floor well inside a triangle
    d = np.repeat(d1[None], N, 0).astype(F32)
    t, prim, uv, of, df, T, pdf, j = pt.glass_closest(o, d, np.arange(N, dtype=np.uint32), 0)
    F = _fresnel_thin64(cos_i, n_ior)
    assert abs(F - 2 * 0.0891867 / 1.0891867) < 1e-6
    stands, refl, trans = (j == 0) & np.isin(prim, (2, 3)), (j == 1) & (prim == -1), (j == 1) & np.isin(prim, (0, 1))
    assert stands.sum() + refl.sum() + trans.sum() == N
    for name, k, p in (("stands", stands.sum(), 1 - tau), ("reflected", refl.sum(), tau * F), ("transmitted", trans.sum(), tau * (1 - F))):
        sd = math.sqrt(N * p * (1 - p))
        print(f"{name}: {int(k)} of {N}, expected {N * p:.1f} +- {sd:.1f}")
        assert abs(k - N * p) <= 5 * sd, name
    # and the Fresnel split among the rays that met the interface
    k, m = int(refl.sum()), int(refl.sum() + trans.sum())
    assert abs(k - m * F) <= 5 * math.sqrt(m * F * (1 - F))
    st = pt.glass_stats()
    assert st["reflections"] == refl.sum() and st["refractions"] == trans.sum() and st["standing"] == m and st["exhausted"] == 0
    pt.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_an_invisible_pane_changes_nothing(gpu):
    w = h = 32
    spp, K = 32, 8
    means = []
    for pane in (True, False):
        desc = _slab(gpu, thin=True, transmission=1.0, ior=1.0, base=(1.0, 1.0, 1.0), emitter=True, pane=pane)
        pt = gpu.PathTracer(0).load_scene(desc)
        m = [float(pt.render(w, h, spp, seed=100 + 7 * k, max_bounces=2)[..., :3].astype(F64).mean()) for k in range(K)]
        if pane:
            st = pt.glass_stats()
            assert st["refractions"] > 0.5 * w * h * spp and st["exhausted"] == 0
        means.append(np.array(m))
        pt.close()
    a, b = means
    se = math.sqrt(a.var(ddof=1) / K + b.var(ddof=1) / K)
    print(f"pane {a.mean():.5f}, no pane {b.mean():.5f}, difference {abs(a.mean() - b.mean()) / se:.2f} combined standard errors ({se:.2e})")
    assert a.mean() > 0.01 and abs(a.mean() - b.mean()) <= 5 * se


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_blend_sheet_under_a_thin_pane(gpu):
    a_sheet, n_ior, N = 0.4, 1.5, 4096
    desc = _slab(gpu, thin=True, transmission=1.0, ior=n_ior, sheet_alpha=a_sheet)
    pt = gpu.PathTracer(0).load_scene(desc)
    sc = ref.Scene(pt, desc)
    assert sc.alpha is not None and pt.alpha_tables()[3] == 6
    for n, o, d, keys in ref.ray_sets(pt):
        for bounce in (0, 2):
            got = pt.glass_closest(o, d, keys, bounce)
            want = ref.resolve_closest(sc, pt.trace_closest, o, d, keys, bounce, 8)
            _same_resolution(got, want[:8], f"mixed n {n} bounce {bounce}")
    cos_i = 0.5
    d1 = np.array([math.sqrt(1 - cos_i * cos_i), -cos_i, 0.0])
    o = np.repeat(np.array([[0.3, 1.0, 0.5]]) - 2.0 * d1[None], N, 0).astype(F32)      # meets the pane, the sheet and the floor well inside a triangle
    d = np.repeat(d1[None], N, 0).astype(F32)
    t, prim, uv, of, df, T, pdf, j = pt.glass_closest(o, d, np.arange(N, dtype=np.uint32) * np.uint32(2654435761), 0)
    p = (1 - _fresnel_thin64(cos_i, n_ior)) * (1 - a_sheet)
    k = int(np.isin(prim, (0, 1)).sum())
    sd = math.sqrt(N * p * (1 - p))
    print(f"floor arrivals: {k} of {N}, expected {N * p:.1f} +- {sd:.1f}")
    assert abs(k - N * p) <= 5 * sd and pt.alpha_stats()["closest_passes"] == k
    pt.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _load_with_tau_zero(pt, desc):
    """load_scene, with ptc_set_material_transmission(transmission = 0, the other fields far from their defaults) on every material that takes it."""
    from pbr_amd.ptc import _f, _ptr
    L, h = pt._L, pt._h
    assert L.ptc_scene_begin(h) == 0
    for m in desc.materials:
        mid = L.ptc_add_material(h, _f(m.base_color)[1], m.metallic, m.roughness, _f(m.emissive)[1], m.tex_color, m.tex_normal, m.tex_mr)
        assert mid >= 0
        if not any(m.emissive):
            pt.set_material_transmission(mid, transmission=0.0, ior=2.0, thin_walled=0, attenuation_color=(0.5, 0.5, 0.5), attenuation_distance=1.0)
    for me in desc.meshes:
        v, i = np.ascontiguousarray(me.vertices), np.ascontiguousarray(me.indices, np.uint32)
        assert L.ptc_add_mesh(h, v.ctypes.data, v.size, _ptr(i), i.size, me.material) >= 0
    for it in desc.instances:
        assert L.ptc_add_instance(h, it.mesh, _f(it.t)[1], _f(it.q_wxyz)[1], _f(it.s)[1]) >= 0
    c = desc.camera
    assert L.ptc_set_camera(h, _f(c.position)[1], _f(c.target)[1], c.fov_y, c.aspect) == 0
    assert L.ptc_scene_commit(h) == 0


def test_tau_zero_is_a_scene_without_the_feature(gpu):
    desc = gpu.scenes.cornell_box()
    pt = gpu.PathTracer(0).load_scene(desc)
    a = pt.render(48, 48, 8, seed=SEED, max_bounces=4)
    sa = pt.stats()
    pt.close()
    pt = gpu.PathTracer(0)
    _load_with_tau_zero(pt, desc)
    pt.set_glass_max_interactions(3)
    assert pt.get_material_transmission(0)["ior"] == 2.0
    b = pt.render(48, 48, 8, seed=SEED, max_bounces=4)
    sb = pt.stats()
    assert _bits_equal(a, b)
    for k in COUNTERS:
        assert sa[k] == sb[k], k
    bits, mats, _, queue = pt.glass_tables()
    assert sa["launches_trace_closest"] == 5 and not bits.any() and not queue         # no glass queue was ever allocated
    assert pt.glass_stats() == dict(reflections=0, refractions=0, standing=0, exhausted=0, seconds_glass=0.0)
    # the hook on such a scene: the plain trace, the rays untouched
    o, d = pt.debug_camera_rays(8, 8, SEED, 0, 1)
    t, prim, uv, of, df, T, pdf, j = pt.glass_closest(o, d, np.arange(64, dtype=np.uint32))
    t0, prim0, uv0 = pt.trace_closest(o, d)
    assert _bits_equal(t, t0) and np.array_equal(prim, prim0) and _bits_equal(uv, uv0) and not j.any()
    assert _bits_equal(of, o) and _bits_equal(df, d) and (T == 1.0).all() and (pdf == 1.0).all()
    pt.close()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _guides(pt, w, h):
    pt.frame_begin(w, h, 1, seed=SEED, max_bounces=1)
    pt.frame_guides()
    prim, uv = pt.read_guide_hit()
    return prim, uv, pt.read_guide(0), pt.read_guide(1)


def test_guides_see_glass_as_the_surface(gpu):
    w = h = 24
    pt = gpu.PathTracer(0).load_scene(_slab(gpu, thin=False, transmission=1.0))
    glass = _guides(pt, w, h)
    pt.load_scene(_slab(gpu, thin=False, transmission=0.0))
    twin = _guides(pt, w, h)
    assert np.isin(glass[0], np.arange(2, 14)).mean() > 0.8
    assert np.array_equal(glass[0], twin[0]) and all(_bits_equal(glass[k], twin[k]) for k in (1, 2, 3))
    pt.close()


# ---- 10 --------------------------------------------------------------------------------------------------------------------------------------------------
def _lit_slab(gpu):
    desc = _slab(gpu, thin=False, transmission=0.9, textured=True, texture_filter="linear", emitter=True, sheet_alpha=0.5, attenuation_color=(0.6, 0.8, 0.9), attenuation_distance=0.5)
    desc.lights = [dict(type="point", position=(0.5, 3.0, -0.5), intensity=(8.0, 8.0, 6.0))]
    desc.env = np.full((4, 8, 3), 0.5, F32)
    return desc


def test_tile_shards_merge_to_the_unsharded_frame(gpu):
    w = h = 48
    pt = gpu.PathTracer(0).load_scene(_lit_slab(gpu))
    whole = pt.render(w, h, 8, seed=SEED, max_bounces=3)
    st = pt.glass_stats()
    assert st["refractions"] > 0 and st["reflections"] > 0 and st["standing"] > 0 and pt.alpha_stats()["closest_passes"] > 0
    merged = np.zeros_like(whole)
    for rank in range(2):
        pt.frame_begin(w, h, 8, seed=SEED, max_bounces=3, tile_rank=rank, tile_count=2)
        pt.frame_add_samples(8)
        pt.frame_resolve()
        part = pt.read_radiance()
        assert (part[merged[..., 3] > 0] == 0).all()
        merged += part
    assert _bits_equal(merged, whole) and (whole[..., :3] > 0).any() and np.isfinite(whole).all()
    pt.close()


def test_adaptive_pixels_hold_the_uniform_frames_bits(gpu):
    w = h = 32
    pt = gpu.PathTracer(0).load_scene(_lit_slab(gpu))
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
    desc = _slab(gpu, thin=False, transmission=0.8, attenuation_color=(0.5, 0.8, 0.95), attenuation_distance=0.7)
    pt = gpu.PathTracer(0).load_scene(desc)
    before = pt.glass_tables()[0].copy()
    assert int(before[0]) == 0b11111111111100
    for k, step in enumerate(("refit", "rebuild")):
        for inst in range(1, len(desc.instances)):                             # the floor stays; the slab's six faces move together
            pt.update_instance(inst, (0.05 * (k + 1), 0.02 * (k + 1), -0.03 * (k + 1)), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        pt.scene_refit() if step == "refit" else pt.scene_rebuild()
        assert np.array_equal(pt.glass_tables()[0], before)
        sc = ref.Scene(pt, desc)
        for n, o, d, keys in ref.ray_sets(pt, (65, 513)):
            got = pt.glass_closest(o, d, keys, 0)
            _same_resolution(got, ref.resolve_closest(sc, pt.trace_closest, o, d, keys, 0, 8)[:8], f"after {step} n {n}")
            assert (got[7] > 0).sum() > 0.5 * n
    pt.close()
