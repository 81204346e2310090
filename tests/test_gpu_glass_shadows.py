"""Transparent shadows on a real MI355X (include/ptc_glass_shadows.h: ptc_set_glass_shadows, ptc_debug_glass_any ...; csrc/pt_glass_shadow.hip, k_glass_filter<.., true> of
csrc/pt_glass.hip).

1.  ptc_debug_glass_any against the float32 restatement, bit for bit, at 1 / 63 / 64 / 65 / 513 records, NEAREST and LINEAR: one pane, a textured tinted pane, three
    panes with tilted normals, a pane over a BLEND and a MASK sheet, a solid slab (0), records that end before the pane (1); the counters against the restatement's.
2.  ... and against the float64 walk on every record it decides.
3.  The mixed scene: records that meet alpha surfaces only have three equal channels with the bits of ptc_debug_alpha_any of the same scene with the feature off.
4.  Exhaustion: L panes are passed with k = L, L + 1 panes occlude and are counted.
5.  One ray through a tilted pane, 4096 keys through ptc_debug_glass_closest: the share transmitted against s, every transmitted T against the base colour.
6.  ptc_debug_glass_closest with the feature on against the restatement with the MIS bookkeeping, bit for bit.
7.  A sun through a tinted pane: every pixel is the pane-less frame's times W; with the feature off it is black.
8.  MIS: an ior-1 white pane under the emitter changes nothing; at ior 1.5 with a tint, on and off agree and on has the lower variance.
9.  Off is today; switching on late; tile shards, adaptive frames, refit and rebuild with the feature on."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glass_reference as gref  # noqa: E402
import glass_shadow_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SEED = gref.SEED


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _ctx(gpu, desc, on=True):
    pt = gpu.PathTracer(0)
    if on is not None:
        pt.set_glass_shadows(on)
    return pt.load_scene(desc)


def _same_any(got, want, what):
    for k, name in enumerate(("Tr", "layers")):
        same = _bits_equal(got[k], want[k]) if name == "Tr" else np.array_equal(got[k], want[k])
        if not same:
            bad = np.flatnonzero((np.asarray(got[k]) != np.asarray(want[k])).reshape(len(got[k]), -1).any(1))
            raise AssertionError(f"{what}: {name} differs at records {bad[:8].tolist()}: {np.asarray(got[k])[bad[:4]].tolist()} want {np.asarray(want[k])[bad[:4]].tolist()}")


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pane", "textured", "stack3", "mixed", "solid"])
@pytest.mark.parametrize("filt", ["nearest", "linear"])
def test_shadow_walk_equals_the_restatement_bit_for_bit(gpu, filt, name):
    desc = ref.record_scenes(gpu, filt)[name]
    pt = _ctx(gpu, desc)
    sc = gref.Scene(pt, desc)
    L = ref.rounds_limit(8, 8, sc.alpha is not None)
    lit = free = dark = 0
    for n, o, d, tmax in ref.shadow_sets(pt):
        got = pt.glass_any(o, d, tmax)
        st = pt.glass_shadow_stats()
        Tr, layers, cnt = ref.resolve_any(sc, pt.trace_closest, pt.trace_any, o, d, tmax, L)
        _same_any(got, (Tr, layers), f"{name} {filt} n {n}")
        assert st == (cnt if name != "solid" else dict(walked=0, passes=0, visible=0, exhausted=0)), (name, n, st, cnt)      # no thin pane: no walk, the flags alone
        lit += int((Tr.any(1) & (layers > 0)).sum()); free += int((Tr == 1.0).all(1).sum()); dark += int((~Tr.any(1)).sum())
        if n > 1:
            short = (np.arange(n) % 5 == 2) & (np.arange(n) % 7 != 3)
            assert (got[0][short] == 1.0).all() and not got[1][short].any()           # they end before any surface
    if name == "solid":
        assert lit == 0 and dark > 300 and free > 80
    else:
        assert lit > 200 and free > 80 and dark > 50, (lit, free, dark)
    pt.close()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pane", "stack3", "mixed", "solid"])
def test_shadow_walk_agrees_with_the_float64_walk(gpu, name):
    """ptc_debug_glass_any against `walk64_any` — float64 throughout, its own search of all triangles — on every record the walk decides
    (tests/test_glass_shadows_host.py::test_the_reference_decides_the_gpu_tests_records measures the undecided share and holds the restatement to the same walk)."""
    desc = ref.record_scenes(gpu)[name]
    pt = _ctx(gpu, desc)
    sc = gref.Scene(pt, desc)
    L = ref.rounds_limit(8, 8, sc.alpha is not None)
    total = und = 0
    for n, o, d, tmax in ref.shadow_sets(pt, (65, 513)):
        Tr, layers = pt.glass_any(o, d, tmax)
        w = ref.walk64_any(sc, o, d, tmax, L)
        m, worst = ref.check_against_walk64(Tr, layers, w, f"{name} n {n}")
        print(f"{name} n={n}: {m} records compared, error / bound at most {worst:.2e}")
        total += n; und += int(w["undecided"].sum())
    assert und <= ref.MAX_UNDECIDED * total
    pt.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_alpha_only_records_keep_alphas_bits(gpu):
    desc = ref.record_scenes(gpu)["mixed"]                                         # sheets at y = 0.75 and 0.5, the pane at y = 1
    on, off = _ctx(gpu, desc, True), _ctx(gpu, desc, False)
    seen = 0
    for n, o, d, tmax in ref.shadow_sets(on):
        tmax = np.minimum(tmax, ((0.9 - o[:, 1]) / np.abs(d[:, 1])).astype(F32))     # they end under the pane
        Tr, layers = on.glass_any(o, d, tmax)
        a = off.alpha_any(o, d, tmax)
        assert _bits_equal(Tr[:, 0], Tr[:, 1]) and _bits_equal(Tr[:, 0], Tr[:, 2]) and _bits_equal(Tr[:, 0], a), n
        seen += int(((a > 0) & (a < 1)).sum())
        flags, _ = off.glass_any(o, d, tmax)                                       # feature off: 0 or 1 from the flags
        assert np.isin(flags, (0.0, 1.0)).all() and np.array_equal(flags[:, 0] == 0, off.trace_any(o, d, tmax) != 0)
    assert seen > 100
    on.close(); off.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 3])
def test_exhaustion(gpu, limit):
    n, o, d, tmax = next(ref.shadow_sets(None, (513,)))
    for panes in (limit, limit + 1):
        desc = gpu.scenes.glass_panes(panes, spacing=0.2)
        pt = _ctx(gpu, desc).set_glass_max_interactions(limit)
        sc = gref.Scene(pt, desc)
        Tr, layers = pt.glass_any(o, d, tmax)
        st = pt.glass_shadow_stats()
        want = ref.resolve_any(sc, pt.trace_closest, pt.trace_any, o, d, tmax, limit)
        _same_any((Tr, layers), want[:2], f"{panes} panes, limit {limit}")
        assert st == want[2]
        through = (np.arange(n) % 5 != 2) & (np.arange(n) % 7 != 3)                   # the records that cross the whole stack
        if panes == limit:
            assert (layers[through] == limit).all() and Tr[through].all() and st["exhausted"] == 0 and st["visible"] == through.sum()
        else:
            assert not Tr[through].any() and st["exhausted"] == through.sum() and st["passes"] == limit * through.sum() and st["visible"] == 0
        pt.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_path_pass_transmits_the_same_share(gpu):
    N = 4096
    base = (0.9, 0.6, 0.3)
    desc = gpu.scenes.glass_panes(1, tilt=0.4, transmission=0.8, base=base)
    pt = _ctx(gpu, desc)
    sc = gref.Scene(pt, desc)
    d1 = np.array([math.sin(1.0), -math.cos(1.0), 0.0])
    o = np.repeat(np.array([[0.3, 1.0, 0.5]]) - 2.0 * d1[None], N, 0).astype(F32)
    d = np.repeat(d1[None], N, 0).astype(F32)
    t0, p0, uv0 = pt.trace_closest(o[:1], d[:1])
    assert p0[0] in (2, 3)
    P, ng, ns, front, b, met, mat = sc.surface(d[:1], p0, uv0)
    assert front[0] and not np.array_equal(ng, ns)
    W, F_t, _ = ref.transmit([0.8], [1.5], [True], ng, ns, d[:1], b, met)
    s = 0.8 * (1.0 - float(F_t[0]))
    Tr, layers = pt.glass_any(o[:1], d[:1], np.array([1.5 * t0[0]], F32))            # the shadow walk of the same ray, ended between the pane and the floor
    assert _bits_equal(Tr, W) and layers[0] == 1
    t, prim, uv, of, df, T, pdf, j = pt.glass_closest(o, d, np.arange(N, dtype=np.uint32), 0)
    trans = (j == 1) & np.isin(prim, (0, 1))
    k = int(trans.sum())
    sd = math.sqrt(N * s * (1 - s))
    print(f"transmitted {k} of {N}, expected {N * s:.1f} +- {sd:.1f}")
    assert abs(k - N * s) <= 5 * sd
    assert _bits_equal(T[trans], np.repeat(np.asarray(base, F32)[None], k, 0))
    assert (pdf[trans] == 1.0).all() and _bits_equal(of[trans], o[trans]) and _bits_equal(df[trans], d[trans])      # straight rays keep their record
    pt.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack3", "mixed", "solid"])
def test_closest_hits_with_the_feature_on_equal_the_restatement(gpu, name):
    desc = ref.record_scenes(gpu)[name]
    for m in desc.materials:
        if m.transmission > 0:
            m.transmission = 0.8
    if name == "solid":                                                              # a thin pane above the solid slab, so that the frame has the feature
        M = gpu.scene.Material
        desc.materials.append(M((0.9, 0.9, 1.0, 1.0), 0.0, 0.2, transmission=0.9, ior=1.4))
        desc.meshes.append(gpu.scene.MeshDesc(*gpu.scenes._quad((-2, 2.5, 2), (2, 2.5, 2), (2, 2.5, -2), (-2, 2.5, -2)), len(desc.materials) - 1))
        desc.instances.append(gpu.scene.InstanceDesc(len(desc.meshes) - 1, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    pt = _ctx(gpu, desc)
    sc = gref.Scene(pt, desc)
    straight = bent = 0
    from test_gpu_glass import _same_resolution
    for n, o, d, keys in gref.ray_sets(pt):
        for bounce in (0, 2):
            got = pt.glass_closest(o, d, keys, bounce)
            want = ref.resolve_closest(sc, pt.trace_closest, o, d, keys, bounce, 8)
            _same_resolution(got, want[:8], f"{name} n {n} bounce {bounce}")
            st = pt.glass_stats()
            assert {k: st[k] for k in want[8]} == want[8]
            t, prim, uv, of, df, T, pdf, j = got
            s = (j >= 1) & (pdf == 1.0)
            assert (pdf[j >= 1][~s[j >= 1]] == gref.DELTA_PDF).all() and _bits_equal(of[s], o[s]) and _bits_equal(df[s], d[s])
            hit = s & (prim >= 0)
            if hit.any():      # t counts from the source origin: o + t d is the standing hit, but for the sideways step of at most ray_eps that every pane passed adds (o' lies off the surface along ng)
                old = gref.resolve_closest(sc, pt.trace_closest, o, d, keys, bounce, 8)
                reach = old[3][hit].astype(F64) + old[0][hit, None].astype(F64) * d[hit].astype(F64)
                off = np.abs(o[hit].astype(F64) + t[hit, None].astype(F64) * d[hit].astype(F64) - reach).max(1)
                assert (off <= j[hit] * float(sc.eps) + 1e-5).all(), (off.max(), float(sc.eps))
            straight += int(s.sum()); bent += int(((j >= 1) & ~s).sum())
    assert straight > 100 and bent > (300 if name == "solid" else 30), (straight, bent)
    pt.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_sun_through_a_tinted_pane(gpu):
    w = h = 32
    sun = np.array([0.3, -1.0, 0.2])
    frames = {}
    for pane, on in ((True, True), (True, False), (False, True)):
        desc = gpu.scenes.glass_panes(1 if pane else 0, transmission=0.9, base=(0.9, 0.6, 0.3))
        desc.camera = gpu.scene.CameraDesc((0.2, 0.8, 0.3), (0.0, 0.0, 0.0), math.radians(40.0), 1.0)      # between the pane and the floor
        desc.lights = [dict(type="directional", direction=tuple(sun), intensity=(3.0, 2.5, 2.0))]
        pt = _ctx(gpu, desc, on)
        frames[pane, on] = pt.render(w, h, 16, seed=SEED, max_bounces=1)[..., :3].astype(F64)
        if pane and on:
            up = (-sun / np.linalg.norm(sun)).astype(F32)
            W = pt.glass_any(np.array([[0.0, 0.01, 0.0]], F32), up[None], np.array([10.0], F32))[0][0].astype(F64)
            st = pt.glass_shadow_stats()
        pt.close()
    lit, off, bare = frames[True, True], frames[True, False], frames[False, True]
    assert (bare > 0.1).all() and (W > 0.2).all() and (W < 0.9).all() and W[0] > W[1] > W[2]
    assert not off.any()                                                           # an opaque occluder to every shadow ray
    rel = np.abs(lit / (bare * W) - 1.0).max()
    print(f"sun through the pane: W {W.tolist()}, worst pixel {rel:.2e} relative")
    assert rel <= 1e-6


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _seed_means(gpu, desc, on, w, spp, K, bounces=2):
    pt = _ctx(gpu, desc, on)
    m = np.array([float(pt.render(w, w, spp, seed=300 + 11 * k, max_bounces=bounces)[..., :3].astype(F64).mean()) for k in range(K)])
    st = pt.glass_shadow_stats()
    pt.close()
    return m, st


def test_mis_an_invisible_pane_changes_nothing(gpu):
    """An ior-1, fully transmissive, white pane has W = 1 exactly: with the feature on the frame must have the pane-less frame's mean.  K = 12 seeds of 48x48 at
    64 spp; the standard error of the mean of means is asserted to be at most 1 % of it, so that a double count (up to 2x) or weights built on the last segment's t
    cannot hide."""
    w, spp, K = 48, 64, 12
    a, st = _seed_means(gpu, gpu.scenes.glass_slab(thin=True, transmission=1.0, ior=1.0, base=(1.0, 1.0, 1.0), emitter=True), True, w, spp, K)
    b, _ = _seed_means(gpu, gpu.scenes.glass_slab(thin=True, emitter=True, pane=False), True, w, spp, K)
    assert st["walked"] > 0 and st["visible"] > 0.3 * st["walked"]
    se = math.sqrt(a.var(ddof=1) / K + b.var(ddof=1) / K)
    print(f"pane {a.mean():.5f}, no pane {b.mean():.5f}: difference {abs(a.mean() - b.mean()) / se:.2f} combined standard errors; standard error {100 * se / b.mean():.3f} % of the mean")
    assert se <= 0.01 * b.mean()
    assert abs(a.mean() - b.mean()) <= 5 * se


def test_mis_on_and_off_agree_and_on_is_quieter(gpu):
    """ior 1.5 with a tint: both estimators are unbiased, so the means over K seeds agree; with next-event estimation through the pane the seed-to-seed variance of
    the frame's mean is lower.  Measured on one MI355X: DESIGN.md §2e has the ratio; only the direction is asserted."""
    w, spp, K = 48, 32, 12
    desc = lambda: gpu.scenes.glass_slab(thin=True, transmission=1.0, ior=1.5, base=(0.9, 0.8, 0.6), emitter=True)
    on, _ = _seed_means(gpu, desc(), True, w, spp, K)
    off, _ = _seed_means(gpu, desc(), False, w, spp, K)
    se = math.sqrt(on.var(ddof=1) / K + off.var(ddof=1) / K)
    print(f"on {on.mean():.5f}, off {off.mean():.5f}: difference {abs(on.mean() - off.mean()) / se:.2f} combined standard errors; variance of the mean off / on {off.var(ddof=1) / on.var(ddof=1):.1f}")
    assert on.mean() > 0.01 and abs(on.mean() - off.mean()) <= 5 * se
    assert on.var(ddof=1) < off.var(ddof=1)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _lit_panes(gpu):
    desc = gpu.scenes.glass_panes(2, tilt=0.3, transmission=0.9, emitter=True, sheets=("blend",), textured=True, texture_filter="linear")
    desc.lights = [dict(type="point", position=(0.5, 3.0, -0.5), intensity=(8.0, 8.0, 6.0))]
    desc.env = np.full((4, 8, 3), 0.5, F32)
    return desc


def test_off_is_today(gpu):
    w = h = 32
    desc = _lit_panes(gpu)
    never, zero = _ctx(gpu, desc, None), _ctx(gpu, desc, False)
    a, b = never.render(w, h, 8, seed=SEED, max_bounces=3), zero.render(w, h, 8, seed=SEED, max_bounces=3)
    assert _bits_equal(a, b)
    assert zero.glass_shadow_stats() == dict(walked=0, passes=0, visible=0, exhausted=0) and not zero.get_glass_shadows()
    on = _ctx(gpu, desc, True)
    c = on.render(w, h, 8, seed=SEED, max_bounces=3)
    assert not _bits_equal(a, c) and on.glass_shadow_stats()["passes"] > 0             # and on is not
    for pt in (never, zero, on):
        pt.close()
    # a scene without a thin transmissive material: on renders off's bits, launches what off launches and reports zeros
    solid = gpu.scenes.glass_slab(thin=False, base=(0.9, 0.8, 0.7), emitter=True, sheet_alpha=0.5)
    solid.lights = [dict(type="point", position=(0.5, 3.0, -0.5), intensity=(8.0, 8.0, 6.0))]
    on, off = _ctx(gpu, solid, True), _ctx(gpu, solid, False)
    a, b = on.render(w, h, 8, seed=SEED, max_bounces=3), off.render(w, h, 8, seed=SEED, max_bounces=3)
    sa, sb = on.stats(), off.stats()
    assert _bits_equal(a, b) and (a[..., :3] > 0).any()
    assert all(sa[k] == sb[k] for k in ("paths", "segments", "shadow_rays", "launches_trace_closest", "launches_trace_any"))
    assert on.glass_shadow_stats() == dict(walked=0, passes=0, visible=0, exhausted=0) and on.alpha_stats()["shadow_walked"] == off.alpha_stats()["shadow_walked"] > 0
    on.close(); off.close()


def test_switching_on_late(gpu):
    w = h = 32
    desc = _lit_panes(gpu)
    pt = _ctx(gpu, desc, None)
    first = pt.render(w, h, 8, seed=SEED, max_bounces=3)
    late = pt.set_glass_shadows(True).render(w, h, 8, seed=SEED, max_bounces=3)        # the glass queue has no flag bytes yet
    fresh_pt = _ctx(gpu, desc, True)
    fresh = fresh_pt.render(w, h, 8, seed=SEED, max_bounces=3)
    assert _bits_equal(late, fresh) and not _bits_equal(late, first) and pt.glass_shadow_stats() == fresh_pt.glass_shadow_stats()
    again = pt.set_glass_shadows(False).render(w, h, 8, seed=SEED, max_bounces=3)      # and off again
    assert _bits_equal(again, first)
    pt.close(); fresh_pt.close()


def test_tile_shards_merge_to_the_unsharded_frame(gpu):
    w = h = 48
    pt = _ctx(gpu, _lit_panes(gpu))
    whole = pt.render(w, h, 8, seed=SEED, max_bounces=3)
    st = pt.glass_shadow_stats()
    assert st["walked"] > 0 and st["passes"] > 0 and st["visible"] > 0
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
    pt = _ctx(gpu, _lit_panes(gpu))
    img = pt.render_adaptive(w, h, 32, seed=SEED, max_bounces=2, threshold=0.05, radius=1, min_samples=8, step_samples=8)
    counts = pt.read_sample_counts()
    seen = np.unique(counts)
    assert set(seen.tolist()) <= {8, 16, 24, 32}, seen
    for n in seen:
        uniform = pt.render(w, h, int(n), seed=SEED, max_bounces=2)
        assert _bits_equal(img[counts == n], uniform[counts == n]), int(n)
    pt.close()


def test_the_walk_survives_refit_and_rebuild(gpu):
    desc = ref.record_scenes(gpu)["stack3"]
    pt = _ctx(gpu, desc)
    for k, step in enumerate(("refit", "rebuild")):
        for inst in range(1, len(desc.instances)):                                   # the floor stays; the panes move together
            pt.update_instance(inst, (0.05 * (k + 1), 0.02 * (k + 1), -0.03 * (k + 1)), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        pt.scene_refit() if step == "refit" else pt.scene_rebuild()
        sc = gref.Scene(pt, desc)
        for n, o, d, tmax in ref.shadow_sets(pt, (65, 513)):
            got = pt.glass_any(o, d, tmax)
            want = ref.resolve_any(sc, pt.trace_closest, pt.trace_any, o, d, tmax, 8)
            _same_any(got, want[:2], f"after {step} n {n}")
            assert pt.glass_shadow_stats() == want[2] and (got[1] == 3).sum() > 0.5 * n
    pt.close()
