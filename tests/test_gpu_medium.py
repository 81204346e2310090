"""The participating medium on a real MI355X (include/ptc_medium.h, csrc/pt_medium.hip).

1. ptc_debug_medium_step against the numpy restatement (tests/medium_reference.py), bit for bit, on 1 / 63 / 64 / 65 / 513 / 1537 rays (one, two and four segments) at
   bounces 0, 2 and max_bounces: fog_box with its emitter, with a point and a spot light, with two point lights; shade_sky (an environment) and shade_lobes under that
   environment (emitters and an environment); rays that stand against ptc_debug_shade_step and ptc_debug_punctual_nee with their shadow records attenuated; a set where
   every ray scatters, one where none does, a segment without a scatter event; the counters.  Every set against the float64 reference written from the definitions, on
   every ray it decides.  The pass's text of the environment sampler and lookup against k_shade's own, bit for bit.
2. Statistics over 65,536 keys on one ray: the scatter share, the distances over 64 equiprobable cells, the directions over 256 cells of equal solid angle.
3. Physics: single scattering from a point light and from a small emitter against the float64 airlight integral; the furnace.
4. Frames: sigma_t = 0 and a cleared medium are a context that never called the feature and the frame recorded on the commit before it, bit for bit; tile shards, an
   adaptive frame, refit and rebuild with fog; a sun shaft's attenuation; ptc_render --fog scene:."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lights_reference as lref  # noqa: E402
import medium_reference as ref  # noqa: E402
import shade_reference as sref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
COUNTS = (1, 63, 64, 65, 513, 1537)
MAXB = 4
TWO_LIGHTS = [dict(type="point", position=(0.0, 0.9, 0.3), intensity=(3.0, 3.0, 3.0)),
              dict(type="spot", position=(-1.0, 1.2, 0.0), direction=(0.3, -1.0, 0.1), intensity=(5.0, 4.0, 3.0), cos_inner=0.9, cos_outer=0.6, sampling_weight=2.0)]
TWO_POINTS = [dict(type="point", position=(0.0, 0.9, 0.3), intensity=(3.0, 3.0, 3.0)),
              dict(type="point", position=(-1.0, 2.5, 0.0), intensity=(5.0, 4.0, 3.0), sampling_weight=2.0)]


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _rays(n, seed, kind="mixed"):
    """Rays from the camera's side into fog_box's fog.  mixed: towards points of the box; away: every ray points away from it; half: the rays from slot 320 on (the second
    segment of a 513-ray set) point away."""
    rng = np.random.default_rng(seed)
    o = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.2, 1.3, n), rng.uniform(2.5, 4.0, n)]).astype(F32)
    tgt = np.column_stack([rng.uniform(-1.8, 1.8, n), rng.uniform(0.0, 1.4, n), rng.uniform(-1.8, 1.8, n)])
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    if kind == "away":
        d[:, 2] = np.abs(d[:, 2])
    if kind == "half":
        d[320:, 2] = np.abs(d[320:, 2])
    if kind == "inside":
        o = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.2, 1.3, n), rng.uniform(-1.5, 1.5, n)]).astype(F32)
    if kind == "floor":      # shade_lobes / shade_sky: from above onto the 3 x 3 floor at y = 0, through a fog box that lies on it
        o = np.column_stack([rng.uniform(-1, 1, n), rng.uniform(1.5, 2.5, n), rng.uniform(-1, 1, n)]).astype(F32)
        tgt = np.column_stack([rng.uniform(-1.2, 1.2, n), np.zeros(n), rng.uniform(-1.2, 1.2, n)])
        d = tgt - o
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    T = rng.uniform(0.2, 1.0, (n, 3)).astype(F32)
    T[: (n + 2) // 3] = 1.0      # a third with throughput 1: where the punctual pass's own contribution (its hook stages T = 1) can be compared bit for bit
    keys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return o, d, T, keys, np.full(n, 0.7, F32)


seen_T1 = [0]      # standing punctual records with T = 1 that crossed the fog, over the whole module


def _check_step(pt, md, lights, o, d, T, keys, pp, bounce, what, env=None):
    """One ptc_debug_medium_step against the restatement (bit for bit) and the float64 reference; returns the restatement's result."""
    n = len(o)
    t, prim, _ = pt.trace_closest(o, d)
    _, emit, cdf = pt.shading_tables()
    if not pt.stats()["n_emitters"]:
        emit, cdf = None, None
    table = lref.light_table(lights) if lights else None
    want = ref.scatter_step(md, o, d, T, keys, t, prim >= 0, bounce, MAXB, emit, cdf, 1.0, table, F32, env=env)
    sh = pt.shade_step(o, d, T, pp, keys, bounce=bounce, max_bounces=MAXB)
    got = pt.medium_step(o, d, T, pp, keys, bounce=bounce, max_bounces=MAXB)
    st = pt.medium_stats()
    sc = want["scattered"]
    # the hit record as k_shade saw it: the miss record for a scattered ray, the trace's own otherwise
    assert np.array_equal(got["word"][sc], np.full(sc.sum(), -1)) and np.array_equal(got["t"][sc], np.full(sc.sum(), -1.0, F32)), what
    assert _bits_equal(got["t"][~sc], sh["t"][~sc]) and np.array_equal(got["word"][~sc], sh["word"][~sc]), what
    assert st["crossed"] == int(want["crossed"].sum()) and st["scattered"] == int(sc.sum()), (what, st)
    if bounce == MAXB:      # the last bounce: a scattered ray simply ends, nothing is appended
        assert not got["alive"].any() and not got["shadow"].any() and not got["punctual"].any(), what
        return want, None, st
    # continuations: the medium's for a scattered ray, k_shade's own for one that stands
    alive = np.where(sc, want["alive"], sh["alive"])
    assert np.array_equal(got["alive"], alive), what
    cont = np.where(sc[:, None], want["cont"], np.column_stack([sh["o"], sh["d"], sh["T"], sh["pdf"]]))
    assert _bits_equal(np.column_stack([got["o"], got["d"], got["T"], got["pdf"]])[alive], cont[alive]), what
    # shadow records: the medium's (attenuated by the restatement), k_shade's attenuated here
    s_att, s_hit = ref.attenuate(md, sh["so"], sh["sd"], sh["tmax"], sh["contrib"])
    shadow = np.where(sc, want["shadow"], sh["shadow"])
    assert np.array_equal(got["shadow"], shadow), what
    srec = np.where(sc[:, None], want["srec"], np.column_stack([sh["so"], sh["sd"], sh["tmax"], s_att]))
    assert _bits_equal(np.column_stack([got["so"], got["sd"], got["tmax"], got["contrib"]])[shadow], srec[shadow]), what
    m = sc & want["shadow"]
    n_att = int(ref.span(md, want["srec"][m, 0:3], want["srec"][m, 3:6], want["srec"][m, 6])[0].sum()) + int((s_hit & ~sc & sh["shadow"]).sum())
    if lights:
        # k_shade_punctual's own records: the hook stages throughput 1, its contribution is linear in T
        pv, po, pd, ptm, pc = pt.punctual_nee(o, d, keys, bounce=bounce)
        p_att, p_hit = ref.attenuate(md, po, pd, ptm, pc)
        punctual = np.where(sc, want["punctual"], pv)
        assert np.array_equal(got["punctual"], punctual), what
        m = sc & punctual
        assert _bits_equal(np.column_stack([got["po"], got["pd"], got["ptmax"], got["pcontrib"]])[m], want["prec"][m]), what
        m = ~sc & punctual      # a standing ray: origin, direction and tmax are the punctual pass's own, bit for bit; so is the attenuated contribution where T = 1
        assert _bits_equal(np.column_stack([got["po"], got["pd"], got["ptmax"]])[m], np.column_stack([po, pd, ptm])[m]), what
        m1 = m & (T == 1.0).all(1)
        assert _bits_equal(got["pcontrib"][m1], p_att[m1]), what
        seen_T1[0] += int((m1 & p_hit).sum())
        mp = sc & want["punctual"]
        n_att += int(ref.span(md, want["prec"][mp, 0:3], want["prec"][mp, 3:6], want["prec"][mp, 6])[0].sum()) + int((p_hit & m).sum())
    # the float64 reference (written from the definitions) at the device's own directions, on every ray it decides
    g2 = ref.as_got(got, d, scattered=sc)
    r64 = ref.reference64(md, o, d, T, keys, t, prim >= 0, bounce, MAXB, g2, emit, cdf, table, env)
    bad, und = ref.check(md, g2, r64, what)
    assert bad == [], bad
    assert und <= (0 if n == 1 else int(0.02 * n)), (what, und)
    return want, n_att, st


FLOOR_FOG = dict(box_lo=(-1.5, 0.05, -1.5), box_hi=(1.5, 1.2, 1.5), sigma_t=1.1, albedo=(0.8, 0.9, 1.0), g=0.4)


@pytest.mark.parametrize("scene", ["emitters", "punctual", "points", "sky", "mixed"])
def test_step_equals_the_restatement_bit_for_bit(gpu, scene):
    """fog_box with its emitter; with a point and a spot light and no emitter; with two point lights and the emitter; shade_sky (an environment alone: p_env = 1);
    shade_lobes under shade_sky's environment (emitters and an environment: the kind is drawn with p_env = 0.5)."""
    from pbr_amd import scenes
    lights = {"punctual": TWO_LIGHTS, "points": TWO_POINTS}.get(scene, [])
    if scene in ("sky", "mixed"):
        desc = scenes.shade_sky()
        if scene == "mixed":
            env = desc.env
            desc = scenes.shade_lobes()
            desc.env = env
        desc.medium = dict(FLOOR_FOG)
        kind = "floor"
    else:
        desc = scenes.fog_box(sigma_t=1.3, albedo=(0.9, 0.7, 0.5), g=0.6, emitter=8.0 if scene != "punctual" else 0.0)
        kind = "mixed"
    pt = gpu.PathTracer(0).load_scene(desc)
    for l in lights:
        pt.add_light(l)
    env = None
    if desc.env is not None:
        tab, marg, cond, ok = pt.env_tables()
        assert ok
        env = (tab, marg, cond, ok)
        assert (pt.stats()["n_emitters"] > 0) == (scene == "mixed")
    md = ref.Medium(**desc.medium)
    seen = dict(scattered=0, alive=0, shadow=0, punctual=0, stand=0, use_env=0, use_area=0)
    for n in COUNTS:
        for bounce in (0, 2, MAXB):
            o, d, T, keys, pp = _rays(n, 100 * n + bounce, kind)
            want, n_att, st = _check_step(pt, md, lights, o, d, T, keys, pp, bounce, f"{scene} n={n} b={bounce}", env)
            assert n_att is None or st["attenuated"] == n_att, (scene, n, bounce, st, n_att)
            for k in ("scattered", "alive", "shadow", "punctual"):
                seen[k] += int(want[k].sum())
            seen["stand"] += int((want["crossed"] & ~want["scattered"]).sum())
            seen["use_env"] += int((want["shadow"] & want["use_env"]).sum())
            seen["use_area"] += int((want["shadow"] & ~want["use_env"]).sum())
    assert seen["scattered"] > 1000 and seen["alive"] > 500 and seen["stand"] > 100, seen
    assert (seen["shadow"] > 300) == (scene != "punctual") and (seen["punctual"] > 300) == bool(lights), seen
    assert (seen["use_env"] > 200) == (scene in ("sky", "mixed")) and (seen["use_area"] > 200) == (scene in ("emitters", "points", "mixed")), seen
    if scene == "punctual":
        assert seen_T1[0] > 20, seen_T1


def test_all_scatter_none_scatter_and_an_empty_segment(gpu):
    from pbr_amd import scenes
    desc = scenes.fog_box(sigma_t=1.3, albedo=(0.9, 0.7, 0.5), g=-0.6)
    pt = gpu.PathTracer(0).load_scene(desc)
    md = ref.Medium(**desc.medium)
    # none: every ray points away from the box — nothing is written, the step is k_shade's own
    o, d, T, keys, pp = _rays(513, 7, "away")
    want, n_att, st = _check_step(pt, md, [], o, d, T, keys, pp, 0, "away")
    assert not want["crossed"].any() and st["crossed"] == st["scattered"] == 0
    # a segment without a scatter event beside one with many
    o, d, T, keys, pp = _rays(513, 8, "half")
    want, n_att, st = _check_step(pt, md, [], o, d, T, keys, pp, 0, "half")
    assert want["scattered"][:320].sum() > 50 and not want["crossed"][320:].any()
    # every ray scatters: origins inside a thick fog
    dense = dict(desc.medium, sigma_t=4000.0)
    pt.set_medium(**dense)
    md = ref.Medium(**dense)
    o, d, T, keys, pp = _rays(1537, 9, "inside")
    want, n_att, st = _check_step(pt, md, [], o, d, T, keys, pp, 0, "dense")
    assert want["scattered"].all() and st["scattered"] == 1537 and st["attenuated"] == n_att


def test_environment_text_equals_k_shades(gpu):
    """The pass has a second text of k_shade's environment sampler and lookup (pt_kernels.hip is hashed).  ptc_debug_medium_env runs it on its own: the direction it
    samples from (r1, r2) is, bit for bit, the direction of the shadow record k_shade writes for the same numbers (ptc_debug_shade_step on shade_sky, the numbers
    recomputed through the tests' rng_f); the radiance it looks up is, bit for bit, what k_shade adds for a miss at bounce 0 with throughput 1; its pdf is the map's
    texel pmf over the texel's solid angle in float64."""
    from lens_reference import rng_f
    from pbr_amd import scenes
    pt = gpu.PathTracer(0).load_scene(scenes.shade_sky())
    env, _, _, ok = pt.env_tables()
    h, w = env.shape[0], env.shape[1]
    rng = np.random.default_rng(21)
    n = 1537
    o = np.column_stack([rng.uniform(-1, 1, n), rng.uniform(0.5, 2.0, n), rng.uniform(-1, 1, n)]).astype(F32)
    tgt = np.column_stack([rng.uniform(-1.2, 1.2, n), np.zeros(n), rng.uniform(-1.2, 1.2, n)])
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    keys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    one3, one = np.ones((n, 3), F32), np.ones(n, F32)
    for bounce in (0, 2):
        sh = pt.shade_step(o, d, one3, one, keys, bounce=bounce, max_bounces=MAXB)
        wi, _, _ = pt.medium_env(rng_f(keys, bounce + 1, 1), rng_f(keys, bounce + 1, 2), d)
        m = sh["shadow"]
        assert m.sum() > n // 4 and _bits_equal(sh["sd"][m], wi[m]), bounce
    up = rng.normal(size=(n, 3))
    up[:, 1] = np.abs(up[:, 1]) + 1e-3
    up[: n // 8, 1] *= 50.0                                          # many near the pole, where the map is brightest and sin(theta) small
    up = (up / np.linalg.norm(up, axis=1, keepdims=True)).astype(F32)
    sky = pt.shade_step(np.tile(np.asarray([[0.0, 1.0, 0.0]], F32), (n, 1)), up, one3, one, keys, bounce=0, max_bounces=MAXB)
    assert (sky["word"] == -1).all()
    _, Le, pdf = pt.medium_env(np.zeros(n, F32), np.zeros(n, F32), up)
    assert _bits_equal(Le, sky["lpath"])
    u64 = up.astype(F64)
    phi, theta = np.arctan2(u64[:, 2], u64[:, 0]), np.arccos(np.clip(u64[:, 1], -1, 1))
    xs, ys = (phi / (2 * np.pi) + 0.5) * w, theta / np.pi * h
    near = np.minimum(np.abs(xs - np.round(xs)) * (2 * np.pi / w), np.abs(ys - np.round(ys)) * (np.pi / h)) < 4 * sref.ATAN_MARGIN
    x, y = np.clip(np.floor(xs).astype(int), 0, w - 1), np.clip(np.floor(ys).astype(int), 0, h - 1)
    st = np.sqrt(np.maximum(1 - u64[:, 1] ** 2, 0))
    want = env[y, x, 3].astype(F64) * w * h / (2 * np.pi ** 2 * np.maximum(st, 1e-6))
    assert _bits_equal(Le[~near], env[y, x, 0:3][~near])
    tol = 2.0 ** -23 * (4 + 1 / np.maximum(st * st, 1e-12))           # five roundings, and sqrt(1 - y^2) from a float32 y^2
    assert near.mean() < 0.05 and (np.abs(pdf - want)[~near] <= (tol * want)[~near]).all(), (np.abs(pdf / want - 1) / tol)[~near].max()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [-0.6, 0.0, 0.8])
def test_statistics_over_65536_keys(gpu, g):
    from pbr_amd import scenes
    sigma, L = 0.5, 4.0
    desc = scenes.fog_box(sigma_t=sigma, albedo=1.0, g=g, emitter=0.0)
    pt = gpu.PathTracer(0).load_scene(desc)
    n = 65536
    o, d = np.tile(np.asarray([[0.0, 0.75, 3.5]], F32), (n, 1)), np.tile(np.asarray([[0.0, 0.0, -1.0]], F32), (n, 1))      # crosses the box from z = 2 to z = -2, hits nothing
    keys = np.random.default_rng(int(100 + 10 * g)).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    got = pt.medium_step(o, d, np.ones((n, 3), F32), np.ones(n, F32), keys, bounce=0, max_bounces=MAXB)
    sc = got["alive"]      # T = 1, albedo 1, bounce 0: every scattered ray goes on (the ray misses the scene: a standing ray has the miss record as well)
    assert pt.medium_stats()["scattered"] == int(sc.sum()) and (got["word"] == -1).all()
    p = 1.0 - math.exp(-sigma * L)
    assert abs(sc.mean() - p) <= 5 * math.sqrt(p * (1 - p) / n), (sc.mean(), p)
    # distances: 64 cells of equal probability of the truncated exponential
    s = 2.0 - got["o"][sc, 2].astype(F64)
    cell = np.minimum(((1.0 - np.exp(-sigma * s)) / p * 64).astype(int), 63)
    stat, dof, pv = sref.chi2_test(np.bincount(cell, minlength=64), np.full(64, sc.sum() / 64.0))
    assert pv >= 1e-6, (stat, dof, pv)
    # directions: 16 x 16 cells of equal solid angle about d
    wi = got["d"][sc].astype(F64)
    c = np.clip(-wi[:, 2], -1, 1)
    tx, ty = ref.onb(np.asarray([[0.0, 0.0, -1.0]]), F64)
    phi = np.arctan2(wi @ ty[0], wi @ tx[0]) % (2 * np.pi)
    ci, pi_ = np.minimum(((c + 1) / 2 * 16).astype(int), 15), np.minimum((phi / (2 * np.pi) * 16).astype(int), 15)
    edges = np.linspace(-1, 1, 17)
    cdf = (edges + 1) / 2 if abs(g) < 1e-3 else (1 - g * g) / (2 * g) * (1 / np.sqrt(1 + g * g - 2 * g * edges) - 1 / (1 + g))
    expected = np.repeat(np.diff(cdf) * sc.sum() / 16.0, 16)
    stat, dof, pv = sref.chi2_test(np.bincount(ci * 16 + pi_, minlength=256), expected)
    assert pv >= 1e-6, (g, stat, dof, pv)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _airlight_scene(pbr, light, emitter):
    """A fog box in front of the camera, a tiny black triangle out of view as the scene's geometry, and a point light or a small downward emitter above the view."""
    from pbr_amd import scenes
    from pbr_amd.scene import CameraDesc, InstanceDesc, Material, MeshDesc, SceneDesc
    mats = [Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0), Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (40.0, 30.0, 20.0))]
    v, i = scenes._quad((50.0, 50.0, 50.0), (50.01, 50.0, 50.0), (50.01, 50.0, 50.01), (50.0, 50.0, 50.01))
    meshes = [MeshDesc(v, i, 0)]
    if emitter:
        ev, ei = scenes._quad(*emitter)
        meshes.append(MeshDesc(ev, ei, 1))
    inst = [InstanceDesc(k, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0)) for k in range(len(meshes))]
    desc = SceneDesc(mats, meshes, inst, CameraDesc((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), math.radians(30.0), 1.0), "airlight")
    desc.medium = dict(box_lo=(-1.5, -1.5, -1.5), box_hi=(1.5, 1.5, 1.5), sigma_t=0.6, albedo=(0.9, 0.8, 0.7), g=0.5)
    pt = pbr.PathTracer(0).load_scene(desc)
    if light:
        pt.add_light(light)
    return pt, ref.Medium(**desc.medium)


def _airlight(md, o, d, points, weight, normal=None, ns=300, pdf_area=None):
    """The float64 single-scattering integral along the rays (o, d): the sum over the light's points (positions, radiant weights I or Le dA, the emitter's normal) of
    int sigma_s e^(-sigma (s - t0)) e^(-sigma 0.999 dist) ph W cosl / dist^2 ds, by the midpoint rule.  (n, 3)."""
    ok, t0, t1 = ref.span(md, o, d, np.full(len(o), ref.T_INF), F64)
    u = (np.arange(ns) + 0.5) / ns
    s = t0[:, None] + (t1 - t0)[:, None] * u[None, :]
    P = o.astype(F64)[:, None, :] + d.astype(F64)[:, None, :] * s[..., None]
    out = np.zeros((len(o), ns))
    sig = F64(md.sigma_t)
    for y in points:
        dv = y[None, None, :] - P
        dist = np.linalg.norm(dv, axis=2)
        wi = dv / dist[..., None]
        cosl = 1.0 if normal is None else np.maximum(-(wi @ normal), 0.0)
        ph = ref.hg_phase(md.g, (wi * d.astype(F64)[:, None, :]).sum(2), F64)
        # the light lies inside the box, so the whole segment to it does.  The next-event sample's shadow segment ends 0.1 % before the light; the emitter hit of the
        # phase-function sample travels the whole distance.  The two estimators share the integrand by their MIS weights (an area pdf pl against ph)
        if normal is None:
            tr = np.exp(-sig * 0.999 * dist)
        else:
            pl = pdf_area * dist * dist / np.maximum(cosl, 1e-9)
            w_nee = np.where(cosl > 0, pl * pl / (pl * pl + ph * ph), 1.0)      # seen from behind the emitter gives nothing either way
            tr = w_nee * np.exp(-sig * 0.999 * dist) + (1 - w_nee) * np.exp(-sig * dist)
        out += np.exp(-sig * (s - t0[:, None])) * tr * ph * cosl / (dist * dist)
    val = out.sum(1) * (t1 - t0) / ns * sig * ok
    return val[:, None] * (md.albedo.astype(F64) * np.asarray(weight, F64))[None, :]


def _block_means(img, b=8):
    h, w = img.shape[0], img.shape[1]
    return img[..., :3].astype(F64).reshape(h // b, b, w // b, b, 3).mean((1, 3))


@pytest.mark.parametrize("kind", ["point", "emitter"])
def test_single_scattering_against_quadrature(gpu, kind):
    """max_bounces = 1, 32 x 32 x 64 spp, 12 seeds: the block means against the airlight integral, within 5 standard errors of the seed-to-seed mean.  With the emitter the
    next-event sample at bounce 0 and the emitter hit at bounce 1 sum to the integral only if their two MIS weights sum to one."""
    if kind == "point":
        pt, md = _airlight_scene(gpu, dict(type="point", position=(0.3, 1.4, 0.2), intensity=(4.0, 3.0, 2.0)), None)
        points, weight, normal = [np.asarray([0.3, 1.4, 0.2])], (4.0, 3.0, 2.0), None
    else:
        a, b, c, e = (0.1, 1.45, 0.0), (0.5, 1.45, 0.0), (0.5, 1.45, 0.4), (0.1, 1.45, 0.4)      # faces down, above the view
        pt, md = _airlight_scene(gpu, None, (a, b, c, e))
        k = 5
        g1 = (np.arange(k) + 0.5) / k
        points = [np.asarray([0.1 + 0.4 * x, 1.45, 0.4 * z]) for x in g1 for z in g1]
        weight, normal = np.asarray((40.0, 30.0, 20.0)) * (0.16 / (k * k)), np.asarray([0.0, -1.0, 0.0])
    imgs = np.stack([_block_means(pt.render(32, 32, 64, seed=1000 + s, max_bounces=1)) for s in range(12)])
    mean, se = imgs.mean(0), imgs.std(0, ddof=1) / math.sqrt(12)
    # the integral over a block's pixels by 8 jittered rays per pixel (512 per block), 300 steps per ray, 5 x 5 points on the emitter
    spp_q = 8
    o, d = pt.debug_camera_rays(32, 32, 77, 0, spp_q)
    want = _airlight(md, o, d, points, weight, normal, pdf_area=None if normal is None else 1.0 / 0.16).reshape(spp_q, 32, 32, 3).mean(0)      # one emitter quad of two equal triangles: pmf / A = 1 / 0.16
    want = want.reshape(4, 8, 4, 8, 3).mean((1, 3))
    print(kind, "worst |mean - integral| / se:", float((np.abs(mean - want) / se).max()), "relative:", float((np.abs(mean - want) / want).max()))
    assert (want > 0).all() and (np.abs(mean - want) <= 5 * se).all(), (np.abs(mean - want) / se).max()
    st = pt.medium_stats()
    assert st["scattered"] > 0 and st["attenuated"] > 0 and st["seconds_medium"] > 0.0


def test_furnace(gpu):
    """A constant environment of 1, albedo 1, max_bounces 64: every pixel's expectation is 1 (roulette does not act: T stays 1)."""
    from pbr_amd import scenes
    from pbr_amd.scene import CameraDesc, InstanceDesc, Material, MeshDesc, SceneDesc
    v, i = scenes._quad((50.0, 50.0, 50.0), (50.01, 50.0, 50.0), (50.01, 50.0, 50.01), (50.0, 50.0, 50.01))
    desc = SceneDesc([Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0)], [MeshDesc(v, i, 0)], [InstanceDesc(0, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))],
                     CameraDesc((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), math.radians(30.0), 1.0), "furnace")
    desc.env = np.ones((8, 16, 3), F32)
    desc.medium = dict(box_lo=(-1.5, -1.5, -1.5), box_hi=(1.5, 1.5, 1.5), sigma_t=1.5, albedo=1.0, g=0.7)
    pt = gpu.PathTracer(0).load_scene(desc)
    imgs = np.stack([pt.render(16, 16, 16, seed=50 + s, max_bounces=64)[..., :3].astype(F64).mean() for s in range(8)])
    se = imgs.std(ddof=1) / math.sqrt(8)
    assert abs(imgs.mean() - 1.0) <= 5 * se, (imgs.mean(), se)
    assert pt.medium_stats()["scattered"] > 1000


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_medium_off_is_a_context_that_never_called_the_feature(gpu):
    from pbr_amd import scenes
    desc = scenes.fog_box(sigma_t=0.0)
    sun = dict(type="directional", direction=(0.15, -1.0, 0.05), intensity=(6.0, 5.5, 5.0))
    plain = gpu.PathTracer(0).load_scene(desc)
    plain.add_light(sun)
    base = plain.render(48, 48, 8, seed=3, max_bounces=4)
    # the frame's bits on the commit before the feature (recorded there, tests/golden)
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fog_box_sun_off_48x48x8_seed3.npy"))
    assert _bits_equal(base, golden)
    pt = gpu.PathTracer(0).load_scene(desc)
    pt.add_light(sun)
    fog = dict(box_lo=(-2.0, 0.0, -2.0), box_hi=(2.0, 1.5, 2.0), sigma_t=0.7, albedo=0.9, g=0.3)
    pt.set_medium(**dict(fog, sigma_t=0.0))
    assert _bits_equal(pt.render(48, 48, 8, seed=3, max_bounces=4), base)
    pt.set_medium(**fog)
    foggy = pt.render(48, 48, 8, seed=3, max_bounces=4)
    assert np.isfinite(foggy).all() and not _bits_equal(foggy, base) and pt.medium_stats()["scattered"] > 0
    pt.clear_medium()
    assert _bits_equal(pt.render(48, 48, 8, seed=3, max_bounces=4), base)
    assert pt.medium_stats() == dict(crossed=0, scattered=0, attenuated=0, seconds_medium=0.0)
    # with fog: the tile shards of a frame are the frame; refit and rebuild between frames keep the medium; an adaptive frame runs
    pt.set_medium(**fog)
    whole = pt.render(48, 48, 8, seed=3, max_bounces=4)
    assert _bits_equal(whole, foggy)
    parts = np.zeros_like(whole)
    for r in range(3):
        pt.frame_begin(48, 48, 8, seed=3, max_bounces=4, tile_rank=r, tile_count=3)
        pt.frame_add_samples(8)
        pt.frame_resolve()
        pt.sync()
        parts += pt.read_radiance()
    assert _bits_equal(parts, whole)
    pt.update_instance(0, t=(0.0, 0.0, 0.0), q_wxyz=(1.0, 0.0, 0.0, 0.0), s=(1.0, 1.0, 1.0))
    pt.scene_refit()
    moved = pt.render(48, 48, 8, seed=3, max_bounces=4)
    assert np.isfinite(moved).all() and abs(moved[..., :3].mean() / whole[..., :3].mean() - 1.0) < 0.02 and pt.get_medium() is not None
    pt.scene_rebuild()
    again = pt.render(48, 48, 8, seed=3, max_bounces=4)
    assert np.isfinite(again).all() and pt.medium_stats()["scattered"] > 0
    ad = pt.render_adaptive(48, 48, 16, seed=3, max_bounces=4)
    img = ad[0] if isinstance(ad, tuple) else ad
    assert np.isfinite(np.asarray(img)).all() and pt.medium_stats()["scattered"] > 0


def test_sun_shaft_is_attenuated_by_the_transmittance(gpu):
    """A sun through fog_box's slit with albedo = 0 fog in a slab under the blocker that no camera ray to the floor crosses: every lit floor pixel is the fog-free
    frame times e^(-sigma x the sun's path through the slab), within the measured transmittance bound (and the sums' roundings).  max_bounces 1 and no emitter: the
    floor's radiance is the sun's direct light alone, and the slab's only effect is step 6 on the punctual pass's shadow records."""
    from pbr_amd import scenes
    desc = scenes.fog_box(sigma_t=0.0, emitter=0.0)
    sun_dir = np.asarray((0.15, -1.0, 0.05))
    sun = dict(type="directional", direction=tuple(sun_dir), intensity=(6.0, 5.5, 5.0))
    pt = gpu.PathTracer(0).load_scene(desc)
    pt.add_light(sun)
    clear = pt.render(64, 64, 16, seed=9, max_bounces=1)[..., :3].astype(F64)
    sigma, lo_y, hi_y = 1.7, 1.0, 1.4
    pt.set_medium(box_lo=(-3.0, lo_y, -3.0), box_hi=(3.0, hi_y, 3.0), sigma_t=sigma, albedo=0.0, g=0.0)
    fog = pt.render(64, 64, 16, seed=9, max_bounces=1)[..., :3].astype(F64)
    st = pt.medium_stats()
    lit = clear.max(2) > 0
    assert lit.sum() > 50 and st["attenuated"] > 0
    path = (hi_y - lo_y) / abs(sun_dir[1] / np.linalg.norm(sun_dir))
    want = clear * math.exp(-float(F32(sigma)) * path)
    rel = np.abs(fog - want)[lit].max(1) / want[lit].max(1)
    assert (rel <= ref.K_TRANS + 2.0 ** -18).all(), rel.max()      # 2^-18: t1 - t0 of a slab 0.4 thick at t ~ 1 (3 ulp of t), and the sums over 16 samples
    assert np.array_equal(fog[~lit], clear[~lit])


def test_cli_fog_scene_box(gpu):
    """ptc_render --fog scene:sigma_t[:albedo[:g]] takes the committed scene's bounding box (its faces moved out a little) and prints it; the frame is, bit for bit, the
    one --fog renders with that box given as corners, and not the fog-free frame.  The test is about the command line, so it starts it."""
    import json
    import subprocess
    import tempfile

    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    base = [exe, "--scene", "cornell", "--width", "48", "--height", "48", "--spp", "4", "--seed", "6", "--bounces", "4"]

    def pfm(path):
        return np.frombuffer(open(path, "rb").read().split(b"-1.0\n", 1)[1], "<f4")

    with tempfile.TemporaryDirectory() as td:
        a, b, c = (os.path.join(td, n) for n in ("a.pfm", "b.pfm", "c.pfm"))
        r = subprocess.run(base + ["--out", a, "--fog", "scene:0.5:0.8:0.3"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        box = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"fog_box"')]
        assert len(box) == 1 and box[0]["sigma_t"] == 0.5
        lo, hi = np.asarray(box[0]["fog_box"][0]), np.asarray(box[0]["fog_box"][1])
        assert (lo < -1.0).all() and (lo > -1.01).all() and (hi > 1.0).all() and (hi < 1.01).all()      # the Cornell box is [-1, 1]^3
        spec = ",".join(repr(float(v)) for v in lo) + ":" + ",".join(repr(float(v)) for v in hi) + ":0.5:0.8:0.3"
        r = subprocess.run(base + ["--out", b, "--fog", spec], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        r = subprocess.run(base + ["--out", c], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(pfm(a).view(np.uint32), pfm(b).view(np.uint32)) and not np.array_equal(pfm(a), pfm(c)) and np.isfinite(pfm(a)).all()
        for bad in ("scene:", "scene", "1,2,3:4,5,6"):
            r = subprocess.run(base + ["--out", c, "--fog", bad], capture_output=True, text=True, timeout=120)
            assert r.returncode != 0 and "--fog" in (r.stderr + r.stdout), bad
        r = subprocess.run(base + ["--out", c, "--raster", "--fog", "scene:0.5"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "path integrator" in (r.stderr + r.stdout)
