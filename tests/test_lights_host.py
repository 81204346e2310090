"""Punctual lights without a GPU (include/ptc.h: ptc_add_light ... ptc_clear_lights, ptc_debug_light_sample, ptc_debug_get_light_table): symbols and defaults,
the validation table and the lights' lifetime, the host evaluation of csrc/pt_lights.h and the uploaded table against their numpy restatement
(tests/lights_reference.py) bit for bit, the physics of the specification in float64 against closed forms, and the glTF loader's KHR_lights_punctual."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lights_reference as ref  # noqa: E402

NEW = ("ptc_light_default_params", "ptc_add_light", "ptc_update_light", "ptc_get_light", "ptc_light_count", "ptc_clear_lights",
       "ptc_debug_light_sample", "ptc_debug_get_light_table", "ptc_debug_punctual_nee")
E_ARG, E_STATE, E_DEVICE = -1, -2, -3
F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24          # unit roundoff of binary32


def _ctx(pbr):
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    assert pbr.load_library().ptc_scene_begin(pt._h) == 0
    return pt


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _random_lights(rng, n, kind=None):
    out = []
    for i in range(n):
        t = kind or ("point", "spot", "directional")[i % 3]
        ci = float(rng.uniform(-0.5, 1.0))
        out.append(dict(type=t, position=rng.uniform(-3, 3, 3), direction=rng.normal(size=3) * rng.uniform(0.1, 5.0), intensity=rng.uniform(0, 40, 3),
                        range=float(rng.choice([0.0, rng.uniform(0.5, 6.0)])), cos_inner=ci, cos_outer=float(rng.uniform(-1.0, ci - 1e-3)),
                        sampling_weight=float(rng.uniform(0.05, 9.0))))
    return out


def test_symbols_abi_and_defaults(pbr):
    header = open(os.path.join(ROOT, "include", "ptc.h")).read()
    L = pbr.load_library()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in pbr.ptc.ABI_SYMBOLS and hasattr(L, sym) and getattr(L, sym).argtypes is not None, sym
    assert re.search(r"typedef struct ptc_light_params \{", header)
    assert "#define PTC_ABI_VERSION 4" in header and L.ptc_abi_version() == 4            # additive: the ABI version stays
    assert C.sizeof(pbr.ptc.PtcLightParams) == 56
    d = pbr.ptc.light_default_params()
    assert d["type"] == pbr.ptc.LIGHT_POINT and d["position"] == (0, 0, 0) and d["direction"] == (0, 0, -1) and d["intensity"] == (1, 1, 1)
    assert d["range"] == 0 and d["cos_inner"] == 1 and d["cos_outer"] == float(F32(0.70710678)) and d["sampling_weight"] == 1
    L.ptc_light_default_params(None)                                                       # a NULL pointer is ignored
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    assert pt.light_count() == 0
    for m in ("add_light", "update_light", "get_light", "light_count", "clear_lights", "light_table", "punctual_nee"):
        assert callable(getattr(pbr.PathTracer, m)), m
    assert pbr.scene.SceneDesc([], [], [], None).lights == []                              # a description has no lights by default
    assert pbr.scene.LightDesc().type == "point"
    assert L.ptc_add_light(None, None) == E_ARG and L.ptc_light_count(None) == E_ARG and L.ptc_clear_lights(None) == E_ARG
    assert pt.light_table()[0].shape == (0, 16)
    z = np.zeros((1, 3), F32)
    with pytest.raises(pbr.PtcError):
        pt.punctual_nee(z, z + 1, np.zeros(1, np.uint32))                                  # the kernel needs the device


def test_validation_leaves_the_lights_unchanged(pbr):
    pt = _ctx(pbr)
    L = pbr.load_library()
    good = [dict(type="point", position=(1, 2, 3), intensity=(4, 5, 6), range=2.5, sampling_weight=2.0),
            dict(type="spot", position=(0, 1, 0), direction=(0, -2, 0), intensity=(1, 0, 0), cos_inner=0.9, cos_outer=0.5),
            dict(type="directional", direction=(3, -4, 0), intensity=(0, 0, 0))]
    assert [pt.add_light(g) for g in good] == [0, 1, 2]
    before = [pt.get_light(i) for i in range(3)]
    tab_before = pt.light_table()
    nan, inf = float("nan"), float("inf")
    bad = [dict(type=3), dict(type=-1),
           dict(position=(nan, 0, 0)), dict(intensity=(0, inf, 0)), dict(type="spot", direction=(0, nan, 1)), dict(range=inf), dict(type="spot", cos_inner=nan),
           dict(intensity=(1, -1e-3, 1)), dict(range=-1.0),
           dict(type="spot", direction=(0, 0, 0)), dict(type="directional", direction=(0, 0, 0)),
           dict(type="spot", cos_inner=0.5, cos_outer=0.5), dict(type="spot", cos_inner=0.4, cos_outer=0.6), dict(type="spot", cos_inner=1.5, cos_outer=0.5),
           dict(type="spot", cos_inner=0.5, cos_outer=-1.5),
           dict(sampling_weight=0.0), dict(sampling_weight=-1.0), dict(sampling_weight=inf), dict(sampling_weight=nan)]
    for b in bad:
        p = pbr.ptc.light_params(**b)
        assert L.ptc_add_light(pt._h, C.byref(p)) == E_ARG, b
        assert L.ptc_update_light(pt._h, 1, C.byref(p)) == E_ARG, b
        assert L.ptc_debug_light_sample(C.byref(p), (C.c_float * 3)(), (C.c_float * 3)(), C.byref(C.c_float()), (C.c_float * 3)()) == E_ARG, b
    ok = pbr.ptc.light_params()
    assert L.ptc_update_light(pt._h, 3, C.byref(ok)) == E_ARG and L.ptc_update_light(pt._h, -1, C.byref(ok)) == E_ARG
    assert L.ptc_get_light(pt._h, 3, C.byref(ok)) == E_ARG and L.ptc_add_light(pt._h, None) == E_ARG
    assert pt.light_count() == 3 and [pt.get_light(i) for i in range(3)] == before
    assert all(_same_bits(a, b) for a, b in zip(pt.light_table(), tab_before))
    # a point light needs no direction: a zero one is accepted and kept
    assert pt.add_light(type="point", direction=(0, 0, 0)) == 3 and pt.get_light(3)["direction"] == (0, 0, 0)
    # the 257th light
    for i in range(4, pbr.ptc.MAX_LIGHTS):
        assert pt.add_light(ok) == i
    assert L.ptc_add_light(pt._h, C.byref(ok)) == E_ARG and pt.light_count() == 256 and "PTC_MAX_LIGHTS" in L.ptc_last_error(pt._h).decode()
    assert [pt.get_light(i) for i in range(3)] == before


def test_get_returns_what_was_set_and_lifetimes(pbr):
    pt = _ctx(pbr)
    L = pbr.load_library()
    spot = dict(type="spot", position=(1, 2, 3), direction=(3, -4, 12), intensity=(7, 8, 9), range=5.0, cos_inner=0.75, cos_outer=0.25, sampling_weight=3.0)
    i = pt.add_light(spot)
    g = pt.get_light(i)
    d = np.array((3, -4, 12), F32)
    want = d * (F32(1.0) / np.sqrt(ref.dot3(d, d)))                       # normalize3's expression
    assert _same_bits(g["direction"], want)
    assert (g["type"], g["position"], g["intensity"], g["range"], g["cos_inner"], g["cos_outer"], g["sampling_weight"]) == (1, (1, 2, 3), (7, 8, 9), 5.0, 0.75, 0.25, 3.0)
    pt.update_light(i, type="directional", direction=(0, -2, 0), intensity=(1, 1, 1))
    assert pt.get_light(i)["type"] == 2 and pt.get_light(i)["direction"] == (0, -1, 0) and pt.light_count() == 1
    pt.clear_lights()
    assert pt.light_count() == 0 and L.ptc_get_light(pt._h, 0, C.byref(pbr.ptc.light_params())) == E_ARG
    pt.add_light(spot)
    pt.add_light(spot)
    assert L.ptc_scene_begin(pt._h) == 0 and pt.light_count() == 0        # ptc_scene_begin drops all lights
    # a description's lights arrive with load_scene, and lights need no commit: they can be added and changed behind one
    desc = pbr.scenes.cornell_box()
    desc.lights = [pbr.scene.LightDesc("point", position=(0, 1, 0), intensity=(2, 2, 2)), pbr.scene.LightDesc("directional", direction=(0, -1, 0))]
    pt.load_scene(desc)
    assert pt.light_count() == 2 and pt.get_light(0)["intensity"] == (2, 2, 2) and pt.get_light(1)["type"] == 2
    assert pt.add_light(spot) == 2
    pt.load_scene(pbr.scenes.cornell_box())
    assert pt.light_count() == 0


@pytest.mark.parametrize("kind", ["point", "spot", "directional"])
def test_host_sample_equals_the_restatement_bit_for_bit(pbr, kind):
    rng = np.random.default_rng({"point": 11, "spot": 12, "directional": 13}[kind])
    n_checked = 0
    for l in _random_lights(rng, 40, kind):
        P = rng.uniform(-4, 4, (8, 3)).astype(F32)
        rec = ref.light_record(l)
        if kind == "spot":      # points on the cone's edges and around them: along directions at exactly the inner / outer angle from the axis
            ax = rec[4:7].astype(F64)
            perp = np.cross(ax, (0.3, 0.5, 0.8))
            perp /= np.linalg.norm(perp)
            for c in (rec[14], rec[15], 0.5 * (rec[14] + rec[15])):
                dvec = float(c) * ax + math.sqrt(max(0.0, 1 - float(c) ** 2)) * perp
                P = np.vstack([P, (rec[0:3] + 1.7 * dvec).astype(F32)])
        if kind != "directional":
            P = np.vstack([P, rec[0:3]])                                    # a point on the light: no sample
            if rec[7] > 0:                                                  # on the range, just inside, beyond
                P = np.vstack([P, rec[0:3] + np.array((rec[7], 0, 0), F32), rec[0:3] + np.array((0, rec[7] * F32(0.99), 0), F32), rec[0:3] + np.array((0, 0, rec[7] * F32(1.5)), F32)])
        ok, wi, dist, Li = pbr.ptc.light_sample(l, P)
        rok, rwi, rdist, rLi = ref.light_sample(rec, P)
        assert np.array_equal(ok, rok) and _same_bits(wi, rwi) and _same_bits(dist, rdist) and _same_bits(Li, rLi), l
        if kind != "directional":
            assert not ok[np.all(P == rec[0:3], 1)].any()
            if rec[7] > 0:
                assert (Li[-1] == 0).all()                                  # beyond the range
        else:
            assert ok.all() and (dist == F32(3.0e38)).all() and _same_bits(wi, np.tile(-rec[4:7], (len(P), 1))) and _same_bits(Li, np.tile(rec[8:11], (len(P), 1)))
        n_checked += len(P)
    assert n_checked >= 300


@pytest.mark.parametrize("n", [1, 2, 256])
def test_light_table_equals_the_restatement_bit_for_bit(pbr, n):
    rng = np.random.default_rng(100 + n)
    lights = _random_lights(rng, n)
    pt = _ctx(pbr)
    for l in lights:
        pt.add_light(l)
    rec, cdf = pt.light_table()
    rrec, rcdf = ref.light_table(lights)
    assert rec.shape == (n, 16) and np.array_equal(_bits(rec), _bits(rrec)) and _same_bits(cdf, rcdf)
    assert cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all() and (n == 1 or len(set(rec[:, 11])) > 1)      # unequal weights: unequal pmfs
    assert abs(float(rec[:, 11].astype(F64).sum()) - 1.0) <= n * EPS * 4
    # the choice of the light follows the table
    keys = rng.integers(0, 2 ** 32, 4096, dtype=np.uint64)
    li = ref.choose_light(cdf, keys, 2)
    assert np.array_equal(li, np.minimum(np.searchsorted(cdf, ref.rng_f(keys, ref.RNG_BASE + 3, 0), side="right"), n - 1))


def test_physics_against_closed_forms(pbr):
    """The specification in float64.  Bound: a sample is dv (3 subtractions), dot3 (3 roundings), sqrt, 1 / dist, wi (1 product each), 1 / dist2, I * att, and for the window /
    the cone at most 8 more (range * range, q, q * q, 1 - ., att * w; cd's 3, the fma, s * s, att * .): below 24 roundings of relative size 2^-24 each, plus the
    cancellation in dv of points up to 8 units from the light at coordinates up to 8 (amplification <= 16 for distances >= 1) — 64 * 2^-24 relative holds all of it."""
    tol = 64 * EPS
    rng = np.random.default_rng(5)
    rho = np.array((0.8, 0.5, 0.3))
    n_pl = np.array((0.0, 1.0, 0.0))                              # a Lambert plane y = 0 facing +y
    P = np.column_stack([rng.uniform(-3, 3, 200), np.zeros(200), rng.uniform(-3, 3, 200)]).astype(F32)
    # point light: rho / pi * I cos(theta) / d^2
    I = np.array((10.0, 20.0, 5.0))
    pos = np.array((0.5, 2.0, -0.25))
    ok, wi, dist, Li = pbr.ptc.light_sample(dict(type="point", position=pos, intensity=I), P)
    dv = pos - P.astype(F64)
    d2 = (dv ** 2).sum(1)
    want = rho / math.pi * I * (dv @ n_pl / np.sqrt(d2) / d2)[:, None]
    got = rho / math.pi * Li.astype(F64) * (wi.astype(F64) @ n_pl)[:, None]
    assert ok.all() and np.allclose(got, want, rtol=tol, atol=0) and np.allclose(dist, np.sqrt(d2), rtol=tol, atol=0)
    # directional: rho / pi * E cos(theta)
    E = np.array((3.0, 2.0, 1.0))
    dr = np.array((1.0, -2.0, 0.5))
    ok, wi, dist, Li = pbr.ptc.light_sample(dict(type="directional", direction=dr, intensity=E), P)
    want = rho / math.pi * E * (-dr @ n_pl / np.linalg.norm(dr))
    got = rho / math.pi * Li.astype(F64) * (wi.astype(F64) @ n_pl)[:, None]
    assert ok.all() and np.allclose(got, np.tile(want, (200, 1)), rtol=tol, atol=0)
    # spot: 0 outside the outer cone, the point value inside the inner cone, the squared ramp between
    ci, co = math.cos(math.radians(20)), math.cos(math.radians(35))
    spot = dict(type="spot", position=pos, direction=(0, -1, 0), intensity=I, cos_inner=ci, cos_outer=co)
    ok, wi, dist, Li = pbr.ptc.light_sample(spot, P)
    cd = dv[:, 1] / np.sqrt(d2)                                   # cos of the angle to the axis (0, -1, 0), seen from the light: -wi . axis
    point_val = I * (1 / d2)[:, None]
    s = np.clip((cd - float(F32(co))) / (float(F32(ci)) - float(F32(co))), 0, 1)
    margin = 1e-5                                                 # away from the two cosines by more than the float32 error of cd
    outside, inside, ramp = cd < co - margin, cd > ci + margin, (cd > co + margin) & (cd < ci - margin)
    assert outside.sum() > 10 and inside.sum() > 10 and ramp.sum() > 10
    assert (Li[outside] == 0).all()
    assert np.allclose(Li[inside], point_val[inside], rtol=tol, atol=0)
    # on the ramp s itself carries the absolute error of cd (a few 2^-24) over (ci - co): relative 2^-24 * 8 / ((ci - co) * s) in s, twice that in s^2
    ramp_tol = tol + 2 * 8 * EPS / ((ci - co) * s[ramp])
    assert (np.abs(Li[ramp].astype(F64) - point_val[ramp] * (s[ramp] ** 2)[:, None]) <= ramp_tol[:, None] * point_val[ramp] * (s[ramp] ** 2)[:, None]).all()
    # the range window: clamp(1 - (d / r)^4, 0, 1); it reaches 0 at the range
    r = 2.75
    ok, wi, dist, Li = pbr.ptc.light_sample(dict(type="point", position=pos, intensity=I, range=r), P)
    w = np.clip(1 - (d2 / float(F32(r)) ** 2) ** 2, 0, 1)
    near = w > 1e-3                                               # 1 - q^2 cancels near the range: absolute error 4 * 2^-24 there
    assert near.sum() > 20 and (w == 0).sum() > 20
    assert np.allclose(Li[near], (point_val * w[:, None])[near], rtol=tol + 8 * EPS / 1e-3, atol=0)
    assert (Li[w == 0] == 0).all()


def test_gltf_lights_load_and_pose(pbr, tmp_path):
    """A write_glb asset with one light of each type under rotated, nested nodes loads on a description-only context into the expected ptc_get_light values;
    ptc_gltf_asset_pose moves them with their nodes."""
    from pbr_amd import gltf

    def quat(axis, deg):
        a = np.asarray(axis, F64) / np.linalg.norm(axis)
        return (math.cos(math.radians(deg) / 2), *(math.sin(math.radians(deg) / 2) * a))      # w, x, y, z

    def rot(q):
        w, x, y, z = q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])

    desc = pbr.scenes.cornell_box()
    q0, q1 = quat((1, 2, 0.5), 40), quat((0, 1, 1), -75)
    t0, t1 = np.array((0.5, 1.0, -2.0)), np.array((0.25, -0.5, 1.5))
    lights = [dict(type="point", color=(1.0, 0.5, 0.25), intensity=8.0, range=4.0, translation=t0, rotation=q0),
              dict(type="spot", color=(0.5, 1.0, 0.5), intensity=3.0, inner=0.3, outer=0.6, translation=t1, rotation=q1, parent=0),
              dict(type="directional", color=(1.0, 1.0, 0.5), intensity=2.0, rotation=q1, parent=1)]
    n0 = len(desc.instances)                                                                  # the first light's node: behind the instances' nodes
    moved = np.array((2.0, -1.0, 0.5))
    anim = [{"channels": [{"node": n0, "path": "translation", "times": [0.0, 1.0], "values": [t0, moved]}]}]
    path = str(tmp_path / "lights.glb")
    gltf.write_glb(desc, path, lights=lights, animations=anim)
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    asset = gltf.Asset(path)
    asset.load_into(pt, desc.camera)
    assert pt.light_count() == 3
    R0, R1 = rot(q0), rot(q1)
    # world positions and axes to the rounding of the matrix products: up to three 4x4 float32 products with entries up to 4 in size, 4 terms per entry, each
    # term and each sum rounded: 3 products x 8 roundings x 2^-24 x 4
    tol = 3 * 8 * EPS * 4

    def check(t_root):
        g = [pt.get_light(i) for i in range(3)]
        assert [x["type"] for x in g] == [0, 1, 2]
        p1 = R0 @ t1 + t_root
        assert np.allclose(g[0]["position"], t_root, atol=tol, rtol=0) and np.allclose(g[1]["position"], p1, atol=tol, rtol=0)
        assert np.allclose(g[1]["direction"], R0 @ R1 @ (0, 0, -1), atol=tol, rtol=0) and np.allclose(g[2]["direction"], R0 @ R1 @ R1 @ (0, 0, -1), atol=tol, rtol=0)
        assert np.allclose(g[0]["intensity"], (8.0, 4.0, 2.0), rtol=2 * EPS) and g[0]["range"] == 4.0 and g[1]["range"] == 0.0
        assert np.allclose(g[1]["intensity"], (1.5, 3.0, 1.5), rtol=2 * EPS) and np.allclose(g[2]["intensity"], (2.0, 2.0, 1.0), rtol=2 * EPS)
        assert abs(g[1]["cos_inner"] - math.cos(0.3)) <= EPS and abs(g[1]["cos_outer"] - math.cos(0.6)) <= EPS

    check(t0)
    asset.pose(pt, 0, 1.0)                                                                    # the root light's node moves: its children follow
    check(moved)
    asset.pose(pt, 0, 0.5)
    check(0.5 * (t0 + moved))
    # the stateless loader adds the same lights
    pt2 = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    gltf.load_into(pt2, path, desc.camera)
    assert [pt2.get_light(i) for i in range(3)] == [dict(pt.get_light(i), position=pt2.get_light(i)["position"]) for i in range(3)]
    assert np.allclose(pt2.get_light(1)["position"], R0 @ t1 + t0, atol=tol, rtol=0)
    asset.close()
