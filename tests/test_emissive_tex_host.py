"""Textured emission without a GPU (include/ptc_emissive_tex.h, csrc/pt_emissive_tex.h), on description-only contexts.

1. The binding's table and struct mirrors against include/ptc_emissive_tex.h.
2. The argument and state rules: every refusal, both directions with alpha and transmission, after the commit, ptc_scene_begin drops it.
3. Table, cdf and primitive map against the numpy restatement (tests/emissive_tex_reference.py), bit for bit: one triangle, a quad under a 2 x 1 black | white
   texture, 65 triangles over a 5 x 3 texture with uv from -0.7 to 1.9, an all-zero texture (the sample side is off), a degenerate triangle (weight 0, never drawn);
   again after a non-uniform scale + ptc_scene_refit with both builders, where it equals a fresh commit of the same transforms.  ptc_scene_rebuild needs a device, so
   the same check after a rebuild, with both builders, is tests/test_gpu_emissive_tex.py::test_refit_and_rebuild_equal_a_fresh_commit.
4. ptc_debug_emissive_tex_sample against the restatement, bit for bit, NEAREST and LINEAR.
5. Closed form: the irradiance at a floor point under the half-black quad from 65,536 host samples of the definition against a float64 quadrature.
6. glTF emissiveTexture through the writer and the loader, and the loader's switch back to the uniform factor."""
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emissive_tex_reference as ref  # noqa: E402
from lens_reference import rng_f  # noqa: E402

F32, F64 = np.float32, np.float64
E_ARG, E_STATE = -1, -2
I16 = np.eye(4, dtype=F32).reshape(16)
BW = np.array([[[0, 0, 0, 255], [255, 255, 255, 255]]], np.uint8)                  # 2 x 1: black | white


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def trs_matrix(t=(0, 0, 0), angle_y=0.0, s=(1, 1, 1)):
    """Column-major 4x4 of translate(t) rotate_y(angle) scale(s), float32."""
    c, sn = math.cos(angle_y), math.sin(angle_y)
    R = np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]], F64)
    M = np.eye(4)
    M[:3, :3] = R @ np.diag(s)
    M[:3, 3] = t
    return M.T.reshape(16).astype(F32)


def emitter_scene(pbr, tex=BW, factor=(1.0, 1.0, 1.0), linear=False, emitter=None, matrix=I16, builder=None, floor_material=None):
    """A floor at y = 0 (primitives 0, 1) and an emitter mesh of material 1, which has the emission texture 0; the default emitter is the quad [-1, 1]^2 at y = 2
    facing down with u along x: under BW its x > 0 half is lit."""
    S, Q = pbr.scene, pbr.scenes._quad
    mats = [floor_material or S.Material((0.8, 0.8, 0.8, 1.0), 0.0, 1.0), S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, emissive_texture=0, emissive_texture_factor=tuple(factor))]
    fv, fi = Q((-12, 0, 12), (12, 0, 12), (12, 0, -12), (-12, 0, -12))
    ev, ei = emitter if emitter is not None else Q((-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1))
    cam = S.CameraDesc((0.0, 1.0, 4.0), (0.0, 0.8, 0.0), math.radians(45.0), 1.5)
    d = S.SceneDesc(mats, [S.MeshDesc(fv, fi, 0), S.MeshDesc(ev, ei, 1)], [S.InstanceDesc(0, matrix=I16), S.InstanceDesc(1, matrix=matrix)], cam, "emissive_tex",
                    textures=[np.ascontiguousarray(tex, np.uint8)])
    d.texture_filter = "linear" if linear else "nearest"
    d.bvh_builder = builder
    return d


def strip_mesh(pbr, n_tris, uv_lo=-0.7, uv_hi=1.9, seed=3):
    """n_tris triangles in a fan-free strip at y = 2 facing down, texture coordinates spread over [uv_lo, uv_hi]^2."""
    rng = np.random.default_rng(seed)
    pos, uv, idx = [], [], []
    for k in range(n_tris):
        x0 = -2.0 + 4.0 * k / n_tris
        w = 4.0 / n_tris
        pos += [(x0, 2.0, -0.5), (x0 + w, 2.0, -0.5), (x0 + 0.5 * w, 2.0, 0.5)]
        uv += [tuple(rng.uniform(uv_lo, uv_hi, 2)) for _ in range(3)]
        idx += [3 * k, 3 * k + 1, 3 * k + 2]
    v = pbr.scenes._verts(pos, [(0, -1, 0)] * len(pos), [(1, 0, 0)] * len(pos), uv)
    return v, np.array(idx, np.uint32)


def tex_5x3(seed=11):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    t[1, 2, :3] = 0                                                               # one black texel
    return t


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_structs(pbr):
    import c_header
    m = pbr.ptc
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(ROOT, "include", "ptc_emissive_tex.h")
    macros = dict(re.findall(r"^#define (ptc_\w+) (ptcx_\w+)$", open(path).read(), flags=re.M))
    h = c_header.Header(path, "ptc_")
    table = m._EMISSIVE_TEX_PROTOTYPES
    assert list(h.prototypes) == list(table) == list(macros) and len(table) == 6
    assert all(macros[n] == "ptcx_" + n[4:] for n in macros)
    assert c_header.check_prototypes(h, table) == []
    assert list(h.structs) == ["ptc_emissive_tex_stats", "ptc_emissive_tex_sample"]
    assert c_header.check_struct(h.structs["ptc_emissive_tex_stats"], m.PtcEmissiveTexStats) == []
    assert c_header.check_struct(h.structs["ptc_emissive_tex_sample"], m.PtcEmissiveTexSample) == []
    L = m.load_library()
    for name, (restype, argtypes) in table.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert hasattr(L, "ptcx_" + name[4:])
    assert L.ptc_abi_version() == 4 and not set(table) & set(m.ABI_SYMBOLS)
    assert '#include "ptc_emissive_tex.h"' in open(os.path.join(ROOT, "include", "ptc.h")).read()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _describe(pbr, pt, desc, commit=False):
    """The description of `desc` without its emission textures, uncommitted (commit: committed)."""
    L, h = pt._L, pt._h
    assert L.ptc_scene_begin(h) == 0
    for t in desc.textures:
        assert L.ptc_add_texture_rgba8(h, pbr.ptc._ptr(t), t.shape[1], t.shape[0]) >= 0
    for mm in desc.materials:
        assert L.ptc_add_material(h, pbr.ptc._f(mm.base_color)[1], mm.metallic, mm.roughness, pbr.ptc._f(mm.emissive)[1], mm.tex_color, mm.tex_normal, mm.tex_mr) >= 0
    for me in desc.meshes:
        v, i = np.ascontiguousarray(me.vertices), np.ascontiguousarray(me.indices, np.uint32)
        assert L.ptc_add_mesh(h, v.ctypes.data, v.size, pbr.ptc._ptr(i), i.size, me.material) >= 0
    for it in desc.instances:
        assert L.ptc_add_instance_matrix(h, it.mesh, pbr.ptc._f(np.asarray(it.matrix, F32))[1]) >= 0
    c = desc.camera
    assert L.ptc_set_camera(h, pbr.ptc._f(c.position)[1], pbr.ptc._f(c.target)[1], c.fov_y, c.aspect) == 0
    if commit:
        assert L.ptc_scene_commit(h) == 0


def test_argument_and_state_rules(pbr):
    import ctypes as C
    m, S = pbr.ptc, pbr.scene
    desc = emitter_scene(pbr)
    desc.materials += [S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, (2.0, 0.0, 0.0)), S.Material((0.5, 0.5, 0.5, 0.5), 0.0, 1.0), S.Material((0.5, 0.5, 0.5, 1.0), 0.0, 0.2)]
    pt = pbr.PathTracer(m.DEVICE_NONE)
    L, h = pt._L, pt._h
    _describe(pbr, pt, desc)                                                       # materials: 0 floor, 1 the emitter's, 2 emissive, 3 to become BLEND, 4 to become glass
    f3 = lambda *v: (C.c_float * 3)(*v)
    none = (-1, (0.0, 0.0, 0.0))
    state = lambda: [(t, tuple(float(x) for x in f)) for t, f in (pt.get_material_emission_texture(k) for k in range(5))]
    assert state() == [none] * 5
    pt.set_material_emission_texture(1, 0, (2.0, 0.5, 0.0))
    want = [none, (0, (2.0, 0.5, 0.0)), none, none, none]
    assert state() == want
    nan, inf = float("nan"), float("inf")
    for bad in ((nan, 1, 1), (1, inf, 1), (1, 1, -0.5), (-inf, 1, 1)):
        assert L.ptc_set_material_emission_texture(h, 1, 0, f3(*bad)) == E_ARG and b"factor" in L.ptc_last_error(h), bad
    assert L.ptc_set_material_emission_texture(h, 1, 1, f3(1, 1, 1)) == E_ARG and b"texture id" in L.ptc_last_error(h)      # one texture: id 1 is out of range
    assert L.ptc_set_material_emission_texture(h, 5, 0, f3(1, 1, 1)) == E_ARG and L.ptc_set_material_emission_texture(h, -1, 0, f3(1, 1, 1)) == E_ARG
    assert L.ptc_set_material_emission_texture(h, 1, 0, None) == E_ARG
    assert L.ptc_set_material_emission_texture(h, 2, 0, f3(1, 1, 1)) == E_ARG and b"emissive factor" in L.ptc_last_error(h)
    assert L.ptc_get_material_emission_texture(h, 5, None, None) == E_ARG
    assert state() == want
    # an emitter stays opaque: both directions with alpha and with transmission
    pt.set_material_alpha(3, "blend")
    assert L.ptc_set_material_emission_texture(h, 3, 0, f3(1, 1, 1)) == E_ARG and b"OPAQUE" in L.ptc_last_error(h)
    pt.set_material_transmission(4, transmission=0.5)
    assert L.ptc_set_material_emission_texture(h, 4, 0, f3(1, 1, 1)) == E_ARG and b"transmissive" in L.ptc_last_error(h)
    assert L.ptc_set_material_alpha(h, 1, m.ALPHA_BLEND, 0.5) == E_ARG and b"emission texture" in L.ptc_last_error(h)
    assert L.ptc_set_material_alpha(h, 1, m.ALPHA_MASK, 0.5) == E_ARG
    assert L.ptc_set_material_transmission(h, 1, C.byref(m.transmission_params(transmission=0.5))) == E_ARG and b"emission texture" in L.ptc_last_error(h)
    assert state() == want and pt.get_material_alpha(1)[0] == m.ALPHA_OPAQUE and pt.get_material_transmission(1)["transmission"] == 0.0
    pt.set_material_alpha(1, "opaque")
    pt.set_material_transmission(1, transmission=0.0)                              # what changes nothing is accepted
    # removal: the material may then take an alpha mode; a zero factor is allowed
    pt.set_material_emission_texture(1, -1)
    assert state() == [none] * 5
    pt.set_material_alpha(1, "mask", 0.5).set_material_alpha(1, "opaque")
    pt.set_material_emission_texture(1, 0, (0.0, 0.0, 0.0)).set_material_emission_texture(1, 0, (2.0, 0.5, 0.0))
    # once committed the description is fixed
    assert L.ptc_scene_commit(h) == 0
    assert L.ptc_set_material_emission_texture(h, 1, 0, f3(1, 1, 1)) == E_STATE and L.ptc_set_material_emission_texture(h, 1, -1, None) == E_STATE
    assert state() == want and pt.emissive_tex_stats()["entries"] == 2
    # ptc_scene_begin drops it
    _describe(pbr, pt, desc, commit=True)
    assert state() == [none] * 5
    recs, cdf, pm, total = pt.emissive_tex_table()
    assert recs.shape == (0, 28) and cdf.size == 0 and pm.size == 0 and total == 0.0 and pt.emissive_tex_stats()["entries"] == 0
    pt.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _cases(pbr):
    one = pbr.scenes._verts([(-1, 2, -1), (1, 2, -1), (0, 2, 1)], [(0, -1, 0)] * 3, [(1, 0, 0)] * 3, [(0.1, 0.2), (0.9, 0.3), (0.4, 0.8)]), np.array([0, 1, 2], np.uint32)
    dv, di = pbr.scenes._quad((-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1))
    dv = np.concatenate([dv, dv[:1]])                                               # a third triangle (a, a, b): degenerate
    di = np.concatenate([di, np.array([0, 4, 1], np.uint32)])
    return {"one": dict(emitter=one, tex=tex_5x3(), factor=(1.5, 1.0, 0.25)),
            "quad_bw": dict(),
            "strip65": dict(emitter=strip_mesh(pbr, 65), tex=tex_5x3(), factor=(0.5, 2.0, 1.0)),
            "zero": dict(tex=np.zeros((2, 2, 4), np.uint8)),
            "degenerate": dict(emitter=(dv, di))}


def _check_table(pt, desc, matrices=None):
    recs, cdf, pm, total = pt.emissive_tex_table()
    rr, rc, rp, rt = ref.table(desc, matrices)
    assert np.array_equal(pm, rp)
    assert _bits_equal(recs, rr), np.flatnonzero((recs.view(np.uint32) != rr.view(np.uint32)).any(1))
    assert _bits_equal(cdf, rc) and F32(total) == F32(rt)
    assert pt.emissive_tex_stats()["entries"] == len(recs)
    return recs, cdf, pm, total


@pytest.mark.parametrize("case", ["one", "quad_bw", "strip65", "zero", "degenerate"])
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_table_equals_the_restatement_bit_for_bit(pbr, case, builder):
    desc = emitter_scene(pbr, builder=builder, **_cases(pbr)[case])
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)
    recs, cdf, pm, total = _check_table(pt, desc)
    n = {"one": 1, "quad_bw": 2, "strip65": 65, "zero": 2, "degenerate": 3}[case]
    assert len(recs) == n and np.array_equal(pm, np.concatenate([[-1, -1], np.arange(n)]))
    if case == "zero":
        assert total == 0.0 and not cdf.any() and not recs[:, 7].any()            # the pass is off
    else:
        assert total > 0 and cdf[-1] == 1.0 and (np.diff(cdf) >= 0).all() and abs(float(recs[:, 7].astype(F64).sum()) - 1.0) < 1e-5
    if case == "quad_bw":                                                          # triangle (a, b, c) holds more of the lit half than (a, c, d): 12 of its 16 cells against 4
        assert abs(float(recs[0, 7]) - 0.75) < 1e-6 and abs(float(recs[1, 7]) - 0.25) < 1e-6
    if case == "degenerate":                                                       # weight 0: no area, a zero normal, never drawn — the cdf is 1 from the entry before it on
        assert recs[2, 3] == 0 and recs[2, 7] == 0 and not recs[2, 12:15].any() and cdf[1] == 1.0 and cdf[2] == 1.0
        from lights_reference import cdf_search
        assert (cdf_search(cdf, rng_f(np.arange(4096, dtype=np.uint32), 5, 0)) < 2).all()
    # a non-uniform scale and a turn, then a refit: the table of a fresh commit of the same transforms
    M2 = trs_matrix((0.3, 0.5, -0.2), 0.7, (2.0, 1.0, 0.5))
    pt.update_instance(1, matrix=M2).scene_refit()
    moved = _check_table(pt, desc, [I16, M2])
    desc2 = emitter_scene(pbr, builder=builder, matrix=M2, **_cases(pbr)[case])
    fresh = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc2)
    got = fresh.emissive_tex_table()
    assert _bits_equal(moved[0], got[0]) and _bits_equal(moved[1], got[1]) and np.array_equal(moved[2], got[2]) and moved[3] == got[3]
    if case != "zero":
        assert not _bits_equal(moved[0][:, 0:3], recs[:, 0:3])                     # it did move
    fresh.close()
    pt.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("linear", [False, True])
def test_sample_equals_the_restatement_bit_for_bit(pbr, linear):
    tex = tex_5x3()
    desc = emitter_scene(pbr, tex=tex, factor=(0.5, 2.0, 1.0), emitter=strip_mesh(pbr, 9), linear=linear)
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)
    recs, cdf, _, _ = pt.emissive_tex_table()
    pt.close()
    rng = np.random.default_rng(21)
    n = 600
    P = rng.uniform((-3, 0, -2), (3, 3.5, 2), (n, 3)).astype(F32)                   # some points lie above the emitter: they see its back
    r1, r2 = rng.random(n).astype(F32), rng.random(n).astype(F32)
    hu = rng.random(n).astype(F32)
    hv = (rng.random(n).astype(F32) * (F32(1.0) - hu)).astype(F32)
    b = rng.integers(0, 3, n)
    pb, ht, hc = rng.uniform(0.05, 30.0, n).astype(F32), rng.uniform(0.1, 6.0, n).astype(F32), rng.uniform(0.01, 1.0, n).astype(F32)
    ei = rng.integers(0, len(recs), n)
    seen_ok = seen_back = 0
    for i in range(n):
        E = recs[ei[i]]
        got = pbr.ptc.emissive_tex_sample(E, tex, linear, P=P[i], r1=r1[i], r2=r2[i], hit_u=hu[i], hit_v=hv[i], bounce=int(b[i]), prev_pdf=pb[i], hit_t=ht[i], hit_cos=hc[i])
        ok, y, wi, pl, Le = ref.sample(E, [tex], linear, P[i], r1[i], r2[i])
        assert got["ok"] == int(ok[0]), i
        assert _bits_equal(got["y"], y[0]) and _bits_equal(got["wi"], wi[0]) and _bits_equal(got["pl"], pl[0]) and _bits_equal(got["Le"], Le[0]), (i, got)
        assert _bits_equal(got["hit_Le"], ref.radiance(E, [tex], linear, hu[i], hv[i])[0]), i
        assert _bits_equal(got["hit_weight"], ref.hit_weight(E, int(b[i]), pb[i], ht[i], hc[i])[0]), i
        seen_ok += int(ok[0]); seen_back += int(not ok[0])
    assert seen_ok > 200 and seen_back > 30
    assert pbr.ptc.load_library().ptc_debug_emissive_tex_sample(None, None, 1, 1, 0, None) == E_ARG


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_irradiance_under_the_half_black_quad(pbr):
    """E(x) = integral of Le cos cos / d^2 over the lit half, at a floor point off the axis.  The estimator is the definition's: an entry by the cdf, a point by
    pt_emtex_sample, Le cos_x / pl.  5 standard errors of the sample set's own spread."""
    from lights_reference import cdf_search
    factor = (3.0, 2.0, 1.0)
    desc = emitter_scene(pbr, factor=factor)
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)
    recs, cdf, _, _ = pt.emissive_tex_table()
    pt.close()
    x, nx = np.array([0.4, 0.0, -0.3], F32), np.array([0.0, 1.0, 0.0])
    n = 65536
    keys = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)
    u0, r1, r2 = (rng_f(keys, ref.RNG_BASE + 1, k) for k in range(3))
    ei = cdf_search(cdf, u0)
    est = np.zeros((n, 3))
    for i in range(n):
        s = pbr.ptc.emissive_tex_sample(recs[ei[i]], BW, False, P=x, r1=r1[i], r2=r2[i])
        if s["ok"]:
            est[i] = np.array(s["Le"], F64) * max(float(np.dot(nx, s["wi"])), 0.0) / s["pl"]
    mean, se = est.mean(0), est.std(0, ddof=1) / math.sqrt(n)
    want = np.array([ref.irradiance64((-1, 2, -1), (2, 0, 0), (0, 0, 2), (0, -1, 0), [(0.5, 1.0, 0.0, 1.0)], f, x, nx, sub=256) for f in factor])
    print("irradiance: mean", mean, "want", want, "se", se, "z", np.abs(mean - want) / se)
    assert (se > 0).all() and (se / want < 0.01).all()
    assert (np.abs(mean - want) <= 5.0 * se).all()
    assert (est > 0).any(1).mean() > 0.3 and (est == 0).all(1).mean() > 0.05        # lit samples, and samples on the black half (drawable by the 1 % floor)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_gltf_emissive_texture_round_trip(pbr, tmp_path):
    """write_glb writes emissiveTexture with the factor as emissiveFactor x KHR_materials_emissive_strength; the loader gives the material its emission texture and a
    base emission of zero, and keeps today's precedence: an emissive material stays opaque and without transmission.  With the loader's switch off (what ptc_render
    --no-emissive-textures sets) the materials are the old ones: uniform emitters of the factor."""
    from pbr_amd import gltf
    M = pbr.scene.Material
    desc = emitter_scene(pbr, tex=tex_5x3(), factor=(6.0, 3.0, 1.5))
    desc.textures.append(BW)
    desc.materials += [M((0.5, 0.5, 0.5, 0.5), 0.0, 1.0, alpha_mode="blend", transmission=0.5, emissive_texture=1, emissive_texture_factor=(0.5, 0.25, 1.0)),      # the emission wins
                       M((0.2, 0.2, 0.9, 1.0), 0.0, 1.0, (2.0, 0.0, 0.0))]                                                                     # a plain emitter
    path = str(tmp_path / "emissive_tex.glb")
    gltf.write_glb(desc, path)
    doc = open(path, "rb").read()
    assert doc.count(b'"emissiveTexture":{"index":') == 2 and b'"emissiveStrength":6.0' in doc and b'"emissiveFactor":[1.0,0.5,0.25]' in doc
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    gltf.load_into(pt, path, desc.camera)
    got = [pt.get_material_emission_texture(k) for k in range(4)]
    assert got[0][0] == -1 and got[3][0] == -1 and got[1][0] >= 0 and got[2][0] >= 0 and got[1][0] != got[2][0]
    assert _bits_equal(got[1][1], (6.0, 3.0, 1.5)) and _bits_equal(got[2][1], (0.5, 0.25, 1.0))
    factors = lambda k: pt.description()[0][k][0][6:9]
    assert not np.any(factors(1)) and not np.any(factors(2)) and _bits_equal(factors(3), (2.0, 0.0, 0.0))
    assert pt.get_material_alpha(2)[0] == pbr.ptc.ALPHA_OPAQUE and pt.get_material_transmission(2)["transmission"] == 0.0
    recs, cdf, pm, total = pt.emissive_tex_table()
    want = ref.table(desc)
    assert len(recs) == 2 and np.array_equal(pm, want[2]) and total > 0
    tex_ids = np.ascontiguousarray(recs[:, 11]).view(np.int32)
    assert (tex_ids == got[1][0]).all() and np.array_equal(pt.description()[1][got[1][0]], tex_5x3())
    keep = [k for k in range(28) if k != 11]                                          # the loader numbers textures in the order the materials use them
    assert _bits_equal(recs[:, keep], want[0][:, keep]) and _bits_equal(cdf, want[1])
    # the switch: today's reading
    assert gltf.emissive_textures() is True
    gltf.load_into(pt, path, desc.camera, emissive_textures=False)
    assert gltf.emissive_textures() is True
    assert [pt.get_material_emission_texture(k)[0] for k in range(4)] == [-1] * 4
    assert _bits_equal(factors(1), (6.0, 3.0, 1.5)) and _bits_equal(factors(2), (0.5, 0.25, 1.0)) and _bits_equal(factors(3), (2.0, 0.0, 0.0))
    assert pt.emissive_tex_table()[0].shape == (0, 28) and pt.stats()["n_emitters"] == 2
    pt.close()
