"""Alpha coverage without a GPU (include/ptc_alpha.h: ptc_set_material_alpha ..., csrc/pt_alpha.h).

1. ptc_debug_alpha_decide against the numpy restatement, bit for bit.
2. The argument and state rules of ptc_set_material_alpha / ptc_set_alpha_max_layers, and the alpha tables of a description-only commit.
3. glTF alphaMode / alphaCutoff through the loader.
4. The float64 reference alone on the GPU test's ray set: the share of rays float32 and float64 need not agree about stays under the cap."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alpha_reference as ref  # noqa: E402

F32 = np.float32
E_ARG, E_STATE = -1, -2


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_symbols_and_constants(pbr):
    m = pbr.ptc
    assert (m.ALPHA_OPAQUE, m.ALPHA_MASK, m.ALPHA_BLEND) == (ref.OPAQUE, ref.MASK, ref.BLEND) == (0, 1, 2)
    # include/ptc_alpha.h against the binding's table, with the reader that holds ptc.h to its table: same functions, same order, same classes of types; the struct's mirror
    import c_header
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(ROOT, "include", "ptc_alpha.h")).read()
    import re
    macros = dict(re.findall(r"^#define (ptc_\w+) (ptcx_\w+)$", text, flags=re.M))
    h = c_header.Header(os.path.join(ROOT, "include", "ptc_alpha.h"), "ptc_")
    assert list(h.prototypes) == m.ALPHA_SYMBOLS == list(macros) and len(m.ALPHA_SYMBOLS) == 8
    assert all(macros[n] == "ptcx_" + n[4:] for n in macros)
    assert c_header.check_prototypes(h, m._ALPHA_PROTOTYPES) == []
    assert list(h.structs) == ["ptc_alpha_stats"] and c_header.check_struct(h.structs["ptc_alpha_stats"], m.PtcAlphaStats) == []
    L = m.load_library()
    for name, (restype, argtypes) in m._ALPHA_PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the core interface is what it was: ABI version 4, none of the new names in its table
    assert L.ptc_abi_version() == 4 and not set(m.ALPHA_SYMBOLS) & set(m.ABI_SYMBOLS)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_decide_equals_the_restatement_bit_for_bit(pbr):
    nxt = lambda x, to: np.nextafter(F32(x), F32(to))
    cutoffs = [F32(0.0), F32(0.3), F32(0.5), F32(128.0 / 255.0), F32(1.0)]
    us = [F32(0.0), F32(0.25), F32(0.5), nxt(0.5, 0), nxt(0.5, 1), F32(16777215.0 / 16777216.0)]
    n = 0
    for mode in (ref.OPAQUE, ref.MASK, ref.BLEND):
        for c in cutoffs:
            avals = [F32(0.0), F32(1.0), c, nxt(c, -1), nxt(c, 2), F32(0.25), F32(0.5), nxt(0.5, 0), nxt(0.5, 1), F32(1.5), F32(-0.25), nxt(1.0, 0), nxt(1.0, 2), F32(1e-30), F32(-0.0)]
            for a in avals:
                for u in us:
                    acc, tr = pbr.ptc.alpha_decide(mode, c, a, u)
                    assert acc == bool(ref.accept(mode, c, a, u)), (mode, c, a, u)
                    assert _bits_equal(tr, ref.transmit(mode, c, a)), (mode, c, a)
                    n += 1
    assert n == 3 * 5 * 15 * 6
    # closed forms: an opaque surface blocks, a mask is all or nothing, blend lets 1 - a through
    assert pbr.ptc.alpha_decide("opaque", 0.5, 0.0, 0.9) == (True, F32(0.0))
    assert pbr.ptc.alpha_decide("mask", 0.5, 0.5, 0.9) == (True, F32(0.0)) and pbr.ptc.alpha_decide("mask", 0.5, nxt(0.5, 0), 0.0) == (False, F32(1.0))
    assert pbr.ptc.alpha_decide("blend", 0.5, 0.25, 0.25) == (False, F32(0.75)) and pbr.ptc.alpha_decide("blend", 0.5, 0.25, nxt(0.25, 0))[0] is True
    with pytest.raises(pbr.PtcError):
        pbr.ptc.alpha_decide(3, 0.5, 0.5, 0.5)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _describe(pbr, pt, desc):
    """load_scene without the commit and without the alpha modes: textures, materials, meshes, instances, camera."""
    from pbr_amd.ptc import _f, _ptr
    L, h = pt._L, pt._h
    assert L.ptc_scene_begin(h) == 0
    for t in desc.textures:
        t = np.ascontiguousarray(t, np.uint8)
        assert L.ptc_add_texture_rgba8(h, _ptr(t), t.shape[1], t.shape[0]) >= 0
    for m in desc.materials:
        assert L.ptc_add_material(h, _f(m.base_color)[1], m.metallic, m.roughness, _f(m.emissive)[1], m.tex_color, m.tex_normal, m.tex_mr) >= 0
    for me in desc.meshes:
        v, i = np.ascontiguousarray(me.vertices), np.ascontiguousarray(me.indices, np.uint32)
        assert L.ptc_add_mesh(h, v.ctypes.data, v.size, _ptr(i), i.size, me.material) >= 0
    for it in desc.instances:
        assert L.ptc_add_instance(h, it.mesh, _f(it.t)[1], _f(it.q_wxyz)[1], _f(it.s)[1]) >= 0
    c = desc.camera
    assert L.ptc_set_camera(h, _f(c.position)[1], _f(c.target)[1], c.fov_y, c.aspect) == 0


def test_argument_and_state_rules(pbr):
    desc = pbr.scenes.alpha_layers()
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    L, h = pt._L, pt._h
    _describe(pbr, pt, desc)
    nm = len(desc.materials)
    state = lambda: [pt.get_material_alpha(m) for m in range(nm)]
    assert state() == [(0, 0.5)] * nm                                          # every material starts OPAQUE
    pt.set_material_alpha(2, "mask", 0.25).set_material_alpha(3, "blend")
    want = [(0, 0.5), (0, 0.5), (1, 0.25), (2, 0.5)] + [(0, 0.5)] * (nm - 4)
    assert state() == want
    # each refusal leaves the state as it was
    for args in ((2, 3, 0.5), (2, -1, 0.5), (nm, 1, 0.5), (-1, 1, 0.5), (2, 1, float("nan")), (2, 1, float("inf")), (2, 1, -0.01), (2, 1, 1.5),
                 (1, 1, 0.5), (1, 2, 0.5), (1, 0, 0.5)):                       # material 1 is the emitter: refused whatever the mode
        assert L.ptc_set_material_alpha(h, args[0], args[1], args[2]) == E_ARG, args
        assert state() == want
    assert b"emissive" in L.ptc_last_error(h)
    assert L.ptc_get_material_alpha(h, nm, None, None) == E_ARG
    # the cutoff's ends are allowed; a material can go back to OPAQUE
    pt.set_material_alpha(2, "mask", 0.0).set_material_alpha(2, "mask", 1.0).set_material_alpha(3, "opaque")
    assert state()[2:4] == [(1, 1.0), (0, 0.5)]
    # max_layers: 1 .. 16
    for n in (0, -3, 17, 1 << 20):
        assert L.ptc_set_alpha_max_layers(h, n) == E_ARG
    assert L.ptc_set_alpha_max_layers(h, 1) == 0 and L.ptc_set_alpha_max_layers(h, 16) == 0
    # once committed the modes are fixed
    assert L.ptc_scene_commit(h) == 0
    assert L.ptc_set_material_alpha(h, 2, 2, 0.5) == E_STATE and state()[2] == (1, 1.0)
    # ptc_scene_begin drops the modes
    _describe(pbr, pt, desc)
    assert state() == [(0, 0.5)] * nm
    assert L.ptc_set_material_alpha(h, 2, 1, 0.5) == 0
    pt.close()


@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_tables_of_a_description_only_commit(pbr, builder):
    desc = pbr.scenes.alpha_layers(texture_filter="linear")
    desc.bvh_builder = builder
    desc.materials[3].alpha_cutoff = 0.3
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)

    def check():
        _, _, tri_mat = pt.flat_scene()
        bits, mode, cutoff, n_prims, queue = pt.alpha_tables()
        rb, rm, rc = ref.tables(tri_mat, desc.materials)
        assert n_prims == len(tri_mat) == 14 and not queue
        assert np.array_equal(bits, rb) and np.array_equal(mode, rm) and _bits_equal(cutoff, rc)
        # the quads were added last: floor and emitter keep the ids 0..3 and stay opaque, every layer primitive has its bit
        assert int(bits[0]) == 0b11111111110000
        assert list(mode) == [0, 0, 1, 1, 1, 2, 2] and cutoff[3] == F32(0.3)

    check()
    pt.update_instance(3, (0.1, 0.05, -0.2), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0)).scene_refit()
    check()
    # a scene without alpha materials: all zero
    pt.load_scene(pbr.scenes.cornell_box())
    bits, mode, cutoff, n_prims, queue = pt.alpha_tables()
    assert not bits.any() and not mode.any() and n_prims == 12 and not queue
    st = pt.alpha_stats()
    assert st == dict(closest_passes=0, shadow_walked=0, shadow_passes=0, exhausted=0, seconds_alpha=0.0)
    pt.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_gltf_alpha_modes(pbr, tmp_path):
    from pbr_amd import gltf
    M = pbr.scene.Material
    desc = pbr.scenes.cornell_box()
    desc.materials = [M((0.7, 0.7, 0.7, 0.8), 0.0, 1.0, alpha_mode="mask", alpha_cutoff=0.3), M((0.6, 0.1, 0.1, 0.4), 0.0, 1.0, alpha_mode="blend"),
                      M((0.1, 0.5, 0.1, 1.0), 0.0, 1.0, alpha_mode="OPAQUE"), M((0.0, 0.0, 0.0, 0.5), 0.0, 1.0, (15.0, 15.0, 15.0), alpha_mode="blend"),
                      M((0.2, 0.2, 0.9, 1.0), 0.0, 1.0)]
    desc.meshes[1].material = 4                                                # the ceiling takes the material without an alphaMode
    path = str(tmp_path / "alpha.glb")
    gltf.write_glb(desc, path)
    doc = open(path, "rb").read()
    assert doc.count(b'"alphaMode"') == 4 and doc.count(b'"alphaCutoff"') == 1
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    gltf.load_into(pt, path, desc.camera)
    got = [pt.get_material_alpha(m) for m in range(5)]
    assert [g[0] for g in got] == [ref.MASK, ref.BLEND, ref.OPAQUE, ref.OPAQUE, ref.OPAQUE]      # the emissive BLEND material stays opaque
    assert got[0][1] == float(F32(0.3)) and got[1][1] == 0.5
    _, _, tri_mat = pt.flat_scene()
    bits, mode, _, n_prims, _ = pt.alpha_tables()
    assert np.array_equal(ref.prim_is_alpha(bits, np.arange(n_prims)), np.isin(tri_mat, (0, 1)))
    pt.close()
    # an unknown mode fails, and the text says which material
    desc.materials[1].alpha_mode = "DITHER"
    bad = str(tmp_path / "bad.glb")
    gltf.write_glb(desc, bad)
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    with pytest.raises(Exception) as e:
        gltf.load_into(pt, bad, desc.camera)
    assert "material 1" in str(e.value) and "DITHER" in str(e.value)
    pt.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", ["nearest", "linear"])
def test_the_reference_decides_the_gpu_tests_rays(pbr, filt):
    """tests/test_gpu_alpha.py leaves out the rays `walk_closest` calls undecided and asserts that they are at most 2 %.  Whether that holds is a property of the
    scene, the ray set and the margins alone, so it is checked here, where no GPU is needed: the scene's spacing, texture size and camera were chosen for it."""
    desc = pbr.scenes.alpha_layers(3, 2, filt)
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)
    verts, idx, tri_mat = pt.flat_scene()
    total = und = hits = passed = 0
    for n, o, d, keys in ref.ray_sets(pt):
        t, prim, layers, undecided = ref.walk_closest(verts, idx, tri_mat, desc.materials, desc.textures, filt == "linear", o, d, keys, 0, 8)
        total += n; und += int(undecided.sum()); hits += int((prim >= 0).sum()); passed += int((layers > 0).sum())
        assert (layers <= 8).all() and ((prim >= 0) == np.isfinite(t)).all()
    print(f"alpha_layers {filt}: {total} rays, {und} undecided ({100.0 * und / total:.2f} %), {hits} hits, {passed} passed at least one layer")
    assert und <= ref.MAX_UNDECIDED * total
    assert hits > 0.5 * total and passed > 0.2 * total                          # the set is about alpha: most rays hit, many pass through a layer
    pt.close()
