"""Transparent shadows without a GPU (include/ptc_glass_shadows.h: ptc_set_glass_shadows ..., csrc/pt_glass_shadow.h).

1. ptc_debug_glass_shadow_transmit against the numpy restatement, bit for bit, over the random cases of test_glass_host.py; solid materials give 0.
2. Closed forms in float64 at ns = ng, and the float32 restatement against float64.
3. The share pt_glass_interact transmits, swept over u_e, against 1 - F_t, fallback cases included; a transmitted ray's tint is the base colour.
4. The argument and state rules, zeros from a description-only context.
5. The binding's table against include/ptc_glass_shadows.h.
6. The float64 shadow walk on the GPU tests' record sets: the share of records float32 and float64 need not agree about, and the float32 restatement (fed by a
   float32 search of all triangles) against it on every other record."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glass_reference as gref  # noqa: E402
import glass_shadow_reference as ref  # noqa: E402
from test_glass_host import _random_cases  # noqa: E402

F32, F64 = np.float32, np.float64
E_ARG = -1


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_structs(pbr):
    m = pbr.ptc
    import c_header
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(ROOT, "include", "ptc_glass_shadows.h")
    text = open(path).read()
    macros = dict(re.findall(r"^#define (ptc_\w+) (ptcx_\w+)$", text, flags=re.M))
    h = c_header.Header(path, "ptc_")
    names = ["ptc_set_glass_shadows", "ptc_get_glass_shadows", "ptc_get_glass_shadow_stats", "ptc_debug_glass_any", "ptc_debug_glass_shadow_transmit"]
    assert list(h.prototypes) == list(m._GLASS_SHADOW_PROTOTYPES) == list(macros) == names
    assert all(macros[n] == "ptcx_" + n[4:] for n in macros)
    assert c_header.check_prototypes(h, m._GLASS_SHADOW_PROTOTYPES) == []
    assert list(h.structs) == ["ptc_glass_shadow_stats", "ptc_glass_shadow_hit"]
    for name, mirror in (("ptc_glass_shadow_stats", m.PtcGlassShadowStats), ("ptc_glass_shadow_hit", m.PtcGlassShadowHit)):
        assert c_header.check_struct(h.structs[name], mirror) == [], name
    L = m.load_library()
    for name, (restype, argtypes) in m._GLASS_SHADOW_PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the core interface and ptc_glass.h are what they were
    assert L.ptc_abi_version() == 4 and not set(names) & set(m.ABI_SYMBOLS) and not set(names) & set(m.GLASS_SYMBOLS) and len(m.GLASS_SYMBOLS) == 8
    assert '#include "ptc_glass_shadows.h"' in open(os.path.join(ROOT, "include", "ptc.h")).read()


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_transmit_equals_the_restatement_bit_for_bit(pbr):
    m = pbr.ptc
    rng = np.random.default_rng(5)
    n = 3000
    c = _random_cases(rng, n)
    W, F_t, fb = ref.transmit(c["tau"], c["ior"], c["thin"], c["ng"], c["ns"], c["d"], c["base"], c["metallic"])
    seen = dict(solid=0, thin=0, fallback=0, opaque=0)
    for i in range(n):
        p = m.transmission_params(transmission=c["tau"][i], ior=c["ior"][i], thin_walled=int(c["thin"][i]))
        got = m.glass_shadow_transmit(p, ng=c["ng"][i], ns=c["ns"][i], d=c["d"][i], base=c["base"][i], metallic=c["metallic"][i])
        assert _bits_equal(got["W"], W[i]) and _bits_equal(got["F_t"], F_t[i]), (i, got, W[i], F_t[i])
        if not c["thin"][i]:
            assert got["W"] == (0.0, 0.0, 0.0) and got["F_t"] == 0.0
        seen["solid" if not c["thin"][i] else "thin"] += 1
        seen["fallback"] += int(fb[i]); seen["opaque"] += int(c["thin"][i] and not W[i].any())
    assert all(v > 10 for v in seen.values()), seen
    # a ray that does not arrive against ng gives 0
    p = m.transmission_params(transmission=1.0)
    z = np.array([0.0, 0.0, 1.0], F32)
    for d in (z, np.array([1.0, 0.0, 0.0], F32)):
        assert m.glass_shadow_transmit(p, ng=z, ns=z, d=d, base=np.ones(3, F32), metallic=0.0)["W"] == (0.0, 0.0, 0.0)
    import ctypes as C
    assert m.load_library().ptc_debug_glass_shadow_transmit(None, C.byref(m.PtcGlassShadowHit())) == E_ARG
    assert m.load_library().ptc_debug_glass_shadow_transmit(C.byref(p), None) == E_ARG


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _fresnel64(cos_i, n):
    eta = 1.0 / n
    s2 = eta * eta * (1.0 - cos_i * cos_i)
    ct = np.sqrt(1.0 - s2)
    rs, rp = (eta * cos_i - ct) / (eta * cos_i + ct), (cos_i - eta * ct) / (cos_i + eta * ct)
    return 0.5 * (rs * rs + rp * rp)


def test_closed_forms_in_float64():
    z = np.array([[0.0, 0.0, 1.0]])
    base = np.array([[0.9, 0.5, 0.25]])
    for n in (1.0, 1.33, 1.5, 2.4):
        for tau, met in ((1.0, 0.0), (0.6, 0.25)):
            for th in np.linspace(0.0, np.pi / 2, 91)[:-1]:
                d = np.array([[np.sin(th), 0.0, -np.cos(th)]])
                W, F_t, fb = ref.transmit([tau], [n], [True], z, z, d, base, [met], F64)
                F = _fresnel64(np.cos(th), n)
                assert not fb[0] and abs(F_t[0] - 2.0 * F / (1.0 + F)) < 1e-14
                assert np.allclose(W[0], tau * (1.0 - met) * (1.0 - 2.0 * F / (1.0 + F)) * base[0], rtol=0, atol=1e-14)
                if n == 1.0 and tau == 1.0:
                    assert np.array_equal(W[0], base[0])                     # ior 1: the pane reflects nothing
            # grazing incidence: W -> 0
            for th, bound in ((np.pi / 2 - 1e-3, 2e-2), (np.pi / 2 - 1e-5, 2e-4)):
                if n > 1.0:
                    d = np.array([[np.sin(th), 0.0, -np.cos(th)]])
                    assert ref.transmit([tau], [n], [True], z, z, d, base, [met], F64)[0].max() < bound
    assert not ref.transmit([1.0], [1.5], [False], z, z, -z, base, [0.0], F64)[0].any()      # a solid


def test_float32_against_float64():
    """The float32 restatement against the same formulas in float64 over ior 1 .. 3, the full angle range and tilted shading normals: W stays within the
    project's bound on F (gref.F_BOUND = 5e-5) times p_t x base, plus two roundings of the products.  The fallback cases are compared where both
    precisions take the same branch."""
    rng = np.random.default_rng(9)
    n = 20000
    ng = np.repeat(np.array([[0.0, 0.0, 1.0]], F32), n, 0)
    th = rng.uniform(0.0, np.pi / 2, n)
    ph = rng.uniform(0.0, 2 * np.pi, n)
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)], 1).astype(F32)
    ns = ng + rng.normal(size=(n, 3)) * rng.choice([0.0, 0.05, 0.5], n)[:, None]
    ns = (ns / np.linalg.norm(ns, axis=1, keepdims=True)).astype(F32)
    ns = np.where(((ns * -d).sum(1) > 0)[:, None], ns, ng).astype(F32)
    tau, ior, met = rng.uniform(0.1, 1.0, n).astype(F32), rng.uniform(1.0, 3.0, n).astype(F32), rng.choice([0.0, 0.3], n).astype(F32)
    base = rng.uniform(0.1, 1.0, (n, 3)).astype(F32)
    thin = np.ones(n, bool)
    W32, _, fb32 = ref.transmit(tau, ior, thin, ng, ns, d, base, met)
    W64, _, fb64 = ref.transmit(tau.astype(F64), ior.astype(F64), thin, ng.astype(F64), ns.astype(F64), d.astype(F64), base.astype(F64), met.astype(F64), F64)
    same = fb32 == fb64
    assert (~same).sum() <= 5 and fb32.sum() > 100
    p_t = tau.astype(F64) * (1.0 - met.astype(F64))
    bound = (gref.F_BOUND * p_t)[:, None] * base + 3 * 2.0 ** -23 * W64
    err = np.abs(W32.astype(F64) - W64)
    print(f"float32 against float64: worst |W32 - W64| / bound {float((err / bound)[same].max()):.3f} over {int(same.sum())} cases, {int(fb32.sum())} with the ng fallback")
    assert (err[same] <= bound[same]).all()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_transmit_probability_is_what_interact_transmits(pbr):
    m = pbr.ptc
    z = np.array([0.0, 0.0, 1.0], F32)
    G = 400                                                            # u_e = (g + 0.5) / G
    base = np.array([0.9, 0.5, 0.25], F32)
    cases = []
    for th in (0.0, 0.8, 1.3, 1.5):
        d = np.array([np.sin(th), 0.0, -np.cos(th)], F32)
        cases.append((z, d))                                          # ns = ng
        for tilt in (0.3, 1.2, 2.5):                                  # ns leaning away from the ray: the stronger ones reflect below the surface -> the ng fallback
            ns = np.array([-tilt, 0.2, 1.0]); ns = (ns / np.linalg.norm(ns)).astype(F32)
            if float(ns @ -d) > 0:
                cases.append((ns, d))
    fallbacks = 0
    for ior in (1.0, 1.5, 2.4):
        p = m.transmission_params(transmission=1.0, ior=ior)
        for ns, d in cases:
            sh = m.glass_shadow_transmit(p, ng=z, ns=ns, d=d, base=base, metallic=0.0)
            _, _, fb = ref.transmit([1.0], [ior], [True], z[None], ns[None], d[None], base[None], [0.0])
            fallbacks += int(fb[0])
            k = 0
            for g in range(G):
                got = m.glass_interact(p, P=np.zeros(3, F32), ng=z, ns=ns, front=1, d=d, T=np.ones(3, F32), t=1.0, base=base, metallic=0.0, u_s=0.0, u_e=(g + 0.5) / G, j=0,
                                       max_interactions=8, ray_eps=F32(1e-4))
                if got["outcome"] == gref.TRANSMIT:
                    k += 1
                    assert _bits_equal(got["T_out"], base) and _bits_equal(got["d_out"], d)
            assert abs(k / G - (1.0 - sh["F_t"])) <= 1.0 / G + 1e-6, (ior, ns, d, k / G, sh)
            assert _bits_equal(sh["W"], (F32(1.0) * (F32(1.0) - F32(sh["F_t"]))) * base)
    assert fallbacks >= 6


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_rules(pbr):
    import ctypes as C
    m = pbr.ptc
    pt = pbr.PathTracer(m.DEVICE_NONE)
    L, h = pt._L, pt._h
    assert pt.get_glass_shadows() is False
    for bad in (-1, 2, 7):
        assert L.ptc_set_glass_shadows(h, bad) == E_ARG and pt.get_glass_shadows() is False
    assert L.ptc_set_glass_shadows(None, 1) == E_ARG and L.ptc_get_glass_shadows(h, None) == E_ARG
    pt.set_glass_shadows(True)
    assert pt.get_glass_shadows() is True
    pt.load_scene(pbr.scenes.glass_panes(2))                           # ptc_scene_begin keeps it
    assert pt.get_glass_shadows() is True
    assert pt.glass_shadow_stats() == dict(walked=0, passes=0, visible=0, exhausted=0)
    assert L.ptc_get_glass_shadow_stats(h, None) == E_ARG
    o = np.zeros((1, 3), F32)
    tr, lay = np.ones((1, 3), F32), np.ones(1, np.uint32)
    from pbr_amd.ptc import _ptr
    assert L.ptc_debug_glass_any(h, _ptr(o), _ptr(o), _ptr(np.ones(1, F32)), 1, _ptr(tr), _ptr(lay)) < 0      # no device
    pt.set_glass_shadows(False)
    assert pt.get_glass_shadows() is False
    pt.close()


def test_the_panes_scene(pbr):
    """scenes.glass_panes: the primitive ids, the tilted vertex normals, the sheets last."""
    desc = pbr.scenes.glass_panes(3, tilt=0.4, emitter=True, sheets=("blend", "mask"))
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)
    verts, idx, tri_mat = pt.flat_scene()
    assert list(tri_mat) == [0, 0, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3, 4, 4]
    bits, mats, n_prims, _ = pt.glass_tables()
    assert int(bits[0]) == 0b00001111110000 and pt.alpha_tables()[0][0] == 0b11110000000000
    nrm = verts[:, 3:6][8:20]
    assert (np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-6).all() and (nrm[:, 1] < 0.999).all() and (nrm[:, 1] > 0.8).all() and len(np.unique(nrm.round(5), axis=0)) == 4
    flat = pbr.scenes.glass_panes(3)
    assert (np.asarray(flat.meshes[1].vertices["normal"]) == (0.0, 1.0, 0.0)).all()
    pt.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pane", "stack3", "mixed", "solid"])
def test_the_reference_decides_the_gpu_tests_records(pbr, name):
    """The float64 shadow walk (`walk64_any`) on the record sets of tests/test_gpu_glass_shadows.py, next to the float32 restatement (`resolve_any`) fed by float32
    searches of all triangles, so that no device is needed.  A record is left out only where a hit lies within 1e-4 in barycentrics of a triangle edge, within the t
    bound of rem, or where the texel, the cutoff or the ng fallback is undecided; at most 2 % are.  Expected on unit-scale quads with at most 9 surfaces per record:
    about 9 x 3e-4 = 0.3 %.  Measured here over 578 records per scene: pane 0.00 %, stack3 0.00 %, mixed 0.52 % (the 8x8 textures' texel edges add to the triangles'
    edges), solid 0.00 %.
    On every decided record the restatement passes the same surfaces and its Tr stays within the first-order bound the walk carries."""
    desc = ref.record_scenes(pbr)[name]
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)
    sc = gref.Scene(pt, desc)
    trace, trace_any = gref.trace32(sc), ref.any32(sc)
    L = ref.rounds_limit(8, 8, sc.alpha is not None)
    total = und = compared = lit = 0
    for n, o, d, tmax in ref.shadow_sets(pt, (65, 513)):
        w = ref.walk64_any(sc, o, d, tmax, L)
        Tr, layers, cnt = ref.resolve_any(sc, trace, trace_any, o, d, tmax, L)
        m, worst = ref.check_against_walk64(Tr, layers, w, f"{name} n {n}")
        print(f"{name} n={n}: {m} records compared, error / bound at most {worst:.2e}, counters {cnt}")
        total += n; und += int(w["undecided"].sum()); compared += m; lit += int((Tr.any(1) & (layers > 0)).sum())
        assert cnt["exhausted"] == 0 and cnt["walked"] > 0.5 * n
    print(f"{name}: {total} records, {und} undecided ({100.0 * und / total:.2f} %), {lit} lit through a surface")
    assert und <= ref.MAX_UNDECIDED * total and compared == total - und
    assert (lit == 0) if name == "solid" else (lit > 0.3 * total)
    pt.close()
