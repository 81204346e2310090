"""The participating medium without a GPU (include/ptc_medium.h, csrc/pt_medium.h).

1. ptc_debug_medium_sample against the numpy restatement, bit for bit: origins inside, outside and on a face of the box, direction components 0.0, -0.0 and 1e-30,
   rays that graze an edge, g in {-0.99, -0.6, 0, 5e-4, 0.8, 0.99}.
2. Closed forms in float64, for the library's own values (ptc_debug_medium_sample) and the restatement: the phase function integrates to one and has mean cosine g,
   the free flight has the cdf 1 - exp(-sigma s), the transmittance is exp.
3. The float32 arithmetic against float64: the measured ratios under the bounds of medium_reference.py; the float64 step reference written from the definitions
   stays inside its cap of undecided rays, passes the restatement and catches each mutation of it.
4. Argument and state rules, the lifetime across ptc_scene_begin, commit and refit, the refusal with alpha and with glass on a description-only context.
5. The binding's table against include/ptc_medium.h; the ptc_ symbol list is what it was."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lights_reference as lref  # noqa: E402
import medium_reference as ref  # noqa: E402

F32, F64 = np.float32, np.float64
E_ARG, E_STATE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS = (-0.99, -0.6, 0.0, 5e-4, 0.8, 0.99)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_structs(pbr):
    m = pbr.ptc
    import c_header
    path = os.path.join(ROOT, "include", "ptc_medium.h")
    text = open(path).read()
    macros = dict(re.findall(r"^#define (ptc_\w+) (ptcx_\w+)$", text, flags=re.M))
    h = c_header.Header(path, "ptc_")
    assert list(h.prototypes) == list(m._MEDIUM_PROTOTYPES) == list(macros)
    assert list(macros) == ["ptc_set_medium", "ptc_get_medium", "ptc_clear_medium", "ptc_get_medium_stats", "ptc_debug_medium_sample", "ptc_debug_medium_step", "ptc_debug_medium_env"]
    assert all(macros[n] == "ptcx_" + n[4:] for n in macros)
    assert c_header.check_prototypes(h, m._MEDIUM_PROTOTYPES) == []
    assert list(h.structs) == ["ptc_medium_params", "ptc_medium_stats", "ptc_medium_sample"]
    for name, mirror in (("ptc_medium_params", m.PtcMediumParams), ("ptc_medium_stats", m.PtcMediumStats), ("ptc_medium_sample", m.PtcMediumSample)):
        assert c_header.check_struct(h.structs[name], mirror) == [], name
    L = m.load_library()
    for name, (restype, argtypes) in m._MEDIUM_PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert hasattr(L, "ptcx_" + name[4:])
    # the core interface is what it was: ABI version 4, the same 129 ptc_ symbols, none of the new names among them, no new public integer constant
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", m.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [line.split()[-1] for line in out.splitlines() if line.split()[-2] in "TW"]
    assert len([s for s in exported if s.startswith("ptc_")]) == 129 and not [s for s in exported if s.startswith("ptc_") and "medium" in s]
    assert L.ptc_abi_version() == 4 and not set(m._MEDIUM_PROTOTYPES) & set(m.ABI_SYMBOLS)
    assert not [k for k in vars(m) if k.isupper() and "MEDIUM" in k and isinstance(getattr(m, k), int)]
    assert '#include "ptc_medium.h"' in open(os.path.join(ROOT, "include", "ptc.h")).read()


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------------------
LO, HI = (-1.0, 0.0, -2.0), (1.5, 1.25, 0.5)


def _cases(rng, n):
    lo, hi = np.asarray(LO, F32), np.asarray(HI, F32)
    o = rng.uniform(-3, 3, (n, 3)).astype(F32)
    inside = rng.random(n) < 0.35
    o = np.where(inside[:, None], rng.uniform(lo, hi, (n, 3)), o).astype(F32)
    d = _unit(rng, n)
    aim = rng.random(n) < 0.5                                      # half of the outside rays aim at a point of the box
    tgt = rng.uniform(lo, hi, (n, 3))
    da = tgt - o
    da = (da / np.maximum(np.linalg.norm(da, axis=1, keepdims=True), 1e-9)).astype(F32)
    d = np.where((aim & ~inside)[:, None], da, d).astype(F32)
    k = rng.integers(0, 3, n)
    r = np.arange(n)
    face = rng.random(n) < 0.15                                    # origins exactly on a face
    o[r[face], k[face]] = np.where(rng.random(face.sum()) < 0.5, lo[k[face]], hi[k[face]])
    special = rng.random(n)
    for lo_p, hi_p, v in ((0.0, 0.08, 0.0), (0.08, 0.16, -0.0), (0.16, 0.24, 1e-30)):
        sel = (special >= lo_p) & (special < hi_p)
        d[r[sel], k[sel]] = F32(v)
    two = (special >= 0.24) & (special < 0.30)                     # two zero components: axis-parallel rays
    d[r[two], k[two]] = 0.0
    d[r[two], (k[two] + 1) % 3] = -0.0
    d = (d / np.linalg.norm(d.astype(F64), axis=1, keepdims=True)).astype(F32)
    graze = rng.random(n) < 0.1                                    # along an edge of the box: the origin on the edge's line, the direction the edge's
    e = rng.integers(0, 3, n)
    for i in np.nonzero(graze)[0]:
        a = int(e[i])
        p = np.where(rng.random(3) < 0.5, lo, hi).astype(F32)
        p[a] = F32(rng.uniform(-3, 3))
        o[i] = p
        d[i] = 0.0
        d[i, a] = rng.choice([-1.0, 1.0])
    t_end = np.where(rng.random(n) < 0.4, ref.T_INF, rng.uniform(0.05, 6.0, n)).astype(F32)
    return o, d, t_end


def test_sample_equals_the_restatement_bit_for_bit(pbr):
    m = pbr.ptc
    rng = np.random.default_rng(11)
    n = 2400
    o, d, t_end = _cases(rng, n)
    so, sd, stmax = _cases(rng, n)
    u = rng.random((n, 3)).astype(F32)
    u[rng.random(n) < 0.02, 0] = 0.0
    gs = np.asarray(GS, F32)[rng.integers(0, len(GS), n)]
    sig = rng.choice([0.05, 0.7, 3.0, 40.0], n).astype(F32)
    seen = dict(cross=0, empty=0, scatter=0, stand=0, face=0, zero=0, att=0)
    for g in GS:
        for s in (0.05, 0.7, 3.0, 40.0):
            sel = np.nonzero((gs == F32(g)) & (sig == F32(s)))[0]
            md = ref.Medium(LO, HI, s, 0.8, g)
            p = m.medium_params(**md.params())
            cr, t0, t1 = ref.span(md, o[sel], d[sel], t_end[sel])
            fl = ref.free_flight(md, t0, u[sel, 0])
            c = ref.hg_cos(g, u[sel, 1])
            wi = ref.hg_direction(d[sel], c, u[sel, 2])
            ph = ref.hg_phase(g, c)
            scr, s0, s1 = ref.span(md, so[sel], sd[sel], stmax[sel])
            tr = np.where(scr, ref.transmittance(md, s0, s1), F32(1.0))
            P = ref.vfma(d[sel], fl, o[sel])
            for j, i in enumerate(sel):
                got = m.medium_sample(p, o=o[i], d=d[i], t_end=t_end[i], u0=u[i, 0], u1=u[i, 1], u2=u[i, 2], so=so[i], sd=sd[i], stmax=stmax[i])
                assert bool(got["crosses"]) == bool(cr[j]), (i, got)
                assert _bits_equal(got["t0"], t0[j]) and _bits_equal(got["t1"], t1[j]), (i, got, t0[j], t1[j])
                if cr[j]:
                    assert _bits_equal(got["s"], fl[j]) and bool(got["scatters"]) == bool(fl[j] < t1[j]) and _bits_equal(got["P"], P[j]), (i, got, fl[j])
                else:
                    assert got["s"] == 0.0 and not got["scatters"]
                assert _bits_equal(got["cos_theta"], c[j]) and _bits_equal(got["wi"], wi[j]) and _bits_equal(got["pdf"], ph[j]), (i, got, c[j], wi[j], ph[j])
                assert _bits_equal(got["transmittance"], tr[j]), (i, got, tr[j])
                seen["cross"] += int(cr[j]); seen["empty"] += int(not cr[j]); seen["att"] += int(scr[j])
                seen["scatter"] += int(cr[j] and fl[j] < t1[j]); seen["stand"] += int(cr[j] and not fl[j] < t1[j])
                seen["face"] += int(((o[i] == md.lo) | (o[i] == md.hi)).any()); seen["zero"] += int((d[i] == 0).any())
    assert all(v > 50 for v in seen.values()), seen


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _library_values(pbr, g, sigma, u):
    """ptc_debug_medium_sample for a ray along +x through the box from outside, per number u: (cos_theta, pdf, s - t0, transmittance of the segment 0 .. s - t0)."""
    m = pbr.ptc
    p = m.medium_params(box_lo=(0.0, -1.0, -1.0), box_hi=(1000.0, 1.0, 1.0), sigma_t=sigma, albedo=1.0, g=g)
    out = []
    for x in u:
        r = m.medium_sample(p, o=(-1.0, 0.0, 0.0), d=(1.0, 0.0, 0.0), t_end=3.0e38, u0=x, u1=x, u2=0.25, so=(0.0, 0.0, 0.0), sd=(1.0, 0.0, 0.0), stmax=1.0)
        q = m.medium_sample(p, o=(-1.0, 0.0, 0.0), d=(1.0, 0.0, 0.0), t_end=3.0e38, u0=x, u1=x, u2=0.25, so=(0.0, 0.0, 0.0), sd=(1.0, 0.0, 0.0), stmax=min(r["s"] - r["t0"], 999.0))
        out.append((r["cos_theta"], r["pdf"], r["s"] - r["t0"], q["transmittance"]))
    return np.asarray(out, F64)


def test_closed_forms_in_float64(pbr):
    # the library's own float32 values against the closed forms: the density at the sampled cosine, the cdf the sampler inverts, the free flight, the transmittance
    for g in GS:
        u = np.linspace(0.02, 0.98, 13).astype(F32)
        lib = _library_values(pbr, g, 1.7, u)
        sig = float(F32(1.7))
        gg = float(F32(g))
        want_c = 1 - 2 * u.astype(F64) if abs(g) < 1e-3 else (1 + gg * gg - ((1 - gg * gg) / (1 - gg + 2 * gg * u.astype(F64))) ** 2) / (2 * gg)
        assert np.abs(lib[:, 0] - want_c).max() <= ref.K_COS, g
        want_ph = (1 - gg * gg) / (4 * np.pi * (1 + gg * gg - 2 * gg * lib[:, 0]) ** 1.5)
        assert (np.abs(lib[:, 1] / want_ph - 1) <= ref.phase_bound(g)).all(), g
        assert np.abs(lib[:, 2] * sig - (-np.log(1 - u.astype(F64)))).max() <= ref.K_FLIGHT + 2.0 ** -22, g      # t0 = 1 is subtracted from s again: one more ulp of s
        assert (np.abs(lib[:, 3] / np.exp(-sig * np.minimum(lib[:, 2], 999.0)) - 1) <= ref.K_TRANS).all(), g
    c = np.cos((np.arange(200000) + 0.5) * (np.pi / 200000))
    w = np.sin((np.arange(200000) + 0.5) * (np.pi / 200000)) * (np.pi / 200000) * 2 * np.pi       # midpoint rule over theta
    for g in GS:
        ph = ref.hg_phase(g, c, F64)
        assert abs((ph * w).sum() - 1.0) < 1e-6, g
        assert abs((ph * w * c).sum() - g) < 1e-6, g
        # the sampler inverts the cdf: P(cos <= c(u)) = u
        u = np.linspace(0.01, 0.99, 25).astype(F32)
        cu = ref.hg_cos(g, u, F64)
        cdf = np.array([(ph * w)[c <= x].sum() for x in cu])
        want = 1.0 - u if abs(g) < 1e-3 else u                        # the isotropic branch c = 1 - 2 u runs the other way
        assert np.abs(cdf - want).max() < 1e-3, (g, np.abs(cdf - want).max())      # the resolution of the sum: whole cells, and at |g| = 0.99 one cell of the peak holds 3e-4
    md = ref.Medium(LO, HI, 1.7)
    u = np.linspace(0.0, 0.999, 400).astype(F32)
    s = ref.free_flight(md, np.zeros_like(u), u, F64)
    assert np.abs((1.0 - np.exp(-F64(md.sigma_t) * s)) - u.astype(F64)).max() < 1e-12
    t0, t1 = np.zeros(50), np.linspace(0, 9, 50)
    assert np.abs(ref.transmittance(md, t0, t1, F64) - np.exp(-1.7 * t1)).max() < 1e-6      # sigma_t is a float32
    # a wi built from (c, u2) has that cosine with d and unit length
    rng = np.random.default_rng(3)
    d = _unit(rng, 500)
    cs = rng.uniform(-1, 1, 500)
    wi = ref.hg_direction(d, cs, rng.random(500).astype(F32), F64)
    assert np.abs((wi * d.astype(F64)).sum(1) - cs).max() < 1e-6 and np.abs(np.linalg.norm(wi, axis=1) - 1).max() < 1e-6


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_float32_against_float64(pbr):
    """The library's float32 values are the restatement's (a sample of them here, all of them in test_sample_equals_the_restatement_bit_for_bit), so what is measured
    below is the library's arithmetic.  The worst ratios of the float32 restatement to the float64 one; the bounds are four times these, rounded up to a power of two (DESIGN.md §2f has the table)."""
    for g in GS:
        uu = np.linspace(0.02, 0.98, 13).astype(F32)
        lib = _library_values(pbr, g, 0.7, uu)
        md = ref.Medium((0.0, -1.0, -1.0), (1000.0, 1.0, 1.0), 0.7, 1.0, g)
        c32 = ref.hg_cos(g, uu)
        assert _bits_equal(lib[:, 0], c32) and _bits_equal(lib[:, 1], ref.hg_phase(g, c32))
        assert _bits_equal(lib[:, 2], ref.free_flight(md, np.ones(13, F32), uu) - F32(1.0))
    rng = np.random.default_rng(17)
    n = 200000
    c = rng.uniform(-1, 1, n)
    c[: n // 10] = 1.0 - rng.uniform(0, 1e-3, n // 10)
    c[n // 10: n // 5] = -1.0 + rng.uniform(0, 1e-3, n // 10)
    u = rng.random(n).astype(F32)
    worst = dict(cos=0.0, flight=0.0, trans=0.0)
    for g in GS:
        # the phase function's x = 1 + g^2 - 2 g c cancels down to (1 - |g|)^2: its bound is the condition of that sum (medium_reference.phase_bound), not a constant
        p32, p64 = ref.hg_phase(g, c.astype(F32), F32), ref.hg_phase(g, c.astype(F32).astype(F64), F64)
        rel = float((np.abs(p32 - p64) / p64).max())
        print(f"phase g={g}: worst {rel:.3e}, bound {ref.phase_bound(g):.3e}")
        assert rel <= ref.phase_bound(g), (g, rel)
        worst["cos"] = max(worst["cos"], float(np.abs(ref.hg_cos(g, u, F32) - ref.hg_cos(g, u, F64)).max()))
    for s in (0.05, 0.7, 3.0, 40.0):
        md = ref.Medium(LO, HI, s)
        uu = u[u < 1.0 - np.exp(-16.0)]
        f32, f64 = ref.free_flight(md, np.zeros_like(uu), uu, F32), ref.free_flight(md, np.zeros_like(uu), uu, F64)
        worst["flight"] = max(worst["flight"], float((np.abs(f32 - f64) * F64(md.sigma_t)).max()))
        t1 = rng.uniform(0, 16.0 / s, 50000).astype(F32)
        z = np.zeros_like(t1)
        a, b = ref.transmittance(md, z, t1, F32), ref.transmittance(md, z, t1, F64)
        worst["trans"] = max(worst["trans"], float((np.abs(a - b) / b).max()))
    print("float32 against float64, worst ratios:", {k: f"{v:.3e}" for k, v in worst.items()})
    for k, bound in (("cos", ref.K_COS), ("flight", ref.K_FLIGHT), ("trans", ref.K_TRANS)):
        assert 4 * worst[k] <= bound <= 8 * worst[k], f"{k}: the bound {bound:.3e} is not four times the measured {worst[k]:.3e} rounded up to a power of two"


def _step_inputs(pbr, n, seed):
    """fog_box on a description-only context: rays from the camera side through the fog, their hits by the float32 search of all triangles."""
    from pbr_amd import scenes
    desc = scenes.fog_box(sigma_t=1.3, albedo=(0.9, 0.7, 0.5), g=0.6)
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)
    _, lights, cdf = pt.shading_tables()
    rng = np.random.default_rng(seed)
    o = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.2, 1.3, n), rng.uniform(2.5, 4.0, n)]).astype(F32)
    tgt = np.column_stack([rng.uniform(-1.8, 1.8, n), rng.uniform(0.0, 1.4, n), rng.uniform(-1.8, 1.8, n)])
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    T = rng.uniform(0.2, 1.0, (n, 3)).astype(F32)
    keys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    verts, idx, _ = pt.flat_scene()
    t, prim = _closest(verts, idx, o, d)
    md = ref.Medium(**desc.medium)
    # two point lights without a range: a cone's or a window's falloff goes to zero at its edge, where no relative bound holds (the bit-for-bit tests cover spots)
    two = lref.light_table([dict(type="point", position=(0.0, 0.9, 0.3), intensity=(3.0, 3.0, 3.0)),
                            dict(type="point", position=(-1.0, 2.5, 0.0), intensity=(5.0, 4.0, 3.0), sampling_weight=2.0)])
    return md, o, d, T, keys, t, prim >= 0, lights, cdf, two


def _closest(verts, idx, o, d):
    """float64 Moeller-Trumbore over all triangles: (t, prim), -1 for a miss."""
    P = np.asarray(verts, F64)[:, 0:3]
    tri = P[np.asarray(idx).reshape(-1, 3)]
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    best_t, best_p = np.full(len(o), np.inf), np.full(len(o), -1)
    for k in range(len(tri)):
        pv = np.cross(d.astype(F64), e2[k])
        det = pv @ e1[k]
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = o.astype(F64) - v0[k]
            uu = (tv * pv).sum(1) * inv
            qv = np.cross(tv, e1[k])
            vv = (d.astype(F64) * qv).sum(1) * inv
            tt = qv @ e2[k] * inv
        ok = (np.abs(det) > 1e-12) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (tt > 1e-6) & (tt < best_t)
        best_t, best_p = np.where(ok, tt, best_t), np.where(ok, k, best_p)
    return np.where(best_p >= 0, best_t, -1).astype(F32), best_p


@pytest.mark.parametrize("n", [1, 63, 513])
def test_step_reference_decides_and_the_checker_has_teeth(pbr, n):
    """The float64 step reference (medium_reference.reference64: written from the definitions, evaluated at the records' own directions) alone stays inside the cap — undecided rays at most 2 % of a set of 63 rays or more, none of the 1-ray set — the float32 restatement
    passes the checker, and each mutation of it is caught with the shipped bounds."""
    md, o, d, T, keys, t, is_hit, emit, cdf, two = _step_inputs(pbr, n, 23 + n)
    for bounce in (0, 2):
        a = ref.scatter_step(md, o, d, T, keys, t, is_hit, bounce, 8, emit, cdf, 1.0, two, F32)
        got = ref.as_got(a, d)
        r = ref.reference64(md, o, d, T, keys, t, is_hit, bounce, 8, got, emit, cdf, two)
        bad, und = ref.check(md, got, r, f"n={n} b={bounce}")
        assert bad == [], bad
        assert und <= (0 if n == 1 else int(0.02 * n)), (n, bounce, und)
        if n < 63:
            continue
        assert a["scattered"].sum() > n // 4 and a["shadow"].sum() > n // 8 and a["punctual"].sum() > n // 8
        for mut in ref.MUTATIONS:
            w = ref.as_got(ref.scatter_step(md, o, d, T, keys, t, is_hit, bounce, 8, emit, cdf, 1.0, two, F32, mutation=mut), d)
            bad, _ = ref.check(md, w, ref.reference64(md, o, d, T, keys, t, is_hit, bounce, 8, w, emit, cdf, two), mut)
            assert bad, f"mutation {mut} passed the checker at n={n}, bounce {bounce}"


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_rules(pbr):
    from pbr_amd import scenes
    m = pbr.ptc
    pt = pbr.PathTracer(m.DEVICE_NONE)
    L, h = pt._L, pt._h
    assert pt.get_medium() is None
    good = dict(box_lo=(-1, 0, -1), box_hi=(1, 2, 1), sigma_t=0.5, albedo=(0.9, 0.8, 0.7), g=0.3)
    pt.set_medium(**good)
    kept = pt.get_medium()
    assert kept["sigma_t"] == 0.5 and kept["box_hi"] == (1.0, 2.0, 1.0) and abs(kept["g"] - 0.3) < 1e-7
    for bad in (dict(box_lo=(1, 0, -1)), dict(box_hi=(1, 0, 1)), dict(box_lo=(float("nan"), 0, 0)), dict(box_hi=(float("inf"), 2, 1)), dict(sigma_t=-0.1), dict(sigma_t=float("inf")),
                dict(sigma_t=float("nan")), dict(albedo=(1.1, 0.5, 0.5)), dict(albedo=(0.5, -0.1, 0.5)), dict(g=1.0), dict(g=-0.995), dict(g=float("nan"))):
        p = m.medium_params(**dict(good, **bad))
        assert L.ptc_set_medium(h, p) == E_ARG, bad
        assert pt.get_medium() == kept, bad                       # nothing changed
        assert L.ptc_debug_medium_sample(p, m.PtcMediumSample()) == E_ARG
    assert L.ptc_set_medium(h, None) == E_ARG and L.ptc_set_medium(None, m.medium_params(**good)) == E_ARG
    assert L.ptc_debug_medium_sample(None, m.PtcMediumSample()) == E_ARG
    pt.set_medium(**dict(good, sigma_t=0.0, g=0.99))              # the edges of the ranges are inside
    pt.clear_medium()
    assert pt.get_medium() is None
    st = pt.medium_stats()                                         # a description-only context: zeros
    assert st == dict(crossed=0, scattered=0, attenuated=0, seconds_medium=0.0)
    # the lifetime of the lights: ptc_scene_begin drops the medium; commit and refit keep it
    pt.set_medium(**good)
    pt.load_scene(scenes.cornell_box())
    assert pt.get_medium() is None
    pt.set_medium(**good)
    pt.update_instance(0, t=(0.0, 0.1, 0.0), q_wxyz=(1.0, 0.0, 0.0, 0.0), s=(1.0, 1.0, 1.0))
    pt.scene_refit()
    assert pt.get_medium() == kept
    pt.load_scene(scenes.fog_box())                                # a description that carries a medium sets it behind ptc_scene_begin
    assert pt.get_medium()["sigma_t"] == pytest.approx(0.7)


def test_medium_refuses_alpha_and_glass_scenes(pbr):
    """ptc_frame_begin of the path integrator with a medium on and a committed scene with alpha coverage or transmission: PTC_E_STATE with the remedy in the message,
    decided on a description-only context (without the medium, or with sigma_t = 0, the same call gets as far as needing a device)."""
    from pbr_amd import scenes
    m = pbr.ptc
    E_DEVICE = -3
    fog = dict(box_lo=(-5, -5, -5), box_hi=(5, 5, 5), sigma_t=0.2)
    for desc, remedy in ((scenes.alpha_layers(), "--no-alpha"), (scenes.glass_slab(), "--no-transmission")):
        pt = pbr.PathTracer(m.DEVICE_NONE).load_scene(desc)
        L, h = pt._L, pt._h
        rc_plain = L.ptc_frame_begin(h, 8, 8, 1, 1, 4, m.INTEGRATOR_PATH, 0, 1)
        assert rc_plain != E_STATE and rc_plain < 0                 # no device
        pt.set_medium(**fog)
        assert L.ptc_frame_begin(h, 8, 8, 1, 1, 4, m.INTEGRATOR_PATH, 0, 1) == E_STATE
        msg = L.ptc_last_error(h).decode()
        assert remedy in msg and "medium" in msg, msg
        assert L.ptc_frame_begin(h, 8, 8, 1, 1, 4, m.INTEGRATOR_RASTER_COMPAT, 0, 1) == rc_plain      # the raster integrators ignore the medium
        pt.set_medium(**dict(fog, sigma_t=0.0))
        assert L.ptc_frame_begin(h, 8, 8, 1, 1, 4, m.INTEGRATOR_PATH, 0, 1) == rc_plain
        pt.set_medium(**fog)
        pt.clear_medium()
        assert L.ptc_frame_begin(h, 8, 8, 1, 1, 4, m.INTEGRATOR_PATH, 0, 1) == rc_plain
    pt = pbr.PathTracer(m.DEVICE_NONE).load_scene(scenes.cornell_box())      # an opaque scene is not refused
    pt.set_medium(**fog)
    assert pt._L.ptc_frame_begin(pt._h, 8, 8, 1, 1, 4, m.INTEGRATOR_PATH, 0, 1) not in (0, E_STATE)
