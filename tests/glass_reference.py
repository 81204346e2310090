"""numpy restatement of dielectric transmission (csrc/pt_glass.h, csrc/pt_glass.hip), for tests/test_glass_host.py and tests/test_gpu_glass.py.

Parts:
  log2 / exp2 / sigma2 / beer / event / interact   pt_log2, pt_exp2 and the definition of pt_glass.h, elementwise; dt = float32 follows the sources operation for
                                                   operation (bit for bit), dt = float64 evaluates the same formulas in double
  tables                                           the bit table per primitive and the record per material the commit builds
  Scene / resolve_closest                          the rounds of k_glass_filter: the candidate hits come from a `trace(o, d)` callable (float32: the library's own
                                                   ptc_debug_trace_closest, or `trace32`, a float32 search of all triangles that needs no device), the surface, Beer,
                                                   the choice and the event are restated here
  walk64 / check_against_walk64                    the independent walk in float64 throughout, with a search of all triangles of its own; it also says which rays
                                                   the two precisions need not agree about and carries a first-order error bound per ray, to which a float32
                                                   resolution (the restatement's or the device's) is held on every other ray"""
import numpy as np

import alpha_reference as aref
import lights_reference as lref
import trace_reference as tref
from lens_reference import F32, F64, U64, _fma, rng_f

RNG_BASE = 0x08000000
DELTA_PDF = F32(1.0e18)
STANDS, EXHAUSTED, REFLECT, TRANSMIT = 0, 1, 2, 3
# |float32 - float64| of the closed forms over ior 1..3 and the full angle range (rounding only: both evaluate the same formulas), measured by
# test_glass_host.py::test_float32_against_float64, and the bounds the tests use: four times the largest deviation seen.
# The largest deviations sit next to the critical angle, where sqrt(1 - s2) amplifies the rounding of s2.
F_BOUND = 4 * 1.25e-5         # the reflectance F (thin and solid)
DIR_BOUND = 4 * 3.0e-6        # a component of the refracted or reflected direction
BEER_BOUND = 4 * 1.5e-7       # exp2(-(sigma2 t)) relative, for sigma2 t <= 16


def _dt(a, dt):
    return np.asarray(a, dt)


def fma(a, b, c, dt=F32):
    return _fma(a, b, c, dt)


def dot3(a, b, dt=F32):
    return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0], dt), dt)


def normalize3(a, dt=F32):
    inv = dt(1.0) / np.sqrt(dot3(a, a, dt))
    return a * inv[..., None]


def log2(x):
    """pt_log2 in float32."""
    x = np.ascontiguousarray(x, F32)
    u = x.view(np.uint32)
    e = ((u >> np.uint32(23)) & np.uint32(0xff)).astype(np.int32) - 127
    m = ((u & np.uint32(0x007fffff)) | np.uint32(0x3f800000)).view(F32)
    big = m > F32(1.41421356)
    m = np.where(big, m * F32(0.5), m).astype(F32)
    e = np.where(big, e + 1, e)
    z = (m - F32(1.0)) / (m + F32(1.0))
    z2 = z * z
    p = fma(z2, fma(z2, fma(z2, fma(z2, F32(0.3205989), F32(0.4121984)), F32(0.5770780)), F32(0.9617967)), F32(2.8853901))
    return fma(z, p, e.astype(F32))


def exp2(x):
    """pt_exp2 in float32."""
    x = np.ascontiguousarray(x, F32)
    zero = x < F32(-126.0)
    x = np.where(x > F32(127.0), F32(127.0), x).astype(F32)
    x = np.where(zero, F32(0.0), x).astype(F32)
    fl = np.floor(x)
    f = x - fl
    p = fma(f, fma(f, fma(f, fma(f, fma(f, F32(1.8775767e-3), F32(8.9893397e-3)), F32(5.5826318e-2)), F32(2.4015361e-1)), F32(6.9315308e-1)), F32(9.9999994e-1))
    s = ((fl.astype(np.int32) + 127).astype(np.uint32) << np.uint32(23)).view(F32)
    return np.where(zero, F32(0.0), p * s).astype(F32)


def sigma2(color, distance):
    """pt_glass_sigma2 per channel: -log2(clamp(c, 2^-20, 1)) / distance, 0 where distance is not above 0."""
    c = np.asarray(color, F32)
    c = np.where(c > F32(2.0 ** -20), c, F32(2.0 ** -20)).astype(F32)
    c = np.where(c < F32(1.0), c, F32(1.0)).astype(F32)
    d = F32(distance)
    if not d > 0:
        return np.zeros_like(c)
    return (-log2(c) / d).astype(F32)


class Mat:
    """pt_glass_mat of a material (scene.Material or anything with its fields)."""

    def __init__(self, m=None, **kw):
        g = (lambda k, dflt: kw.get(k, getattr(m, k, dflt)))
        self.tau, self.ior, self.thin = F32(g("transmission", 0.0)), F32(g("ior", 1.5)), bool(g("thin_walled", True))
        self.sigma2 = sigma2(g("attenuation_color", (1.0, 1.0, 1.0)), g("attenuation_distance", 0.0))

    def row(self):
        r = np.zeros(8, F32)
        r[0], r[1], r[4:7] = self.tau, self.ior, self.sigma2
        r[2:3].view(np.int32)[0] = 1 if self.thin else 0
        return r


def tables(tri_mat, materials):
    """(bits, mats (n, 8)) as pt_glass_tables builds them from flat_scene()'s material ids."""
    mats = np.stack([Mat(m).row() for m in materials])
    on = mats[np.asarray(tri_mat, np.int64), 0] > 0
    bits = np.zeros((len(tri_mat) + 31) // 32, np.uint32)
    for p in np.flatnonzero(on):
        bits[p >> 5] |= np.uint32(1 << (p & 31))
    return bits, mats


def prim_is_glass(bits, prim):
    return aref.prim_is_alpha(bits, prim)


def beer(thin, sig2, front, t, T, dt=F32):
    """pt_glass_beer, elementwise over rays: thin (n,), sig2 (n, 3), front (n,), t (n,), T (n, 3).  Returns (T', changed)."""
    sig2, T, t = _dt(sig2, dt), _dt(T, dt), _dt(t, dt)
    on = ~np.asarray(thin, bool) & ~np.asarray(front, bool) & (sig2 != 0).any(-1)
    x = -(sig2 * t[..., None])
    with np.errstate(invalid="ignore", over="ignore"):
        a = exp2(x) if dt is F32 else np.exp2(x)
        out = np.where(on[..., None], T * a, T).astype(dt)
    return out, on


def event(n, d, wo, eta, thin, u_e, dt=F32):
    """pt_glass_event, elementwise: (reflect, d', F)."""
    n, d, wo, eta, u_e = _dt(n, dt), _dt(d, dt), _dt(wo, dt), _dt(eta, dt), _dt(u_e, dt)
    thin = np.asarray(thin, bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ci = dot3(n, wo, dt)
        cos_i = np.where(ci < dt(1.0), ci, dt(1.0)).astype(dt)
        s2 = eta * eta * (dt(1.0) - cos_i * cos_i)
        tir = s2 >= dt(1.0)
        cos_t = np.where(tir, dt(0.0), np.sqrt(np.where(tir, dt(0.0), dt(1.0) - s2))).astype(dt)
        rs = (eta * cos_i - cos_t) / (eta * cos_i + cos_t)
        rp = (cos_i - eta * cos_t) / (cos_i + eta * cos_t)
        F = np.where(tir, dt(1.0), dt(0.5) * (rs * rs + rp * rp)).astype(dt)
        F = np.where(thin, (dt(2.0) * F) / (dt(1.0) + F), F).astype(dt)
        reflect = u_e < F
        dr = fma(n, (dt(2.0) * cos_i)[..., None], d, dt)
        k = (eta * cos_i - cos_t)[..., None]
        dtr = normalize3((d * eta[..., None] + n * k).astype(dt), dt)
        dn = np.where(reflect[..., None], dr, np.where(thin[..., None], d, dtr)).astype(dt)
    return reflect, dn, F


def interact(tau, ior, thin, P, ng, ns, front, base, metallic, ray_eps, u_s, u_e, j, max_interactions, d, T, dt=F32):
    """pt_glass_interact, elementwise over rays.  Returns (outcome (n,), o' (n, 3), d' (n, 3), T' (n, 3), F (n,), fallback (n,) bool: the event was evaluated with ng)."""
    tau, ior, metallic, u_s = _dt(tau, dt), _dt(ior, dt), _dt(metallic, dt), _dt(u_s, dt)
    P, ng, ns, d, T, base = (_dt(x, dt) for x in (P, ng, ns, d, T, base))
    thin, front = np.asarray(thin, bool), np.asarray(front, bool)
    n = len(d)
    p_t = tau * (dt(1.0) - metallic)
    with np.errstate(invalid="ignore"):
        wants = u_s < p_t
    wo = -d
    eta = np.where(thin | front, dt(1.0) / ior, ior).astype(dt)
    r1, d1, F1 = event(ns, d, wo, eta, thin, u_e, dt)
    side = dot3(ng, d1, dt)
    with np.errstate(invalid="ignore"):
        wrong = np.where(r1, ~(side > 0), ~(side < 0))
    r2, d2, F2 = event(ng, d, wo, eta, thin, u_e, dt)
    refl = np.where(wrong, r2, r1)
    dn = np.where(wrong[:, None], d2, d1).astype(dt)
    F = np.where(wrong, F2, F1).astype(dt)
    eps = dt(ray_eps)
    o = np.where(refl[:, None], fma(ng, eps, P, dt), fma(ng, -eps, P, dt)).astype(dt)
    tint = ~refl & (thin | front)
    Tn = np.where(tint[:, None], T * base, T).astype(dt)
    outcome = np.where(~wants, STANDS, np.where(np.asarray(j) == max_interactions, EXHAUSTED, np.where(refl, REFLECT, TRANSMIT)))
    ev = outcome >= REFLECT
    z = np.zeros((n, 3), dt)
    return outcome, np.where(ev[:, None], o, z), np.where(ev[:, None], dn, d).astype(dt), np.where(ev[:, None], Tn, T).astype(dt), np.where(ev, F, dt(0.0)).astype(dt), wrong & ev


# ---- the surface of a hit as k_shade rebuilds it (pt_shading.h): float32, from the committed shading records -------------------------------------------------
def surface32(shade, stride, materials, textures, linear, d, prim, uv):
    """(P, ng, ns, front, base (n, 3), metallic, material id) of the hits (prim (n,), uv (n, 2)) of rays with directions d: lights_reference.punctual_nee's surface."""
    d = np.asarray(d, F32)
    R = np.asarray(shade, F32).reshape(-1, stride * 4)[np.asarray(prim, np.int64)]
    hu, hv = np.asarray(uv, F32)[:, 0], np.asarray(uv, F32)[:, 1]
    hw = F32(1.0) - hu - hv
    Pa, Pb, Pc = R[:, 0:3], R[:, 4:7], R[:, 8:11]
    Na, Nb, Nc = R[:, 11:14], R[:, 14:17], R[:, 17:20]
    bary = lambda a, b, c: _fma(c, hv[:, None], _fma(b, hu[:, None], a * hw[:, None]))
    M, Tx = lref.material_table(materials)
    mat = np.ascontiguousarray(R[:, 3]).view(np.int32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        P = bary(Pa, Pb, Pc)
        ng = lref.normalize3(lref.cross3(Pb - Pa, Pc - Pa))
        ni = bary(Na, Nb, Nc)
        ns = lref.normalize3(ni)
        base = np.concatenate([M[mat, 0:3], M[mat, 8:9]], 1).copy()
        metallic, roughness = M[mat, 3].copy(), M[mat, 7].copy()
        tc, tn, tm = Tx[mat, 0], Tx[mat, 1], Tx[mat, 2]
        if stride == 12:
            X = R[:, 20:44]
            tu = _fma(X[:, 4], hv, _fma(X[:, 2], hu, X[:, 0] * hw))
            tv = _fma(X[:, 5], hv, _fma(X[:, 3], hu, X[:, 1] * hw))
            ti = bary(X[:, 6:9], X[:, 9:12], X[:, 12:15])
            bi = bary(X[:, 15:18], X[:, 18:21], X[:, 21:24])
            for t_id in np.unique(tc[tc >= 0]):
                m = tc == t_id
                base[m] = base[m] * lref.tex_fetch(textures[t_id], tu[m], tv[m], linear)
            for t_id in np.unique(tm[tm >= 0]):
                m = tm == t_id
                metallic[m] = metallic[m] * lref.tex_fetch(textures[t_id], tu[m], tv[m], linear)[:, 2]
            for t_id in np.unique(tn[tn >= 0]):
                m = tn == t_id
                cn = lref.tex_fetch(textures[t_id], tu[m], tv[m], linear)
                nx, ny, nz = (F32(2.0) * cn[:, k:k + 1] - F32(1.0) for k in range(3))
                ns[m] = lref.normalize3(_fma(ti[m], nx, _fma(bi[m], ny, ni[m] * nz)))
        wo = -d
        front = lref.dot3(ng, wo) > 0
        ns = np.where((lref.dot3(ns, ng) < 0)[:, None], -ns, ns)
        ng = np.where(front[:, None], ng, -ng)
        ns = np.where(front[:, None], ns, -ns)
        ns = np.where((lref.dot3(ns, wo) > 0)[:, None], ns, ng)
    return P.astype(F32), ng.astype(F32), ns.astype(F32), front, base[:, 0:3].astype(F32), metallic.astype(F32), mat


MISS = (F32(-1.0), -1, F32(0.0), F32(0.0))


class Scene:
    """What the restatement reads of a committed scene: shading records, materials, textures, filter, ray epsilon, the glass tables; dt = float64 reads the flat
    scene (positions, normals, texture coordinates per vertex) instead of the float32 shading records and supports untextured, flat-or-smooth-shaded glass."""

    def __init__(self, pt, desc):
        self.shade = pt.shading_tables()[0]
        self.stride = self.shade.shape[1] // 4
        self.verts, self.idx, self.tri_mat = pt.flat_scene()
        self.eps = lref.scene_ray_eps(self.verts[:, 0:3])
        self.materials, self.textures = desc.materials, getattr(desc, "textures", [])
        self.linear = getattr(desc, "texture_filter", "nearest") == "linear"
        self.bits, self.mats = tables(self.tri_mat, desc.materials)
        self.alpha = aref.Scene32(pt, desc) if (aref.material_modes(desc.materials)[0] != aref.OPAQUE).any() else None

    def surface(self, d, prim, uv):
        return surface32(self.shade, self.stride, self.materials, self.textures, self.linear, d, prim, uv)


def resolve_closest(sc, trace, o, d, keys, bounce, max_interactions, alpha_layers=8):
    """ptc_debug_glass_closest in float32: (t, prim, uv, o, d, T, pdf word, j, counters dict).  trace(o, d) -> (t, prim, uv) is ptc_debug_trace_closest; a scene with
    alpha materials resolves every segment's hits with alpha_reference.resolve_closest, as the library does."""
    o, d, keys = np.array(o, F32), np.array(d, F32), np.asarray(keys, np.uint32)
    n = len(o)
    b = int(bounce)

    def traced(oo, dd, kk, alpha_bounce):
        if sc.alpha is None:
            return tuple(x.copy() for x in trace(oo, dd))
        return aref.resolve_closest(sc.alpha, trace, oo, dd, kk, alpha_bounce, alpha_layers)[:3]

    t, prim, uv = traced(o, d, keys, b)
    T = np.ones((n, 3), F32)
    pdf = np.ones(n, F32)
    jn = np.zeros(n, np.uint32)
    cnt = dict(reflections=0, refractions=0, standing=0, exhausted=0)
    live = np.arange(n)
    ct, cp, cuv = t.copy(), prim.copy(), uv.copy()
    j = 0
    while len(live):
        hit = cp >= 0
        decide = hit.copy()
        decide[hit] = prim_is_glass(sc.bits, cp[hit])
        outcome = np.full(len(live), STANDS)
        no, nd, nT = o[live].copy(), d[live].copy(), T[live].copy()
        if decide.any():
            P, ng, ns, front, base, metallic, mat = sc.surface(d[live][decide], cp[decide], cuv[decide])
            g = sc.mats[mat]
            thin = np.ascontiguousarray(g[:, 2]).view(np.int32) != 0
            Tb, _ = beer(thin, g[:, 4:7], front, ct[decide], nT[decide])
            idx = RNG_BASE + (b + 1) * 64 + j
            kk = keys[live][decide]
            oc, o2, d2, T2, _, _ = interact(g[:, 0], g[:, 1], thin, P, ng, ns, front, base, metallic, sc.eps, rng_f(kk, idx, 0), rng_f(kk, idx, 1), j, max_interactions, nd[decide], Tb)
            ev = oc >= REFLECT
            outcome[decide] = oc
            sub = np.flatnonzero(decide)
            no[sub[ev]] = o2[ev]
            nd[sub] = d2
            nT[sub] = T2
            cnt["reflections"] += int((oc == REFLECT).sum()); cnt["refractions"] += int((oc == TRANSMIT).sum())
        go = outcome >= REFLECT
        exh = outcome == EXHAUSTED
        done = ~go
        s = live[done]
        if j > 0:
            t[s], prim[s], uv[s] = ct[done], cp[done], cuv[done]
            t[live[exh]], prim[live[exh]], uv[live[exh]] = MISS[0], MISS[1], (MISS[2], MISS[3])
            nT[exh] = 0
            o[s], d[s], T[s], pdf[s], jn[s] = no[done], nd[done], nT[done], DELTA_PDF, j
            cnt["standing"] += int((done & ~exh).sum()); cnt["exhausted"] += int(exh.sum())
        else:
            T[s] = nT[done]
        live = live[go]
        if not len(live):
            break
        o[live], d[live], T[live] = no[go], nd[go], nT[go]
        ct, cp, cuv = traced(o[live], d[live], keys[live], 0x01000000 + (b + 1) * 64 + j)
        j += 1
    return t, prim, uv, o, d, T, pdf, jn, cnt


def trace32(sc):
    """trace(o, d) -> (t, prim, uv) with ptc_debug_trace_closest's conventions (a miss is MISS), by Möller–Trumbore in float32 of every ray against EVERY triangle of the
    flat scene: no tree, no device.  The nearest hit with t > 0 inside the triangle (edge margin >= 0)."""
    a, b, c = (x.astype(F32) for x in tref.triangles(sc.verts, sc.idx))

    def trace(o, d):
        o, d = np.asarray(o, F32), np.asarray(d, F32)
        t, u, v, m, _, _ = tref.pair_terms(a[None], b[None], c[None], o[:, None], d[:, None], F32)
        with np.errstate(invalid="ignore"):
            ts = np.where((m >= 0) & (t > 0) & np.isfinite(t), t, np.inf)
        k = ts.argmin(1)
        r = np.arange(len(o))
        hit = np.isfinite(ts[r, k])
        uv = np.where(hit[:, None], np.stack([u[r, k], v[r, k]], 1), F32(0.0)).astype(F32)
        return np.where(hit, ts[r, k], MISS[0]).astype(F32), np.where(hit, k, MISS[1]).astype(np.int32), uv

    return trace


# ---- float64: the independent walk ---------------------------------------------------------------------------------------------------------------------------
EDGE_MARGIN = 1e-4
T_MARGIN = 1e-5


def walk64(sc, o, d, keys, bounce, max_interactions):
    """Per ray, in float64 throughout: the nearest hit of ALL triangles (t > 0) from the current origin, the surface from the flat scene's vertices (interpolated
    normals, no textures: the scenes this is used on have untextured glass), Beer, the choice and the event with the SAME random numbers.  Returns
    (t, prim, o, d, T, j, exhausted, undecided): prim -1 on a miss.  A ray is undecided when a hit it took lies within EDGE_MARGIN of a triangle edge or a second
    candidate within T_MARGIN relative in t, when u_s lies within F_BOUND of p_t or u_e within F_BOUND of F, or when the event fell back to ng.

    It also carries, per ray, how far a float32 evaluation of the same walk may lie from it, to first order, for flat-shaded glass (e_o, e_d, e_t, e_T in the result):
      a hit:    e_hit = (e_o + t e_d) / c + 8 2^-23 R    the origin's and the direction's error projected along the ray onto the plane, c = |ng . d|, plus the
                                                         rounding of the float32 trace and of P (R = |o_0| + path length so far bounds every coordinate);  e_t = e_hit + e_o
      an event: e_o = e_hit + ray_eps;  e_d = g e_d + DIR_BOUND with g = max(1, eta, eta cos_i / cos_t) for a refraction (Snell's law differentiated; eta itself
                for a perturbation out of the plane of incidence) and 1 for a reflection or a thin pane;  e_T (relative) grows by 2^-23 for the tint and by
                BEER_BOUND + 2^-23 + ln 2 max(sigma2) e_t where Beer applied."""
    V = np.asarray(sc.verts)
    Pv, Nv = V[:, 0:3].astype(F64), V[:, 3:6].astype(F64)
    idx = np.asarray(sc.idx).reshape(-1, 3).astype(np.int64)
    A, B, C = Pv[idx[:, 0]], Pv[idx[:, 1]], Pv[idx[:, 2]]
    M, _ = lref.material_table(sc.materials)
    n = len(o)
    b = int(bounce)
    out = dict(t=np.full(n, np.inf), prim=np.full(n, -1, np.int64), o=np.array(o, F64), d=np.array(d, F64), T=np.ones((n, 3)), j=np.zeros(n, np.int64),
               exhausted=np.zeros(n, bool), undecided=np.zeros(n, bool), e_o=np.zeros(n), e_d=np.zeros(n), e_t=np.zeros(n), e_T=np.zeros(n))
    eps = float(sc.eps)
    ulp8 = 8 * 2.0 ** -23
    for r in range(n):
        oo, dd, T = np.array(o[r], F64), np.array(d[r], F64), np.ones(3)
        j = 0
        e_o = e_d = e_t = e_T = 0.0
        reach = float(np.linalg.norm(oo))
        while True:
            t, u, v, m, _, _ = tref.pair_terms(A, B, C, oo[None], dd[None])
            with np.errstate(invalid="ignore"):
                cand = np.flatnonzero((m > -EDGE_MARGIN) & (t > 0) & np.isfinite(t))
            cand = cand[np.lexsort((cand, t[cand]))]
            cand_in = [p for p in cand if m[p] >= 0]
            if not cand_in:
                if len(cand):
                    out["undecided"][r] = True
                out["t"][r], out["prim"][r] = np.inf, -1
                break
            p = cand_in[0]
            k = list(cand).index(p)
            if abs(m[p]) <= EDGE_MARGIN or k > 0 or (k + 1 < len(cand) and t[cand[k + 1]] - t[p] <= T_MARGIN * max(t[p], 1.0)):
                out["undecided"][r] = True
            out["t"][r], out["prim"][r] = t[p], p
            ng = np.cross(B[p] - A[p], C[p] - A[p]); ng /= np.linalg.norm(ng)
            reach += t[p]
            e_hit = (e_o + t[p] * e_d) / abs(ng @ dd) + ulp8 * reach
            e_t = e_hit + e_o
            g = Mat(sc.materials[int(sc.tri_mat[p])])
            if not g.tau > 0:
                break
            w0 = 1.0 - u[p] - v[p]
            P = A[p] * w0 + B[p] * u[p] + C[p] * v[p]
            ns = Nv[idx[p, 0]] * w0 + Nv[idx[p, 1]] * u[p] + Nv[idx[p, 2]] * v[p]; ns /= np.linalg.norm(ns)
            wo = -dd
            front = ng @ wo > 0
            if ns @ ng < 0: ns = -ns
            if not front: ng, ns = -ng, -ns
            if not ns @ wo > 0: ns = ng
            mrow = M[int(sc.tri_mat[p])]
            T, attenuated = beer(np.array([g.thin]), g.sigma2[None].astype(F64), np.array([front]), np.array([t[p]]), T[None], F64)
            T = T[0]
            if attenuated[0]:
                e_T += BEER_BOUND + 2.0 ** -23 + np.log(2.0) * float(g.sigma2.max()) * e_t
            ix = RNG_BASE + (b + 1) * 64 + j
            u_s, u_e = float(rng_f(keys[r:r + 1], ix, 0)[0]), float(rng_f(keys[r:r + 1], ix, 1)[0])
            oc, o2, d2, T2, F, fb = interact([float(g.tau)], [float(g.ior)], [g.thin], P[None], ng[None], ns[None], [front], mrow[None, 0:3].astype(F64), [float(mrow[3])],
                                             eps, [u_s], [u_e], j, max_interactions, dd[None], T[None], F64)
            p_t = float(g.tau) * (1.0 - float(mrow[3]))
            if abs(u_s - p_t) <= F_BOUND and 0.0 < p_t < 1.0:
                out["undecided"][r] = True
            if oc[0] == STANDS:
                break
            if oc[0] == EXHAUSTED:
                out["exhausted"][r] = True
                out["t"][r], out["prim"][r] = -1.0, -1
                T = np.zeros(3)
                break
            if abs(u_e - F[0]) <= F_BOUND or fb[0]:
                out["undecided"][r] = True
            gain = 1.0
            if oc[0] == TRANSMIT and not g.thin:
                n_ev = ng if fb[0] else ns
                eta = 1.0 / float(g.ior) if front else float(g.ior)
                gain = max(1.0, eta, eta * abs(n_ev @ dd) / abs(n_ev @ d2[0]))
            e_o, e_d, e_T = e_hit + eps, gain * e_d + DIR_BOUND, e_T + 2.0 ** -23
            oo, dd, T = o2[0], d2[0], T2[0]
            j += 1
        out["o"][r], out["d"][r], out["T"][r], out["j"][r] = oo, dd, T, j
        out["e_o"][r], out["e_d"][r], out["e_t"][r], out["e_T"][r] = e_o, e_d, e_t, e_T
    return out


def check_against_walk64(res, w, what):
    """A float32 resolution `res` = (t, prim, uv, o, d, T, pdf word, j, ...), resolve_closest's or ptc_debug_glass_closest's, against walk64's result `w` of the same
    rays and keys.  On every ray walk64 decides: the same final primitive, the same number of events, exhausted alike, and t, o, d and T within walk64's own
    error bounds; a ray without an event keeps o and d exactly.  Returns (rays compared, the worst ratio error / bound of t, o, d, T)."""
    t, prim, _, o, d, T, _, j = (np.asarray(x) for x in res[:8])
    ok = ~w["undecided"]
    k = np.flatnonzero(ok)
    bad = k[(prim[k] != w["prim"][k]) | (j[k] != w["j"][k])]
    assert not len(bad), f"{what}: rays {bad[:8].tolist()}: prim {prim[bad[:8]].tolist()} j {j[bad[:8]].tolist()}, float64 has prim {w['prim'][bad[:8]].tolist()} j {w['j'][bad[:8]].tolist()}"
    exh = w["exhausted"][k]
    assert (t[k][exh] == MISS[0]).all() and not T[k][exh].any(), what
    ratio = {}
    hit = k[w["prim"][k] >= 0]
    tiny = 1e-300
    ratio["t"] = np.abs(t[hit].astype(F64) - w["t"][hit]) / (w["e_t"][hit] + tiny)
    assert (t[k][(w["prim"][k] < 0)] == MISS[0]).all(), what
    ev = k[w["j"][k] > 0]
    still = k[w["j"][k] == 0]
    assert np.array_equal(o[still].astype(F64), w["o"][still]) and np.array_equal(d[still].astype(F64), w["d"][still]), what
    ratio["o"] = np.abs(o[ev].astype(F64) - w["o"][ev]).max(1) / w["e_o"][ev]
    ratio["d"] = np.abs(d[ev].astype(F64) - w["d"][ev]).max(1) / w["e_d"][ev]
    live = k[~exh]
    ratio["T"] = np.abs(T[live].astype(F64) / w["T"][live] - 1.0).max(1) / (w["e_T"][live] + tiny)
    worst = {n: float(v.max()) if len(v) else 0.0 for n, v in ratio.items()}
    assert all(v <= 1.0 for v in worst.values()), f"{what}: error / bound {worst}"
    return len(k), worst


# ---- the ray sets of the resolution tests (test_glass_host.py runs them on walk64 alone, test_gpu_glass.py on the device) ---------------------------------
SEED = 0x61A55C0FFEE12345
RAY_COUNTS = (1, 63, 64, 65, 513)
MAX_UNDECIDED = 0.02
MAX_EXHAUSTED = 0.01


def ray_sets(pt, counts=RAY_COUNTS):
    """(n, origins, dirs, keys) per count: camera rays of a 24x24 frame of the context's camera in a random order, with random keys; in the larger sets every
    seventh ray is turned away so that misses interleave.  1, 63, 64, 65 sit on and around a wave; 513 rays are two segments (PTC_SEG_MIN_LEN = 512)."""
    o_all, d_all = pt.debug_camera_rays(24, 24, SEED, 0, 1)
    rng = np.random.default_rng(23)
    for n in counts:
        sel = rng.permutation(len(o_all))[:n] if n > 1 else np.array([len(o_all) // 2 + 12])
        o, d = o_all[sel].copy(), d_all[sel].copy()
        if n > 1:
            away = np.arange(n) % 7 == 3
            d[away] = -d[away]
        yield n, o, d, rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
