"""numpy restatement of transparent shadows (csrc/pt_glass_shadow.h, csrc/pt_glass_shadow.hip, k_glass_filter<.., true> of csrc/pt_glass.hip), for
tests/test_glass_shadows_host.py and tests/test_gpu_glass_shadows.py.  It builds on glass_reference.py and alpha_reference.py and changes neither.

Parts:
  transmit                  pt_glass_shadow_transmit, elementwise; dt = float32 follows the source operation for operation (bit for bit), float64 the same formulas
  resolve_any               the rounds of k_glass_filter_shadow in float32: (Tr (n, 3), surfaces passed, counters) as ptc_debug_glass_any and ptc_get_glass_shadow_stats
                            give them; the candidate hits come from a `trace(o, d)` callable, the coarse flags from `trace_any(o, d, tmax)`
  resolve_closest           glass_reference.resolve_closest with the MIS bookkeeping of a frame with transparent shadows: a ray that only went straight through thin
                            panes keeps the pdf word, o and d of its source and gets t_out = dot3(o' - o_src, d) + t
  walk64_any                the independent shadow walk in float64 with a search of all triangles of its own; it says which records the two precisions need not
                            agree about and carries a first-order error bound on Tr per record"""
import numpy as np

import alpha_reference as aref
import glass_reference as gref
import lights_reference as lref
import trace_reference as tref
from lens_reference import F32, F64, rng_f

RAY_COUNTS = gref.RAY_COUNTS
MAX_UNDECIDED = 0.02


def transmit(tau, ior, thin, ng, ns, d, base, metallic, dt=F32):
    """pt_glass_shadow_transmit, elementwise over hits.  Returns (W (n, 3), F_t (n,), fallback (n,): the reflection about ns would not leave on ng's side)."""
    tau, ior, metallic = (np.asarray(x, dt) for x in (tau, ior, metallic))
    ng, ns, d, base = (np.asarray(x, dt) for x in (ng, ns, d, base))
    thin = np.asarray(thin, bool)
    n = len(d)
    always = np.full(n, -1.0, dt)                                     # u_e = -1: the event reflects, so d' is the reflection about the normal
    on = np.ones(n, bool)
    eta = dt(1.0) / ior
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        arrives = gref.dot3(ng, d, dt) < 0
        p_t = tau * (dt(1.0) - metallic)
        _, d_r, F_s = gref.event(ns, d, -d, eta, on, always, dt)
        _, _, F_g = gref.event(ng, d, -d, eta, on, always, dt)
        fallback = ~(gref.dot3(ng, d_r, dt) > 0)
        F_t = np.where(fallback, np.where(F_s < F_g, F_s, F_g), F_s).astype(dt)
        s = p_t * (dt(1.0) - F_t)
        W = (s[:, None] * base).astype(dt)
    ok = thin & arrives
    return np.where(ok[:, None], W, dt(0.0)).astype(dt), np.where(ok, F_t, dt(0.0)).astype(dt), fallback & ok


def rounds_limit(max_interactions, max_layers, has_alpha):
    """L of pt_glass_shadow.h."""
    return max(int(max_interactions), int(max_layers)) if has_alpha else int(max_interactions)


def resolve_any(sc, trace, trace_any, o, d, tmax, L):
    """ptc_debug_glass_any in float32: (Tr (n, 3), layers (n,), counters).  sc: a glass_reference.Scene (sc.alpha is its alpha scene or None); trace(o, d) ->
    (t, prim, uv) is ptc_debug_trace_closest (or gref.trace32), trace_any(o, d, tmax) the coarse flag of ptc_debug_trace_any."""
    o, d, tmax = np.asarray(o, F32), np.asarray(d, F32), np.asarray(tmax, F32)
    n = len(o)
    out, layers = np.zeros((n, 3), F32), np.zeros(n, np.uint32)
    flag = np.asarray(trace_any(o, d, tmax)) != 0
    out[~flag] = 1.0
    live = np.flatnonzero(flag)
    cnt = dict(walked=len(live), passes=0, visible=0, exhausted=0)
    co, rem, Tr = o[live].copy(), tmax[live].copy(), np.ones((len(live), 3), F32)
    k = 0
    while len(live):
        ct, cp, cuv = trace(co, d[live])
        with np.errstate(invalid="ignore"):
            visible = (cp < 0) | ~(ct < rem)
        out[live[visible]], layers[live[visible]] = Tr[visible], k
        cnt["visible"] += int(visible.sum())
        blocked = ~visible
        is_alpha, is_glass = np.zeros(len(live), bool), np.zeros(len(live), bool)
        if sc.alpha is not None:
            is_alpha[blocked] = aref.prim_is_alpha(sc.alpha.bits, cp[blocked])
        is_glass[blocked] = gref.prim_is_glass(sc.bits, cp[blocked]) & ~is_alpha[blocked]
        W = np.zeros((len(live), 3), F32)
        onward = np.zeros((len(live), 3), F32)
        if is_alpha.any():
            a, mat, op = sc.alpha.surface(d[live][is_alpha], cp[is_alpha], cuv[is_alpha])
            W[is_alpha] = aref.transmit(sc.alpha.mode[mat], sc.alpha.cutoff[mat], a)[:, None]
            onward[is_alpha] = op
        if is_glass.any():
            dd = d[live][is_glass]
            P, ng, ns, _, base, metallic, mat = sc.surface(dd, cp[is_glass], cuv[is_glass])
            g = sc.mats[mat]
            thin = np.ascontiguousarray(g[:, 2]).view(np.int32) != 0
            W[is_glass] = transmit(g[:, 0], g[:, 1], thin, ng, ns, dd, base, metallic)[0]
            onward[is_glass] = gref.fma(ng, -F32(sc.eps), P)
        Tr = (Tr * W).astype(F32)
        dark = ~Tr.any(1)
        exhausted = blocked & ~dark & (k == L)
        cnt["exhausted"] += int(exhausted.sum())
        passing = blocked & ~dark & (k != L)
        cnt["passes"] += int(passing.sum())
        live, co, rem, Tr = live[passing], onward[passing], (rem[passing] - ct[passing]).astype(F32), Tr[passing]
        k += 1
    return out, layers, cnt


def resolve_closest(sc, trace, o, d, keys, bounce, max_interactions, shadows=True, alpha_layers=8):
    """ptc_debug_glass_closest of a context with transparent shadows on, in float32: (t, prim, uv, o, d, T, pdf word, j, counters), as gref.resolve_closest.  The rounds
    are gref.resolve_closest's; what differs is what a ray that only went straight through thin panes leaves the pass with.  shadows=False is gref.resolve_closest."""
    if not shadows:
        return gref.resolve_closest(sc, trace, o, d, keys, bounce, max_interactions, alpha_layers)
    o_src, d_src, keys = np.array(o, F32), np.array(d, F32), np.asarray(keys, np.uint32)
    n = len(o_src)
    b = int(bounce)

    def traced(oo, dd, kk, alpha_bounce):
        if sc.alpha is None:
            return tuple(x.copy() for x in trace(oo, dd))
        return aref.resolve_closest(sc.alpha, trace, oo, dd, kk, alpha_bounce, alpha_layers)[:3]

    t, prim, uv = traced(o_src, d_src, keys, b)
    o, d = o_src.copy(), d_src.copy()                               # the ray records the pass leaves
    co, cd = o_src.copy(), d_src.copy()                             # the current segment of every ray
    T = np.ones((n, 3), F32)
    pdf = np.ones(n, F32)
    jn = np.zeros(n, np.uint32)
    bent = np.zeros(n, bool)
    cnt = dict(reflections=0, refractions=0, standing=0, exhausted=0)
    live = np.arange(n)
    ct, cp, cuv = t.copy(), prim.copy(), uv.copy()
    j = 0
    while len(live):
        hit = cp >= 0
        decide = hit.copy()
        decide[hit] = gref.prim_is_glass(sc.bits, cp[hit])
        outcome = np.full(len(live), gref.STANDS)
        no, nd, nT = co[live].copy(), cd[live].copy(), T[live].copy()
        if decide.any():
            P, ng, ns, front, base, metallic, mat = sc.surface(nd[decide], cp[decide], cuv[decide])
            g = sc.mats[mat]
            thin = np.ascontiguousarray(g[:, 2]).view(np.int32) != 0
            Tb, _ = gref.beer(thin, g[:, 4:7], front, ct[decide], nT[decide])
            idx = gref.RNG_BASE + (b + 1) * 64 + j
            kk = keys[live][decide]
            oc, o2, d2, T2, _, _ = gref.interact(g[:, 0], g[:, 1], thin, P, ng, ns, front, base, metallic, sc.eps, rng_f(kk, idx, 0), rng_f(kk, idx, 1), j, max_interactions, nd[decide], Tb)
            ev = oc >= gref.REFLECT
            outcome[decide] = oc
            sub = np.flatnonzero(decide)
            no[sub[ev]] = o2[ev]
            nd[sub] = d2
            nT[sub] = T2
            bent[live[sub]] |= (oc == gref.REFLECT) | ((oc == gref.TRANSMIT) & ~thin)
            cnt["reflections"] += int((oc == gref.REFLECT).sum()); cnt["refractions"] += int((oc == gref.TRANSMIT).sum())
        go = outcome >= gref.REFLECT
        exh = outcome == gref.EXHAUSTED
        done = ~go
        s = live[done]
        if j > 0:
            t[s], prim[s], uv[s] = ct[done], cp[done], cuv[done]
            t[live[exh]], prim[live[exh]], uv[live[exh]] = gref.MISS[0], gref.MISS[1], (gref.MISS[2], gref.MISS[3])
            nT[exh] = 0
            T[s], jn[s] = nT[done], j
            turned = bent[s]
            o[s[turned]], d[s[turned]], pdf[s[turned]] = no[done][turned], nd[done][turned], gref.DELTA_PDF
            far = ~turned & (prim[s] >= 0)                          # it went straight on: o, d and the pdf word stay; the hit's t counts from the source origin
            t[s[far]] = (gref.dot3((no[done][far] - o_src[s[far]]).astype(F32), nd[done][far]) + ct[done][far]).astype(F32)
            cnt["standing"] += int((done & ~exh).sum()); cnt["exhausted"] += int(exh.sum())
        else:
            T[s] = nT[done]
        live = live[go]
        if not len(live):
            break
        co[live], cd[live], T[live] = no[go], nd[go], nT[go]
        ct, cp, cuv = traced(co[live], cd[live], keys[live], 0x01000000 + (b + 1) * 64 + j)
        j += 1
    return t, prim, uv, o, d, T, pdf, jn, cnt


# ---- float64: the independent shadow walk ---------------------------------------------------------------------------------------------------------------------
EDGE_MARGIN = 1e-4
T_MARGIN = 1e-5


def walk64_any(sc, o, d, tmax, L, linear=False):
    """Per shadow record, in float64 throughout: the nearest hit of ALL triangles (t > 0) from the current origin, alpha's coverage from the flat scene's texture
    coordinates (alpha_reference._alpha64), the pane's W from the flat scene's interpolated normals and the material's base colour (untextured panes), walked by the
    rule of pt_glass_shadow.h.  Returns dict(Tr (n, 3), layers, visible, exhausted, undecided, e_Tr: the relative first-order bound of a float32 walk's Tr).
    A record is undecided when a hit it took lies within EDGE_MARGIN in barycentrics of a triangle edge (or a near miss within it), a second candidate lies
    within T_MARGIN relative in t, a hit's t lies within T_MARGIN max(t, 1) + the origin's shift of rem, an alpha lookup lies within alpha_reference's margins of a
    texel edge or the cutoff, or the pane's ng fallback applied.
    The bound: a surface passed multiplies Tr by W_c = p_t (1 - F_t) base_c; the float32 F_t lies within gref.F_BOUND of the float64 one (rounding only,
    test_glass_host.py::test_float32_against_float64), and within a further 16 |grad ns| x the hit point's shift where the vertex normals vary over the pane
    (the walk's origins lie ray_eps off each surface passed, which moves a slanted ray's later hits sideways by less than (k + 1) ray_eps), so the relative
    error grows by (F_BOUND + 16 g (k + 1) ray_eps) / (1 - F_t) + 4 x 2^-23 per pane, g = 1 bounding |grad ns| per unit length of the test scenes' tilted panes;
    an alpha surface's transmit is exact where the texel is decided (NEAREST), + 2^-23 for the product."""
    V = np.asarray(sc.verts)
    Pv, Nv, UV = V[:, 0:3].astype(F64), V[:, 3:6].astype(F64), V[:, 10:12].astype(F64)
    idx = np.asarray(sc.idx).reshape(-1, 3).astype(np.int64)
    A, B, C = Pv[idx[:, 0]], Pv[idx[:, 1]], Pv[idx[:, 2]]
    M, Tx = lref.material_table(sc.materials)
    mode, cutoff = aref.material_modes(sc.materials)
    n = len(o)
    eps = float(sc.eps)
    out = dict(Tr=np.zeros((n, 3)), layers=np.zeros(n, np.int64), visible=np.zeros(n, bool), exhausted=np.zeros(n, bool), undecided=np.zeros(n, bool), e_Tr=np.zeros(n))
    for r in range(n):
        oo, dd, rem = np.array(o[r], F64), np.array(d[r], F64), float(tmax[r])
        Tr, k, e, shift = np.ones(3), 0, 0.0, 0.0
        while True:
            t, u, v, m, _, _ = tref.pair_terms(A, B, C, oo[None], dd[None])
            with np.errstate(invalid="ignore"):
                cand = np.flatnonzero((m > -EDGE_MARGIN) & (t > 0) & np.isfinite(t))
            cand = cand[np.lexsort((cand, t[cand]))]
            cand_in = [p for p in cand if m[p] >= 0]
            near_rem = lambda tt: abs(tt - rem) <= T_MARGIN * max(tt, 1.0) + 2.0 * shift
            if any(near_rem(t[p]) or (t[p] < rem and m[p] < 0) for p in cand):
                out["undecided"][r] = True
            if not cand_in or not t[cand_in[0]] < rem:
                out["Tr"][r], out["layers"][r], out["visible"][r] = Tr, k, True
                break
            p = cand_in[0]
            q = list(cand).index(p)
            if abs(m[p]) <= EDGE_MARGIN or q > 0 or (q + 1 < len(cand) and t[cand[q + 1]] - t[p] <= T_MARGIN * max(t[p], 1.0)):
                out["undecided"][r] = True
            mat = int(sc.tri_mat[p])
            w0 = 1.0 - u[p] - v[p]
            ng = np.cross(B[p] - A[p], C[p] - A[p]); ng /= np.linalg.norm(ng)
            P = A[p] * w0 + B[p] * u[p] + C[p] * v[p]
            g = gref.Mat(sc.materials[mat])
            if mode[mat] != aref.OPAQUE:
                a = float(M[mat, 8])
                if Tx[mat, 0] >= 0:
                    tu, tv = UV[idx[p, 0]] * w0 + UV[idx[p, 1]] * u[p] + UV[idx[p, 2]] * v[p]
                    ta, edge = aref._alpha64(sc.textures[Tx[mat, 0]], tu, tv, linear)
                    a *= ta
                    if edge <= aref.TEXEL_MARGIN:
                        out["undecided"][r] = True
                if mode[mat] == aref.MASK and abs(a - float(cutoff[mat])) <= aref.CUTOFF_MARGIN:
                    out["undecided"][r] = True
                W = np.full(3, float(aref.transmit(int(mode[mat]), float(cutoff[mat]), F32(a))) if mode[mat] == aref.MASK else 1.0 - min(max(a, 0.0), 1.0))
                nn = ng if ng @ dd > 0 else -ng
                onward = P + eps * nn
                e += 2.0 ** -23
            elif g.tau > 0:
                ns = Nv[idx[p, 0]] * w0 + Nv[idx[p, 1]] * u[p] + Nv[idx[p, 2]] * v[p]; ns /= np.linalg.norm(ns)
                wo = -dd
                if ns @ ng < 0: ns = -ns
                if not ng @ wo > 0: ng, ns = -ng, -ns
                if not ns @ wo > 0: ns = ng
                Wv, F_t, fb = transmit([float(g.tau)], [float(g.ior)], [g.thin], ng[None], ns[None], dd[None], M[mat, 0:3].astype(F64)[None], [float(M[mat, 3])], F64)
                W = Wv[0]
                if fb[0]:
                    out["undecided"][r] = True
                onward = P - eps * ng
                e += (gref.F_BOUND + 16.0 * (k + 1) * eps) / max(1.0 - float(F_t[0]), 1e-30) + 4 * 2.0 ** -23
            else:
                W = np.zeros(3)
                onward = P
            Tr = Tr * W
            if not Tr.any():
                break
            if k == L:
                out["exhausted"][r] = True
                break
            oo, rem, k, shift = onward, rem - t[p], k + 1, shift + eps
        out["e_Tr"][r] = e
    return out


def check_against_walk64(Tr, layers, w, what):
    """A float32 shadow resolution (Tr (n, 3), layers) against walk64_any's result of the same records: on every record the walk decides, visible or occluded alike,
    the same number of surfaces passed, and every channel of Tr within the walk's relative bound.  Returns (records compared, the worst error / bound)."""
    Tr, layers = np.asarray(Tr, F64), np.asarray(layers)
    k = np.flatnonzero(~w["undecided"])
    vis = w["visible"][k]
    lit = Tr[k].any(1)
    bad = k[(lit != (vis & w["Tr"][k].any(1))) | (vis & (layers[k] != w["layers"][k]))]
    assert not len(bad), f"{what}: records {bad[:8].tolist()}: Tr {Tr[bad[:8]].tolist()} layers {layers[bad[:8]].tolist()}, float64 has {w['Tr'][bad[:8]].tolist()} {w['layers'][bad[:8]].tolist()}"
    assert not Tr[k[~vis]].any(), what
    v = k[vis & lit]
    passed = v[w["layers"][v] > 0]
    free = v[w["layers"][v] == 0]
    assert (Tr[free] == 1.0).all(), what
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(np.where(w["Tr"][passed] > 0, Tr[passed] / w["Tr"][passed] - 1.0, Tr[passed])).max(1) if len(passed) else np.zeros(0)
    ratio = rel / w["e_Tr"][passed] if len(passed) else np.zeros(0)
    worst = float(ratio.max()) if len(ratio) else 0.0
    assert worst <= 1.0, f"{what}: error / bound {worst}"
    return len(k), worst


def shadow_sets(pt, counts=RAY_COUNTS, seed=31):
    """(n, origins, dirs, tmax) per count: shadow records that start on the floor under the glass and aim at random points of the plane y = 4.5 above it (tmax the
    distance to that point), so that they cross every pane and sheet of the test scenes inside its outline; every fifth record is cut short at 0.2 (it ends
    before any surface: visible, Tr = 1) and every seventh aims below the horizon into the floor's side (a miss or the floor itself)."""
    rng = np.random.default_rng(seed)
    for n in counts:
        o = np.stack([rng.uniform(-1.2, 1.2, n), np.full(n, 0.01), rng.uniform(-1.2, 1.2, n)], 1).astype(F32)
        target = np.stack([rng.uniform(-1.5, 1.5, n), np.full(n, 4.5), rng.uniform(-1.5, 1.5, n)], 1)
        v = target - o
        dist = np.linalg.norm(v, axis=1)
        d = (v / dist[:, None]).astype(F32)
        tmax = dist.astype(F32)
        if n > 1:
            tmax[np.arange(n) % 5 == 2] = F32(0.2)
            down = np.arange(n) % 7 == 3
            d[down, 1] = -d[down, 1]
        yield n, o, d, tmax


def record_scenes(pbr, filt="nearest"):
    """name -> description of the scenes the record sets are resolved in: one pane; a textured, tinted pane; three panes with tilted vertex normals; a pane over a
    BLEND and a MASK sheet; a solid slab (every record that meets it is occluded)."""
    S = pbr.scenes
    return {"pane": S.glass_panes(1, transmission=0.9, texture_filter=filt),
            "textured": S.glass_panes(1, base=(1.0, 0.9, 0.8), textured=True, texture_filter=filt),
            "stack3": S.glass_panes(3, tilt=0.4, ior=1.33, texture_filter=filt),
            "mixed": S.glass_panes(1, sheets=("blend", "mask"), texture_filter=filt),
            "solid": S.glass_slab(thin=False, base=(0.9, 0.8, 0.7), texture_filter=filt)}


def any32(sc):
    """trace_any(o, d, tmax) -> flag, by a float32 search of all triangles (gref.trace32's pairs): does anything lie in (0, tmax)?  What tests without a device use
    for the coarse flag; it only decides whether a record is walked."""
    a, b, c = (x.astype(F32) for x in tref.triangles(sc.verts, sc.idx))

    def trace_any(o, d, tmax):
        o, d = np.asarray(o, F32), np.asarray(d, F32)
        t, _, _, m, _, _ = tref.pair_terms(a[None], b[None], c[None], o[:, None], d[:, None], F32)
        with np.errstate(invalid="ignore"):
            return ((m >= 0) & (t > 0) & (t < np.asarray(tmax, F32)[:, None])).any(1)

    return trace_any
