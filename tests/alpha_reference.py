"""numpy restatement of alpha coverage (csrc/pt_alpha.h, csrc/pt_alpha.hip), for tests/test_alpha_host.py and tests/test_gpu_alpha.py.

Three parts:
  accept / transmit / tables     pt_alpha_accept, pt_alpha_transmit and the tables the commit builds (bit table per primitive, (mode, cutoff) per material), float32
  resolve_closest / resolve_any  the rounds of k_alpha_filter_closest and of alpha's shadow walk (k_glass_filter_shadow of csrc/pt_glass_shadow.hip without a glass table) in
                                 float32, bit for bit: the candidate hits come from a `trace(o, d)` callable (the library's own
                                 ptc_debug_trace_closest), the decision, the onward origin o' and t_base are restated here
  walk_closest                   the INDEPENDENT reference: a float64 search of all triangles per ray, sorted by (t, primitive id), walked with the same decision
                                 rule; it also says which rays float32 and float64 need not agree about (`undecided`)."""
import numpy as np

import lights_reference as lref
import trace_reference as tref
from lens_reference import F32, F64, _fma, rng_f

OPAQUE, MASK, BLEND = 0, 1, 2
RNG_BASE = 0x20000000
_MODES = {"opaque": OPAQUE, "mask": MASK, "blend": BLEND}


def mode_of(m):
    return _MODES[m.lower()] if isinstance(m, str) else int(m)


def accept(mode, cutoff, a, u):
    """pt_alpha_accept, elementwise (float32 comparisons)."""
    mode, cutoff, a, u = np.broadcast_arrays(np.asarray(mode), np.asarray(cutoff, F32), np.asarray(a, F32), np.asarray(u, F32))
    with np.errstate(invalid="ignore"):
        return np.where(mode == MASK, a >= cutoff, np.where(mode == BLEND, u < a, True))


def accept_deterministic(mode, cutoff, a):
    mode = np.asarray(mode)
    return accept(np.where(mode == BLEND, MASK, mode), np.where(mode == BLEND, F32(0.5), np.asarray(cutoff, F32)), a, F32(0.0))


def transmit(mode, cutoff, a):
    """pt_alpha_transmit, elementwise: fmax2(a, 0) = a > 0 ? a : 0 and fmin2(x, 1) = x < 1 ? x : 1, so a NaN alpha clamps to 0."""
    mode, cutoff, a = np.broadcast_arrays(np.asarray(mode), np.asarray(cutoff, F32), np.asarray(a, F32))
    with np.errstate(invalid="ignore"):
        lo = np.where(a > F32(0.0), a, F32(0.0)).astype(F32)
        cl = np.where(lo < F32(1.0), lo, F32(1.0)).astype(F32)
        return np.where(mode == MASK, np.where(a >= cutoff, F32(0.0), F32(1.0)), np.where(mode == BLEND, F32(1.0) - cl, F32(0.0))).astype(F32)


def material_modes(materials):
    """(mode (n,) int32, cutoff (n,) float32) of a description's materials."""
    return (np.array([mode_of(getattr(m, "alpha_mode", "opaque")) for m in materials], np.int32),
            np.array([getattr(m, "alpha_cutoff", 0.5) for m in materials], F32))


def tables(tri_mat, materials):
    """(bits, mode, cutoff) as pt_alpha_tables builds them from flat_scene()'s material ids."""
    mode, cutoff = material_modes(materials)
    tri_mat = np.asarray(tri_mat, np.int64)
    on = mode[tri_mat] != OPAQUE
    bits = np.zeros((len(tri_mat) + 31) // 32, np.uint32)
    for p in np.flatnonzero(on):
        bits[p >> 5] |= np.uint32(1 << (p & 31))
    return bits, mode, cutoff


def prim_is_alpha(bits, prim):
    prim = np.asarray(prim, np.int64)
    return ((bits[prim >> 5] >> (prim & 31).astype(np.uint32)) & 1).astype(bool)


# ---- float32: the surface of a hit as alpha_surface (pt_alpha.hip) rebuilds it ---------------------------------------------------------------------------
def surface(shade, stride, materials, textures, linear, ray_eps, d, prim, uv):
    """(a, material id, o') of the hits (prim (n,), uv (n, 2)) of rays with directions d: a = base[3] as record_material leaves it, o' = vfma(n, ray_eps, P)."""
    R = np.asarray(shade, F32).reshape(-1, stride * 4)[np.asarray(prim, np.int64)]
    hu, hv = np.asarray(uv, F32)[:, 0], np.asarray(uv, F32)[:, 1]
    hw = F32(1.0) - hu - hv
    Pa, Pb, Pc = R[:, 0:3], R[:, 4:7], R[:, 8:11]
    bary = lambda x, y, z: _fma(z, hv[:, None], _fma(y, hu[:, None], x * hw[:, None]))
    M, Tx = lref.material_table(materials)
    mat = np.ascontiguousarray(R[:, 3]).view(np.int32)
    a = M[mat, 8].copy()
    tc = Tx[mat, 0]
    if stride == 12 and (tc >= 0).any():
        X = R[:, 20:44]
        tu = _fma(X[:, 4], hv, _fma(X[:, 2], hu, X[:, 0] * hw))
        tv = _fma(X[:, 5], hv, _fma(X[:, 3], hu, X[:, 1] * hw))
        for t_id in np.unique(tc[tc >= 0]):
            m = tc == t_id
            a[m] = a[m] * lref.tex_fetch(textures[t_id], tu[m], tv[m], linear)[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        P = bary(Pa, Pb, Pc)
        ng = lref.normalize3(lref.cross3(Pb - Pa, Pc - Pa))
    n = np.where((lref.dot3(ng, np.asarray(d, F32)) > 0)[:, None], ng, -ng)
    return a.astype(F32), mat, _fma(n, F32(ray_eps), P).astype(F32)


class Scene32:
    """What the float32 restatement reads of a committed scene: shading records, materials, textures, filter, ray epsilon, the alpha tables."""

    def __init__(self, pt, desc):
        self.shade = pt.shading_tables()[0]
        self.stride = self.shade.shape[1] // 4
        verts, _, tri_mat = pt.flat_scene()
        self.eps = lref.scene_ray_eps(verts[:, 0:3])
        self.materials, self.textures = desc.materials, desc.textures
        self.linear = desc.texture_filter == "linear"
        self.bits, self.mode, self.cutoff = tables(tri_mat, desc.materials)

    def surface(self, d, prim, uv):
        return surface(self.shade, self.stride, self.materials, self.textures, self.linear, self.eps, d, prim, uv)


def resolve_closest(sc, trace, o, d, keys, bounce, max_layers, deterministic=False):
    """ptc_debug_alpha_closest: (t, prim, uv, layers).  trace(o, d) -> (t, prim, uv) is ptc_debug_trace_closest."""
    o, d = np.asarray(o, F32), np.asarray(d, F32)
    n = len(o)
    t, prim, uv = (x.copy() for x in trace(o, d))
    layers = np.zeros(n, np.uint32)
    live = np.arange(n)                      # rays still being resolved, with their current segment's hit
    ct, cp, cuv, co = t.copy(), prim.copy(), uv.copy(), o.copy()
    t_base = np.zeros(n, F32)
    k = 0
    while len(live):
        hit = cp >= 0
        decide = hit.copy()
        decide[hit] = prim_is_alpha(sc.bits, cp[hit])
        passing = np.zeros(len(live), bool)
        onward = np.zeros((len(live), 3), F32)
        if decide.any():
            a, mat, op = sc.surface(d[live][decide], cp[decide], cuv[decide])
            if deterministic:
                acc = accept_deterministic(sc.mode[mat], sc.cutoff[mat], a)
            else:
                acc = accept(sc.mode[mat], sc.cutoff[mat], a, rng_f(keys[live][decide], RNG_BASE + int(bounce) + 1, k))
            passing[decide] = ~acc & (k != max_layers)
            onward[decide] = op
        stand = ~passing
        if k > 0:                            # a ray of round 0 that stands keeps the record the trace wrote
            s = live[stand]
            t[s] = np.where(cp[stand] >= 0, (t_base[stand] + ct[stand]).astype(F32), ct[stand])
            prim[s], uv[s], layers[s] = cp[stand], cuv[stand], k
        live = live[passing]
        if not len(live):
            break
        t_base = (t_base[passing] + ct[passing]).astype(F32)
        co = onward[passing]
        ct, cp, cuv = (x.copy() for x in trace(co, d[live]))
        k += 1
    return t, prim, uv, layers


def resolve_any(sc, trace, trace_any, o, d, tmax, max_layers):
    """ptc_debug_alpha_any: the transmittance per shadow ray, 0 when occluded.  trace_any(o, d, tmax) is ptc_debug_trace_any (the coarse flag)."""
    o, d, tmax = np.asarray(o, F32), np.asarray(d, F32), np.asarray(tmax, F32)
    n = len(o)
    out = np.zeros(n, F32)
    flag = np.asarray(trace_any(o, d, tmax)) != 0
    out[~flag] = 1.0
    live = np.flatnonzero(flag)
    co, rem, Tr = o[live].copy(), tmax[live].copy(), np.ones(len(live), F32)
    k = 0
    while len(live):
        ct, cp, cuv = trace(co, d[live])
        with np.errstate(invalid="ignore"):
            visible = (cp < 0) | ~(ct < rem)
        out[live[visible]] = Tr[visible]
        blocked = ~visible
        decide = blocked.copy()
        decide[blocked] = prim_is_alpha(sc.bits, cp[blocked])
        tr = np.zeros(len(live), F32)
        onward = np.zeros((len(live), 3), F32)
        if decide.any():
            a, mat, op = sc.surface(d[live][decide], cp[decide], cuv[decide])
            tr[decide] = transmit(sc.mode[mat], sc.cutoff[mat], a)
            onward[decide] = op
        Tr = (Tr * tr).astype(F32)
        passing = blocked & (Tr != 0) & (k != max_layers)
        live, co, rem, Tr = live[passing], onward[passing], (rem[passing] - ct[passing]).astype(F32), Tr[passing]
        k += 1
    return out


# ---- float64: the independent walk -------------------------------------------------------------------------------------------------------------------------
EDGE_MARGIN = 1e-4        # a pair whose edge margin m = min(u, v, 1 - u - v) lies within this of 0 is a candidate: a hit to one precision, or from an origin one ray
                          # epsilon off the last surface, and a miss to the other
TEXEL_MARGIN, CUTOFF_MARGIN, BLEND_MARGIN, T_MARGIN = 1e-4, 1e-4, 1e-5, 1e-5


def _alpha64(tex, u, v, linear):
    """alpha of one lookup in float64, and its distance (in u, v units) to the nearest texel edge."""
    h, w = tex.shape[0], tex.shape[1]
    fu, fv = u - np.floor(u), v - np.floor(v)
    edge = min(abs(fu * w - round(fu * w)) / w, abs(fv * h - round(fv * h)) / h)
    al = tex[..., 3].astype(F64) / 255.0
    if not linear:
        return al[min(int(fv * h), h - 1), min(int(fu * w), w - 1)], edge
    x, y = fu * w - 0.5, fv * h - 0.5
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    tx, ty = x - x0, y - y0
    x1, y1 = (x0 + 1) % w, (y0 + 1) % h
    x0, y0 = x0 % w, y0 % h
    a = al[y0, x0] + tx * (al[y0, x1] - al[y0, x0])
    b = al[y1, x0] + tx * (al[y1, x1] - al[y1, x0])
    return a + ty * (b - a), edge


def walk_closest(verts, idx, tri_mat, materials, textures, linear, o, d, keys, bounce, max_layers, deterministic=False):
    """Per ray: the float64 hits of ALL triangles sorted by (t, primitive id), walked layer by layer with pt_alpha_accept.  Returns (t, prim, layers, undecided):
    prim -1 and t inf on a miss.  A ray is undecided when a lookup it crossed lies within TEXEL_MARGIN of a texel edge, a MASK alpha within CUTOFF_MARGIN of
    the cutoff, a BLEND u within BLEND_MARGIN of a, two candidate hits within T_MARGIN relative in t, or a candidate within EDGE_MARGIN of its triangle's edge
    (the quads' shared diagonal is the common case of the last two) — before the walk ended."""
    V = np.asarray(verts)
    P, UV = V[:, 0:3].astype(F64), V[:, 10:12].astype(F64)
    idx = np.asarray(idx).reshape(-1, 3).astype(np.int64)
    A, B, C = P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]
    mode, cutoff = material_modes(materials)
    M, Tx = lref.material_table(materials)
    n = len(o)
    out_t, out_prim, out_layers, undecided = np.full(n, np.inf), np.full(n, -1, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    for r in range(n):
        t, u, v, m, g, _ = tref.pair_terms(A, B, C, np.asarray(o[r], F64)[None], np.asarray(d[r], F64)[None])
        with np.errstate(invalid="ignore"):
            cand = np.flatnonzero((m > -EDGE_MARGIN) & (t > 0) & np.isfinite(t))
        cand = cand[np.lexsort((cand, t[cand]))]
        k = 0
        for j, p in enumerate(cand):
            if abs(m[p]) <= EDGE_MARGIN or (j + 1 < len(cand) and t[cand[j + 1]] - t[p] <= T_MARGIN * t[p]):
                undecided[r] = True
            if m[p] < 0:
                continue
            mat = int(tri_mat[p])
            stands = True
            if mode[mat] != OPAQUE:
                a = float(M[mat, 8])
                if Tx[mat, 0] >= 0:
                    w0 = 1.0 - u[p] - v[p]
                    tu, tv = (UV[idx[p, 0]] * w0 + UV[idx[p, 1]] * u[p] + UV[idx[p, 2]] * v[p])
                    ta, edge = _alpha64(textures[Tx[mat, 0]], tu, tv, linear)
                    a *= ta
                    if edge <= TEXEL_MARGIN:
                        undecided[r] = True
                md, cut = (MASK, 0.5) if (deterministic and mode[mat] == BLEND) else (int(mode[mat]), float(cutoff[mat]))
                if md == MASK:
                    ok = a >= cut
                    if abs(a - cut) <= CUTOFF_MARGIN:
                        undecided[r] = True
                else:
                    uu = float(rng_f(np.asarray([keys[r]]), RNG_BASE + int(bounce) + 1, k)[0])
                    ok = uu < a
                    if abs(uu - a) <= BLEND_MARGIN:
                        undecided[r] = True
                stands = ok or k == max_layers
            if stands:
                out_t[r], out_prim[r], out_layers[r] = t[p], p, k
                break
            k += 1
        else:
            out_layers[r] = k
    return out_t, out_prim, out_layers, undecided


# ---- the ray sets of the resolution tests (test_alpha_host.py runs them on walk_closest alone, test_gpu_alpha.py on the device) ---------------------------------
SEED = 0x0A1FA0C0FFEE1234
RAY_COUNTS = (1, 63, 64, 65, 513)
MAX_UNDECIDED = 0.02


def ray_sets(pt):
    """(n, origins, dirs, keys) per count: camera rays of a 24x24 frame of the context's camera in a random order, with random keys; in the larger sets every
    third ray is turned away so that misses interleave.  1, 63, 64, 65 sit on and around a wave; 513 rays are two segments (PTC_SEG_MIN_LEN = 512)."""
    o_all, d_all = pt.debug_camera_rays(24, 24, SEED, 0, 1)
    rng = np.random.default_rng(11)
    for n in RAY_COUNTS:
        sel = rng.permutation(len(o_all))[:n] if n > 1 else np.array([len(o_all) // 2 + 12])
        o, d = o_all[sel].copy(), d_all[sel].copy()
        if n > 1:
            away = np.arange(n) % 3 == 1
            d[away] = -d[away]
        yield n, o, d, rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def t_bound(t_ref, layers, ray_eps):
    """|t - t_ref| of a resolved hit: each of its layers + 1 segments is measured from an origin shifted by at most ray_eps, with a few ulp of float32 each."""
    return (np.asarray(layers, F64) + 1.0) * (8.0 * 2.0 ** -23 * np.asarray(t_ref, F64) + float(ray_eps))
