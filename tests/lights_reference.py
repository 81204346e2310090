"""numpy restatement of the punctual lights (csrc/pt_lights.h, csrc/pt_lights.hip), for tests/test_lights_host.py and tests/test_gpu_lights.py.

Everything is float32 in the order the sources write it; `_fma` is lens_reference's single-rounding emulation.  Three parts:
  light_table / light_sample   the records and cdf the host builds, and pt_light_sample
  choose_light                 the draw rng_f(key, PT_LIGHTS_RNG_BASE + b + 1, 0) through cdf_search's rule
  punctual_nee                 k_shade_punctual: the surface as k_shade rebuilds it (shading record, material, textures NEAREST / LINEAR, normal map, sign flips),
                               the BSDF value and the shadow record (origin, direction, tmax, contribution)."""
import numpy as np

from lens_reference import F32, F64, U64, _fma, rng_f

POINT, SPOT, DIRECTIONAL = 0, 1, 2
RNG_BASE = 0x10000000
T_INF = F32(3.0e38)
PI = F32(3.14159265358979323846)
INV_PI = F32(0.31830988618379067154)
HIT_CLASS_SHIFT = 28
_TYPES = {"point": POINT, "spot": SPOT, "directional": DIRECTIONAL, "sun": DIRECTIONAL}


def _fm(dt):
    return lambda a, b, c: _fma(a, b, c, dt)


def dot3(a, b, dt=F32):
    f = _fm(dt)
    return f(a[..., 2], b[..., 2], f(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def normalize3(a, dt=F32):
    inv = dt(1.0) / np.sqrt(dot3(a, a, dt))
    return a * inv[..., None]


def cross3(a, b):
    return np.stack([_fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), _fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     _fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1)


def _get(l, k):
    return l[k] if isinstance(l, dict) else getattr(l, k)


def light_fields(l):
    """(type, position, direction, intensity, range, cos_inner, cos_outer, weight) of a dict / LightDesc, float32, with the defaults of ptc_light_default_params."""
    d = dict(type="point", position=(0, 0, 0), direction=(0, 0, -1), intensity=(1, 1, 1), range=0.0, cos_inner=1.0, cos_outer=0.70710678, sampling_weight=1.0)
    if isinstance(l, dict):
        d.update(l)
    else:
        d.update({k: getattr(l, k) for k in d})
    t = _TYPES[d["type"]] if isinstance(d["type"], str) else int(d["type"])
    return (t, np.asarray(d["position"], F32), np.asarray(d["direction"], F32), np.asarray(d["intensity"], F32), F32(d["range"]), F32(d["cos_inner"]), F32(d["cos_outer"]),
            F32(d["sampling_weight"]))


def light_record(l, pmf=1.0):
    """The 16 floats of pt_light_make_rec behind pt_light_normalise: (pos, type bits | dir, range | I, pmf | scale, offset, cos_inner, cos_outer)."""
    t, pos, dr, I, rng, ci, co, _ = light_fields(l)
    if t != POINT:
        dr = (dr * (F32(1.0) / np.sqrt(dot3(dr, dr)))).astype(F32)
    r = np.zeros(16, F32)
    r[0:3] = pos
    r[3:4] = np.array([t], np.int32).view(F32)
    r[4:7], r[7] = dr, rng
    r[8:11], r[11] = I, F32(pmf)
    r[14], r[15] = ci, co
    if t == SPOT:
        r[12] = F32(1.0) / max(F32(ci - co), F32(0.001))
        r[13] = (-co) * r[12]
    return r


def light_table(lights):
    """pt_light_table: (records (n, 16), cdf (n,)) — binary32 running sums, cdf[i] = run / total, the last entry 1."""
    w = [light_fields(l)[7] for l in lights]
    total = F32(0.0)
    for x in w:
        total = F32(total + x)
    run = F32(0.0)
    recs, cdf = np.zeros((len(lights), 16), F32), np.zeros(len(lights), F32)
    for i, l in enumerate(lights):
        run = F32(run + w[i])
        cdf[i] = F32(run / total)
        recs[i] = light_record(l, F32(w[i] / total))
    if len(lights):
        cdf[-1] = 1.0
    return recs, cdf


def rec_type(rec):
    return np.ascontiguousarray(rec[..., 3]).view(np.int32)


def light_sample(rec, P, dt=F32):
    """pt_light_sample for the record(s) `rec` ((16,) or (n, 16)) at the points P (n, 3): (ok, wi, dist, Li).  dt=F64 evaluates the same expressions in float64."""
    P = np.atleast_2d(np.asarray(P, F32)).astype(dt)
    n = P.shape[0]
    rec = np.broadcast_to(np.asarray(rec, F32), (n, 16))
    t = rec_type(np.ascontiguousarray(rec))
    r = rec.astype(dt)
    pos, dr, rng, I, scale, offset = r[:, 0:3], r[:, 4:7], r[:, 7], r[:, 8:11], r[:, 12], r[:, 13]
    f = _fm(dt)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dv = pos - P
        dist2 = dot3(dv, dv, dt)
        ok = dist2 > 0
        dist = np.sqrt(dist2)
        wi = dv * (dt(1.0) / dist)[:, None]
        att = dt(1.0) / dist2
        q = dist2 / (rng * rng)
        w = np.minimum(np.maximum(dt(1.0) - q * q, dt(0.0)), dt(1.0))
        att = np.where(rng > 0, att * w, att)
        cd = dot3(dr, -wi, dt)
        s = np.minimum(np.maximum(f(cd, scale, offset), dt(0.0)), dt(1.0))
        att = np.where(t == SPOT, att * (s * s), att)
        Li = I * att[:, None]
    dirl = t == DIRECTIONAL
    wi = np.where(dirl[:, None], -dr, wi)
    Li = np.where(dirl[:, None], I, Li)
    dist = np.where(dirl, dt(T_INF), dist)
    ok = ok | dirl
    z = lambda a: np.where(ok.reshape((-1,) + (1,) * (a.ndim - 1)), a, dt(0.0)).astype(dt)
    return ok, z(wi), z(dist), z(Li)


def cdf_search(cdf, r):
    """cdf_search's rule, lane by lane."""
    cdf, r = np.asarray(cdf, F32), np.asarray(r, F32)
    lo, hi = np.zeros(r.shape, np.int64), np.full(r.shape, cdf.size - 1, np.int64)
    while (lo < hi).any():
        act = lo < hi
        mid = (lo + hi) >> 1
        up = cdf[mid] > r
        hi = np.where(act & up, mid, hi)
        lo = np.where(act & ~up, mid + 1, lo)
    return lo


def choose_light(cdf, key, bounce):
    return cdf_search(cdf, rng_f(key, RNG_BASE + int(bounce) + 1, 0))


def material_table(materials):
    """(n, 12) float32 — base rgb, metallic | emissive rgb, roughness | base a — and (n, 3) int32 texture ids (colour, normal, metal-rough), as the commit lays them out."""
    M = np.zeros((len(materials), 9), F32)
    T = np.zeros((len(materials), 3), np.int32)
    for i, m in enumerate(materials):
        M[i, 0:3], M[i, 3], M[i, 4:7], M[i, 7], M[i, 8] = np.asarray(m.base_color, F32)[:3], m.metallic, np.asarray(m.emissive, F32), m.roughness, np.asarray(m.base_color, F32)[3]
        T[i] = m.tex_color, m.tex_normal, m.tex_mr
    return M, T


def tex_fetch(tex, u, v, linear):
    """tex_fetch over an (h, w, 4) uint8 image: NEAREST, or bilinear with texel centres at i + 0.5 and REPEAT wrap, lerp(a, b, t) = fma(t, b - a, a), x then y."""
    h, w = tex.shape[0], tex.shape[1]
    rgba = lambda y, x: tex[y, x].astype(F32) / F32(255.0)
    fu, fv = u - np.floor(u), v - np.floor(v)
    if not linear:
        x = np.minimum((fu * F32(w)).astype(np.int32), w - 1)
        y = np.minimum((fv * F32(h)).astype(np.int32), h - 1)
        return rgba(y, x)
    x, y = _fma(fu, F32(w), F32(-0.5)), _fma(fv, F32(h), F32(-0.5))
    x0f, y0f = np.floor(x), np.floor(y)
    tx, ty = (x - x0f)[:, None], (y - y0f)[:, None]
    x0, y0 = x0f.astype(np.int32), y0f.astype(np.int32)
    x1, y1 = x0 + 1, y0 + 1
    x0, y0 = np.where(x0 < 0, x0 + w, x0), np.where(y0 < 0, y0 + h, y0)
    x1, y1 = np.where(x1 > w - 1, x1 - w, x1), np.where(y1 > h - 1, y1 - h, y1)
    c00, c10, c01, c11 = rgba(y0, x0), rgba(y0, x1), rgba(y1, x0), rgba(y1, x1)
    a = _fma(tx, c10 - c00, c00)
    b = _fma(tx, c11 - c01, c01)
    return _fma(ty, b - a, a)


def scene_ray_eps(world_positions):
    """ptc_refit_grid's ray offset from the world vertex positions (n, 3) float32."""
    p = np.asarray(world_positions, F32)
    diag = (p.max(0) - p.min(0)).astype(F32).max()
    return F32(1e-4) * max(diag, F32(1e-6))


def onb(n):
    sg = np.copysign(F32(1.0), n[..., 2])
    a = F32(-1.0) / (sg + n[..., 2])
    bb = n[..., 0] * n[..., 1] * a
    t = np.stack([_fma(sg * n[..., 0], n[..., 0] * a, F32(1.0)), sg * bb, -sg * n[..., 0]], -1)
    b = np.stack([bb, _fma(n[..., 1], n[..., 1] * a, sg), -n[..., 1]], -1)
    return t.astype(F32), b.astype(F32)


def schlick(f0, voh):
    m = np.maximum(F32(1.0) - voh, F32(0.0))
    m2 = m * m
    m5 = (m2 * m2 * m)[..., None]
    return _fma(F32(1.0) - f0, m5, f0)


def smith_g1(x, a2):
    return (F32(2.0) * x) / (x + np.sqrt(_fma(F32(1.0) - a2, x * x, a2)))


def bsdf_f(base, metallic, roughness, lambert, wol, wil):
    """f of bsdf_eval(make_bsdf(base, metallic, roughness, lambert), wol, wil, ...)."""
    mt = metallic
    cd = base * (F32(1.0) - mt)[:, None]
    d = F32(0.04) * (F32(1.0) - mt)
    f0 = _fma(base, mt[:, None], d[:, None])
    alpha = np.maximum(roughness * roughness, F32(0.001))
    fd = cd * INV_PI
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        nol = wil[:, 2]
        nov = np.maximum(wol[:, 2], F32(1e-4))
        h = normalize3(wol + wil)
        noh, voh = h[:, 2], dot3(wol, h)
        a2 = alpha * alpha
        dd = _fma(noh * noh, a2 - F32(1.0), F32(1.0))
        D = a2 / (PI * dd * dd)
        gv, gl = smith_g1(nov, a2), smith_g1(nol, a2)
        F = schlick(f0, voh)
        sp = (D * gv * gl) / (F32(4.0) * nov * nol)
        fg = _fma(F, sp[:, None], fd)
    return np.where(lambert[:, None], fd, fg).astype(F32)


def punctual_nee(shade, stride, materials, textures, linear, ray_eps, table, cdf, dirs, keys, prim, uv, bounce):
    """k_shade_punctual for n rays of throughput 1: dirs (n, 3), keys (n,), the closest hits (prim (n,) int32 or -1, uv (n, 2)).  shade: the shading records
    (ptc_debug_get_shading_tables), stride 5 or 12; materials / textures: the description's; table, cdf: light_table's.
    Returns (valid (n,) bool, origin (n, 3), dir (n, 3), tmax (n,), contrib (n, 3)), zero where not valid."""
    n = len(prim)
    d = np.asarray(dirs, F32)
    hit = np.asarray(prim) >= 0
    pr = np.where(hit, prim, 0).astype(np.int64) & ((1 << HIT_CLASS_SHIFT) - 1)
    R = np.asarray(shade, F32).reshape(-1, stride * 4)[pr]
    hu, hv = np.asarray(uv, F32)[:, 0], np.asarray(uv, F32)[:, 1]
    hw = F32(1.0) - hu - hv
    Pa, Pb, Pc = R[:, 0:3], R[:, 4:7], R[:, 8:11]
    Na, Nb, Nc = R[:, 11:14], R[:, 14:17], R[:, 17:20]
    bary = lambda a, b, c: _fma(c, hv[:, None], _fma(b, hu[:, None], a * hw[:, None]))
    M, Tx = material_table(materials)
    mat = np.ascontiguousarray(R[:, 3]).view(np.int32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        P = bary(Pa, Pb, Pc)
        ng = normalize3(cross3(Pb - Pa, Pc - Pa))
        ni = bary(Na, Nb, Nc)
        ns = normalize3(ni)
        base = np.concatenate([M[mat, 0:3], M[mat, 8:9]], 1).copy()
        metallic, roughness = M[mat, 3].copy(), M[mat, 7].copy()
        tc, tn, tm = Tx[mat, 0], Tx[mat, 1], Tx[mat, 2]
        lambert = (metallic == 0) & (roughness >= 1) & (tm < 0)
        if stride == 12:
            # uv x3: (r5.xy, r5.zw, r6.xy); tangents a = (r6.zw, r7.x) b = r7.yzw c = r8.xyz; bitangents a = (r8.w, r9.xy) b = (r9.zw, r10.x) c = r10.yzw
            X = R[:, 20:44]
            tu = _fma(X[:, 4], hv, _fma(X[:, 2], hu, X[:, 0] * hw))
            tv = _fma(X[:, 5], hv, _fma(X[:, 3], hu, X[:, 1] * hw))
            ti = bary(X[:, 6:9], X[:, 9:12], X[:, 12:15])
            bi = bary(X[:, 15:18], X[:, 18:21], X[:, 21:24])
            for t_id in np.unique(tc[tc >= 0]):
                m = tc == t_id
                base[m] = base[m] * tex_fetch(textures[t_id], tu[m], tv[m], linear)
            for t_id in np.unique(tm[tm >= 0]):
                m = tm == t_id
                cm = tex_fetch(textures[t_id], tu[m], tv[m], linear)
                roughness[m] = roughness[m] * cm[:, 1]
                metallic[m] = metallic[m] * cm[:, 2]
            for t_id in np.unique(tn[tn >= 0]):
                m = tn == t_id
                cn = tex_fetch(textures[t_id], tu[m], tv[m], linear)
                nx, ny, nz = (F32(2.0) * cn[:, k:k + 1] - F32(1.0) for k in range(3))
                ns[m] = normalize3(_fma(ti[m], nx, _fma(bi[m], ny, ni[m] * nz)))
        wo = -d
        front = dot3(ng, wo) > 0
        ns = np.where((dot3(ns, ng) < 0)[:, None], -ns, ns)
        ng = np.where(front[:, None], ng, -ng)
        ns = np.where(front[:, None], ns, -ns)
        ns = np.where((dot3(ns, wo) > 0)[:, None], ns, ng)
        li = choose_light(cdf, keys, bounce)
        L = np.asarray(table, F32)[li]
        ok, wi, _, Li = light_sample(L, P)
        tx, ty = onb(ns)
        wil = np.stack([dot3(tx, wi), dot3(ty, wi), dot3(ns, wi)], -1)
        wol = np.stack([dot3(tx, wo), dot3(ty, wo), dot3(ns, wo)], -1)
        valid = hit & ok & (wil[:, 2] > 0) & (dot3(ng, wi) > 0) & (Li > 0).any(1)
        f = bsdf_f(base[:, 0:3], metallic, roughness, lambert, wol, wil)
        porg = _fma(ng, F32(ray_eps), P)
        k = wil[:, 2] / L[:, 11]
        sv = L[:, 0:3] - porg
        sd = np.sqrt(dot3(sv, sv))
        sdir = sv * (F32(1.0) / sd)[:, None]
        tmax = sd * F32(0.999)
        dirl = rec_type(np.ascontiguousarray(L)) == DIRECTIONAL
        sdir = np.where(dirl[:, None], wi, sdir)
        tmax = np.where(dirl, T_INF, tmax)
        contrib = F32(1.0) * f * Li * k[:, None]
    z = lambda a: np.where(valid.reshape((-1,) + (1,) * (a.ndim - 1)), a, F32(0.0)).astype(F32)
    return valid, z(porg), z(sdir), z(tmax), z(contrib)
