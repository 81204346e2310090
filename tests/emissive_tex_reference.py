"""numpy restatement of textured emission (csrc/pt_emissive_tex.h, csrc/pt_emissive_tex.hip), for tests/test_emissive_tex_host.py and
tests/test_gpu_emissive_tex.py.

Everything is float32 in the order the sources write it; `_fma` is lens_reference's single-rounding emulation.  Parts:
  mean_texel / mean_cells / table   the weights, entries, cdf and primitive map the host builds (instances are given by their 4x4 matrices)
  sample / hit_radiance / hit_weight   pt_emtex_sample and the hit side
  step                              k_shade_emissive_tex: the surface as k_shade rebuilds it, the BSDF value and density, the shadow record and the addition to lpath
  irradiance64                      float64 closed form: the integral of Le cos cos / d^2 over a planar emitter's lit texels, by quadrature"""
import numpy as np

import lights_reference as lref
from lens_reference import F32, F64, _fma, rng_f

RNG_BASE = 0x28000000
FLOOR = F32(0.01)
INV_PI = lref.INV_PI
PI = lref.PI
dot3, cross3, normalize3 = lref.dot3, lref.cross3, lref.normalize3


def _s(x):
    """A one-element result as a float32 scalar."""
    return F32(np.asarray(x).reshape(-1)[0])


def lum(c):
    c = np.asarray(c, F32)
    return _fma(c[..., 2], F32(0.0722), _fma(c[..., 1], F32(0.7152), c[..., 0] * F32(0.2126)))


def fetch(tex, u, v, linear):
    """pt_emtex_fetch: tex_fetch's rgb over an (h, w, 4) uint8 image, u and v arrays."""
    return lref.tex_fetch(tex, np.atleast_1d(np.asarray(u, F32)), np.atleast_1d(np.asarray(v, F32)), linear)[:, :3].astype(F32)


def mean_texel(tex):
    """pt_emtex_mean_texel: the exact byte sums over 255 n."""
    s = tex[..., :3].reshape(-1, 3).astype(np.uint64).sum(0)
    return (s.astype(F64) / (255.0 * (tex.shape[0] * tex.shape[1]))).astype(F32)


def uv_at(uv3, bu, bv):
    """pt_emtex_uv for entries' vertex uvs uv3 (..., 3, 2)."""
    bu, bv = np.asarray(bu, F32), np.asarray(bv, F32)
    bw = F32(1.0) - bu - bv
    u = _fma(uv3[..., 2, 0], bv, _fma(uv3[..., 1, 0], bu, uv3[..., 0, 0] * bw))
    v = _fma(uv3[..., 2, 1], bv, _fma(uv3[..., 1, 1], bu, uv3[..., 0, 1] * bw))
    return u, v


def cells():
    """The 16 centroids in the table's order: 10 upright cells, then 6 inverted ones."""
    third, two = F32(1.0) / F32(3.0), F32(2.0) / F32(3.0)
    out = []
    for p, o in ((0, third), (1, two)):
        for i in range(4 - p):
            for j in range(4 - p - i):
                out.append(((F32(i) + o) * F32(0.25), (F32(j) + o) * F32(0.25)))
    return out


def mean_cells(uv3, tex):
    s = np.zeros(3, F32)
    for bu, bv in cells():
        u, v = uv_at(np.asarray(uv3, F32), bu, bv)
        s = (s + fetch(tex, u, v, False)[0]).astype(F32)
    return (s * F32(0.0625)).astype(F32)


def transform_point(m, p):
    """scene_rules::transform_point with a column-major 4x4 (16 floats)."""
    m, p = np.asarray(m, F32).reshape(16), np.asarray(p, F32)
    return np.array([F32(F32(F32(m[r] * p[0]) + F32(m[4 + r] * p[1])) + F32(m[8 + r] * p[2])) + m[12 + r] for r in range(3)], F32)


def table(desc, matrices=None):
    """(records (n, 28), cdf (n,), prim_map (n_tris,) int32, total) of a SceneDesc whose instances carry matrices (or `matrices`: one 16-vector per instance)."""
    recs, weight, prim_map = [], [], []
    tb = 0
    for ii, inst in enumerate(desc.instances):
        mesh = desc.meshes[inst.mesh]
        mat = desc.materials[mesh.material]
        M = np.asarray(matrices[ii] if matrices is not None else inst.matrix, F32).reshape(16)
        nt = mesh.indices.size // 3
        tex_id = getattr(mat, "emissive_texture", -1)
        if tex_id < 0:
            prim_map += [-1] * nt
            tb += nt
            continue
        tex = np.asarray(desc.textures[tex_id], np.uint8)
        f = np.asarray(mat.emissive_texture_factor, F32)
        floor_l = F32(FLOOR * _s(lum(f * mean_texel(tex))))
        for k in range(nt):
            vi = mesh.indices[3 * k:3 * k + 3]
            uv3 = np.asarray(mesh.vertices["texCoords"][vi], F32)
            lumw = max(_s(lum(f * mean_cells(uv3, tex))), floor_l)
            a, b, c = (transform_point(M, mesh.vertices["position"][v]) for v in vi)
            e1, e2 = (b - a).astype(F32), (c - a).astype(F32)
            with np.errstate(invalid="ignore", over="ignore"):
                cr = cross3(e1, e2)
                ln = _s(np.sqrt(dot3(cr, cr)))
                area = F32(0.5) * ln
                w = area * lumw
            r = np.zeros(28, F32)
            r[0:3], r[4:7], r[8:11], r[16:19] = a, e1, e2, f
            r[11:12] = np.array([tex_id], np.int32).view(F32)
            r[20:22], r[22:24], r[24:26] = uv3[0], uv3[1], uv3[2]
            if ln > 0 and np.isfinite(ln) and np.isfinite(w):
                r[3] = area
                r[12:15] = cr * (F32(1.0) / ln)
                weight.append(F32(w))
            else:
                weight.append(F32(0.0))
            prim_map.append(len(recs))
            recs.append(r)
        tb += nt
    n = len(recs)
    recs = np.array(recs, F32).reshape(n, 28)
    cdf = np.zeros(n, F32)
    total = F32(0.0)
    for w in weight:
        total = F32(total + w)
    if not n:
        return recs, cdf, np.zeros(0, np.int32), 0.0
    if total > 0:
        run = F32(0.0)
        for j in range(n):
            run = F32(run + weight[j])
            cdf[j] = F32(run / total)
            recs[j, 7] = F32(weight[j] / total)
        last = n - 1
        while last > 0 and not weight[last] > 0:
            last -= 1
        cdf[last:] = 1.0
    return recs, cdf, np.array(prim_map, np.int32), float(total) if total > 0 else 0.0


def _uv3(E):
    return np.stack([E[..., 20:22], E[..., 22:24], E[..., 24:26]], -2)


def radiance(E, textures, linear, bu, bv):
    """pt_emtex_radiance for entries E (n, 28) at barycentrics (bu, bv): factor x texel."""
    E = np.atleast_2d(np.asarray(E, F32))
    u, v = uv_at(_uv3(E), bu, bv)
    tid = np.ascontiguousarray(E[:, 11]).view(np.int32)
    c = np.zeros((E.shape[0], 3), F32)
    for t in np.unique(tid):
        m = tid == t
        c[m] = fetch(np.asarray(textures[t], np.uint8), u[m], v[m], linear)
    return (E[:, 16:19] * c).astype(F32)


def sample(E, textures, linear, P, r1, r2):
    """pt_emtex_sample, entry by entry: (ok, y, wi, pl, Le), zero where not ok."""
    E = np.atleast_2d(np.asarray(E, F32))
    P = np.atleast_2d(np.asarray(P, F32))
    r1, r2 = np.atleast_1d(np.asarray(r1, F32)), np.atleast_1d(np.asarray(r2, F32))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        su = np.sqrt(r1)
        bu, bv = su * (F32(1.0) - r2), su * r2
        y = _fma(E[:, 8:11], bv[:, None], _fma(E[:, 4:7], bu[:, None], E[:, 0:3]))
        dv = y - P
        dist2 = dot3(dv, dv)
        dist = np.sqrt(dist2)
        wi = dv * (F32(1.0) / dist)[:, None]
        cosl = -dot3(E[:, 12:15], wi)
        ok = (dist2 > 0) & (cosl > 0) & (E[:, 7] > 0)
        pl = (E[:, 7] * dist2) / (E[:, 3] * cosl)
        Le = radiance(E, textures, linear, bu, bv)
    z = lambda a: np.where(ok.reshape((-1,) + (1,) * (a.ndim - 1)), a, F32(0.0)).astype(F32)
    return ok, z(y), z(wi), z(pl), z(Le)


def hit_weight(E, b, pb, ht, cosl):
    E = np.atleast_2d(np.asarray(E, F32))
    pb, ht, cosl = (np.atleast_1d(np.asarray(a, F32)) for a in (pb, ht, cosl))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pl = (E[:, 7] * (ht * ht)) / (E[:, 3] * cosl)
        pb2 = pb * pb
        w = pb2 / _fma(pl, pl, pb2)
    return np.where((b == 0) | (E[:, 7] == 0), F32(1.0), w).astype(F32)


def bsdf_f_pdf(base, metallic, roughness, lambert, wol, wil):
    """(f, pdf) of bsdf_eval(make_bsdf(...), wol, wil, ps = spec_prob(bs, max(wol.z, 1e-4)))."""
    mt = metallic
    cd = base * (F32(1.0) - mt)[:, None]
    d = F32(0.04) * (F32(1.0) - mt)
    f0 = _fma(base, mt[:, None], d[:, None])
    alpha = np.maximum(roughness * roughness, F32(0.001))
    fd = cd * INV_PI
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        nol = wil[:, 2]
        pd = nol * INV_PI
        nov = np.maximum(wol[:, 2], F32(1e-4))
        ld = lum(cd)
        lf = lum(lref.schlick(f0, nov))
        p = np.minimum(np.maximum(lf / (lf + ld), F32(0.1)), F32(0.9))
        ps = np.where(ld > 0, p, F32(1.0)).astype(F32)
        h = normalize3(wol + wil)
        noh, voh = h[:, 2], dot3(wol, h)
        a2 = alpha * alpha
        dd = _fma(noh * noh, a2 - F32(1.0), F32(1.0))
        D = a2 / (PI * dd * dd)
        gv, gl = lref.smith_g1(nov, a2), lref.smith_g1(nol, a2)
        F = lref.schlick(f0, voh)
        sp = (D * gv * gl) / (F32(4.0) * nov * nol)
        fg = _fma(F, sp[:, None], fd)
        pspec = (gv * D) / (F32(4.0) * nov)
        pg = _fma(ps, pspec, (F32(1.0) - ps) * pd)
    return np.where(lambert[:, None], fd, fg).astype(F32), np.where(lambert, pd, pg).astype(F32)


def step(shade, stride, materials, textures, linear, ray_eps, recs, cdf, prim_map, total, dirs, T, prev_pdf, keys, t_hit, prim, uv, bounce, max_bounces, lpath=None):
    """k_shade_emissive_tex for n rays: dirs (n, 3), throughput T (n, 3), pdf word, keys, the closest hits (t, prim or -1, uv).  shade: the shading records
    (ptc_debug_get_shading_tables), stride 5 or 12; recs, cdf, prim_map, total: the table.  Returns (lpath (n, 3), valid (n,), shadow (n, 10)), zero where not valid."""
    n = len(prim)
    d, T, pb_prev = np.asarray(dirs, F32), np.asarray(T, F32), np.asarray(prev_pdf, F32)
    L = np.zeros((n, 3), F32) if lpath is None else np.array(lpath, F32).reshape(n, 3)
    hit = np.asarray(prim) >= 0
    pr = np.where(hit, prim, 0).astype(np.int64) & ((1 << lref.HIT_CLASS_SHIFT) - 1)
    R = np.asarray(shade, F32).reshape(-1, stride * 4)[pr]
    hu, hv = np.asarray(uv, F32)[:, 0], np.asarray(uv, F32)[:, 1]
    hw = F32(1.0) - hu - hv
    Pa, Pb, Pc = R[:, 0:3], R[:, 4:7], R[:, 8:11]
    Na, Nb, Nc = R[:, 11:14], R[:, 14:17], R[:, 17:20]
    bary = lambda a, b, c: _fma(c, hv[:, None], _fma(b, hu[:, None], a * hw[:, None]))
    M, Tx = lref.material_table(materials)
    mat = np.ascontiguousarray(R[:, 3]).view(np.int32)
    recs = np.asarray(recs, F32).reshape(-1, 28)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        P = bary(Pa, Pb, Pc)
        ng = normalize3(cross3(Pb - Pa, Pc - Pa))
        wo = -d
        front = dot3(ng, wo) > 0
        # ---- hit side ----
        entry = np.where(hit, np.asarray(prim_map, np.int32)[pr], -1)
        add = hit & (entry >= 0) & front
        if add.any():
            E = recs[entry[add]]
            Le = radiance(E, textures, linear, hu[add], hv[add])
            wgt = hit_weight(E, bounce, pb_prev[add], np.asarray(t_hit, F32)[add], dot3(ng, wo)[add])
            L[add] = _fma(T[add] * Le, wgt[:, None], L[add])
        valid = np.zeros(n, bool)
        shadow = np.zeros((n, 10), F32)
        if not (bounce < max_bounces and total > 0):
            return L, valid, shadow
        # ---- sample side: the surface as k_shade_punctual rebuilds it ----
        ni = bary(Na, Nb, Nc)
        ns = normalize3(ni)
        base = np.concatenate([M[mat, 0:3], M[mat, 8:9]], 1).copy()
        metallic, roughness = M[mat, 3].copy(), M[mat, 7].copy()
        tc, tn, tm = Tx[mat, 0], Tx[mat, 1], Tx[mat, 2]
        lambert = (metallic == 0) & (roughness >= 1) & (tm < 0)
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
                cm = lref.tex_fetch(textures[t_id], tu[m], tv[m], linear)
                roughness[m] = roughness[m] * cm[:, 1]
                metallic[m] = metallic[m] * cm[:, 2]
            for t_id in np.unique(tn[tn >= 0]):
                m = tn == t_id
                cn = lref.tex_fetch(textures[t_id], tu[m], tv[m], linear)
                nx, ny, nz = (F32(2.0) * cn[:, k:k + 1] - F32(1.0) for k in range(3))
                ns[m] = normalize3(_fma(ti[m], nx, _fma(bi[m], ny, ni[m] * nz)))
        ns = np.where((dot3(ns, ng) < 0)[:, None], -ns, ns)
        ng = np.where(front[:, None], ng, -ng)
        ns = np.where(front[:, None], ns, -ns)
        ns = np.where((dot3(ns, wo) > 0)[:, None], ns, ng)
        rb = RNG_BASE + int(bounce) + 1
        ei = lref.cdf_search(cdf, rng_f(keys, rb, 0))
        E = recs[ei]
        ok, y, wi, pl, Le = sample(E, textures, linear, P, rng_f(keys, rb, 1), rng_f(keys, rb, 2))
        tx, ty = lref.onb(ns)
        wil = np.stack([dot3(tx, wi), dot3(ty, wi), dot3(ns, wi)], -1)
        wol = np.stack([dot3(tx, wo), dot3(ty, wo), dot3(ns, wo)], -1)
        valid = hit & ok & (wil[:, 2] > 0) & (dot3(ng, wi) > 0) & (Le > 0).any(1)
        f, pb = bsdf_f_pdf(base[:, 0:3], metallic, roughness, lambert, wol, wil)
        pl2 = pl * pl
        wgt = pl2 / _fma(pb, pb, pl2)
        k = (wil[:, 2] * wgt) / pl
        porg = _fma(ng, F32(ray_eps), P)
        sv = y - porg
        sd = np.sqrt(dot3(sv, sv))
        sdir = sv * (F32(1.0) / sd)[:, None]
        contrib = T * f * Le * k[:, None]
        shadow = np.concatenate([porg, sdir, (sd * F32(0.999))[:, None], contrib], 1).astype(F32)
    shadow = np.where(valid[:, None], shadow, F32(0.0)).astype(F32)
    return L, valid, shadow


def irradiance64(corner, du, dv, normal, lit, Le, x, nx, sub=64):
    """E(x) = integral over the parallelogram corner + s du + t dv, (s, t) in the boxes `lit` [(s0, s1, t0, t1), ...], of Le cos_x cos_y / d^2 dA, by the midpoint rule
    on sub x sub cells per box, in float64.  normal: the emitter's unit normal (it emits on that side); nx: the receiver's unit normal."""
    corner, du, dv, normal, x, nx = (np.asarray(a, F64) for a in (corner, du, dv, normal, x, nx))
    dA = np.linalg.norm(np.cross(du, dv))
    tot = 0.0
    for s0, s1, t0, t1 in lit:
        s = s0 + (np.arange(sub) + 0.5) / sub * (s1 - s0)
        t = t0 + (np.arange(sub) + 0.5) / sub * (t1 - t0)
        S, Tt = np.meshgrid(s, t, indexing="ij")
        y = corner + S[..., None] * du + Tt[..., None] * dv
        dvec = y - x
        d2 = (dvec ** 2).sum(-1)
        d = np.sqrt(d2)
        cx = np.maximum((dvec @ nx) / d, 0.0)
        cy = np.maximum(-(dvec @ normal) / d, 0.0)
        tot += (cx * cy / d2).sum() * dA * (s1 - s0) * (t1 - t0) / (sub * sub)
    return Le * tot
