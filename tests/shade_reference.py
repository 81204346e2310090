"""One k_shade step per ray, written from the definitions (csrc/pt_kernels.hip P5-P8), for tests/test_shade_host.py and
tests/test_gpu_shade_step.py.

Not a restatement of the kernel: numpy over rays, every function with a `dt` argument.  dt = float64 is the reference; dt = float32 evaluates the same
formulas in float32 and is the yardstick the error bounds are measured with.  The inputs are the flat scene (true vertices), the description's materials,
textures and environment image, the rays, and a hit (primitive, u, v, t) per ray.  The emitter table, its cdf and the environment tables are rebuilt here from
the geometry and the image (`Scene.tables`): the device's tables are never read, except by the table-consistency test, which tests them.

Parts:
  Scene                  geometry, materials, textures, environment; emitter and environment pmf / cdf in `dt`
  surface / Bsdf         P, ng, ns (textures, normal map through the interpolated TBN, the orientation rules), Lambert + GGX (D, Smith G1, Schlick) and
                         the mixture pdf with the VNDF density
  step                   the whole step from the random numbers: emission and environment miss with MIS, the NEE sample, the continuation sample, Russian
                         roulette; with the decision margins and the condition numbers of every quantity
  check                  a candidate step (the device's records, or step(dt=float32)) against step(dt=float64): every quantity evaluated AT THE CANDIDATE'S
                         directions, and the candidate's directions against the recomputed samples
  ray_sets / edge_sets   the ray sets of the tests
  chi2_*                 the chi-square test of the sampler-density tests

ERROR BOUNDS.  A compared quantity q of class c is held to |q - q64| <= K_c 2^-23 kappa (relative for pdfs, throughputs and contributions, absolute for unit
vectors).  kappa is the condition of the quantity from its terms: 1/dd for D (dd = 1 + (n.h)^2 (alpha^2 - 1)), 1/(n.l), 1/(n.v), 1/|wo + wi| for the BSDF,
1/cos(theta_l) and (|y| + |P|)/d for the emitter pdf, 1/sin(theta) for the environment, (texel size)/(cdf step) for the position inside an environment texel, and for a
bilinear texture the texel offset w |u| + h |v| the coordinates' rounding moves the taps by (added: a texel value changes by at most 1 per texel).  K_c is MEASURED: the worst ratio error / (2^-23 kappa) of step(dt=float32) against step(dt=float64)
over all ray sets of the GPU test, times four, rounded up to a power of two (test_shade_host.py::test_float32_lies_within_the_bounds holds the constants to
that rule).  The factor four covers another order of operations on the device.

UNDECIDED.  A ray whose float64 decision margin is below the bound of what is compared — lobe choice |u - p_s|, Russian roulette |u - p|, a NEAREST or
environment texel boundary (pt_atan2 is good to 1e-5 rad), ng.wo, ns.wo, ng.wi, ns.wi near 0, an emitter cdf boundary — is left out of the comparisons that
depend on the decision and counted; at most MAX_UNDECIDED of a set of 63 rays or more."""
import math

import numpy as np

import glass_reference as gref
import lights_reference as lref
import trace_reference as tref
from lens_reference import F32, F64, rng_f

EPS = 2.0 ** -23
PI = math.pi
RR_START, RR_PMIN, ALPHA_MIN, NOV_MIN, SIN_MIN, SEGMENT = 3, 0.05, 1e-3, 1e-4, 1e-6, 0.999
SPEC_MIN, SPEC_MAX = 0.1, 0.9          # the clamp of the lobe-choice probability
T_INF = float(F32(3.0e38))
ATAN_MARGIN = 1e-5                     # pt_atan2's error in radians
MAX_UNDECIDED = gref.MAX_UNDECIDED
RAY_COUNTS = gref.RAY_COUNTS

# K per quantity class: the smallest power of two >= 4 x the worst ratio error / (2^-23 kappa) of step(float32) against step(float64), over every ray set of
# tests/test_gpu_shade_step.py with hits from trace_reference.closest_all.  Measured worst ratios (test_shade_host.py prints them):
K = {
    "bsdf": 32.0,      # f cos / pdf and pdf_out at the candidate's wi                          worst 5.10 (shade_textured, NEAREST)
    "contrib": 16.0,   # the NEE contribution T f cos w / p_l at the candidate's direction       worst 3.02 (shade_sky)
    "emit": 16.0,      # emission and environment-miss radiance with their MIS weight            worst 2.15 (shade_textured, the rays aimed at its emitter)
    "dir": 32.0,       # a component of a sampled direction, recomputed from the random numbers  worst 4.64 (shade_lobes, shade_sky)
    "org": 8.0,        # a component of P + eps ng                                               worst 1.02 (shade_sky)
    "tmax": 8.0,       # the shadow segment's length                                             worst 1.24 (shade_lobes)
    "ps": 8.0,         # the lobe-choice probability p_s                                         worst 1.01 (shade_textured, LINEAR)
    "normal": 8.0,     # a component of ng or ns                                                 worst 1.32 (shade_textured, LINEAR)
}
# On the MI355X (test_gpu_shade_step.py prints them), worst ratio per scene, lobes / textured NEAREST / textured LINEAR / sky:
#   bsdf 4.01 / 3.29 / 3.12 / 4.01   contrib 1.12 / 1.11 / 1.00 / 2.99   emit 0.58 / 2.12 / 2.12 / 2.08   dir 4.64 / 4.01 / 3.77 / 4.64
#   org 0.62 / 0.45 / 0.45 / 0.83    tmax 1.24 / 0.79 / 0.79 / -         (ps and normal are measured on the float32 evaluation alone: the device does not return them)
# Undecided share per set, the float64 reference alone and on the device alike: 0 on every camera set of shade_lobes and shade_textured, 1 of 128 on the grazing
# set of every scene, and on shade_sky 1 of 64 (64 rays), 1 of 513, 1 of 64 (normal incidence, float64 hits only).
MUTATIONS = ("balance", "no_p_area", "no_sin", "rr_no_division", "tmax_full", "g1_no_alpha", "vndf_no_warp", "bitangent_sign")


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(a):
    with np.errstate(all="ignore"):
        return a / np.sqrt(_dot(a, a))[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _lum(c):
    return c[..., 0] * 0.2126 + c[..., 1] * 0.7152 + c[..., 2] * 0.0722


def _sincos_turn(u, dt):
    """(sin, cos)(2 pi u), u in [0, 1): the quarter turn is taken off exactly, so float32 loses nothing to the size of the angle."""
    x4 = u * 4
    q = np.minimum(np.floor(x4), 3)
    a = (x4 - q) * (PI / 2)
    s, c = np.sin(a), np.cos(a)
    q = q.astype(np.int64)
    S = np.select([q == 0, q == 1, q == 2], [s, c, -s], -c)
    C = np.select([q == 0, q == 1, q == 2], [c, -s, -c], s)
    return S.astype(dt), C.astype(dt)


def _mis(p, q, mutation):
    """the weight of the strategy with pdf p against the one with pdf q: power heuristic, exponent 2."""
    with np.errstate(all="ignore"):
        if mutation == "balance":
            return p / (p + q)
        return (p * p) / (p * p + q * q)


class Scene:
    """The scene of a context: flat_scene() (true world vertices), description() and the environment image of the description."""

    def __init__(self, pt, desc):
        verts, idx, tri_mat = pt.flat_scene()
        mats, texs = pt.description()
        self.verts, self.idx, self.tri_mat = np.asarray(verts, F32), np.asarray(idx, np.int64).reshape(-1, 3), np.asarray(tri_mat, np.int64)
        self.textures = [np.asarray(t) for t in texs]
        self.linear = getattr(desc, "texture_filter", "nearest") == "linear"
        F = np.stack([m[0] for m in mats]).astype(F32)
        self.base, self.metallic, self.roughness, self.emissive = F[:, 0:4], F[:, 4], F[:, 5], F[:, 6:9]
        self.tex = np.asarray([m[1] for m in mats], np.int64)
        # the material classes of DESIGN.md §2, P6: a material without metal, of roughness 1 and without a metal-rough texture is a Lambert surface
        self.lambert = (self.metallic == 0) & (self.roughness >= 1) & (self.tex[:, 2] < 0)
        self.ray_eps = float(lref.scene_ray_eps(self.verts[:, 0:3]))
        self.scale = float(np.abs(self.verts[:, 0:3]).max())
        P = self.verts[:, 0:3].astype(F64)
        a, b, c = (P[self.idx[:, k]] for k in range(3))
        nrm = _cross(b - a, c - a)
        self.area = 0.5 * np.sqrt(_dot(nrm, nrm))
        w = self.area * _lum(self.emissive[self.tri_mat].astype(F64))
        self.em_prims = np.flatnonzero(w > 0)                      # emitters in primitive order
        self.em_of_prim = np.full(len(self.idx), -1, np.int64)
        self.em_of_prim[self.em_prims] = np.arange(len(self.em_prims))
        self.em_weight = w[self.em_prims]
        env = getattr(desc, "env", None)
        self.env = None if env is None else np.asarray(env, F32)
        self.env_ok = False
        if self.env is not None:
            h = self.env.shape[0]
            sin_row = np.sin(PI * (np.arange(h) + 0.5) / h)
            self.env_weight = np.maximum(_lum(self.env.astype(F64)) * sin_row[:, None], 0.0)
            self.env_ok = bool(self.env_weight.sum() > 0)
        self.n_em = len(self.em_prims)
        # light-kind selection: the environment is sampled when it has power, with probability 1/2 beside emitters
        self.p_env = (0.5 if self.n_em else 1.0) if self.env_ok else 0.0
        self.p_area = 1.0 - self.p_env
        self._tabs = {}

    def tables(self, dt):
        """pmf and cdf of the emitters (A_i lum_i / sum) and of the environment texels (lum sin(theta_row) / sum: row marginal, per-row conditional), summed in `dt`."""
        if dt in self._tabs:
            return self._tabs[dt]
        t = {}
        if self.n_em:
            w = self.em_weight.astype(dt)
            run = np.cumsum(w, dtype=dt)
            t["em_pmf"], t["em_cdf"] = w / run[-1], run / run[-1]
            t["em_cdf"][-1] = 1
        if self.env_ok:
            f = self.env_weight.astype(dt)
            rows = np.cumsum(f, 1, dtype=dt)
            rowsum = rows[:, -1]
            total = np.cumsum(rowsum, dtype=dt)
            w_ = f.shape[1]
            with np.errstate(all="ignore"):
                cond = np.where(rowsum[:, None] > 0, rows / rowsum[:, None], (np.arange(w_, dtype=dt) + 1) / w_).astype(dt)
            cond[:, -1] = 1
            marg = (total / total[-1]).astype(dt)
            marg[-1] = 1
            t["env_pmf"], t["env_marg"], t["env_cond"] = f / total[-1], marg, cond
        self._tabs[dt] = t
        return t


def _texel(tex, y, x, dt):
    return tex[y, x].astype(dt) / dt(255)


def tex_fetch(tex, u, v, linear, dt):
    """(rgba (n, 4), margin): REPEAT wrap; NEAREST takes the texel the point lies in, LINEAR blends the four texels around it (centres at i + 0.5).  margin: the
    distance to the nearest texel boundary in texels (NEAREST), infinity for LINEAR, which is continuous."""
    h, w = tex.shape[0], tex.shape[1]
    fu, fv = u - np.floor(u), v - np.floor(v)
    xs, ys = fu * w, fv * h
    if not linear:
        x, y = np.minimum(xs.astype(np.int64), w - 1), np.minimum(ys.astype(np.int64), h - 1)
        margin = np.minimum(np.abs(xs - np.round(xs)), np.abs(ys - np.round(ys))).astype(F64)
        return _texel(tex, y, x, dt), margin
    x, y = xs - dt(0.5), ys - dt(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    tx, ty = (x - x0)[:, None], (y - y0)[:, None]
    x0, y0 = x0.astype(np.int64) % w, y0.astype(np.int64) % h
    x1, y1 = (x0 + 1) % w, (y0 + 1) % h
    lerp = lambda a, b, t: a + t * (b - a)
    top = lerp(_texel(tex, y0, x0, dt), _texel(tex, y0, x1, dt), tx)
    bot = lerp(_texel(tex, y1, x0, dt), _texel(tex, y1, x1, dt), tx)
    return lerp(top, bot, ty).astype(dt), np.full(len(u), np.inf)


def surface(sc, d, prim, u, v, dt=F64, mutation=None):
    """The surface of the hits (prim, u, v) seen against d.  Rays with prim < 0 get primitive 0: mask them."""
    k = np.maximum(np.asarray(prim, np.int64), 0)
    V = sc.verts[sc.idx[k]].astype(dt)                      # (n, 3 corners, 12)
    u, v = np.asarray(u).astype(dt), np.asarray(v).astype(dt)
    w = 1 - u - v
    bary = lambda X: X[:, 0] * w[:, None] + X[:, 1] * u[:, None] + X[:, 2] * v[:, None]
    d = np.asarray(d).astype(dt)
    wo = -d
    S = {}
    with np.errstate(all="ignore"):
        pos = V[:, :, 0:3]
        S["P"] = bary(pos)
        ng = _unit(_cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]))
        ni = bary(V[:, :, 3:6])
        ns = _unit(ni)
        mat = sc.tri_mat[k]
        base, metallic, roughness = sc.base[mat].astype(dt).copy(), sc.metallic[mat].astype(dt).copy(), sc.roughness[mat].astype(dt).copy()
        margin = np.full(len(k), np.inf)
        ktex = np.zeros(len(k))
        tids = sc.tex[mat]
        if (tids >= 0).any():
            uv = bary(V[:, :, 10:12])
            tu, tv = uv[:, 0], uv[:, 1]

            def fetch(col):
                out = np.ones((len(k), 4), dt)
                for t_id in np.unique(tids[:, col][tids[:, col] >= 0]):
                    m = tids[:, col] == t_id
                    out[m], mg = tex_fetch(sc.textures[t_id], tu[m], tv[m], sc.linear, dt)
                    margin[m] = np.minimum(margin[m], mg)
                    if sc.linear:
                        th, tw = sc.textures[t_id].shape[:2]
                        ktex[m] = np.maximum(ktex[m], (tw * np.abs(tu[m]) + th * np.abs(tv[m])).astype(F64))
                return out
            cc, cn, cm = fetch(0), fetch(1), fetch(2)
            has = tids >= 0
            base = np.where(has[:, 0:1], base * cc, base)
            roughness = np.where(has[:, 2], roughness * cm[:, 1], roughness)          # glTF: G = roughness, B = metallic
            metallic = np.where(has[:, 2], metallic * cm[:, 2], metallic)
            nt = 2 * cn[:, 0:3] - 1
            N, Tg = V[:, :, 3:6], V[:, :, 6:9]
            Bt = _cross(N, Tg)
            if mutation != "bitangent_sign":
                Bt = Bt * V[:, :, 9:10]                      # the bitangent of a vertex: normalize(cross(N, T) * handedness)
            Bt = _unit(Bt)
            mapped = _unit(bary(Tg) * nt[:, 0:1] + bary(Bt) * nt[:, 1:2] + ni * nt[:, 2:3])
            ns = np.where(has[:, 1:2], mapped, ns)
        # orientation: both normals on wo's side; a shading normal that still looks away from wo gives way to the face normal
        gw, sg = _dot(ng, wo), _dot(ns, ng)
        front = gw > 0
        ns = np.where((sg < 0)[:, None], -ns, ns)
        flip = np.where(front, 1, -1).astype(dt)[:, None]
        ng, ns = ng * flip, ns * flip
        sw = _dot(ns, wo)
        ns = np.where((sw > 0)[:, None], ns, ng)
    S.update(ng=ng, ns=ns, front=front, wo=wo, base=base[:, 0:3], metallic=metallic, roughness=roughness, lambert=sc.lambert[mat], mat=mat, tex_margin=margin,
             ktex=ktex, side_margin=np.minimum(np.abs(gw), np.minimum(np.abs(sg), np.abs(sw)) / (1 + ktex)).astype(F64), em=sc.em_of_prim[k], Le=sc.emissive[mat].astype(dt))
    return S


def _sub(S, sel):
    return {k: v[sel] for k, v in S.items()}


def onb(n):
    """Duff et al. 2017, "Building an orthonormal basis, revisited": (t, b) with t x b = n."""
    sg = np.copysign(1, n[..., 2]).astype(n.dtype)
    with np.errstate(all="ignore"):
        a = -1 / (sg + n[..., 2])
        bb = n[..., 0] * n[..., 1] * a
        t = np.stack([1 + sg * n[..., 0] * n[..., 0] * a, sg * bb, -sg * n[..., 0]], -1)
        b = np.stack([bb, sg + n[..., 1] * n[..., 1] * a, -n[..., 1]], -1)
    return t, b


class Bsdf:
    """Lambert, or Lambert + GGX microfacet reflection (glTF metallic-roughness): cd = base (1 - metallic), F0 = 0.04 (1 - metallic) + base metallic,
    alpha = max(roughness^2, ALPHA_MIN).  Evaluated in world space against the shading normal."""

    def __init__(self, S, dt, mutation=None):
        self.S, self.dt, self.mutation = S, dt, mutation
        m = S["metallic"][:, None]
        self.cd = S["base"] * (1 - m)
        self.f0 = 0.04 * (1 - m) + S["base"] * m
        self.alpha = np.maximum(S["roughness"] * S["roughness"], dt(ALPHA_MIN))
        self.lambert = S["lambert"]
        self.nv_raw = _dot(S["ns"], S["wo"])
        self.nv = np.maximum(self.nv_raw, dt(NOV_MIN))
        # lobe choice: the luminance of the Fresnel reflectance at n.v against the diffuse albedo's, clamped; no diffuse albedo -> always the specular lobe
        with np.errstate(all="ignore"):
            lf, ld = _lum(self.fresnel(self.nv)), _lum(self.cd)
            ps = np.where(ld > 0, np.clip(lf / (lf + ld), SPEC_MIN, SPEC_MAX), 1)
        self.ps = np.where(self.lambert, 0, ps).astype(dt)
        self.ps_margin = np.where((ld > 0) & (ld < 1e-5) & ~self.lambert, 0.0, np.inf)      # an albedo that is zero to one precision only

    def fresnel(self, c):
        m = np.maximum(1 - c, 0)
        return self.f0 + (1 - self.f0) * (m ** 5)[:, None]

    def g1(self, x):
        a2 = self.alpha * self.alpha
        if self.mutation == "g1_no_alpha":
            return 2 * x / (x + np.sqrt(x * x + (1 - x * x)))
        return 2 * x / (x + np.sqrt(x * x + a2 * (1 - x * x)))

    def eval(self, wi):
        """(f (n, 3), pdf, kappa) at the world direction wi: pdf = p_s G1(v) D / (4 n.v) + (1 - p_s) n.l / pi."""
        S, dt = self.S, self.dt
        with np.errstate(all="ignore"):
            nl = _dot(S["ns"], wi)
            fd = self.cd / PI
            pd = nl / PI
            hv = S["wo"] + wi
            hl = np.sqrt(_dot(hv, hv))
            h = hv / hl[:, None]
            noh, voh = _dot(S["ns"], h), _dot(S["wo"], h)
            a2 = self.alpha * self.alpha
            dd = 1 + noh * noh * (a2 - 1)
            D = a2 / (PI * dd * dd)
            gv, gl = self.g1(self.nv), self.g1(nl)
            spec = D * gv * gl / (4 * self.nv * nl)
            f = fd + self.fresnel(voh) * spec[:, None]
            pdf = self.ps * (gv * D / (4 * self.nv)) + (1 - self.ps) * pd
            lam = self.lambert
            self.parts = (np.where(lam, 0, gv * D / (4 * self.nv)), pd)          # the two densities of the mixture
            f = np.where(lam[:, None], fd, f).astype(dt)
            pdf = np.where(lam, pd, pdf).astype(dt)
            # D G1(v) / (4 n.v) enters f with the share s_f (per channel) and the pdf with the share s_p: its condition 1/dd weighs on a quantity by the share it has of it
            s_f = np.where(lam[:, None], 0, self.fresnel(voh) * spec[:, None] / f)
            s_p = np.where(lam, 0, self.ps * (gv * D / (4 * self.nv)) / pdf)
            s_f, s_p = np.nan_to_num(s_f.astype(F64), nan=1.0), np.nan_to_num(s_p.astype(F64), nan=1.0)
            # so does G1(v) / (4 n.v), the other factor the two share
            rest = np.where(lam, 1 / np.abs(nl), 1 + 1 / np.abs(nl) + 1 / hl).astype(F64)
            kd = np.where(lam, 0, 1 / np.abs(dd) + 1 / self.nv).astype(F64)
            tex = S["ktex"]
            kappa = dict(pdf=rest + s_p * kd + tex, ratio=rest + np.abs(s_f - s_p[:, None]).max(1) * kd + tex, f=rest + (s_f.max(1) + 2 * s_p) * kd + tex)
        return f, pdf, kappa

    def sample(self, ul, s1, s2):
        """wi from three random numbers: the lobe by ul < p_s, cosine-weighted hemisphere or Heitz 2018 ("Sampling the GGX distribution of visible normals") in the
        basis of onb(ns).  Returns (wi world, ok, kappa of a component, lobe margin |ul - p_s|)."""
        S, dt = self.S, self.dt
        tx, ty = onb(S["ns"])
        wo = np.stack([_dot(tx, S["wo"]), _dot(ty, S["wo"]), self.nv_raw], -1)
        sn, cs = _sincos_turn(s2, dt)
        with np.errstate(all="ignore"):
            r = np.sqrt(s1)
            cosine = np.stack([r * cs, r * sn, np.sqrt(np.maximum(1 - s1, 0))], -1)
            a = self.alpha[:, None]
            vh = _unit(np.concatenate([a * wo[:, 0:2], wo[:, 2:3]], -1))
            lensq = vh[:, 0] * vh[:, 0] + vh[:, 1] * vh[:, 1]
            il = 1 / np.sqrt(lensq)
            zero = np.zeros_like(il)
            t1 = np.where((lensq > 0)[:, None], np.stack([-vh[:, 1] * il, vh[:, 0] * il, zero], -1), np.stack([zero + 1, zero, zero], -1))
            t2 = _cross(vh, t1)
            p1, p2 = r * cs, r * sn
            if self.mutation != "vndf_no_warp":
                s = 0.5 * (1 + vh[:, 2])
                p2 = (1 - s) * np.sqrt(np.maximum(1 - p1 * p1, 0)) + s * p2
            pz = np.sqrt(np.maximum(1 - p1 * p1 - p2 * p2, 0))
            nh = t1 * p1[:, None] + t2 * p2[:, None] + vh * pz[:, None]
            hs = np.concatenate([a * nh[:, 0:2], np.maximum(nh[:, 2:3], 0)], -1)      # its length is the condition of the half vector: nh is good to 2^-23, absolutely
            hsl = np.sqrt(_dot(hs, hs))
            h = hs / hsl[:, None]
            ggx = 2 * _dot(wo, h)[:, None] * h - wo
            spec = ul < self.ps
            wil = np.where(spec[:, None], ggx, cosine).astype(dt)
            wi = tx * wil[:, 0:1] + ty * wil[:, 1:2] + S["ns"] * wil[:, 2:3]
            lxy = np.sqrt(wo[:, 0] * wo[:, 0] + wo[:, 1] * wo[:, 1])
            k_spec = 1 + 1 / np.maximum(pz, 1e-30) + np.where(lxy > 0, self.alpha / np.maximum(lxy, 1e-30), 0) + 1 / np.maximum(hsl, 1e-30)
            kappa = np.where(spec, k_spec, 1).astype(F64) + S["ktex"]
        return wi.astype(dt), wil[:, 2] > 0, wil[:, 2].astype(F64), kappa, np.minimum(np.abs(ul.astype(F64) - self.ps.astype(F64)), self.ps_margin)


def env_at(sc, tabs, d, dt, mutation=None):
    """The lat-long environment in direction d (row 0 = +y, u = atan2(z, x) / 2 pi + 1/2, v = theta / pi): (Le, solid-angle pdf of the environment sampler,
    sin(theta) clamped at SIN_MIN, the angular distance to the nearest texel boundary, (y, x))."""
    h, w = sc.env.shape[0], sc.env.shape[1]
    with np.errstate(all="ignore"):
        phi = np.arctan2(d[:, 2], d[:, 0])
        dy = np.clip(d[:, 1], -1, 1)
        st = np.sqrt(np.maximum(1 - dy * dy, 0))
        theta = np.arctan2(st, dy)
        xs, ys = (phi / (2 * PI) + 0.5) * w, (theta / PI) * h
        x, y = np.clip(np.floor(xs).astype(np.int64), 0, w - 1), np.clip(np.floor(ys).astype(np.int64), 0, h - 1)
        my = np.where((np.round(ys) > 0) & (np.round(ys) < h), np.abs(ys - np.round(ys)) * (PI / h), np.inf)      # the poles are no boundaries
        margin = np.minimum(np.abs(xs - np.round(xs)) * (2 * PI / w), my).astype(F64)
        Le = sc.env[y, x].astype(dt)
        stc = np.maximum(st, dt(SIN_MIN))
        if sc.env_ok:
            pdf = tabs["env_pmf"][y, x] * (w * h) / (2 * PI * PI * (1 if mutation == "no_sin" else stc))
        else:
            pdf = np.zeros(len(d), dt)
    return Le, pdf.astype(dt), stc.astype(F64), margin, (y, x)


def _search(cdf, r):
    """the first index whose cdf exceeds r (the last one at most), and the distance of r to the nearest cdf step."""
    i = np.minimum(np.searchsorted(cdf, r, side="right"), len(cdf) - 1)
    return i, np.abs(cdf.astype(F64)[None, :] - np.asarray(r, F64)[:, None]).min(1)


def env_sample(sc, tabs, r1, r2, dt):
    """The environment sampler: the row by the marginal cdf, the column by the row's conditional cdf, uniform inside the texel.  Returns (direction, kappa of a
    component, the distance to the nearest cdf step over the number of float32 additions behind that step)."""
    h, w = sc.env.shape[0], sc.env.shape[1]
    marg, cond = tabs["env_marg"], tabs["env_cond"]
    y, m_y = _search(marg, r1)
    m0, m1 = np.where(y > 0, marg[np.maximum(y - 1, 0)], 0).astype(dt), marg[y]
    row = cond[y]
    x = np.minimum((row <= r2[:, None]).sum(1), w - 1)
    m_x = np.abs(row.astype(F64) - r2.astype(F64)[:, None]).min(1)
    r = np.arange(len(y))
    c0, c1 = np.where(x > 0, row[r, np.maximum(x - 1, 0)], 0).astype(dt), row[r, x]
    with np.errstate(all="ignore"):
        xv = np.clip(np.where(m1 > m0, (r1 - m0) / (m1 - m0), 0.5), 0, 0.999999).astype(dt)
        xu = np.clip(np.where(c1 > c0, (r2 - c0) / (c1 - c0), 0.5), 0, 0.999999).astype(dt)
        u, v = (x + xu) / w, (y + xv) / h
        s2, c2 = _sincos_turn(u, dt)
        st, ct = _sincos_turn(v * dt(0.5), dt)
        wi = np.stack([st * -c2, ct, st * -s2], -1).astype(dt)
        kappa = (1 + (PI / h) / np.maximum(m1 - m0, 1e-30) + (2 * PI / w) / np.maximum(c1 - c0, 1e-30)).astype(F64)      # the texel's size over its cdf step
    return wi, kappa, np.minimum(m_y / (w + h + 1), m_x / (w + 1))


def nee_eval(sc, tabs, S, B, T, wi, light, dt, mutation=None, y=None):
    """The next-event contribution T f cos w / p_l of the direction wi towards `light` (-1: the environment, else the emitter's index, with y the point on it).
    Returns (valid, contribution, kappa, texel margin)."""
    n = len(wi)
    with np.errstate(all="ignore"):
        f, pb, kb = B.eval(wi)
        nl = _dot(S["ns"], wi)
        valid = (nl > 0) & (_dot(S["ng"], wi) > 0)
        margin = np.full(n, np.inf)
        env = light < 0
        Le, pl, kl = np.zeros((n, 3), dt), np.ones(n, dt), np.ones(n)
        if env.any():
            Le_e, pe, st, mg, _ = env_at(sc, tabs, wi[env], dt, mutation)
            Le[env], pl[env], kl[env], margin[env] = Le_e, pe * dt(sc.p_env), 1 / st, mg
        if (~env).any():
            e = np.flatnonzero(~env)
            j = light[e]
            tri = sc.verts[sc.idx[sc.em_prims[j]]][:, :, 0:3].astype(dt)
            nrm = _unit(_cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]))
            dv = y[e] - S["P"][e]
            d2 = _dot(dv, dv)
            cosl = -_dot(nrm, wi[e])
            area = sc.area[sc.em_prims[j]].astype(dt)
            pl[e] = tabs["em_pmf"][j] * d2 / (area * cosl) * dt(sc.p_area)
            Le[e] = sc.emissive[sc.tri_mat[sc.em_prims[j]]].astype(dt)
            valid[e] &= (cosl > 0) & (d2 > 0)
            kl[e] = 1 / np.abs(cosl) + (np.sqrt(_dot(y[e], y[e])) + np.sqrt(_dot(S["P"][e], S["P"][e]))) / np.sqrt(d2)
        valid &= pl > 0
        wgt = _mis(pl, pb, mutation)
        contrib = T * f * Le * (nl * wgt / pl)[:, None]
    return valid, contrib.astype(dt), (kb["f"] + kl).astype(F64), margin


def cont_eval(S, B, T, wi, rb, keys, dt, mutation=None):
    """The continuation along wi: (ok, pdf_out, T_out, kappa of pdf_out and of T_out, the Russian-roulette survival value max T_out before its clamp and the
    random number it is compared with; both infinite where there is no roulette)."""
    with np.errstate(all="ignore"):
        f, pdf, kb = B.eval(wi)
        nl = _dot(S["ns"], wi)
        ok = (nl > 0) & (_dot(S["ng"], wi) > 0) & (pdf > 0)
        To = T * f * (nl / pdf)[:, None]
        rr = (np.full(len(wi), np.inf), np.full(len(wi), np.inf))
        if rb >= RR_START:
            q = To.max(1)
            p = np.clip(q, dt(RR_PMIN), 1)
            ur = rng_f(keys, rb, 6).astype(dt)
            rr = (q.astype(F64), ur.astype(F64))
            ok &= (q > 0) & (ur < p)
            if mutation != "rr_no_division":
                To = To / p[:, None]
    return ok, pdf, To.astype(dt), kb, rr


def step(sc, rays, hit, bounce, max_bounces, dt=F64, mutation=None):
    """One shading step of the rays (o, d, T, pdf, keys) with the hits (prim, u, v, t) at `bounce`, from the random numbers of bounce + 1.  A dict of the
    records the step produces — lpath, alive / o / d / T / pdf, shadow / so / sd / tmax / contrib — with, per ray, the decision margins (m_*), the condition
    numbers (k_*) and what the NEE sample chose (light: -1 the environment, else the emitter)."""
    o, d, T, pp, keys = (np.asarray(rays[k]) for k in ("o", "d", "T", "pdf", "keys"))
    prim, t = np.asarray(hit["prim"], np.int64), np.asarray(hit["t"]).astype(dt)
    n, b, rb = len(keys), int(bounce), int(bounce) + 1
    d, T, pp = d.astype(dt), T.astype(dt), pp.astype(dt)
    tabs = sc.tables(dt)
    z3, z1, inf = (lambda: np.zeros((n, 3), dt)), (lambda: np.zeros(n, dt)), (lambda: np.full(n, np.inf))
    R = dict(lpath=z3(), alive=np.zeros(n, bool), o=z3(), d=z3(), T=z3(), pdf=z1(), shadow=np.zeros(n, bool), so=z3(), sd=z3(), tmax=z1(), contrib=z3(),
             light=np.full(n, -2, np.int64), y=z3(), k_emit=np.ones(n), k_dir_nee=np.ones(n), k_dir=np.ones(n), m_texel=inf(), m_side=inf(), m_lobe=inf(),
             m_cdf=inf(), m_wi=inf(), m_nee=inf(), ps=z1(), ktex=z1().astype(F64), hitm=prim >= 0)
    hitm = prim >= 0
    miss = ~hitm
    with np.errstate(all="ignore"):
        if sc.env is not None and miss.any():      # the environment seen by a ray that left the scene, weighted against the environment's NEE
            Le, pe, st, mg, _ = env_at(sc, tabs, d[miss], dt, mutation)
            w = 1 if b == 0 else _mis(pp[miss], pe * dt(sc.p_env), mutation)
            R["lpath"][miss] = T[miss] * Le * np.asarray(w, dt)[..., None]
            R["k_emit"][miss], R["m_texel"][miss] = 1 / st, mg
        if not hitm.any():
            return R
        S = surface(sc, d, prim, hit["u"], hit["v"], dt, mutation)
        R["m_texel"][hitm] = S["tex_margin"][hitm]      # in texels: a texture coordinate is good to far less than the 2e-5 the angles are held to
        R["m_side"][hitm] = S["side_margin"][hitm]
        R["ktex"][hitm] = S["ktex"][hitm]
        em = hitm & (S["em"] >= 0) & S["front"]
        if em.any():      # emission of a front face, weighted against the emitters' NEE: p_l = P(select) d^2 / (A cos) p_area
            j = S["em"][em]
            cosl = _dot(S["ng"], S["wo"])[em]
            w = 1
            if b > 0:
                pl = tabs["em_pmf"][j] * (t[em] * t[em]) / (sc.area[sc.em_prims[j]].astype(dt) * cosl)
                if mutation != "no_p_area":
                    pl = pl * dt(sc.p_area)
                w = _mis(pp[em], pl, mutation)
            R["lpath"][em] = T[em] * S["Le"][em] * np.asarray(w, dt)[..., None]
            R["k_emit"][em] = 1 / np.abs(cosl)
        if b >= int(max_bounces):
            return R
        B = Bsdf(S, dt, mutation)
        R["ps"], R["ng"], R["ns"] = B.ps, S["ng"], S["ns"]
        porg = S["P"] + S["ng"] * dt(sc.ray_eps)
        # ---- next-event estimation: one light sample, the environment or an emitter ----
        use_env = np.zeros(n, bool)
        if sc.env_ok:
            use_env = hitm & (np.ones(n, bool) if sc.n_em == 0 else rng_f(keys, rb, 7) < sc.p_env)
        r1, r2 = rng_f(keys, rb, 1).astype(dt), rng_f(keys, rb, 2).astype(dt)
        wi, light, y, sdir, tmax = z3(), np.full(n, -2, np.int64), z3(), z3(), z1()
        if use_env.any():
            wi[use_env], R["k_dir_nee"][use_env], R["m_cdf"][use_env] = env_sample(sc, tabs, r1[use_env], r2[use_env], dt)
            light[use_env], sdir[use_env], tmax[use_env] = -1, wi[use_env], T_INF
        em_nee = hitm & ~use_env & (sc.n_em > 0)
        if em_nee.any():
            u0 = rng_f(keys, rb, 0)[em_nee].astype(dt)
            j, mc = _search(tabs["em_cdf"], u0)
            R["m_cdf"][em_nee] = mc / (sc.n_em + 1)
            tri = sc.verts[sc.idx[sc.em_prims[j]]][:, :, 0:3].astype(dt)
            su = np.sqrt(r1[em_nee])
            yy = tri[:, 0] + (tri[:, 1] - tri[:, 0]) * (su * (1 - r2[em_nee]))[:, None] + (tri[:, 2] - tri[:, 0]) * (su * r2[em_nee])[:, None]
            dv = yy - S["P"][em_nee]
            dist = np.sqrt(_dot(dv, dv))
            sv = yy - porg[em_nee]
            sl = np.sqrt(_dot(sv, sv))
            wi[em_nee], light[em_nee], y[em_nee], sdir[em_nee] = dv / dist[:, None], j, yy, sv / sl[:, None]
            tmax[em_nee] = sl * (1.0 if mutation == "tmax_full" else SEGMENT)
            R["k_dir_nee"][em_nee] = (np.sqrt(_dot(yy, yy)) + np.sqrt(_dot(S["P"][em_nee], S["P"][em_nee]))).astype(F64) / np.minimum(dist, sl)
        nee = use_env | em_nee
        if nee.any():
            sub = _sub(S, nee)
            Bn = Bsdf(sub, dt, mutation)
            valid, contrib, _, mg = nee_eval(sc, tabs, sub, Bn, T[nee], wi[nee], light[nee], dt, mutation, y[nee])
            R["m_texel"][nee] = np.minimum(R["m_texel"][nee], np.where(valid, mg, np.inf))
            R["m_nee"][nee] = np.minimum(np.abs(_dot(sub["ns"], wi[nee])), np.abs(_dot(sub["ng"], wi[nee]))).astype(F64)
            idx = np.flatnonzero(nee)[valid]
            R["shadow"][idx] = True
            R["so"][idx], R["sd"][idx], R["tmax"][idx], R["contrib"][idx] = porg[idx], sdir[idx], tmax[idx], contrib[valid]
            R["light"][nee], R["y"][nee] = light[nee], y[nee]
        # ---- the continuation and Russian roulette ----
        ul, s1, s2 = (rng_f(keys, rb, k).astype(dt) for k in (3, 4, 5))
        wi_c, ok_s, wz, R["k_dir"], R["m_lobe"] = B.sample(ul, s1, s2)
        ok, pdf, To, kb, R["rr"] = cont_eval(S, B, T, wi_c, rb, keys, dt, mutation)
        R["k_ratio"] = kb["ratio"]
        R["m_wi"] = np.minimum(np.abs(wz), np.abs(_dot(S["ng"], wi_c)).astype(F64))
        alive = hitm & ok_s & ok
        R["alive"] = alive
        for k, v in (("o", porg), ("d", wi_c), ("T", To)):
            R[k][alive] = v[alive]
        R["pdf"][alive] = pdf[alive]
        R["m_lobe"] = np.where(hitm & ~B.lambert & ((B.ps < 1) | (B.ps_margin == 0)), R["m_lobe"], np.inf)
    return R


def hits_of(sc, o, d, grazing=False):
    """The hits of the float64 search of all triangles (trace_reference.closest_all): dict(prim, u, v, t), float64.  grazing: the nearest triangle whose
    interior the ray meets, however flat the angle (closest_all leaves a ray that nearly lies in a triangle's plane without a hit: no precision decides it; the
    grazing set aims at interiors, where the hit is decided and only the angle is extreme)."""
    if grazing:
        a, b, c = tref.triangles(sc.verts, sc.idx)
        with np.errstate(all="ignore"):
            t, u, v, m, _, _ = tref.pair_terms(a[None], b[None], c[None], np.asarray(o, F64)[:, None], np.asarray(d, F64)[:, None])
            t = np.where((m > 0) & (t > 0), t, np.inf)
        prim = np.where(np.isfinite(t.min(1)), t.argmin(1), -1)
    else:
        prim = tref.closest_all(sc.verts, sc.idx, o, d).prim
    t, u, v, _, _, _ = tref.pair_at(sc.verts, sc.idx, o, d, prim)
    hit = prim >= 0
    return dict(prim=np.where(hit, prim, -1), u=np.where(hit, u, 0.0), v=np.where(hit, v, 0.0), t=np.where(hit, t, -1.0))


def _which_emitter(sc, so, sd, tmax):
    """The emitter a shadow record points at, in float64: the emitter whose plane the ray meets inside the triangle (1e-3 slack) nearest to tmax / SEGMENT.
    Returns (index or -1, the point on its plane, its edge margin min(u, v, 1 - u - v))."""
    tri = sc.verts[sc.idx[sc.em_prims]][:, :, 0:3].astype(F64)            # (m, 3, 3)
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    nrm = _cross(e1, e2)
    with np.errstate(all="ignore"):
        tt = ((a[None] - so[:, None]) * nrm[None]).sum(-1) / (sd[:, None] * nrm[None]).sum(-1)      # (n, m)
        y = so[:, None] + sd[:, None] * tt[..., None]
        q = y - a[None]
        d11, d12, d22 = _dot(e1, e1)[None], _dot(e1, e2)[None], _dot(e2, e2)[None]
        q1, q2 = (q * e1[None]).sum(-1), (q * e2[None]).sum(-1)
        det = d11 * d22 - d12 * d12
        bu, bv = (q1 * d22 - q2 * d12) / det, (q2 * d11 - q1 * d12) / det
        mb = np.minimum(np.minimum(bu, bv), 1 - bu - bv)
        off = np.where((mb > -1e-3) & (tt > 0), np.abs(tt - tmax[:, None] / SEGMENT), np.inf)
        near = off <= off.min(1)[:, None] + 1e-3 * tmax[:, None]
        j = np.where(near, mb, -np.inf).argmax(1)           # of the emitters met at that distance (a shared edge), the one the point lies deepest in
    r = np.arange(len(so))
    return np.where(np.isfinite(off[r, j]), j, -1), y[r, j], mb[r, j]


def check(sc, rays, hit, bounce, max_bounces, got, what="", report=None):
    """A candidate step `got` (ptc_debug_shade_step's records, or step(dt=float32)) against the float64 reference.  On every ray: finite, non-negative outputs;
    lpath; every record evaluated at the candidate's own directions within the bounds.  On every decided ray: the records exist where the reference has them,
    and the candidate's directions are the recomputed samples.  Returns (undecided share, worst ratio error / (2^-23 kappa) per quantity class); `report`, a
    dict, collects the worst ratios instead of the assertions on K (the measurement)."""
    n, b, rb = len(rays["keys"]), int(bounce), int(bounce) + 1
    ref = step(sc, rays, hit, bounce, max_bounces, F64)
    g = {k: np.asarray(v) for k, v in got.items()}
    G = lambda k: g[k].astype(F64)
    T_in = np.asarray(rays["T"], F64)
    hitm = ref["hitm"]
    worst = {k: 0.0 for k in K}
    fails = []

    def hold(cls, err, kappa, sel, label):
        if not np.any(sel):
            return
        ratio = np.where(sel, err / (EPS * kappa), 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        i = int(ratio.argmax())
        worst[cls] = max(worst[cls], float(ratio[i]))
        if report is None and ratio[i] > K[cls]:
            fails.append(f"{label}: ray {i} error / (2^-23 kappa) = {ratio[i]:.3g} > K[{cls}] = {K[cls]} (kappa {np.broadcast_to(kappa, ratio.shape)[i]:.3g})")

    def rel(a, r):      # the largest relative deviation over the channels; exact zeros must be zeros
        with np.errstate(all="ignore"):
            e = np.abs(a - r) / np.abs(r)
        return np.where(r == 0, np.where(a == 0, 0.0, np.inf), e).max(-1) if a.ndim > 1 else np.where(r == 0, np.where(a == 0, 0.0, np.inf), e)

    # ---- always, with no tolerance ----
    for k in ("lpath", "o", "d", "T", "pdf", "so", "sd", "tmax", "contrib"):
        assert np.isfinite(g[k]).all(), f"{what}: {k} is not finite"
    assert (g["T"] >= 0).all() and (g["contrib"] >= 0).all() and (g["lpath"] >= 0).all(), f"{what}: a negative throughput, contribution or radiance"
    assert (g["pdf"][g["alive"]] > 0).all(), f"{what}: a continuation without a positive pdf"
    if b >= int(max_bounces):
        assert not g["alive"].any() and not g["shadow"].any(), f"{what}: a record at the last bounce"
    # ---- decisions ----
    bd = K["dir"] * EPS
    why = dict(texel=ref["m_texel"] < 2 * ATAN_MARGIN, side=ref["m_side"] < 2 * K["normal"] * EPS)
    if b < int(max_bounces):
        why["lobe"] = ref["m_lobe"] < K["ps"] * EPS * (1 + ref["ktex"])
        if "rr" in ref:      # the survival probability clamp(q, RR_PMIN, 1) over q's bound against the random number
            q, ur = ref["rr"]
            dq = K["bsdf"] * EPS * np.minimum(ref["k_ratio"], 1e30)
            with np.errstate(all="ignore"):
                lo, hi = np.clip(q * (1 - dq), RR_PMIN, 1), np.clip(q * (1 + dq), RR_PMIN, 1)
                why["rr"] = hitm & np.isfinite(q) & (q > 0) & (ur >= lo - EPS) & (ur <= hi + EPS) & ~((lo == 1) & (hi == 1))
        why["wi"] = hitm & (ref["m_wi"] < 2 * bd * np.minimum(ref["k_dir"], 1e30))
        has_nee = ref["light"] > -2
        why["nee"] = has_nee & (ref["m_nee"] < 2 * bd * np.minimum(ref["k_dir_nee"], 1e30))
        why["cdf"] = has_nee & (ref["m_cdf"] < 2.0 ** -24)      # a float32 running sum of n terms is good to n 2^-24, and the random numbers lie on that grid
    und = np.zeros(n, bool)
    for m in why.values():
        und |= m
    dec = ~und
    # ---- emission and environment: lpath ----
    hold("emit", rel(G("lpath"), ref["lpath"]), ref["k_emit"], dec, "lpath")
    quiet = ~(ref["lpath"] > 0).any(1)
    assert not g["lpath"][quiet & dec].any(), f"{what}: radiance where nothing emits"
    if b < int(max_bounces):
        S = surface(sc, rays["d"], hit["prim"], hit["u"], hit["v"], F64)
        Bf = Bsdf(S, F64)
        porg = S["P"] + S["ng"] * sc.ray_eps
        tabs = sc.tables(F64)
        # ---- records exist where the reference has them ----
        for k in ("alive", "shadow"):
            bad = np.flatnonzero(dec & (g[k] != ref[k]))
            assert not len(bad), f"{what}: rays {bad[:8].tolist()}: {k} {g[k][bad[:8]].tolist()}, float64 has {ref[k][bad[:8]].tolist()}"
        assert not (g["alive"] | g["shadow"])[~hitm].any(), f"{what}: a record of a ray that hit nothing"
        # ---- the continuation at the candidate's direction ----
        a = g["alive"]
        wi = G("d")
        hold("dir", np.abs(np.sqrt(_dot(wi, wi)) - 1), 1.0, a, "|wi|")
        assert (_dot(S["ns"], wi)[a] > 0).all() and (_dot(S["ng"], wi)[a] > 0).all(), f"{what}: a continuation below a normal"
        hold("org", np.abs(G("o") - porg).max(1), sc.scale, a, "continuation origin")
        _, pdf, To, kb, _ = cont_eval(S, Bf, T_in, wi, rb, rays["keys"], F64)
        hold("bsdf", rel(G("pdf"), pdf), kb["pdf"], a, "pdf_out")
        hold("bsdf", rel(G("T"), To), kb["ratio"], a, "T_out")
        hold("dir", np.abs(wi - ref["d"]).max(1), ref["k_dir"], a & dec & ref["alive"], "wi against the recomputed sample")
        if "ps" in g:      # what only a candidate evaluation of this module carries: the measurement of the two classes the decisions rest on
            hold("ps", np.abs(G("ps") - ref["ps"]), 1 + S["ktex"], hitm, "p_s")
            hold("normal", np.maximum(np.abs(G("ng") - S["ng"]).max(1), np.abs(G("ns") - S["ns"]).max(1)), 1 + S["ktex"], hitm, "normals")
        # ---- the shadow record at the candidate's direction ----
        s = g["shadow"]
        if s.any():
            so, sd, tmax = G("so"), G("sd"), G("tmax")
            env = s & (tmax >= 1e38)
            emi = s & ~env
            hold("dir", np.abs(np.sqrt(_dot(sd, sd)) - 1), 1.0, s, "|shadow direction|")
            hold("org", np.abs(so - porg).max(1), sc.scale, s, "shadow origin")
            assert (g["tmax"][env] == F32(T_INF)).all(), f"{what}: an environment shadow ray that ends"
            light, y, wi_s = np.full(n, -1, np.int64), np.zeros((n, 3)), sd.copy()
            if emi.any():
                e = np.flatnonzero(emi)
                assert sc.n_em, f"{what}: a finite shadow ray in a scene without emitters"
                j, yy, mb = _which_emitter(sc, so[e], sd[e], tmax[e])
                assert (j >= 0).all(), f"{what}: rays {e[j < 0][:8].tolist()}: the shadow ray points at no emitter"
                light[e], y[e] = j, yy
                dv = yy - S["P"][e]
                wi_s[e] = dv / np.sqrt(_dot(dv, dv))[:, None]
                sl = np.sqrt(_dot(yy - so[e], yy - so[e]))
                kt = np.ones(n)
                kt[e] = (np.sqrt(_dot(yy, yy)) + np.sqrt(_dot(so[e], so[e]))) / sl
                full = np.zeros(n)
                full[e] = np.abs(tmax[e] - SEGMENT * sl) / (SEGMENT * sl)
                hold("tmax", full, kt, emi, "tmax against 0.999 of the segment")
                wrong = e[dec[e] & ref["shadow"][e] & (ref["light"][e] != j) & (mb > 1e-4)]
                assert not len(wrong), f"{what}: rays {wrong[:8].tolist()}: the record points at emitter {light[wrong[:8]].tolist()}, the float64 cdf chose {ref['light'][wrong[:8]].tolist()}"
            assert not (env & dec & ref["shadow"] & (ref["light"] >= 0)).any() and not (emi & dec & ref["shadow"] & (ref["light"] < 0)).any(), f"{what}: the wrong kind of light"
            k = np.flatnonzero(s)
            Ss = _sub(S, k)
            valid, contrib, kc, mg = nee_eval(sc, tabs, Ss, Bsdf(Ss, F64), T_in[k], wi_s[k], light[k], F64, None, y[k])
            at = mg >= 2 * ATAN_MARGIN
            assert valid[at].all(), f"{what}: rays {k[at & ~valid][:8].tolist()}: a shadow record the reference has no light for"
            full_c, full_k, full_at = np.zeros(n), np.ones(n), np.zeros(n, bool)
            full_c[k], full_k[k], full_at[k] = rel(G("contrib")[k], contrib), kc, at
            hold("contrib", full_c, full_k, full_at, "NEE contribution")
            hold("dir", np.abs(sd - ref["sd"]).max(1), ref["k_dir_nee"], s & dec & ref["shadow"], "shadow direction against the recomputed sample")
    assert not fails, f"{what} (bounce {b}): " + "; ".join(fails[:6])
    share = float(und.mean())
    if report is not None:
        for k, v in worst.items():
            report[k] = max(report.get(k, 0.0), v)
        report["why"] = {k: int(m.sum()) for k, m in why.items() if m.any()}
    return share, worst


# ---- the ray sets ------------------------------------------------------------------------------------------------------------------------------------------
BOUNCES = (0, 1, 2, 5)                 # no MIS weights; MIS; Russian roulette (bounce + 1 >= RR_START); and bounce = max_bounces, emission only
MAX_BOUNCES = 8
THROUGHPUTS = np.asarray([(1.0, 1.0, 1.0), (1e-3, 1e-3, 1e-3), (0.7, 0.0, 0.4), (0.0, 0.0, 0.0)], F32)      # ones; survival clamped at RR_PMIN; a zero channel; all zero


def ray_sets(pt):
    """(n, rays) per count of glass_reference.ray_sets (1, 63, 64, 65 around a wave, 513 two segments; every seventh ray turned away): camera rays with random
    keys, throughputs cycling through THROUGHPUTS and previous pdfs spread over 0.05 .. 50."""
    rng = np.random.default_rng(61)
    for n, o, d, keys in gref.ray_sets(pt):
        T = THROUGHPUTS[np.arange(n) % 4]
        yield n, dict(o=o, d=d, T=T.copy(), pdf=np.exp(rng.uniform(np.log(0.05), np.log(50.0), n)).astype(F32), keys=keys)


def _rays_at(points, dirs, seed, height=1.0):
    points, dirs = np.asarray(points, F64), np.asarray(dirs, F64)
    dirs = dirs / np.sqrt(_dot(dirs, dirs))[:, None]
    n = len(points)
    rng = np.random.default_rng(seed)
    d32 = dirs.astype(F32)
    return dict(o=(points - dirs * height).astype(F32), d=d32, T=np.ones((n, 3), F32), pdf=np.exp(rng.uniform(np.log(0.05), np.log(50.0), n)).astype(F32),
                keys=rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))


def edge_sets(half=1.5):
    """("grazing", rays): 128 rays onto the floor z = 0 with n.v from 1e-2 down to 1e-5; ("normal", rays): 32 rays at exact normal incidence from above
    (n = (0, 0, 1)) and 32 from below (the back face: n = (0, 0, -1))."""
    rng = np.random.default_rng(67)
    n = 128
    pts = np.concatenate([rng.uniform(-0.9 * half, 0.9 * half, (n, 2)), np.zeros((n, 1))], 1)
    cosv = np.exp(np.linspace(np.log(1e-2), np.log(1e-5), n))
    az = rng.uniform(0, 2 * PI, n)
    sinv = np.sqrt(1 - cosv * cosv)
    yield "grazing", _rays_at(pts, np.stack([sinv * np.cos(az), sinv * np.sin(az), -cosv], 1), 71, height=0.05)
    pts = np.concatenate([rng.uniform(-0.9 * half, 0.9 * half, (64, 2)), np.zeros((64, 1))], 1)
    dirs = np.zeros((64, 3))
    dirs[:32, 2], dirs[32:, 2] = -1.0, 1.0
    yield "normal", _rays_at(pts, dirs, 73)


def emitter_set(sc, n=64):
    """n rays aimed at the front of the scene's emitters from 0.3 to 1.5 away, the cosine at the emitter from 1 down to 0.02: what the camera rays hardly ever
    do.  Run at bounce = max_bounces: emission with its MIS weight alone (a ray on an emitter samples that emitter's own plane in its next-event step, which
    no precision decides)."""
    rng = np.random.default_rng(79)
    j = rng.integers(0, sc.n_em, n)
    tri = sc.verts[sc.idx[sc.em_prims[j]]][:, :, 0:3].astype(F64)
    bu, bv = rng.uniform(0.15, 0.35, n), rng.uniform(0.15, 0.35, n)
    P = tri[:, 0] + (tri[:, 1] - tri[:, 0]) * bu[:, None] + (tri[:, 2] - tri[:, 0]) * bv[:, None]
    nrm = _unit(_cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]))
    tx, ty = onb(nrm)
    cosl = np.exp(rng.uniform(np.log(0.02), 0.0, n))
    az = rng.uniform(0, 2 * PI, n)
    sinl = np.sqrt(1 - cosl * cosl)
    out = tx * (sinl * np.cos(az))[:, None] + ty * (sinl * np.sin(az))[:, None] + nrm * cosl[:, None]
    rays = _rays_at(P, -out, 83, height=1.0)
    rays["o"] = (P + out * rng.uniform(0.3, 1.5, n)[:, None]).astype(F32)
    rays["T"] = THROUGHPUTS[np.arange(n) % 4].copy()
    return rays


# ---- chi-square ----------------------------------------------------------------------------------------------------------------------------------------------
def chi2_sf(x, k):
    """P(chi^2_k > x): the regularised upper incomplete gamma function Q(k / 2, x / 2), by its series below a + 1 and its continued fraction above."""
    a, x = 0.5 * k, 0.5 * x
    if x <= 0:
        return 1.0
    lg = -x + a * math.log(x) - math.lgamma(a)
    if x < a + 1:
        term = total = 1.0 / a
        ap = a
        for _ in range(100000):
            ap += 1
            term *= x / ap
            total += term
            if abs(term) < abs(total) * 1e-16:
                break
        return 1.0 - total * math.exp(lg)
    tiny = 1e-300
    bb = x + 1 - a
    c, dd = 1 / tiny, 1 / bb
    hh = dd
    for i in range(1, 100000):
        an = -i * (i - a)
        bb += 2
        dd = an * dd + bb
        dd = tiny if abs(dd) < tiny else dd
        c = bb + an / c
        c = tiny if abs(c) < tiny else c
        dd = 1 / dd
        de = dd * c
        hh *= de
        if abs(de - 1) < 1e-16:
            break
    return math.exp(lg) * hh


def chi2_test(counts, expected, level=1e-6, min_expected=10.0, min_cells=64):
    """Pearson's statistic of observed counts against expected counts (cells below min_expected pooled into one), its degrees of freedom and P(chi^2 > it);
    asserts at least min_cells cells and P >= level."""
    counts, expected = np.asarray(counts, F64).reshape(-1), np.asarray(expected, F64).reshape(-1)
    small = expected < min_expected
    c, e = np.append(counts[~small], counts[small].sum()), np.append(expected[~small], expected[small].sum())
    if e[-1] < min_expected:      # the pool itself is small: it joins the smallest cell
        i = int(e[:-1].argmin())
        c[i] += c[-1]; e[i] += e[-1]
        c, e = c[:-1], e[:-1]
    assert len(c) >= min_cells, f"{len(c)} cells of at least {min_expected} expected samples: fewer than {min_cells}"
    stat = float(((c - e) ** 2 / e).sum())
    p = chi2_sf(stat, len(c) - 1)
    return stat, len(c) - 1, p


def hemisphere_cells(wil, nz=16, nphi=16):
    """Counts of local directions (z = the normal) over nz x nphi cells of equal solid angle: z = cos(theta) and the azimuth, both uniform."""
    z = np.clip(wil[:, 2], 0, 1 - 1e-12)
    phi = np.arctan2(wil[:, 1], wil[:, 0]) % (2 * PI)
    i = np.minimum((z * nz).astype(np.int64), nz - 1) * nphi + np.minimum((phi / (2 * PI) * nphi).astype(np.int64), nphi - 1)
    return np.bincount(i, minlength=nz * nphi).astype(F64)


def hemisphere_expected(pdf_of, n_samples, nz=16, nphi=16, sub=48):
    """The expected counts of hemisphere_cells for the solid-angle density pdf_of(local directions): midpoint quadrature with sub x sub points per cell.
    Also returns the integral of the density over the hemisphere."""
    zz = (np.arange(nz * sub) + 0.5) / (nz * sub)
    pp = (np.arange(nphi * sub) + 0.5) / (nphi * sub) * 2 * PI
    Z, Pp = np.meshgrid(zz, pp, indexing="ij")
    s = np.sqrt(1 - Z * Z)
    w = np.stack([s * np.cos(Pp), s * np.sin(Pp), Z], -1).reshape(-1, 3)
    dens = pdf_of(w).reshape(nz, sub, nphi, sub).sum((1, 3)) * (2 * PI / (nz * sub * nphi * sub))
    return dens.reshape(-1) * n_samples, float(dens.sum())
