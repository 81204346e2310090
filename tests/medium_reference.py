"""numpy restatement of the participating medium (csrc/pt_medium.h, csrc/pt_medium.hip), for tests/test_medium_host.py and tests/test_gpu_medium.py.

Every function takes dt: float32 follows the sources operation for operation (bit for bit: numpy's + - * / sqrt on float32 are correctly rounded, fma is
lens_reference._fma, pt_log2 / pt_exp2 are glass_reference's); float64 evaluates the same formulas in double with numpy's own log2 / exp2, and is what the
float32 results are held to within the bounds below.

  span / free_flight / hg_phase / hg_cos / hg_direction / roulette / transmittance     the definition, elementwise
  Medium                                                                               the record pt_medium_make builds
  atan2_32 / env_lookup32 / env_sample32                                               pt_atan2 and the environment's lookup and sampler, float32, from ptc_debug_get_env_tables
  scatter_step                                                                         k_medium_decide for rays whose hit records are given: the decision, the light
                                                                                       kind, the continuation, the environment, emitter and punctual records
  attenuate                                                                            step 6 on shadow records
  reference64 / check                                                                  one step in float64 written from the definitions (not from pt_medium.h) at the
                                                                                       device's own record directions, and a float32 result held to it
"""
import numpy as np

import glass_reference as gref
import lights_reference as lref
from lens_reference import F32, F64, _fma, rng_f, sincos2pi

RNG_BASE = 0x18000000
RNG_PUNCTUAL = 0x1c000000
T_INF = F32(3.0e38)
G_ISO = F32(1e-3)
LN2 = F32(0.693147180559945309)
LOG2E = F32(1.44269504088896341)
FOUR_PI = F32(12.5663706143591730)
RR_START, RR_PMIN = 3, F32(0.05)
MUTATIONS = ("g_sign", "balance", "no_attenuation", "albedo_twice", "offset_origin")

# |float32 - float64| relative to the float64 value, measured by test_medium_host.py::test_float32_against_float64 over its case sets (the table is in DESIGN.md
# §2f): the bound is four times the worst ratio seen, rounded up to a power of two.  Rounding only: both evaluate the same formulas.
K_COS = 2.0 ** -13          # the sampled cosine, absolute; worst seen 2.54e-5 (|g| = 0.99: the quotient's denominator cancels like the phase function's x)
K_FLIGHT = 2.0 ** -18       # (s - t0) sigma_t, absolute in mean free paths up to 16; worst seen 8.44e-7 (pt_log2's polynomial)
K_TRANS = 2.0 ** -17        # the transmittance, relative, for sigma_t (t1 - t0) <= 16; worst seen 1.42e-6 (pt_exp2's polynomial)
# A shadow record's contribution, relative to its largest channel, away from the phase function's and the distance's cancellations: six float32 products and
# quotients (3 ulp = 2^-21.4), the MIS weight (two more) and the attenuation K_TRANS, rounded up to a power of two.  check adds the conditioned terms per record.
# K_CONTRIB, K_THROUGHPUT and phase_bound are not "four times a measured worst ratio": a record's error has no worst ratio over a ray set — it grows without limit
# towards a light, a cone's edge, a pole of the map or |g| = 1 — so each is the count of roundings of its well-conditioned part plus, per record, the condition
# numbers of the parts that cancel (reference64 computes them); test_float32_against_float64 holds phase_bound to the measured ratios for every g it lists.
K_CONTRIB = 2.0 ** -16
K_THROUGHPUT = 2.0 ** -20   # T' = T albedo (/ the survival probability): two roundings, 2^-23 each, times four, up to a power of two


def phase_bound(g):
    """Relative error of the float32 ph(c): x = 1 + g^2 - 2 g c is a sum of terms up to 4 that cancels down to (1 - |g|)^2, so x carries 4 ulp / (1 - |g|)^2
    relative and ph = .. / (x sqrt x) 1.5 times that, plus the four roundings behind it."""
    return 1.5 * 4 * 2.0 ** -23 / (1.0 - abs(float(g))) ** 2 + 4 * 2.0 ** -23


def _f(dt):
    return lambda a, b, c: _fma(a, b, c, dt)


def dot3(a, b, dt=F32):
    f = _f(dt)
    return f(a[..., 2], b[..., 2], f(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


class Medium:
    def __init__(self, box_lo, box_hi, sigma_t, albedo=(1.0, 1.0, 1.0), g=0.0):
        self.lo, self.hi = np.asarray(box_lo, F32), np.asarray(box_hi, F32)
        self.sigma_t = F32(sigma_t)
        self.albedo = np.asarray((albedo,) * 3 if np.isscalar(albedo) else albedo, F32)
        self.g = F32(g)
        with np.errstate(divide="ignore"):
            self.ff = F32(LN2 / self.sigma_t)
        self.sl = F32(self.sigma_t * LOG2E)

    def params(self):
        return dict(box_lo=tuple(self.lo), box_hi=tuple(self.hi), sigma_t=float(self.sigma_t), albedo=tuple(self.albedo), g=float(self.g))


def span(m, o, d, t_end, dt=F32):
    """pt_medium_span: (crosses, t0, t1) of the rays (o, d) (n, 3) with segment ends t_end (n,)."""
    o, d = np.asarray(o, F32).astype(dt), np.asarray(d, F32).astype(dt)
    n = o.shape[0]
    tn, tf = np.zeros(n, dt), np.asarray(t_end, F32).astype(dt).copy()
    ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for k in range(3):
            lo, hi = dt(m.lo[k]), dt(m.hi[k])
            zero = d[:, k] == 0
            inside = (o[:, k] >= lo) & (o[:, k] <= hi)
            a, b = (lo - o[:, k]) / d[:, k], (hi - o[:, k]) / d[:, k]
            near, far = np.where(a < b, a, b), np.where(a > b, a, b)                 # fmin2, fmax2
            tn2, tf2 = np.where(tn > near, tn, near), np.where(tf < far, tf, far)     # fmax2(tn, n), fmin2(tf, f)
            live = ok & ~zero
            tn, tf = np.where(live, tn2, tn), np.where(live, tf2, tf)
            ok = ok & (~zero | inside)
    t0, t1 = np.where(ok, tn, 0).astype(dt), np.where(ok, tf, 0).astype(dt)
    return ok & (t0 < t1), t0, t1


def free_flight(m, t0, u0, dt=F32):
    """pt_medium_free_flight: s = t0 - pt_log2(1 - u0) (ln 2 / sigma_t)."""
    u0 = np.asarray(u0, F32)
    if dt is F32:
        l = gref.log2(F32(1.0) - u0)
        return (np.asarray(t0, F32) - l * m.ff).astype(F32)
    with np.errstate(divide="ignore"):
        return np.asarray(t0, F64) - np.log(1.0 - u0.astype(F64)) / F64(m.sigma_t)


def hg_phase(g, c, dt=F32):
    g, c = dt(g), np.asarray(c, dt)
    g2 = g * g
    x = (dt(1.0) + g2) - ((dt(2.0) * g) * c)
    den = (dt(FOUR_PI) * x) * np.sqrt(x) if dt is F32 else (4.0 * np.pi * x) * np.sqrt(x)
    return ((dt(1.0) - g2) / den).astype(dt)


def hg_cos(g, u1, dt=F32):
    g, u1 = dt(g), np.asarray(u1, F32).astype(dt)
    if abs(g) < dt(G_ISO):
        c = dt(1.0) - dt(2.0) * u1
    else:
        g2 = g * g
        q = (dt(1.0) - g2) / ((dt(1.0) - g) + ((dt(2.0) * g) * u1))
        c = ((dt(1.0) + g2) - q * q) / (dt(2.0) * g)
    return np.clip(c, dt(-1.0), dt(1.0)).astype(dt)


def onb(n, dt=F32):
    f = _f(dt)
    sg = np.copysign(dt(1.0), n[..., 2]).astype(dt)
    with np.errstate(all="ignore"):
        a = dt(-1.0) / (sg + n[..., 2])
        bb = n[..., 0] * n[..., 1] * a
        t = np.stack([f(sg * n[..., 0], n[..., 0] * a, dt(1.0)), sg * bb, -sg * n[..., 0]], -1)
        b = np.stack([bb, f(n[..., 1], n[..., 1] * a, sg), -n[..., 1]], -1)
    return t.astype(dt), b.astype(dt)


def vfma(a, s, b, dt=F32):
    return _f(dt)(a, np.asarray(s, dt)[..., None], b).astype(dt)


def hg_direction(d, c, u2, dt=F32):
    d, c = np.asarray(d, F32).astype(dt), np.asarray(c, dt)
    sn = np.sqrt(np.maximum(dt(0.0), dt(1.0) - c * c))
    sp, cp = sincos2pi(np.asarray(u2, F32), dt)
    tx, ty = onb(d, dt)
    return vfma(tx, sn * cp, vfma(ty, sn * sp, d * c[..., None], dt), dt)


def roulette(rb, ur, T, dt=F32):
    """P8 on T (n, 3): (alive, T after the division)."""
    T = np.asarray(T, dt)
    if rb < RR_START:
        return np.ones(len(T), bool), T
    qq = T.max(1)
    pr = np.minimum(np.maximum(qq, dt(RR_PMIN)), dt(1.0))
    alive = (qq > 0) & ~(np.asarray(ur, F32).astype(dt) >= pr)
    with np.errstate(all="ignore"):
        return alive, np.where(alive[:, None], T / pr[:, None], T).astype(dt)


def transmittance(m, t0, t1, dt=F32):
    if dt is F32:
        return gref.exp2((-m.sl) * (np.asarray(t1, F32) - np.asarray(t0, F32)))
    return np.exp(-F64(m.sigma_t) * (np.asarray(t1, F64) - np.asarray(t0, F64)))


def attenuate(m, so, sd, tmax, contrib, dt=F32):
    """Step 6: (contribution after attenuation, which records crossed the box)."""
    hit, t0, t1 = span(m, so, sd, tmax, dt)
    tr = transmittance(m, t0, t1, dt)
    c = np.asarray(contrib, dt)
    return np.where(hit[:, None], c * tr[:, None], c).astype(dt), hit


PI32, INV_PI32, HALF_PI32 = F32(3.14159265358979323846), F32(0.31830988618379067154), F32(1.57079632679489661923)


def atan2_32(y, x):
    """pt_atan2 (csrc/pt_device.h) in float32."""
    y, x = np.asarray(y, F32), np.asarray(x, F32)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.where(ax > ay, ax, ay), np.where(ax < ay, ax, ay)
    with np.errstate(all="ignore"):
        a = (mn / mx).astype(F32)
    a2 = a * a
    p = _fma(a2, _fma(a2, _fma(a2, _fma(a2, _fma(a2, F32(-0.01172120), F32(0.05265332)), F32(-0.11643287)), F32(0.19354346)), F32(-0.33262347)), F32(0.99997726))
    r = a * p
    r = np.where(ay > ax, HALF_PI32 - r, r).astype(F32)
    r = np.where(x < 0, PI32 - r, r).astype(F32)
    r = np.where(y < 0, -r, r).astype(F32)
    return np.where(mx > 0, r, F32(0.0)).astype(F32)


def env_lookup32(env, ok, d):
    """env_lookup (pt_kernels.hip; the medium pass's second text) in float32: (Le (n, 3), pdf (n,), (y, x)) of the unit directions d.  env: (h, w, 4) = rgb, texel pmf."""
    d = np.asarray(d, F32)
    h, w = env.shape[0], env.shape[1]
    u = atan2_32(d[:, 2], d[:, 0]) * (F32(0.5) * INV_PI32) + F32(0.5)
    dy = np.minimum(np.maximum(d[:, 1], F32(-1.0)), F32(1.0))
    st = np.sqrt(np.maximum(F32(0.0), F32(1.0) - dy * dy))
    vv = atan2_32(st, dy) * INV_PI32
    x = np.clip((u * F32(w)).astype(np.int64), 0, w - 1)
    y = np.clip((vv * F32(h)).astype(np.int64), 0, h - 1)
    t = env[y, x]
    den = F32(2.0) * PI32 * PI32 * np.maximum(st, F32(1e-6))
    pdf = (t[:, 3] * F32(w) * F32(h)) / den if ok else np.zeros(len(d), F32)
    return t[:, 0:3].astype(F32), pdf.astype(F32), (y, x)


def env_sample32(marg, cond, r1, r2):
    """env_sample in float32: the row by the marginal cdf, the column by the row's conditional cdf (the guided search finds the index of the plain one: the first
    entry above r, the last at most), uniform inside the texel."""
    marg, cond, r1, r2 = np.asarray(marg, F32), np.asarray(cond, F32), np.asarray(r1, F32), np.asarray(r2, F32)
    h, w = cond.shape
    y = np.minimum((marg[None, :] <= r1[:, None]).sum(1), h - 1)
    m0, m1 = np.where(y > 0, marg[np.maximum(y - 1, 0)], F32(0.0)).astype(F32), marg[y]
    row = cond[y]
    x = np.minimum((row <= r2[:, None]).sum(1), w - 1)
    k = np.arange(len(y))
    c0, c1 = np.where(x > 0, row[k, np.maximum(x - 1, 0)], F32(0.0)).astype(F32), row[k, x]
    with np.errstate(all="ignore"):
        xv = np.where(m1 > m0, (r1 - m0) / (m1 - m0), F32(0.5)).astype(F32)
        xu = np.where(c1 > c0, (r2 - c0) / (c1 - c0), F32(0.5)).astype(F32)
    xu = np.minimum(np.maximum(xu, F32(0.0)), F32(0.999999))
    xv = np.minimum(np.maximum(xv, F32(0.0)), F32(0.999999))
    u, vv = (x.astype(F32) + xu) / F32(w), (y.astype(F32) + xv) / F32(h)
    s2, c2 = sincos2pi(u)
    st, ct = sincos2pi(F32(0.5) * vv)
    return np.stack([st * -c2, ct, st * -s2], -1).astype(F32)


def scatter_step(m, o, d, T, keys, t_hit, is_hit, bounce, max_bounces, emitters=None, cdf=None, p_area=1.0, lights=None, dt=F32, mutation=None, wi_nee=None, wi_cont=None, env=None):
    """k_medium_decide for the rays (o, d, T, key) whose closest hits are (t_hit, is_hit), at `bounce` of a frame of `max_bounces`, in a scene whose emitters are
    `emitters` (n_e, 20) with power cdf `cdf` (ptc_debug_get_shading_tables), whose punctual table is `lights` = (records (n_l, 16), cdf) or None and whose environment
    is `env` = ptc_debug_get_env_tables' (env, marg, cond, ok) or None (float32 only); p_env and p_area follow from what the scene has, as in k_shade.  A dict per ray: crossed, t0, t1, s, scattered, P, alive, cont (10), shadow, srec (10), punctual, prec (10), records as ptc_debug_medium_step
    returns them, shadow contributions AFTER attenuation.  dt = float64: the same formulas in double, the record directions taken from wi_nee / wi_cont where
    given (the device's own, as DESIGN.md §1b evaluates a record).  mutation: one of MUTATIONS, a wrong formula the checker must catch."""
    o32, d32 = np.asarray(o, F32), np.asarray(d, F32)
    n = o32.shape[0]
    keys = np.asarray(keys, np.uint32)
    idx = RNG_BASE + int(bounce) + 1
    g = -m.g if mutation == "g_sign" else m.g
    t_end = np.where(is_hit, np.asarray(t_hit, F32), T_INF).astype(F32)
    crossed, t0, t1 = span(m, o32, d32, t_end, dt)
    s = free_flight(m, t0, rng_f(keys, idx, 0), dt)
    scattered = crossed & (s < t1)
    od, dd = o32.astype(dt), d32.astype(dt)
    P = vfma(dd, np.where(scattered, s, 0).astype(dt), od, dt)
    Tp = (np.asarray(T, F32).astype(dt) * m.albedo.astype(dt)[None, :]).astype(dt)
    if mutation == "albedo_twice":
        Tp = (Tp * m.albedo.astype(dt)[None, :]).astype(dt)
    go = scattered & (bounce < max_bounces) & (Tp.max(1) > 0)
    out = dict(crossed=crossed, t0=t0, t1=t1, s=np.where(crossed, s, 0).astype(dt), scattered=scattered, P=P)
    z10 = np.zeros((n, 10), dt)
    # ---- the light kind: k_shade's p_env / p_area ----
    has_emit = emitters is not None and len(emitters) > 0
    env_nee = env is not None and bool(env[3]) and env[0].size > 0
    p_env = (F32(0.5) if has_emit else F32(1.0)) if env_nee else F32(0.0)
    p_area = F32(1.0) - p_env
    u_kind = rng_f(keys, idx, 4)
    use_env = np.full(n, env_nee) & (np.full(n, not has_emit) | (u_kind < p_env))
    out.update(use_env=use_env, kind_margin=np.abs(u_kind.astype(F64) - float(p_env)) if (env_nee and has_emit) else np.ones(n))
    # ---- the environment record (float32 only) ----
    shadow, srec = np.zeros(n, bool), z10.copy()
    if env_nee:
        wi = env_sample32(env[1], env[2], rng_f(keys, idx, 6), rng_f(keys, idx, 7))
        Le, pe, _ = env_lookup32(env[0], env[3], wi)
        pl = pe * p_env
        with np.errstate(all="ignore"):
            ph = hg_phase(g, dot3(d32, wi), F32)
            pl2 = pl * pl
            wgt = pl / (ph + pl) if mutation == "balance" else pl2 / _fma(ph, ph, pl2)
            k = (ph * wgt) / pl
            contrib = (Tp.astype(F32) * Le * k[:, None]).astype(F32)
        e_ok = go & use_env & (pl > 0)
        tmax = np.full(n, T_INF, F32)
        if mutation != "no_attenuation":
            contrib, _ = attenuate(m, P.astype(F32), wi, tmax, contrib)
        shadow = e_ok
        srec = np.where(e_ok[:, None], np.concatenate([P.astype(F32), wi, tmax[:, None], contrib], 1), 0).astype(dt)
    # ---- the emitter record ----
    if has_emit:
        E = np.asarray(emitters, F32)
        lo = lref.cdf_search(cdf, rng_f(keys, idx, 5))
        r1, r2 = rng_f(keys, idx, 6).astype(dt), rng_f(keys, idx, 7).astype(dt)
        L = E[lo].astype(dt)
        v0, area, e1, pmf, e2, nl, Le = L[:, 0:3], L[:, 3], L[:, 4:7], L[:, 7], L[:, 8:11], L[:, 12:15], L[:, 16:19]
        with np.errstate(all="ignore"):
            su = np.sqrt(r1)
            bu, bv = su * (dt(1.0) - r2), su * r2
            y = vfma(e2, bv, vfma(e1, bu, v0, dt), dt)
            Pn = P + dt(1e-2) if mutation == "offset_origin" else P
            dv = y - Pn
            dist2 = dot3(dv, dv, dt)
            dist = np.sqrt(dist2)
            wi = dv * (dt(1.0) / dist)[:, None]
            if wi_nee is not None:
                wi = np.asarray(wi_nee, F32).astype(dt)
            cosl = -dot3(nl, wi, dt)
            pl = ((pmf * dist2) / (area * cosl)) * dt(p_area)
            ph = hg_phase(g, dot3(dd, wi, dt), dt)
            pl2 = pl * pl
            wgt = pl / (ph + pl) if mutation == "balance" else pl2 / _f(dt)(ph, ph, pl2)
            k = (ph * wgt) / pl
            contrib = Tp * Le * k[:, None]
            a_ok = go & ~use_env & (dist2 > 0) & (cosl > 0)
            tmax = dist * dt(F32(0.999))
            if mutation != "no_attenuation":
                contrib, _ = attenuate(m, P, wi, tmax, contrib, dt)
            srec = np.where(a_ok[:, None], np.concatenate([P, wi, tmax[:, None], contrib], 1), srec).astype(dt)
            shadow = shadow | a_ok
    # ---- the punctual record ----
    punctual, prec = np.zeros(n, bool), z10.copy()
    if lights is not None and len(lights[0]):
        recs, lcdf = lights
        li = lref.cdf_search(lcdf, rng_f(keys, RNG_PUNCTUAL + int(bounce) + 1, 0))
        R = np.asarray(recs, F32)[li]
        ok, wi, dist, Li = lref.light_sample(R, P.astype(F32) if dt is F32 else P, dt)
        with np.errstate(all="ignore"):
            k = hg_phase(g, dot3(dd, wi, dt), dt) / R[:, 11].astype(dt)
            sv = R[:, 0:3].astype(dt) - P
            sd_ = np.sqrt(dot3(sv, sv, dt))
            sdir = sv * (dt(1.0) / sd_)[:, None]
            direc = lref.rec_type(np.ascontiguousarray(R)) == lref.DIRECTIONAL
            sdir = np.where(direc[:, None], wi, sdir)
            tmax = np.where(direc, dt(T_INF), sd_ * dt(F32(0.999)))
            contrib = Tp * Li * k[:, None]
            punctual = go & ok & (Li.max(1) > 0)
            if mutation != "no_attenuation":
                contrib, _ = attenuate(m, P, sdir, tmax, contrib, dt)
            prec = np.where(punctual[:, None], np.concatenate([P, sdir, tmax[:, None], contrib], 1), 0).astype(dt)
    # ---- the continuation ----
    c = hg_cos(g, rng_f(keys, idx, 1), dt)
    wi = hg_direction(d32, c, rng_f(keys, idx, 2), dt)
    pdf = hg_phase(g, c, dt)
    if wi_cont is not None:
        wi = np.asarray(wi_cont, F32).astype(dt)
        pdf = hg_phase(g, dot3(dd, wi, dt), dt)
    alive, Tc = roulette(int(bounce) + 1, rng_f(keys, idx, 3), Tp, dt)
    alive = alive & go
    cont = np.where(alive[:, None], np.concatenate([P, wi, Tc, pdf[:, None]], 1), 0).astype(dt)
    out.update(alive=alive, cont=cont, shadow=shadow, srec=srec, punctual=punctual, prec=prec, Tp=Tp, rr_margin=np.abs(rng_f(keys, idx, 3).astype(F64) - np.clip(Tp.max(1), RR_PMIN, 1)),
               flight_margin=np.abs((s - t1).astype(F64)) * F64(m.sigma_t))
    return out


def _inside_length(m, o, wi, tmax):
    """The length of the segment o + t wi, 0 <= t <= tmax, inside the box: the interval of t where every coordinate lies between the faces."""
    lo, hi = m.lo.astype(F64), m.hi.astype(F64)
    a, b = np.zeros(len(o)), np.asarray(tmax, F64).copy()
    with np.errstate(all="ignore"):
        for k in range(3):
            par = wi[:, k] == 0
            t1, t2 = (lo[k] - o[:, k]) / wi[:, k], (hi[k] - o[:, k]) / wi[:, k]
            enter, leave = np.minimum(t1, t2), np.maximum(t1, t2)
            outside = par & ((o[:, k] < lo[k]) | (o[:, k] > hi[k]))
            a = np.where(par, a, np.maximum(a, enter))
            b = np.where(outside, -1.0, np.where(par, b, np.minimum(b, leave)))
    return np.maximum(b - a, 0.0), a, b


def reference64(m, o, d, T, keys, t_hit, is_hit, bounce, max_bounces, got, emitters=None, cdf=None, lights=None, env=None):
    """One medium step in float64, written from the definitions and not from pt_medium.h: Beer-Lambert free flight -ln(1 - u) / sigma behind the box's entry, the
    Henyey-Greenstein density (1 - g^2) / (4 pi (1 + g^2 - 2 g cos)^(3/2)) and its inverse cdf, the area-to-solid-angle density pmf d^2 / (A cos) of an emitter sample
    (d by intersecting the device's direction with the emitter's plane), the lat-long map's pmf w h / (2 pi^2 sin) of an environment sample, the power heuristic, the
    inverse-square law, the spot's smoothstep and the range window of KHR_lights_punctual, and exp(-sigma x the shadow segment's length inside the box).  Each record
    is evaluated at the DEVICE's own origin and direction (`got`, a medium_step result), as DESIGN.md 1b does.  Returns the expected flags and values with, per ray,
    the margins of its decisions and the condition numbers of its records."""
    o, d, T = np.asarray(o, F32).astype(F64), np.asarray(d, F32).astype(F64), np.asarray(T, F32).astype(F64)
    n = len(o)
    keys = np.asarray(keys, np.uint32)
    sigma, g, alb = float(m.sigma_t), float(m.g), m.albedo.astype(F64)
    idx = RNG_BASE + int(bounce) + 1
    u = lambda dim: rng_f(keys, idx, dim).astype(F64)
    t_end = np.where(is_hit, np.asarray(t_hit, F64), float(T_INF))
    L, t0, t1 = _inside_length(m, o, d, t_end)
    crossed = L > 0
    with np.errstate(all="ignore"):
        s = t0 - np.log(1.0 - u(0)) / sigma
    scattered = crossed & (s < t1)
    r = dict(crossed=crossed, scattered=scattered, sliver=crossed & (L < 2.0 ** -18 * np.maximum(t1, 1.0)), flight_margin=np.where(crossed, np.abs(s - t1) * sigma, 1.0))
    P = o + d * np.where(scattered, s, 0.0)[:, None]
    Tp = T * alb[None, :]
    go = scattered & (bounce < max_bounces) & (Tp.max(1) > 0)
    hg = lambda c: (1.0 - g * g) / (4.0 * np.pi * (1.0 + g * g - 2.0 * g * c) ** 1.5)

    def through(origin, wi, tmax):
        return np.exp(-sigma * _inside_length(m, origin, wi, tmax)[0])

    # ---- the emitter-or-environment record ----
    has_emit = emitters is not None and len(emitters) > 0
    env_nee = env is not None and bool(env[3]) and env[0].size > 0
    p_env = (0.5 if has_emit else 1.0) if env_nee else 0.0
    use_env = np.full(n, env_nee) & (np.full(n, not has_emit) | (u(4) < p_env))
    r["kind_margin"] = np.abs(u(4) - p_env) if (env_nee and has_emit) else np.ones(n)
    so, wi, tmax = np.asarray(got["so"], F64), np.asarray(got["sd"], F64), np.asarray(got["tmax"], F64)
    shadow, contrib, cond, step_margin = np.zeros(n, bool), np.zeros((n, 3)), np.zeros(n), np.ones(n)
    cosd = (wi * d).sum(1)
    with np.errstate(all="ignore"):
        if env_nee:
            tab = env[0].astype(F64)
            h, w = tab.shape[0], tab.shape[1]
            phi, theta = np.arctan2(wi[:, 2], wi[:, 0]), np.arccos(np.clip(wi[:, 1], -1, 1))
            xs, ys = (phi / (2 * np.pi) + 0.5) * w, theta / np.pi * h
            x, y = np.clip(np.floor(xs).astype(int), 0, w - 1), np.clip(np.floor(ys).astype(int), 0, h - 1)
            sin = np.maximum(np.sqrt(np.maximum(1 - wi[:, 1] ** 2, 0)), 1e-6)
            pl = tab[y, x, 3] * w * h / (2 * np.pi ** 2 * sin) * p_env
            ph = hg(cosd)
            e_ok = go & use_env & np.asarray(got["shadow"])
            val = Tp * tab[y, x, 0:3] * (ph * (pl * pl / (pl * pl + ph * ph)) / pl * through(so, wi, tmax))[:, None]
            contrib, shadow = np.where(e_ok[:, None], val, contrib), shadow | e_ok
            cond = np.where(e_ok, 2 * 2.0 ** -23 / (sin * sin), cond)
            texel = np.minimum(np.abs(xs - np.round(xs)) * (2 * np.pi / w), np.abs(ys - np.round(ys)) * (np.pi / h))
            step_margin = np.where(e_ok, texel / 1e-5, step_margin)      # pt_atan2 is good to 1e-5 rad: nearer a texel's edge the texel is undecided
            r["env_expected"] = go & use_env      # a record unless the sampled texel has no power; the device's flag decides that
        if has_emit:
            E = np.asarray(emitters, F64)
            uc = u(5)
            li = np.minimum(np.searchsorted(np.asarray(cdf, F64), uc, side="right"), len(E) - 1)
            cm = np.abs(np.asarray(cdf, F64)[None, :] - uc[:, None]).min(1)
            Lr = E[li]
            v0, area, e1, pmf, e2, nl, Le = Lr[:, 0:3], Lr[:, 3], Lr[:, 4:7], Lr[:, 7], Lr[:, 8:11], Lr[:, 12:15], Lr[:, 16:19]
            su = np.sqrt(u(6))
            ypt = v0 + e1 * (su * (1 - u(7)))[:, None] + e2 * (su * u(7))[:, None]
            own = ypt - P
            own_d = np.linalg.norm(own, axis=1)
            cos_own = -(nl * own).sum(1) / own_d
            a_ok = go & ~use_env & (cos_own > 0)
            cosl = -(nl * wi).sum(1)
            dist = ((v0 - so) * nl).sum(1) / (nl * wi).sum(1)      # along the device's direction to the emitter's plane
            pl = pmf * dist * dist / (area * cosl) * (1.0 - p_env)
            ph = hg(cosd)
            val = Tp * Le * (ph * (pl * pl / (pl * pl + ph * ph)) / pl * through(so, wi, tmax))[:, None]
            contrib, shadow = np.where(a_ok[:, None], val, contrib), shadow | a_ok
            cond = np.where(a_ok, 4 * 2.0 ** -23 * (1 + np.abs(P).max(1)) / np.maximum(own_d, 1e-30) * (1 + 1 / np.maximum(cos_own, 1e-30)), cond)
            step_margin = np.where(go & ~use_env, np.minimum(cm / 2.0 ** -22, np.abs(cos_own) / 1e-5), step_margin)
            r["dir_error"] = np.where(a_ok, np.linalg.norm(wi - own / own_d[:, None], axis=1), 0.0)
            r["tmax_error"] = np.where(a_ok, np.abs(tmax / (0.999 * own_d) - 1), 0.0)
    r.update(shadow=shadow, contrib=contrib, shadow_cond=cond, step_margin=step_margin)
    # ---- the punctual record ----
    punctual, pcontrib, pcond, pmargin = np.zeros(n, bool), np.zeros((n, 3)), np.zeros(n), np.ones(n)
    if lights is not None and len(lights[0]):
        recs, lcdf = np.asarray(lights[0], F32), np.asarray(lights[1], F64)
        ul = rng_f(keys, RNG_PUNCTUAL + int(bounce) + 1, 0).astype(F64)
        li = np.minimum(np.searchsorted(lcdf, ul, side="right"), len(lcdf) - 1)
        pmargin = np.abs(lcdf[None, :] - ul[:, None]).min(1) / 2.0 ** -22
        R = recs[li].astype(F64)
        kind = lref.rec_type(np.ascontiguousarray(recs[li]))
        pos, axis, rng_, I, cin, cout = R[:, 0:3], R[:, 4:7], R[:, 7], R[:, 8:11], R[:, 14], R[:, 15]
        po, pd, ptm = np.asarray(got["po"], F64), np.asarray(got["pd"], F64), np.asarray(got["ptmax"], F64)
        with np.errstate(all="ignore"):
            to = pos - P
            dist = np.linalg.norm(to, axis=1)
            wl = np.where((kind == lref.DIRECTIONAL)[:, None], -axis, to / dist[:, None])
            fall = np.where(kind == lref.DIRECTIONAL, 1.0, 1.0 / (dist * dist))
            win_raw = 1 - (dist * dist / (rng_ * rng_)) ** 2
            win = np.clip(win_raw, 0, 1)
            fall = np.where((rng_ > 0) & (kind != lref.DIRECTIONAL), fall * win, fall)
            sm_raw = ((axis * -wl).sum(1) - cout) / np.maximum(cin - cout, 0.001)
            sm = np.clip(sm_raw, 0, 1)
            fall = np.where(kind == lref.SPOT, fall * sm * sm, fall)
            p_ok = go & (fall > 0) & (I.max(1) > 0)
            ph = hg((pd * d).sum(1))
            val = Tp * I * (fall * ph / R[:, 11] * through(po, pd, ptm))[:, None]
            # conditions: the distance (twice), and where a cone's or a window's factor comes close to zero its own rounding over its value
            c_d = np.where(kind == lref.DIRECTIONAL, 0.0, 4 * 2.0 ** -23 * (1 + np.abs(P).max(1)) / np.maximum(dist, 1e-30))
            c_s = np.where(kind == lref.SPOT, 8 * 2.0 ** -23 / np.maximum(cin - cout, 0.001) / np.maximum(sm, 1e-30), 0.0)
            c_w = np.where((rng_ > 0) & (kind != lref.DIRECTIONAL), 8 * 2.0 ** -23 / np.maximum(win, 1e-30), 0.0)
        punctual, pcontrib, pcond = p_ok, np.where(p_ok[:, None], val, 0.0), c_d + c_s + c_w
        # a record exists or not by which side of a cone's or a window's edge P lies on: within 1e-5 of the edge (in the factor's own units) is undecided
        edge = np.minimum(np.where(kind == lref.SPOT, np.abs(sm_raw), 1.0), np.where((rng_ > 0) & (kind != lref.DIRECTIONAL), np.abs(win_raw), 1.0))
        pmargin = np.where(go, np.minimum(pmargin, edge / 1e-5), 1.0)
    r.update(punctual=punctual, pcontrib=pcontrib, punctual_cond=pcond, punctual_margin=pmargin)
    # ---- the continuation ----
    u1 = u(1)
    with np.errstate(all="ignore"):
        c = 1 - 2 * u1 if abs(g) < 1e-3 else (1 + g * g - ((1 - g * g) / (1 - g + 2 * g * u1)) ** 2) / (2 * g)
    qq = Tp.max(1)
    pr = np.clip(qq, float(RR_PMIN), 1.0)
    rr = int(bounce) + 1 >= RR_START
    alive = go & (~(u(3) >= pr) if rr else np.ones(n, bool))
    r.update(alive=alive, cos=np.clip(c, -1, 1), T_cont=np.where(alive[:, None], Tp / (pr[:, None] if rr else 1.0), 0.0), rr_margin=np.abs(u(3) - pr) if rr else np.ones(n),
             pdf=hg((np.asarray(got["d"], F64) * d).sum(1)), P=P, go=go)
    return r


def check(m, got, r, what=""):
    """A float32 medium_step result `got` (the device's, or the restatement's in the same layout) against r = reference64(.., got, ..).  Undecided rays are skipped and
    counted, by class: scatter or stand (the free flight within 4 K_FLIGHT mean free paths of the span's end), an empty span (a sliver), the light kind (the number
    within 2^-22 of p_env), a cdf step (within 2^-22 of one; a sampled point seen edge-on; a texel's edge; a cone's or a window's edge), roulette (within 2^-20).
    Returns (problems, undecided)."""
    und = r["sliver"] | (r["crossed"] & (r["flight_margin"] < 4 * K_FLIGHT))
    sc = r["scattered"]
    und = und | (sc & ((r["rr_margin"] < 2.0 ** -20) | (r["kind_margin"] < 2.0 ** -22) | (r["go"] & ((r["step_margin"] < 1.0) | (r["punctual_margin"] < 1.0)))))
    dec = ~und
    bad = []
    g_sh = np.asarray(got["shadow"]) & np.asarray(got["scattered"])
    exp_sh = np.where(r.get("env_expected", np.zeros(len(dec), bool)) & ~r["shadow"], g_sh, r["shadow"])      # an environment texel without power gives no record
    for k, a, b in (("scattered", got["scattered"], sc), ("alive", np.asarray(got["alive"]) & np.asarray(got["scattered"]), r["alive"]), ("shadow", g_sh, exp_sh),
                    ("punctual", np.asarray(got["punctual"]) & np.asarray(got["scattered"]), r["punctual"])):
        if not np.array_equal(np.asarray(a)[dec], np.asarray(b)[dec]):
            bad.append(f"{what}: {k} differs on {int((np.asarray(a)[dec] != np.asarray(b)[dec]).sum())} decided rays")
    if bad:
        return bad, int(und.sum())
    pb = phase_bound(m.g)
    for flag, val, cond, have in (("shadow", "contrib", "shadow_cond", got["contrib"]), ("punctual", "pcontrib", "punctual_cond", got["pcontrib"])):
        sel = dec & r[flag]
        if sel.any():
            a, b = np.asarray(have, F64)[sel], r[val][sel]
            err = np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1e-300)
            tol = K_CONTRIB + pb + r[cond][sel]
            if (err > tol).any():
                i = int(np.argmax(err / tol))
                bad.append(f"{what}: {flag} contribution off by {err[i]:.3e} relative (bound {tol[i]:.3e})")
    sel = dec & r["shadow"] & ("dir_error" in r)
    if sel.any() and ((r["dir_error"][sel] > 1e-5).any() or (r["tmax_error"][sel] > 1e-5).any()):
        bad.append(f"{what}: an emitter record does not point at the sampled point, or does not end 0.1 % before it")
    sel = dec & r["alive"]
    if sel.any():
        wi = np.asarray(got["d"], F64)[sel]
        eT = np.abs(np.asarray(got["T"], F64)[sel] - r["T_cont"][sel]).max(1) / np.maximum(r["T_cont"][sel].max(1), 1e-300)
        ep = np.abs(np.asarray(got["pdf"], F64)[sel] - r["pdf"][sel]) / r["pdf"][sel]
        ec = np.abs((wi * np.asarray(got["d_in"], F64)[sel]).sum(1) - r["cos"][sel])
        eo = np.abs(np.asarray(got["o"], F64)[sel] - r["P"][sel]).max(1) / np.maximum(np.abs(r["P"][sel]).max(1), 1.0)
        if (eT > K_THROUGHPUT).any():
            bad.append(f"{what}: continuation throughput off by {eT.max():.3e}")
        if (ep > pb + K_THROUGHPUT).any():
            bad.append(f"{what}: continuation pdf off by {ep.max():.3e} relative (bound {pb + K_THROUGHPUT:.3e})")
        if (ec > K_COS + 2.0 ** -20).any() or (np.abs(np.linalg.norm(wi, axis=1) - 1) > 2.0 ** -18).any():
            bad.append(f"{what}: continuation direction: cosine off by {ec.max():.3e} (bound {K_COS:.3e}) or not of unit length")
        if (eo > 2.0 ** -20).any():
            bad.append(f"{what}: continuation origin off by {eo.max():.3e}")
    return bad, int(und.sum())


def as_got(res, d_in, scattered=None):
    """A scatter_step result (or a medium_step dict) in the layout check takes."""
    if "srec" in res:
        sr, pr, ct = np.asarray(res["srec"]), np.asarray(res["prec"]), np.asarray(res["cont"])
        return dict(scattered=res["scattered"], alive=res["alive"], shadow=res["shadow"], punctual=res["punctual"], so=sr[:, 0:3], sd=sr[:, 3:6], tmax=sr[:, 6], contrib=sr[:, 7:10],
                    po=pr[:, 0:3], pd=pr[:, 3:6], ptmax=pr[:, 6], pcontrib=pr[:, 7:10], o=ct[:, 0:3], d=ct[:, 3:6], T=ct[:, 6:9], pdf=ct[:, 9], d_in=np.asarray(d_in))
    out = dict(res)
    out.update(scattered=scattered, d_in=np.asarray(d_in))
    return out
