"""The float64 reference of a k_shade step, without a GPU (tests/shade_reference.py; the device is held to it by tests/test_gpu_shade_step.py).

a. The reference against itself: the mixture pdf integrates to 1 over the material grid and from normal to grazing view; the two MIS weights of one direction
   sum to 1; the samplers' histograms match their pdf; step(dt=float32) lies within the bounds of step(dt=float64) — which is the measurement of K.
b. The tables the estimator reads, on description-only contexts: the probability the cdf selects an emitter or an environment texel with against the pmf its
   contribution is divided by, and both against the float64 pmf of the description.
c. Teeth: eight mutations of the float32 evaluation, each caught with the shipped K.
d. The share of undecided rays of the float64 reference alone, on every ray set of the GPU test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shade_reference as ref  # noqa: E402

F32, F64 = np.float32, np.float64
SCENES = ("lobes", "textured-nearest", "textured-linear", "sky")
_cache = {}


def _ctx(pbr, name):
    if name not in _cache:
        s = pbr.scenes
        desc = {"lobes": s.shade_lobes, "textured-nearest": s.shade_textured, "textured-linear": lambda: s.shade_textured("linear"), "sky": s.shade_sky}[name]()
        pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)
        _cache[name] = (pt, ref.Scene(pt, desc))
    return _cache[name]


def _cases(pbr, name):
    """(label, rays, hit, bounce, max_bounces) of every step the GPU test runs on scene `name`, the hits from the float64 search of all triangles."""
    pt, sc = _ctx(pbr, name)
    sets = [(f"{n} rays", rays) for n, rays in ref.ray_sets(pt)] + list(ref.edge_sets())
    for label, rays in sets:
        hit = ref.hits_of(sc, rays["o"], rays["d"], grazing=label == "grazing")
        for b in ref.BOUNCES + (ref.MAX_BOUNCES,):
            yield label, rays, hit, b, ref.MAX_BOUNCES
    if sc.n_em:
        rays = ref.emitter_set(sc)
        hit = ref.hits_of(sc, rays["o"], rays["d"], grazing=True)
        for b in (0, 1, 3):
            yield "emitter rays", rays, hit, b, b


def _flat_surface(metallic, roughness, nv, n=1, base=(0.8, 0.7, 0.6)):
    """A surface dict as shade_reference.surface returns it: the plane z = 0 seen from wo = (sin, 0, nv)."""
    one = np.ones(n)
    z = np.repeat(np.asarray([[0.0, 0.0, 1.0]]), n, 0)
    wo = np.repeat(np.asarray([[np.sqrt(1 - nv * nv), 0.0, nv]]), n, 0)
    lam = metallic == 0 and roughness >= 1
    return dict(P=z * 0, ng=z, ns=z, wo=wo, front=one > 0, base=np.repeat(np.asarray([base], F64), n, 0), metallic=one * metallic, roughness=one * roughness,
                lambert=(one > 0) & lam, ktex=one * 0)


# ---- a -----------------------------------------------------------------------------------------------------------------------------------------------------
GRID = [(0.0, 1.0), (0.0, 0.0), (0.0, 0.05), (0.0, 0.5), (1.0, 0.0), (1.0, 0.05), (1.0, 0.5), (1.0, 1.0)]


@pytest.mark.parametrize("nv", (1.0, 0.5, 1e-2, 1e-4))
def test_mixture_pdf_integrates_to_one(pbr, nv):
    """Quadrature of the reference's pdf over the upper hemisphere.  The cosine density on a uniform grid in (cos theta, phi).  The VNDF density, far too narrow
    for that grid at alpha = 1e-3, over the half vectors by the GGX distribution's own inverse cdf (tan^2 theta_h = alpha^2 xi / (1 - xi): D cos theta_h dh =
    d xi d phi / 2 pi), with dwi = 4 (v.h) dh.  A visible normal whose reflection leaves below the surface is a sample the step drops: that mass, integrated
    with the textbook D_v(h) = G1(v) (v.h) D(h) / v.z over the same grid, is what the pdf over the hemisphere lacks of 1."""
    assert pbr.scenes.SHADE_GRID == GRID
    N = 768
    xi, ph = np.meshgrid((np.arange(N) + 0.5) / N, (np.arange(N) + 0.5) / N * 2 * np.pi, indexing="ij")
    xi, ph = xi.reshape(-1), ph.reshape(-1)
    worst = 0.0
    for metallic, roughness in GRID:
        S = _flat_surface(metallic, roughness, nv, len(xi))
        B = ref.Bsdf(S, F64)
        # the cosine part: wi on a grid of equal solid angle
        z = xi
        wi = np.stack([np.sqrt(1 - z * z) * np.cos(ph), np.sqrt(1 - z * z) * np.sin(ph), z], -1)
        B.eval(wi)
        I_cos = B.parts[1].mean() * 2 * np.pi
        assert abs(I_cos - 1) < 1e-5, (metallic, roughness, I_cos)
        if B.lambert[0]:
            assert np.array_equal(B.eval(wi)[1], B.parts[1]) and (B.ps == 0).all()
            continue
        a = float(B.alpha[0])
        # towards the horizon of the half vectors (v.h) / cos(theta_h) grows like (1 - xi)^(-1/2): xi = 1 - (1 - s)^2 takes the singularity out of the grid
        xs, jac = 1 - (1 - xi) ** 2, 2 * (1 - xi)
        t2 = a * a * xs / (1 - xs)
        ch = 1 / np.sqrt(1 + t2)
        sh = np.sqrt(t2) * ch
        h = np.stack([sh * np.cos(ph), sh * np.sin(ph), ch], -1)
        v = S["wo"]
        vh = (v * h).sum(1)
        wi = 2 * vh[:, None] * h - v
        up = (wi[:, 2] > 0) & (vh > 0)
        wi_up = np.where(up[:, None], wi, np.asarray([0.0, 0.0, 1.0]))
        B.eval(wi_up)
        D = a * a / (np.pi * (1 + ch * ch * (a * a - 1)) ** 2)
        seen = (jac * np.where(up, B.parts[0] * 4 * vh / (D * ch), 0.0)).mean()      # the pdf's mass above the surface
        g1v = 2 * nv / (nv + np.sqrt(nv * nv + a * a * (1 - nv * nv)))
        below = (jac * np.where(~up & (vh > 0), g1v * vh / (nv * ch), 0.0)).mean()    # D_v's mass that reflects below it
        ps = float(B.ps[0])
        total = ps * seen + (1 - ps) * I_cos
        worst = max(worst, abs(seen + below - 1))
        assert abs(seen + below - 1) < 2e-3, (metallic, roughness, nv, seen, below)
        assert abs(total + ps * below - 1) < 2e-3
    print(f"\nn.v = {nv}: the VNDF density's mass and the dropped mass sum to 1 within {worst:.2e}")


def test_mis_weights_of_one_direction_sum_to_one(pbr):
    """A direction the next-event step samples towards an emitter, and the same direction as a continuation that hits the emitter one bounce later: the weights
    p_l^2 / (p_l^2 + p_b^2) and p_b^2 / (p_b^2 + p_l^2) use one p_l (from P to the sampled point: d^2, the cosine, P(select), p_area) and one p_b."""
    for name in ("lobes", "textured-nearest"):
        pt, sc = _ctx(pbr, name)
        rays = [r for n, r in ref.ray_sets(pt) if n == 513][0]
        rays = dict(rays, T=np.ones_like(rays["T"]))
        hit = ref.hits_of(sc, rays["o"], rays["d"])
        R = ref.step(sc, rays, hit, 0, 8)
        k = np.flatnonzero(R["shadow"] & (R["light"] >= 0))
        assert len(k) >= 50
        S = ref._sub(ref.surface(sc, rays["d"], hit["prim"], hit["u"], hit["v"]), k)
        dv = R["y"][k] - S["P"]
        wi = dv / np.sqrt((dv * dv).sum(1))[:, None]
        f, pb, _ = ref.Bsdf(S, F64).eval(wi)
        # the continuation: from P along wi with pdf p_b, throughput 1; it must reach the sampled point (the NEE ray's offset origin sees the same emitter)
        second = dict(o=S["P"] + wi * 1e-3, d=wi, T=np.ones((len(k), 3)), pdf=pb, keys=rays["keys"][k])
        hit2 = ref.hits_of(sc, second["o"], second["d"], grazing=True)
        same = sc.em_of_prim[np.maximum(hit2["prim"], 0)] == R["light"][k]
        assert same.mean() > 0.9
        hit2["t"] = hit2["t"] + 1e-3                                  # the distance from P
        E = ref.step(sc, second, hit2, 1, 1)
        Le = sc.emissive[sc.tri_mat[sc.em_prims[R["light"][k]]]].astype(F64)
        w_e = (E["lpath"] / Le).max(1)                                # p_b^2 / (p_b^2 + p_l^2)
        nl = (S["ns"] * wi).sum(1)
        with np.errstate(all="ignore"):
            pl = pb * np.sqrt(1 / w_e - 1)
            w_n = (R["contrib"][k] / (f * Le * (nl / pl)[:, None])).max(1)
        ok = same & (w_e > 1e-9) & (w_e < 1 - 1e-9)
        assert ok.sum() >= 40
        assert np.abs(w_n + w_e - 1)[ok].max() < 1e-9, np.abs(w_n + w_e - 1)[ok].max()
    p, q = np.random.default_rng(3).uniform(1e-3, 1e3, (2, 1000))
    assert np.abs(ref._mis(p, q, None) + ref._mis(q, p, None) - 1).max() < 1e-15


@pytest.mark.parametrize("metallic,roughness,nv", [(0.0, 1.0, 0.7), (0.0, 0.5, 0.7), (1.0, 0.5, 0.2), (0.0, 0.05, 0.9)])
def test_sampler_histogram_matches_the_pdf(metallic, roughness, nv):
    """65,536 samples of the reference's cosine and VNDF samplers against its own pdf: chi-square over up to 256 cells of equal solid angle (cells expecting fewer
    than 10 samples pooled; the samples that leave below the surface are one more cell), significance 1e-6 from the chi-square distribution itself."""
    n = 65536
    rng = np.random.default_rng(101)
    grid = lambda: (rng.integers(0, 2 ** 24, n) / 2.0 ** 24)
    S = _flat_surface(metallic, roughness, nv, n)
    wi, ok, _, _, _ = ref.Bsdf(S, F64).sample(grid(), grid(), grid())
    one = _flat_surface(metallic, roughness, nv, 1)

    def pdf_of(w):
        return ref.Bsdf({k: np.repeat(v, len(w), 0) for k, v in one.items()}, F64).eval(w)[1]
    expected, total = ref.hemisphere_expected(pdf_of, n, sub=64 if roughness < 0.1 else 32)
    counts = ref.hemisphere_cells(wi[ok])
    stat, dof, p = ref.chi2_test(np.append(counts, n - ok.sum()), np.append(expected, max(n * (1 - total), 0.0)), min_cells=64 if roughness >= 0.1 else 32)
    print(f"\nmetallic {metallic} roughness {roughness} n.v {nv}: chi^2 = {stat:.1f} at {dof} degrees of freedom, p = {p:.3g}; below the surface {n - ok.sum()}")
    assert p >= 1e-6


def test_chi2_tail_probability():
    """chi2_sf against values of the chi-square distribution's tables, and the test itself on counts drawn from the expected distribution and from a shifted one."""
    for x, k, p in ((3.841, 1, 0.05), (18.307, 10, 0.05), (124.342, 100, 0.05), (23.209, 10, 0.01), (149.449, 100, 0.001), (1e-9, 4, 1.0)):
        assert abs(ref.chi2_sf(x, k) - p) < 5e-3 * p, (x, k, ref.chi2_sf(x, k))      # the tables give x to three decimals
    assert ref.chi2_sf(400.0, 100) < 1e-30
    rng = np.random.default_rng(5)
    e = np.full(100, 655.36)
    assert ref.chi2_test(rng.multinomial(65536, e / e.sum()), e)[2] > 1e-3
    shifted = e * np.where(np.arange(100) < 50, 1.04, 0.96)
    assert ref.chi2_test(rng.multinomial(65536, shifted / shifted.sum()), e)[2] < 1e-6


def test_float32_lies_within_the_bounds(pbr):
    """The measurement of K, and part d.  step(dt=float32) against step(dt=float64) over every step of the GPU test: the worst ratio error / (2^-23 kappa) per
    quantity class.  The shipped K is at least four times the worst ratio, and no more than sixteen times: the smallest power of two with the factor four,
    plus one binade for a numpy whose float32 sine, cosine or arctangent rounds otherwise.  The undecided share of every set stays within the cap."""
    total, shares = {}, {}
    for name in SCENES:
        pt, sc = _ctx(pbr, name)
        rep = {}
        for label, rays, hit, b, mb in _cases(pbr, name):
            cand = ref.step(sc, rays, hit, b, mb, F32)
            share, _ = ref.check(sc, rays, hit, b, mb, cand, f"{name}, {label}", report=rep)
            shares[(name, label)] = max(shares.get((name, label), 0.0), share)
            n = len(rays["keys"])
            assert share <= (ref.MAX_UNDECIDED if n >= 63 else 0.0), f"{name}, {label}, bounce {b}: {share:.4f} of the rays undecided"
        rep.pop("why", None)
        print(f"\n{name}: worst error / (2^-23 kappa) {({k: round(v, 2) for k, v in rep.items()})}")
        for k, v in rep.items():
            total[k] = max(total.get(k, 0.0), v)
    print(f"all scenes: {({k: round(v, 2) for k, v in total.items()})}; K = {ref.K}")
    print("undecided share per set:", {f"{a}, {b}": round(v, 4) for (a, b), v in shares.items() if v})
    assert set(total) == set(ref.K)
    for k, v in total.items():
        assert ref.K[k] / 16 < v <= ref.K[k] / 4, f"K[{k}] = {ref.K[k]} against a worst ratio of {v:.3f}"


# ---- b -----------------------------------------------------------------------------------------------------------------------------------------------------
def _emitter_scene(pbr, n, spread):
    """n emissive triangles side by side whose areas are spread log-uniformly over `spread`, with varying radiance, and a floor."""
    s = pbr.scene
    rng = np.random.default_rng(7 + n)
    area = np.exp(rng.uniform(0.0, np.log(spread), n)) if n > 1 else np.ones(1)
    side = np.sqrt(2 * area) * 1e-3
    V = np.zeros(3 * n, s.MESH_VERTEX)
    x0 = np.arange(n) * 5.0
    P = np.zeros((n, 3, 3))
    P[:, :, 0] = x0[:, None]
    P[:, 1, 0] += side
    P[:, 2, 1] = side
    V["position"], V["normal"], V["tangent"] = P.reshape(-1, 3), (0, 0, 1), (1, 0, 0, 1)
    mats, meshes = [], []
    for m in range(4):      # four radiances
        mats.append(s.Material((0, 0, 0, 1), 0.0, 1.0, tuple(rng.uniform(0.5, 20.0, 3))))
        sel = np.flatnonzero(np.arange(n) % 4 == m)
        if len(sel):
            idx = (sel[:, None] * 3 + np.arange(3)[None]).reshape(-1)
            meshes.append(s.MeshDesc(V, idx.astype(np.uint32), m))
    inst = [s.InstanceDesc(k) for k in range(len(meshes))]
    return s.SceneDesc(mats, meshes, inst, s.CameraDesc((0, 0, 5), (0, 0, 0), 1.0, 1.0), f"emitters{n}")


@pytest.mark.parametrize("n,spread", [(1, 1.0), (2, 10.0), (64, 1e3), (65, 1e3), (5000, 1e6)])
def test_emitter_table_is_consistent(pbr, n, spread):
    """For every emitter: the probability the cdf selects it with, cdf[i] - cdf[i - 1], against the pmf its contribution is divided by, and both against the
    float64 pmf A_i lum_i / sum from the geometry.  Allowed: the float32 running-sum bound n 2^-24 on a cdf value plus the random numbers' grid 2^-24."""
    desc = _emitter_scene(pbr, n, spread)
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)
    sc = ref.Scene(pt, desc)
    assert sc.n_em == n
    _, lights, cdf = pt.shading_tables()
    assert len(cdf) == n
    tri = sc.verts[sc.idx[sc.em_prims]][:, :, 0:3]
    assert np.array_equal(lights[:, 0:3], tri[:, 0]), "the emitter table is not in primitive order"
    pmf64 = sc.tables(F64)["em_pmf"]
    cdf64 = sc.tables(F64)["em_cdf"]
    cdf, pmf = cdf.astype(F64), lights[:, 7].astype(F64)
    select = np.diff(np.concatenate([[0.0], cdf]))
    allowed = n * 2.0 ** -24 + 2.0 ** -24
    assert cdf[-1] == 1.0 and (select >= 0).all()
    found = dict(cdf=np.abs(cdf - cdf64).max(), select_vs_pmf=np.abs(select - pmf).max(), select_vs_pmf64=np.abs(select - pmf64).max(), pmf_vs_pmf64=np.abs(pmf - pmf64).max(),
                 relative=float(np.abs(select / pmf - 1).max()))
    print(f"\n{n} emitters, areas over {spread:g}: allowed {allowed:.3g}, found {({k: float(f'{v:.3g}') for k, v in found.items()})}")
    assert found["cdf"] <= allowed and found["pmf_vs_pmf64"] <= allowed
    assert found["select_vs_pmf"] <= 2 * allowed and found["select_vs_pmf64"] <= 2 * allowed


def _env_case(case):
    rng = np.random.default_rng(11)
    if case == "1x1":
        return np.full((1, 1, 3), 0.7, F32)
    if case == "8x4":
        return rng.uniform(0.1, 2.0, (4, 8, 3)).astype(F32)
    if case == "64x32":
        e = rng.uniform(0.1, 1.0, (32, 64, 3)).astype(F32)
        e[3] = 0.0
        e[17:19] = 0.0
        e[9, 40] *= 1e4
        return e
    return rng.uniform(0.0, 1.0, (256, 512, 3)).astype(F32) ** 4


@pytest.mark.parametrize("case", ("1x1", "8x4", "64x32", "512x256"))
def test_environment_tables_are_consistent(pbr, case):
    """For every environment texel with a non-zero pmf: the probability the two cdfs select it with, (marg[y] - marg[y - 1]) (cond[y][x] - cond[y][x - 1]),
    against the pmf its contribution is divided by, and both against the float64 pmf lum sin(theta_row) / sum of the image.  Allowed on a cdf value: n 2^-24 of
    the running sums behind it (n = w h for the row marginal, w for a row's conditional) plus the grid 2^-24."""
    desc = pbr.scenes.shade_sky()
    desc.env = _env_case(case)
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(desc)
    sc = ref.Scene(pt, desc)
    env, marg, cond, ok = pt.env_tables()
    h, w = desc.env.shape[:2]
    assert ok and env.shape == (h, w, 4) and np.array_equal(env[..., 0:3], desc.env)
    t = sc.tables(F64)
    pmf64, pmf = t["env_pmf"], env[..., 3].astype(F64)
    marg, cond = marg.astype(F64), cond.astype(F64)
    sel = np.diff(np.concatenate([[0.0], marg]))[:, None] * np.diff(np.concatenate([np.zeros((h, 1)), cond], 1), axis=1)
    a_marg, a_cond = (w * h + 1) * 2.0 ** -24, (w + 1) * 2.0 ** -24
    on = pmf > 0
    assert np.array_equal(on, pmf64 > 0) and marg[-1] == 1.0 and (cond[:, -1] == 1.0).all() and (sel >= 0).all()
    rows = pmf64.sum(1) > 0
    found = dict(marg=np.abs(marg - t["env_marg"]).max(), cond=np.abs(cond - t["env_cond"])[rows].max(), select_vs_pmf=np.abs(sel - pmf)[on].max(),
                 select_vs_pmf64=np.abs(sel - pmf64)[on].max(), pmf_vs_pmf64=np.abs(pmf - pmf64).max(), relative=float(np.abs(sel[on] / pmf[on] - 1).max()))
    print(f"\nenvironment {case}: allowed {a_marg:.3g} (marginal) {a_cond:.3g} (conditional), found {({k: float(f'{v:.3g}') for k, v in found.items()})}")
    assert found["marg"] <= a_marg and found["cond"] <= a_cond and found["pmf_vs_pmf64"] <= a_marg
    # a product of two differences: each factor is at most 1, each difference off by at most twice its cdf's allowance
    assert found["select_vs_pmf"] <= 2 * (a_marg + a_cond) and found["select_vs_pmf64"] <= 2 * (a_marg + a_cond)
    assert not sel[~on & rows[:, None]].any(), "a texel without power can be selected"


# ---- c -----------------------------------------------------------------------------------------------------------------------------------------------------
TEETH = {      # mutation -> (scene, bounce) at which it must show
    "balance": ("lobes", 1), "no_p_area": ("textured-nearest", 1), "no_sin": ("sky", 1), "rr_no_division": ("lobes", 2), "tmax_full": ("lobes", 0),
    "g1_no_alpha": ("lobes", 0), "vndf_no_warp": ("lobes", 0), "bitangent_sign": ("textured-nearest", 0),
}


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_mutation_is_caught(pbr, mutation):
    """Each mutation of the float32 evaluation fails the check against the float64 reference with the shipped K; the unmutated evaluation passes the same steps."""
    name, b = TEETH[mutation]
    pt, sc = _ctx(pbr, name)
    caught = clean = 0
    for label, rays, hit, bb, mb in _cases(pbr, name):
        if bb != b or len(rays["keys"]) < 63:
            continue
        ref.check(sc, rays, hit, bb, mb, ref.step(sc, rays, hit, bb, mb, F32), f"{name}, {label}")
        clean += 1
        try:
            ref.check(sc, rays, hit, bb, mb, ref.step(sc, rays, hit, bb, mb, F32, mutation), f"{name}, {label}, {mutation}")
        except AssertionError:
            caught += 1
    assert clean >= 4 and caught >= 1, f"{mutation}: caught in {caught} of {clean} sets"
    print(f"\n{mutation}: caught in {caught} of {clean} sets of {name} at bounce {b}")
