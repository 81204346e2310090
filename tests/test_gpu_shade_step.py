"""One k_shade step on a real MI355X against the per-ray float64 reference (tests/shade_reference.py; include/ptc_shade_debug.h: ptc_debug_shade_step).

The hook runs k_set_counts, k_trace_closest and one launch of k_shade on explicit rays and returns every record the step produced.  The reference takes the
device's hit (primitive, u, v, t) and evaluates the step from the definitions in float64: every quantity at the device's own directions, within its first-order
bound K 2^-23 kappa, and the device's directions against the samples recomputed from the same random numbers, on every ray whose decisions float64 can make.

1. The three scenes (shade_lobes, shade_textured with NEAREST and LINEAR, shade_sky) x the ray sets (1, 63, 64, 65, 513 camera rays, the grazing set, exact
   normal incidence on both sides) x the bounces 0, 1, 2, 5 and max_bounces; the rays aimed at the emitters at bounce = max_bounces.
2. Three chained steps: each fed the continuation of the one before, so the emission weights see real pdfs.
3. The three kernel variants give identical bits.
4. The density of the continuation and next-event directions of 65,536 keys at one point: chi-square against the reference pdf.
5. What the hook refuses."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shade_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
E_ARG = -1
SCENES = ("lobes", "textured-nearest", "textured-linear", "sky")
_cache = {}


def _ctx(pbr, name):
    """(context, reference scene) of a test scene, committed once per session."""
    if name not in _cache:
        s = pbr.scenes
        desc = {"lobes": s.shade_lobes, "textured-nearest": s.shade_textured, "textured-linear": lambda: s.shade_textured("linear"), "sky": s.shade_sky}[name]()
        pt = pbr.PathTracer(0).load_scene(desc)
        _cache[name] = (pt, ref.Scene(pt, desc))
    return _cache[name]


def _step(pt, rays, bounce, max_bounces=ref.MAX_BOUNCES, variant=0):
    dev = pt.shade_step(rays["o"], rays["d"], rays["T"], rays["pdf"], rays["keys"], bounce, max_bounces, variant)
    hit = dict(prim=np.where(dev["word"] < 0, -1, dev["word"] & 0x0fffffff), u=dev["uv"][:, 0], v=dev["uv"][:, 1], t=dev["t"])
    return dev, hit


def _merge(total, worst):
    for k, v in worst.items():
        total[k] = max(total.get(k, 0.0), v)


@pytest.mark.parametrize("name", SCENES)
def test_step_lies_within_the_bounds_of_the_float64_reference(pbr, name):
    pt, sc = _ctx(pbr, name)
    total, shares = {}, {}
    sets = [(f"{n} rays", rays) for n, rays in ref.ray_sets(pt)] + list(ref.edge_sets())
    for label, rays in sets:
        n = len(rays["keys"])
        for b in ref.BOUNCES + (ref.MAX_BOUNCES,):
            dev, hit = _step(pt, rays, b)
            share, worst = ref.check(sc, rays, hit, b, ref.MAX_BOUNCES, dev, f"{name}, {label}")
            _merge(total, worst)
            shares[label] = max(shares.get(label, 0.0), share)
            assert share <= (ref.MAX_UNDECIDED if n >= 63 else 0.0), f"{name}, {label}, bounce {b}: {share:.3f} of the rays undecided"
    if sc.n_em:
        rays = ref.emitter_set(sc)
        for b in (0, 1, 3):
            dev, hit = _step(pt, rays, b, max_bounces=b)
            assert (sc.em_of_prim[hit["prim"][hit["prim"] >= 0]] >= 0).sum() >= 32, "the rays aimed at the emitters do not arrive"
            share, worst = ref.check(sc, rays, hit, b, b, dev, f"{name}, emitter rays")
            _merge(total, worst)
            shares["emitter rays"] = max(shares.get("emitter rays", 0.0), share)
            assert share <= ref.MAX_UNDECIDED
    print(f"\n{name}: worst error / (2^-23 kappa) {({k: round(v, 2) for k, v in total.items() if v})} of K {ref.K}; undecided share per set "
          f"{({k: round(v, 4) for k, v in shares.items()})}")


@pytest.mark.parametrize("name", ("lobes", "textured-nearest", "sky"))
def test_three_chained_steps(pbr, name):
    """Bounces 0, 1, 2 of the 513 camera rays, each step fed the continuation records of the one before: origin, direction, throughput and pdf are the device's.
    The scenes are open: most paths leave after the first bounce, and what they meet then — the environment, an emitter — is weighted with real pdfs."""
    pt, sc = _ctx(pbr, name)
    rays = [r for n, r in ref.ray_sets(pt) if n == 513][0]
    rays = dict(rays, T=np.ones_like(rays["T"]), pdf=np.zeros_like(rays["pdf"]))
    for b in range(3):
        dev, hit = _step(pt, rays, b)
        share, worst = ref.check(sc, rays, hit, b, ref.MAX_BOUNCES, dev, f"{name}, chained")
        assert share <= ref.MAX_UNDECIDED, (b, share)
        a = dev["alive"]
        if b == 0:
            assert a.sum() >= 64, f"{a.sum()} paths left after the first step"
        elif name == "sky":      # the paths that left the floor see the environment, weighted with the pdf the device sampled them with
            assert (dev["lpath"] > 0).any(1).sum() >= 64
        if not a.any():
            break
        rays = dict(o=dev["o"][a], d=dev["d"][a], T=dev["T"][a], pdf=dev["pdf"][a], keys=rays["keys"][a])


@pytest.mark.parametrize("name", SCENES)
def test_the_three_variants_give_identical_bits(pbr, name):
    pt, sc = _ctx(pbr, name)
    sets = [r for n, r in ref.ray_sets(pt) if n in (65, 513)] + [r for _, r in ref.edge_sets()]
    for rays in sets:
        for b in (0, 2, ref.MAX_BOUNCES):
            base, _ = _step(pt, rays, b, variant=0)
            for variant in (1, 2):
                other, _ = _step(pt, rays, b, variant=variant)
                for k, v in base.items():
                    assert np.array_equal(np.ascontiguousarray(v).view(np.uint8), np.ascontiguousarray(other[k]).view(np.uint8)), (name, b, variant, k)


def _one_point_rays(point, incidence, n=65536):
    d = np.asarray([np.sin(incidence), 0.0, -np.cos(incidence)])
    rays = ref._rays_at(np.repeat(np.asarray(point, F64)[None], n, 0), np.repeat(d[None], n, 0), 89)
    rays["keys"] = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345)
    return rays


def _density_of(sc, rays, hit):
    """The reference's mixture pdf of the surface all rays of `rays` hit, as a function of local directions (the floor: local = world)."""
    S = ref.surface(sc, rays["d"][:1], hit["prim"][:1], hit["u"][:1], hit["v"][:1], F64)
    assert np.array_equal(S["ns"][0], (0.0, 0.0, 1.0))

    def pdf_of(w):
        Sw = {k: np.repeat(v, len(w), 0) for k, v in S.items()}
        return ref.Bsdf(Sw, F64).eval(w)[1]
    return pdf_of


@pytest.mark.parametrize("case", ("lambert", "ggx02"))
def test_sampler_density_on_the_floor(pbr, case):
    """65,536 keys at one floor point of shade_lobes: the continuation directions against the mixture pdf over 256 cells of equal solid angle (the samples the
    step drops are one more cell), the next-event points against the emitter pmf x uniform area over 25 cells per emitter."""
    pt, sc = _ctx(pbr, "lobes")
    point = {"lambert": (-1.0, -1.1, 0.0), "ggx02": (0.9, 1.1, 0.0)}[case]
    rays = _one_point_rays(point, 0.7)
    n = len(rays["keys"])
    dev, hit = _step(pt, rays, 0)
    assert (hit["prim"] == hit["prim"][0]).all() and sc.lambert[sc.tri_mat[hit["prim"][0]]] == (case == "lambert")
    expected, total = ref.hemisphere_expected(_density_of(sc, rays, hit), n)
    counts = ref.hemisphere_cells(dev["d"][dev["alive"]].astype(F64))
    lost = n - dev["alive"].sum()
    stat, dof, p = ref.chi2_test(np.append(counts, lost), np.append(expected, max(n * (1.0 - total), 0.0)))
    print(f"\n{case}: continuation chi^2 = {stat:.1f} at {dof} degrees of freedom, p = {p:.3g}; pdf integral {total:.5f}, dropped {lost}")
    assert p >= 1e-6
    # next-event estimation: every sample of this point is valid, the record says which emitter and where on it
    s = dev["shadow"]
    assert s.all()
    j, y, _ = ref._which_emitter(sc, dev["so"].astype(F64), dev["sd"].astype(F64), dev["tmax"].astype(F64))
    tri = sc.verts[sc.idx[sc.em_prims[j]]][:, :, 0:3].astype(F64)
    e1, e2, q = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], y - tri[:, 0]
    d11, d12, d22, q1, q2 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1), (q * e1).sum(1), (q * e2).sum(1)
    det = d11 * d22 - d12 * d12
    bu, bv = (q1 * d22 - q2 * d12) / det, (q2 * d11 - q1 * d12) / det
    su = np.clip(bu + bv, 1e-12, 1.0)
    r1, r2 = su * su, np.clip(bv / su, 0.0, 1.0 - 1e-12)
    cell = j * 25 + np.minimum((r1 * 5).astype(np.int64), 4) * 5 + np.minimum((r2 * 5).astype(np.int64), 4)
    pmf = sc.tables(F64)["em_pmf"]
    stat, dof, p = ref.chi2_test(np.bincount(cell, minlength=25 * sc.n_em), np.repeat(pmf * n / 25.0, 25))
    print(f"{case}: next-event chi^2 = {stat:.1f} at {dof} degrees of freedom, p = {p:.3g}")
    assert p >= 1e-6


def test_sampler_density_of_the_sky(pbr):
    """65,536 keys at one floor point of shade_sky: the next-event directions against the environment's texel pmf, over the texels that lie wholly above the
    floor (the rest, and the samples below the floor, are one more cell)."""
    pt, sc = _ctx(pbr, "sky")
    rays = _one_point_rays((-1.0, -1.1, 0.0), 0.7)
    n = len(rays["keys"])
    dev, hit = _step(pt, rays, 0)
    h, w = sc.env.shape[:2]
    pmf = sc.tables(F64)["env_pmf"]
    # a texel (y, x) spans theta in pi [y, y + 1] / h and phi in 2 pi [x, x + 1] / w - pi; on the floor wi.z = -sin(theta) sin(2 pi u) must be positive
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    above = np.ones((h, w), bool)
    for du in (0.0, 0.5, 1.0):
        above &= -np.sin(2 * np.pi * (xx + du) / w) > 1e-6
    s = dev["shadow"]
    _, _, _, _, (ty, tx) = ref.env_at(sc, sc.tables(F64), dev["sd"][s].astype(F64), F64)
    counts = np.zeros((h, w))
    np.add.at(counts, (ty, tx), 1)
    full = above & (pmf > 0)
    rest_c, rest_e = n - counts[full].sum(), n * (1.0 - pmf[full].sum())
    stat, dof, p = ref.chi2_test(np.append(counts[full], rest_c), np.append(pmf[full] * n, rest_e))
    print(f"\nsky: next-event chi^2 = {stat:.1f} at {dof} degrees of freedom, p = {p:.3g}")
    assert p >= 1e-6
    assert not counts[pmf == 0].any(), "a texel without power was sampled"


def test_refusals(pbr):
    pt, sc = _ctx(pbr, "lobes")
    rays = [r for n, r in ref.ray_sets(pt) if n == 63][0]
    L, h = pt._L, pt._h
    n = 63
    bufs = dict(hit=np.zeros((n, 4), F32), lp=np.zeros((n, 3), F32), alive=np.zeros(n, np.uint8), cont=np.zeros((n, 10), F32), sh=np.zeros(n, np.uint8),
                srec=np.zeros((n, 10), F32))
    P = pbr.ptc._ptr

    def call(o=rays["o"], d=rays["d"], T=rays["T"], pdf=rays["pdf"], keys=rays["keys"], count=n, bounce=0, max_bounces=8, variant=0, drop=None):
        ins = [None if drop == i else P(np.ascontiguousarray(a)) for i, a in enumerate((o, d, T, pdf, keys))]
        outs = [None if drop == 5 + i else P(bufs[k]) for i, k in enumerate(("hit", "lp", "alive", "cont", "sh", "srec"))]
        return L.ptc_debug_shade_step(h, *ins, count, bounce, max_bounces, variant, *outs)

    assert call() == 0
    before = pt.raw_counters()
    for i in range(11):
        assert call(drop=i) == E_ARG, i
    assert call(count=0) == E_ARG and call(variant=3) == E_ARG and call(variant=-1) == E_ARG and call(bounce=2 ** 21) == E_ARG
    for bad in (np.nan, np.inf):
        for k in ("o", "d", "T"):
            a = rays[k].copy()
            a[17, 1] = bad
            assert call(**{k: a}) == E_ARG, (k, bad)
        a = rays["pdf"].copy()
        a[17] = bad
        assert call(pdf=a) == E_ARG
    d = rays["d"].copy()
    d[5] *= F32(1.01)
    assert call(d=d) == E_ARG
    d[5] = 0
    assert call(d=d) == E_ARG
    assert pt.raw_counters() == before, "a refused call launched something"
    assert L.ptc_debug_shade_step(None, *([None] * 5), n, 0, 8, 0, *([None] * 6)) == E_ARG
    # alpha coverage and transmission sit between trace and shade
    for desc in (pbr.scenes.alpha_layers(), pbr.scenes.glass_slab()):
        other = pbr.PathTracer(0).load_scene(desc)
        with pytest.raises(pbr.ptc.PtcError, match="between trace and shade"):
            other.shade_step(rays["o"], rays["d"], rays["T"], rays["pdf"], rays["keys"])
        other.close()
    # a description-only context has no device
    none = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(pbr.scenes.shade_lobes())
    with pytest.raises(pbr.ptc.PtcError):
        none.shade_step(rays["o"], rays["d"], rays["T"], rays["pdf"], rays["keys"])
