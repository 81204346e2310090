"""Punctual lights on a real MI355X (include/ptc.h: ptc_add_light ..., ptc_debug_punctual_nee; csrc/pt_lights.hip).

1. k_shade_punctual against its numpy restatement (tests/lights_reference.py), bit for bit, on textured and plain scenes, at and around a wave and over two segments.
2. The pipeline against the hooks, bit for bit: a frame's radiance is the sum of the hook's contributions whose shadow rays ptc_debug_trace_any reports free.
3. Several lights are unbiased: the weighted choice of one light per hit estimates the sum of the single-light images.
4. Indirect light and throughput: a point light against a small emissive triangle of the same intensity, through three bounces.
5. Invariance: tile shards, lights cleared again, a light changed during a frame."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lens_reference as lref  # noqa: E402
import lights_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SEED = 0x0BADC0FFEE123457


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------------------------
def _kernel_scene(pbr, name):
    if name == "cornell":
        d = pbr.scenes.cornell_box()
        lights = [dict(type="point", position=(0.3, 0.5, 0.2), intensity=(3.0, 2.5, 2.0), range=2.5, sampling_weight=1.0),
                  dict(type="spot", position=(-0.5, 0.9, 0.1), direction=(0.4, -1.0, -0.2), intensity=(6.0, 6.0, 9.0), cos_inner=0.9, cos_outer=0.6, sampling_weight=2.5),
                  dict(type="directional", direction=(0.2, -0.5, -1.0), intensity=(1.5, 1.2, 0.9), sampling_weight=0.7)]
        return d, lights
    d = pbr.scenes.textured_objects()
    d.texture_filter = "linear" if name == "textured_linear" else "nearest"
    lights = [dict(type="spot", position=(1.0, 3.0, 2.0), direction=(-0.3, -1.0, -0.5), intensity=(40.0, 35.0, 30.0), range=9.0, cos_inner=0.95, cos_outer=0.7, sampling_weight=2.0),
              dict(type="directional", direction=(-0.4, -1.0, -0.3), intensity=(2.0, 2.0, 1.8), sampling_weight=1.0)]
    if name == "textured_linear":
        lights.append(dict(type="point", position=(-1.5, 0.5, 1.5), intensity=(5.0, 7.0, 9.0), sampling_weight=0.5))
    return d, lights


@pytest.mark.parametrize("name", ["textured_nearest", "textured_linear", "cornell"])
def test_kernel_equals_reference_bit_for_bit(gpu, name):
    """ptc_debug_punctual_nee = k_trace_closest + k_shade_punctual on explicit rays.  Ray counts 1, 63, 64, 65 sit on and around a wave; 513 rays are two segments
    (PTC_SEG_MIN_LEN = 512: segments of 320 slots, the second holds 193 rays), and one of the two produces no record at all.  The reference is fed from
    ptc_debug_trace_closest's hits and ptc_debug_get_shading_tables."""
    desc, lights = _kernel_scene(gpu, name)
    pt = gpu.PathTracer(0).load_scene(desc)
    for l in lights:
        pt.add_light(l)
    table, cdf = pt.light_table()
    rt, rc = ref.light_table(lights)
    assert _bits_equal(table, rt) and _bits_equal(cdf, rc)
    shade = pt.shading_tables()[0]
    stride = shade.shape[1] // 4
    verts, _, _ = pt.flat_scene()
    eps = ref.scene_ray_eps(verts[:, 0:3])
    linear = desc.texture_filter == "linear"
    o_all, d_all = pt.debug_camera_rays(24, 24, SEED, 0, 1)
    rng = np.random.default_rng(7)
    seen_valid = seen_invalid_hit = 0
    for bounce in (0, 2):
        for n in (1, 63, 64, 65, 513):
            sel = rng.permutation(len(o_all))[:n] if n > 1 else np.array([len(o_all) // 2 + 12])
            o, d = o_all[sel].copy(), d_all[sel].copy()
            away = np.arange(n) % 3 == 1                               # every third ray leaves the scene: hits and misses interleave
            empty_first = name == "cornell"
            if n == 513:                                               # a whole segment of misses: the first 320 slots, or the last 193
                away = away | ((np.arange(n) < 320) if empty_first else (np.arange(n) >= 320))
            if n > 1:
                d[away] = -d[away]
            keys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
            t, prim, uv = pt.trace_closest(o, d)
            if n > 1:
                assert (prim[away] < 0).all() and (prim[~away] >= 0).any()
            valid, so, sd, tm, ct = pt.punctual_nee(o, d, keys, bounce)
            rv, rso, rsd, rtm, rct = ref.punctual_nee(shade, stride, desc.materials, desc.textures, linear, eps, table, cdf, d, keys, prim, uv, bounce)
            what = f"{name} bounce {bounce} n {n}"
            assert np.array_equal(valid, rv), what
            assert _bits_equal(so, rso) and _bits_equal(sd, rsd) and _bits_equal(tm, rtm) and _bits_equal(ct, rct), what
            if n == 513:
                seg_empty = valid[:320] if empty_first else valid[320:]
                seg_full = valid[320:] if empty_first else valid[:320]
                assert not seg_empty.any() and seg_full.any() and not seg_full.all(), what
            seen_valid += int(valid.sum())
            seen_invalid_hit += int(((prim >= 0) & ~valid).sum())
            assert np.isfinite(ct).all() and (ct >= 0).all()
    assert seen_valid > 200 and seen_invalid_hit > 20                  # records, and hits that face away from their light or lie outside its cone / range
    pt.close()


# ---- the plane with an occluding triangle of tests 2, 3 and 5 -----------------------------------------------------------------------------------------
def _plane_scene(pbr):
    S = pbr.scene
    mats = [S.Material((0.8, 0.7, 0.6, 1.0), 0.0, 1.0), S.Material((0.9, 0.9, 0.9, 1.0), 0.5, 0.4)]
    pv, pi = pbr.scenes._quad((-3, 0, 3), (3, 0, 3), (3, 0, -3), (-3, 0, -3))                    # normal +y
    tv = pbr.scenes._verts([(-0.7, 1, 0.5), (0.7, 1, 0.5), (0, 1, -0.7)], [(0, 1, 0)] * 3, [(1, 0, 0)] * 3, [(0, 0), (1, 0), (0, 1)])
    meshes = [S.MeshDesc(pv, pi, 0), S.MeshDesc(tv, np.array([0, 1, 2], np.uint32), 1)]
    cam = S.CameraDesc((0.0, 3.0, 3.0), (0.0, 0.0, 0.0), math.radians(50.0), 1.0)
    return S.SceneDesc(mats, meshes, [S.InstanceDesc(0), S.InstanceDesc(1)], cam, "plane_occluder")


SPOT = dict(type="spot", position=(0.2, 2.5, 0.1), direction=(0.05, -1.0, 0.1), intensity=(30.0, 25.0, 20.0), range=8.0, cos_inner=0.92, cos_outer=0.55)
POINT2 = dict(type="point", position=(-1.5, 1.5, 1.0), intensity=(4.0, 8.0, 12.0))


def _hook_samples(pt, w, h, spp, seed):
    """X[s, pixel, 3]: what sample s of every pixel receives from the context's lights at bounce 0 — the hook's contribution where ptc_debug_trace_any reports the
    shadow ray free, 0 elsewhere — on the rays ptc_debug_camera_rays returns, with the keys of lens_reference.path_key."""
    o, d = pt.debug_camera_rays(w, h, seed, 0, spp)
    pix = np.tile(np.arange(w * h, dtype=np.uint64), spp)
    smp = np.repeat(np.arange(spp, dtype=np.uint64), w * h)
    keys = lref.path_key(lref.seed_hash(seed), pix, smp).astype(np.uint32)
    valid, so, sd, tm, ct = pt.punctual_nee(o, d, keys, 0)
    X = np.zeros((spp * w * h, 3), F32)
    if valid.any():
        occ = pt.trace_any(so[valid], sd[valid], tm[valid])
        idx = np.flatnonzero(valid)[occ == 0]
        X[idx] = ct[idx]
    return X.reshape(spp, w * h, 3), valid.reshape(spp, w * h)


def test_pipeline_equals_hooks_bit_for_bit(gpu):
    """One light (pmf = 1), no emitters, max_bounces = 1: a path's radiance is its bounce-0 punctual sample.  Each pixel is the binary32 sum of its samples' contributions in
    sample order, divided by spp."""
    w = h = 32
    spp = 4
    pt = gpu.PathTracer(0).load_scene(_plane_scene(gpu))
    pt.add_light(SPOT)
    img = pt.render(w, h, spp, seed=SEED, max_bounces=1)
    st = pt.stats()
    X, valid = _hook_samples(pt, w, h, spp, SEED)
    acc = np.zeros((w * h, 3), F32)
    for s in range(spp):
        acc = acc + X[s]
    want = (acc / F32(spp)).reshape(h, w, 3)
    assert _bits_equal(img[..., :3], want)
    assert (img[..., 3] == 1).all()
    lit = (X > 0).any(2)
    umbra = (valid & ~lit).all(0) & valid.any(0)                       # every sample hit the plane, found the light and was occluded
    assert umbra.sum() >= 8 and (img[..., :3].reshape(-1, 3)[umbra] == 0).all()
    assert (want > 0).any(2).sum() > w * h // 4
    assert st["launches_trace_any"] == 1 and st["shadow_rays"] == int(valid.sum())      # no emitters, no environment: the punctual any-hit launch alone
    pt.close()


def test_several_lights_are_unbiased(gpu):
    """Two lights with weights 1 and 3: a sample is X_i / p_i with probability p_i (p = 1/4, 3/4), where X_i is what light i alone gives that sample (test 2's hook
    evaluation with light i as the only light).  Its mean is X_1 + X_2 and its variance sum_i X_i^2 / p_i - (X_1 + X_2)^2; block means over 8 x 8 pixels x 1024 spp must
    lie within 5 standard errors of the block means of X_1 + X_2."""
    w = h = 32
    spp = 1024
    pt = gpu.PathTracer(0).load_scene(_plane_scene(gpu))
    Xs = []
    for l in (SPOT, POINT2):
        pt.clear_lights()
        pt.add_light(l)
        Xs.append(_hook_samples(pt, w, h, spp, SEED)[0].astype(F64))
    pt.clear_lights()
    pt.add_light(dict(SPOT, sampling_weight=1.0))
    pt.add_light(dict(POINT2, sampling_weight=3.0))
    img = pt.render(w, h, spp, seed=SEED, max_bounces=1)[..., :3].astype(F64)
    p = (0.25, 0.75)
    mean = Xs[0] + Xs[1]
    var = Xs[0] ** 2 / p[0] + Xs[1] ** 2 / p[1] - mean ** 2                                      # per sample; samples are independent
    blocks = lambda a: a.reshape(h // 8, 8, w // 8, 8, 3).mean((1, 3))
    want = blocks(mean.mean(0).reshape(h, w, 3))
    se = np.sqrt(blocks(var.sum(0).reshape(h, w, 3) / spp ** 2) / 64.0)                          # variance of a block mean = sum of its pixels' variances / 64^2
    got = blocks(img)
    z = np.abs(got - want) / np.maximum(se, 1e-30)
    print("several lights: max |z| =", z[se > 0].max(), " blocks with light:", int((se > 0).sum()), " max rel SE:", (se / np.maximum(want, 1e-30))[se > 0].max())
    assert (se > 0).sum() >= 3 * 12 and (z[se > 0] <= 5.0).all()
    assert np.allclose(got[se == 0], want[se == 0], rtol=1e-5, atol=0)                           # where only one outcome is ever non-zero... or none: no variance, equality
    pt.close()


# ---- 4. indirect light ----------------------------------------------------------------------------------------------------------------------------------
BOX_H, LOW_H, LIGHT_Y = 20.0, 0.6, 19.9


def _shaft_scene(pbr, emitter_side=None, intensity=None):
    """A closed box [-1, 1]^2 x [0, 20].  Only what lies low reflects: the white floor and a 0.6 high band of the walls (red, green, white, white) — the Cornell box's
    colours; the walls above the band and the ceiling are black, so that every light path starts with a surface the light sees at an emitter cosine close to 1.
    emitter_side: a downward, one-sided emissive equilateral triangle of that side, centred where the point light is, with Le * area = intensity."""
    S, Q = pbr.scene, pbr.scenes._quad
    mats = [S.Material((0.73, 0.73, 0.73, 1.0), 0.0, 1.0), S.Material((0.65, 0.05, 0.05, 1.0), 0.0, 1.0), S.Material((0.12, 0.45, 0.15, 1.0), 0.0, 1.0),
            S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0)]
    quads = [(Q((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1)), 0), (Q((-1, BOX_H, -1), (1, BOX_H, -1), (1, BOX_H, 1), (-1, BOX_H, 1)), 3)]
    for y0, y1, cols in ((0.0, LOW_H, (0, 1, 2, 0)), (LOW_H, BOX_H, (3, 3, 3, 3))):
        quads.append((Q((-1, y0, -1), (1, y0, -1), (1, y1, -1), (-1, y1, -1)), cols[0]))      # back, normal +z
        quads.append((Q((-1, y0, 1), (-1, y0, -1), (-1, y1, -1), (-1, y1, 1)), cols[1]))      # left, normal +x
        quads.append((Q((1, y0, -1), (1, y0, 1), (1, y1, 1), (1, y1, -1)), cols[2]))          # right, normal -x
        quads.append((Q((1, y0, 1), (-1, y0, 1), (-1, y1, 1), (1, y1, 1)), cols[3]))          # front, normal -z
    meshes = [S.MeshDesc(v, i, m) for (v, i), m in quads]
    if emitter_side is not None:
        s = emitter_side
        r = s / math.sqrt(3.0)
        area = math.sqrt(3.0) / 4.0 * s * s
        mats.append(S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, tuple(float(c) / area for c in intensity)))
        ang = [math.radians(a) for a in (90, 210, 330)]
        pos = [(r * math.cos(a), LIGHT_Y, r * math.sin(a)) for a in ang]                          # counter-clockwise seen from below: the normal is -y
        tv = pbr.scenes._verts(pos, [(0, -1, 0)] * 3, [(1, 0, 0)] * 3, [(0, 0), (1, 0), (0, 1)])
        meshes.append(S.MeshDesc(tv, np.array([0, 1, 2], np.uint32), len(mats) - 1))
    cam = S.CameraDesc((0.0, 2.2, 0.95), (0.0, 0.0, -0.25), math.radians(55.0), 1.0)
    return S.SceneDesc(mats, meshes, [S.InstanceDesc(k) for k in range(len(meshes))], cam, "shaft")


def _render_with_statistics(pt, w, h, spp, seed, bounces):
    """(mean (h, w, 3), variance of the mean (h, w, 3)) from the frame's own samples: ptc_set_sample_covariance(1), all spp samples for every pixel."""
    pt.set_sample_covariance(1)
    pt.frame_begin(w, h, spp, seed=seed, max_bounces=bounces)
    pt.frame_set_adaptive()
    pt.frame_add_samples(spp)
    pt.frame_resolve()
    mu = pt.read_radiance()[..., :3].astype(F64)
    q = pt.read_sample_covariance()[..., :3].astype(F64)               # sums of r^2, g^2, b^2
    pt.set_sample_covariance(0)
    var = np.maximum(q / spp - mu ** 2, 0.0) / (spp - 1)
    return mu, var


def test_indirect_light_matches_a_small_emitter(gpu):
    """max_bounces = 3 through the existing emitter path as the reference.  The emitter: an equilateral triangle of side s = d_min / 100 (d_min: from the light to the
    nearest reflecting surface, the top of the low band) with Le * area = I, facing down.

    The bound of replacing it by a point, for a reflecting point x at v0 = light - x, d = |v0| >= d_min, h = the vertical offset, a = n_x . v0 the offset along its normal:
      the triangle sends I cos_l / d^2 towards x where the point sends I / d^2, cos_l = h / d >= c_min: all reflecting surfaces lie below y = 0.6, within
        sqrt(2) of the axis, so c_min = 19.3 / sqrt(19.3^2 + 2);
      over the triangle (|delta| <= r = s / sqrt 3 from its centroid, in the plane of the light, so h is the same for all of it) the integrand (n_x . v) h / |v|^4
        relative to its value at the centroid is (1 + e1)(1 + u)^-2 with e1 = n_x . delta / a, u = (2 v0 . delta + |delta|^2) / d^2, |e1| <= r / a_min =: es
        (a_min = 1: the band of the walls, at distance 1 from the axis), |u| <= 2 rho + rho^2 =: U, rho = r / d_min.  (1 + u)^-2 = 1 - 2u + R, |R| <= 3 U^2 / (1 - U)^4.
        The means of e1 and of v0 . delta over the triangle are 0 (delta is measured from the centroid), so the mean deviates from 1 by at most
        g = 2 rho^2 + 2 es U + (1 + es) 3 U^2 / (1 - U)^4.
      Nothing but the floor and the band reflects, light transport behind the first reflection is linear and the same in both scenes, and no reflecting point is
      shadowed from the light, so every pixel's expectation obeys  c_min (1 - g) <= L_triangle / L_point <= 1 + g."""
    w = h = 64
    spp = 1024
    I = (400.0, 380.0, 350.0)
    d_min = LIGHT_Y - LOW_H
    s = d_min / 100.0
    r = s / math.sqrt(3.0)
    rho, es = r / d_min, r / 1.0
    U = 2 * rho + rho * rho
    g = 2 * rho * rho + 2 * es * U + (1 + es) * 3 * U * U / (1 - U) ** 4
    c_min = d_min / math.sqrt(d_min ** 2 + 2.0)
    lo, hi = c_min * (1 - g), 1 + g
    assert g < 4e-3 and 1 - lo < 8e-3

    pt = gpu.PathTracer(0).load_scene(_shaft_scene(gpu))
    pt.add_light(type="point", position=(0.0, LIGHT_Y, 0.0), intensity=I)
    mu_p, var_p = _render_with_statistics(pt, w, h, spp, 11, 3)
    direct = pt.render(w, h, 64, seed=11, max_bounces=1)[..., :3].astype(F64)      # bounce 0's sample alone, for the share of indirect light below
    pt.close()
    pe = gpu.PathTracer(0).load_scene(_shaft_scene(gpu, s, I))
    assert pe.stats()["n_emitters"] == 1
    mu_e, var_e = _render_with_statistics(pe, w, h, spp, 12, 3)
    pe.close()

    blocks = lambda a: a.reshape(h // 8, 8, w // 8, 8, 3).mean((1, 3))
    bp, be = blocks(mu_p), blocks(mu_e)
    se = np.sqrt((blocks(var_p) + blocks(var_e)) / 64.0)
    use = blocks((mu_p > 0).all(2, keepdims=True).repeat(3, 2).astype(F64)) == 1.0          # blocks that see reflecting surfaces only
    assert use[..., 0].sum() >= 32
    indirect_share = 1.0 - blocks(direct)[use].sum() / bp[use].sum()
    upper, lower = bp * hi + 5 * se, bp * lo - 5 * se
    slack = np.minimum(upper - be, be - lower)[use] / se[use]
    print("indirect: g =", g, " c_min =", c_min, " share of indirect light:", indirect_share, " max rel SE:", (se / bp)[use].max(),
          " min slack in SE:", slack.min(), " mean ratio:", (be[use] / bp[use]).mean())
    assert (se / bp)[use].max() < 0.02
    assert ((be <= upper) & (be >= lower))[use].all()
    # the same over all those blocks together, where the standard error is that of a few thousand pixels: this is what holds the indirect light.  An indirect term
    # off by half — a bounce left out, a throughput applied twice — moves the total by half its share, which must lie outside what the check allows
    tp, te = bp[use].sum(), be[use].sum()
    se_all = math.sqrt((se[use] ** 2).sum())
    print("indirect, all blocks: ratio =", te / tp, " allowed:", lo - 5 * se_all / tp, "..", hi + 5 * se_all / tp)
    assert tp * lo - 5 * se_all <= te <= tp * hi + 5 * se_all
    assert 0.5 * indirect_share > (hi - lo) + 5 * se_all / tp


# ---- 5. invariance --------------------------------------------------------------------------------------------------------------------------------------
def test_tile_shards_merge_to_the_unsharded_frame(gpu):
    w = h = 48
    pt = gpu.PathTracer(0).load_scene(_plane_scene(gpu))
    pt.add_light(dict(SPOT, sampling_weight=1.0))
    pt.add_light(dict(POINT2, sampling_weight=3.0))
    whole = pt.render(w, h, 8, seed=SEED, max_bounces=3)
    merged = np.zeros_like(whole)
    for rank in range(2):
        pt.frame_begin(w, h, 8, seed=SEED, max_bounces=3, tile_rank=rank, tile_count=2)
        pt.frame_add_samples(8)
        pt.frame_resolve()
        part = pt.read_radiance()
        assert (part[merged[..., 3] > 0] == 0).all()                   # the shares are disjoint
        merged += part
    assert _bits_equal(merged, whole) and (whole[..., :3] > 0).any()
    pt.close()


def test_cleared_lights_leave_no_trace(gpu):
    """BASELINE config 1 (the Cornell box, seed 1, 8 bounces) at a reduced size: a context that had lights and cleared them renders the bits, and launches the kernels, of
    a context that never had any."""
    w = h = 64
    desc = gpu.scenes.cornell_box()
    a = gpu.PathTracer(0).load_scene(desc)
    plain = a.render(w, h, 16, seed=1, max_bounces=8)
    st_a = a.stats()
    b = gpu.PathTracer(0).load_scene(desc)
    b.add_light(type="point", position=(0.0, 0.5, 0.0), intensity=(5.0, 5.0, 5.0))
    b.add_light(type="directional", direction=(0.0, -1.0, -1.0))
    lit = b.render(w, h, 16, seed=1, max_bounces=8)
    st_lit = b.stats()
    assert st_lit["launches_trace_any"] == 2 * st_a["launches_trace_any"] and st_lit["shadow_rays"] > st_a["shadow_rays"]
    assert (lit[..., :3] >= plain[..., :3]).all() and (lit[..., :3] > plain[..., :3]).mean() > 0.5      # the lights' term adds, and changes nothing else
    b.clear_lights()
    again = b.render(w, h, 16, seed=1, max_bounces=8)
    st_b = b.stats()
    assert _bits_equal(again, plain)
    for k in ("launches_trace_any", "launches_trace_closest", "shadow_rays", "segments", "hits"):
        assert st_b[k] == st_a[k], k
    a.close()
    b.close()


def test_a_light_changed_during_a_frame_waits_for_the_next_frame_begin(gpu):
    w = h = 32
    pt = gpu.PathTracer(0).load_scene(_plane_scene(gpu))
    lid = pt.add_light(SPOT)
    first = pt.render(w, h, 8, seed=SEED, max_bounces=2)
    pt.frame_begin(w, h, 8, seed=SEED, max_bounces=2)
    pt.frame_add_samples(4)
    pt.update_light(lid, dict(SPOT, intensity=(1.0, 90.0, 1.0)))       # recorded only
    pt.add_light(POINT2)
    pt.frame_add_samples(4)
    pt.frame_resolve()
    assert _bits_equal(pt.read_radiance(), first)
    changed = pt.render(w, h, 8, seed=SEED, max_bounces=2)
    assert not _bits_equal(changed, first) and pt.light_count() == 2
    pt.close()
