"""Textured emission on a real MI355X (include/ptc_emissive_tex.h, csrc/pt_emissive_tex.hip).

1. k_shade_emissive_tex against its numpy restatement (tests/emissive_tex_reference.py), bit for bit, through ptc_debug_emissive_tex_step: shadow records and lpath.
2. The pipeline against the hooks, bit for bit: a frame's radiance is the sum rebuilt per bounce from the hooks — alone, and beside a punctual light.
3. Equivalence with geometry: a black | white texture on a quad against the white half as a plain emitter, over Lambert and near-mirror floors; the same comparison
   against a plain emitter of 1.1 x the radiance fails; a constant texture against a plain emitter.
   The same beside an alpha-mask material and a light: shadow records through the alpha walk, continuation rays through the alpha resolution.
4. No cost where unused, dynamics (refit and rebuild against a fresh commit, a morphed emitter), the refusal of a medium, tile shards beside an alpha-mask material and a light."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emissive_tex_reference as ref  # noqa: E402
import lens_reference as lref  # noqa: E402
import lights_reference as liref  # noqa: E402
from test_emissive_tex_host import BW, I16, emitter_scene, strip_mesh, tex_5x3, trs_matrix  # noqa: E402

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
def _kernel_scene(pbr, linear):
    """The strip of 9 textured emitters over a near-mirror floor; the LINEAR variant's floor has a colour texture, so its shading records have their textured units."""
    S = pbr.scene
    floor = S.Material((0.9, 0.8, 0.7, 1.0), 0.6, 0.3, (0, 0, 0), 1 if linear else -1)
    d = emitter_scene(pbr, tex=tex_5x3(), factor=(0.5, 2.0, 1.0), emitter=strip_mesh(pbr, 9), linear=linear, floor_material=floor)
    if linear:
        d.textures.append(np.random.default_rng(4).integers(40, 256, (7, 6, 4), dtype=np.uint8))
    return d


def _rays(rng, n, empty_first):
    """Rays by kind, interleaved: 0 up to the emitter's front, 1 down onto its back, 2 down to the floor, 3 away from everything.  513 rays: a whole segment (the
    first 320 slots, or the last 193) of rays that meet no textured emitter — floor hits and misses."""
    kind = np.arange(n) % 4
    if n == 513:
        no_emitter = (np.arange(n) < 320) if empty_first else (np.arange(n) >= 320)
        kind = np.where(no_emitter & (kind < 2), kind + 2, kind)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    on_strip = np.stack([rng.uniform(-1.9, 1.9, n), np.full(n, 2.0), rng.uniform(-0.3, 0.1, n)], 1)
    on_floor = np.stack([rng.uniform(-2.5, 2.5, n), np.zeros(n), rng.uniform(-2.5, 2.5, n)], 1)
    below = np.stack([rng.uniform(-2, 2, n), rng.uniform(0.3, 1.5, n), rng.uniform(-2, 2, n)], 1)
    above = np.stack([rng.uniform(-2, 2, n), rng.uniform(2.5, 4.0, n), rng.uniform(-2, 2, n)], 1)
    for k, (src, dst) in enumerate(((below, on_strip), (above, on_strip), (below, on_floor), (above, above + (0.1, 1.0, 0.2)))):
        m = kind == k
        o[m], d[m] = src[m], (dst - src)[m]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(F32), d.astype(F32), kind


@pytest.mark.parametrize("linear", [False, True])
def test_kernel_equals_reference_bit_for_bit(gpu, linear):
    """Ray counts 1, 63, 64, 65 sit on and around a wave; 513 rays are two segments (PTC_SEG_MIN_LEN = 512: segments of 320 slots, the second holds 193 rays), one of
    which holds no hit on a textured emitter.  Bounces 0, 2 and max_bounces (the hit side alone); throughputs 1, 1e-3 and one zero channel."""
    desc = _kernel_scene(gpu, linear)
    pt = gpu.PathTracer(0).load_scene(desc)
    recs, cdf, pm, total = pt.emissive_tex_table()
    rr, rc, rp, rt = ref.table(desc)
    assert _bits_equal(recs, rr) and _bits_equal(cdf, rc) and np.array_equal(pm, rp) and F32(total) == F32(rt) and total > 0
    shade = pt.shading_tables()[0]
    stride = shade.shape[1] // 4
    assert stride == (12 if linear else 5)
    verts, _, _ = pt.flat_scene()
    eps = liref.scene_ray_eps(verts[:, 0:3])
    rng = np.random.default_rng(9)
    MAXB = 4
    seen = dict(front=0, back=0, shadow=0, no_shadow=0)
    for bounce in (0, 2, MAXB):
        for n in (1, 63, 64, 65, 513):
            empty_first = bounce == 2
            o, d, kind = _rays(rng, n, empty_first)
            if n == 1:
                o, d = np.array([[0.2, 0.5, -0.1]], F32), np.array([[0.0, 1.0, 0.0]], F32)
            keys = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
            T = np.ones((n, 3), F32)
            T[np.arange(n) % 3 == 1] = F32(1e-3)
            T[np.arange(n) % 5 == 2, 1] = 0.0
            pb = rng.uniform(0.05, 40.0, n).astype(F32)
            L0 = rng.uniform(0.0, 2.0, (n, 3)).astype(F32) * (np.arange(n) % 2)[:, None].astype(F32)
            t, prim, uv = pt.trace_closest(o, d)
            L, valid, sh = pt.emissive_tex_step(o, d, T, pb, keys, bounce, MAXB, lpath=L0)
            rL, rv, rsh = ref.step(shade, stride, desc.materials, desc.textures, linear, eps, recs, cdf, pm, total, d, T, pb, keys, t, prim, uv, bounce, MAXB, lpath=L0)
            what = f"linear {linear} bounce {bounce} n {n}"
            assert np.array_equal(valid, rv), what
            assert _bits_equal(L, rL), what
            assert _bits_equal(sh, rsh), (what, np.flatnonzero((sh.view(np.uint32) != rsh.view(np.uint32)).any(1)))
            on_emitter = prim >= 2
            changed = (L.view(np.uint32) != L0.view(np.uint32)).any(1)
            if n > 1:
                assert (changed <= on_emitter).all() and not changed[on_emitter & (kind == 1)].any(), what      # only front-facing hits on the emitter add; hits on its back do not
                seen["front"] += int(changed.sum()); seen["back"] += int((on_emitter & (kind == 1)).sum())
            if bounce == MAXB:
                assert not valid.any(), what
            else:
                seen["shadow"] += int(valid.sum()); seen["no_shadow"] += int(((prim >= 0) & ~valid).sum())
            if n == 513:
                seg_none = slice(0, 320) if empty_first else slice(320, 513)
                assert not on_emitter[seg_none].any() and not changed[seg_none].any() and on_emitter.any(), what
                if bounce < MAXB:
                    assert valid[seg_none].any(), what                                      # its floor hits still sample the set
            assert np.isfinite(sh).all() and np.isfinite(L).all() and (sh[:, 7:10] >= 0).all()
            st = pt.emissive_tex_stats()
            assert st["hit_additions"] == int((on_emitter & (d[:, 1] > 0)).sum()), what      # every emitter faces down: a ray that goes up sees its front
            assert st["shadow_records"] == int(valid.sum()) and st["entries"] == 9
    assert seen["front"] > 100 and seen["back"] > 100 and seen["shadow"] > 200 and seen["no_shadow"] > 50, seen
    pt.close()


# ---- 2. the pipeline ----------------------------------------------------------------------------------------------------------------------------------------
def _hook_frame(pt, w, h, spp, seed, light=False, opaque_twin=None):
    """The image of a max_bounces = 1 frame rebuilt from the hooks, path by path in the pipeline's order: [the punctual sample of bounce 0 where free,] textured
    emission at the bounce-0 hit, the textured sample where free, then, on k_shade's continuation ray, textured emission at the bounce-1 hit.  Each pixel is the
    binary32 sum of its samples in sample order, divided by spp.
    opaque_twin: the scene has alpha materials that no camera ray meets.  Shadow records then go through the frame's alpha walk (ptc_debug_alpha_any: a MASK lets a
    record through whole or not at all), ptc_debug_emissive_tex_step resolves its hits by the alpha pass itself, and k_shade's continuation rays — ptc_debug_shade_step
    refuses a scene with alpha materials — come from the twin context: the same scene with those materials OPAQUE, whose bounce-0 hits, records and ray offset are the same."""
    def free(so, sd, tm):
        if opaque_twin is None:
            return pt.trace_any(so, sd, tm) == 0
        tr = pt.alpha_any(so, sd, tm)
        assert np.isin(tr, (0.0, 1.0)).all()
        return tr == 1.0

    o, d = pt.debug_camera_rays(w, h, seed, 0, spp)
    n = len(o)
    pix = np.tile(np.arange(w * h, dtype=np.uint64), spp)
    smp = np.repeat(np.arange(spp, dtype=np.uint64), w * h)
    keys = lref.path_key(lref.seed_hash(seed), pix, smp).astype(np.uint32)
    one, zero = np.ones((n, 3), F32), np.zeros(n, F32)
    L = np.zeros((n, 3), F32)
    n_shadow = 0
    if light:
        valid, so, sd, tm, ct = pt.punctual_nee(o, d, keys, 0)
        idx = np.flatnonzero(valid)[free(so[valid], sd[valid], tm[valid])]
        L[idx] = L[idx] + ct[idx]
        n_shadow += int(valid.sum())
    L, valid, sh = pt.emissive_tex_step(o, d, one, zero, keys, 0, 1, lpath=L)
    vis = free(sh[valid, 0:3], sh[valid, 3:6], sh[valid, 6])
    idx = np.flatnonzero(valid)[vis]
    L[idx] = L[idx] + sh[idx, 7:10]
    n_shadow += int(valid.sum())
    _hook_frame.blocked = int((~vis).sum())
    c = (opaque_twin or pt).shade_step(o, d, one, zero, keys, 0, 1)
    a = c["alive"]
    assert not c["shadow"].any() and not c["lpath"].any()                              # no plain emitter, no environment: k_shade itself adds nothing
    L1, v1, _ = pt.emissive_tex_step(c["o"][a], c["d"][a], c["T"][a], c["pdf"][a], keys[a], 1, 1, lpath=L[a])
    assert not v1.any()
    hit_side_b1 = (L1.view(np.uint32) != L[a].view(np.uint32)).any(1).sum()
    L[a] = L1
    acc = np.zeros((w * h, 3), F32)
    for s in range(spp):
        acc = acc + L.reshape(spp, w * h, 3)[s]
    return (acc / F32(spp)).reshape(h, w, 3), n_shadow, int(hit_side_b1)


@pytest.mark.parametrize("light", [False, True])
def test_pipeline_equals_hooks_bit_for_bit(gpu, light):
    w, h, spp = 48, 32, 3
    S = gpu.scene
    desc = emitter_scene(gpu, factor=(3.0, 2.0, 1.0), floor_material=S.Material((0.9, 0.8, 0.7, 1.0), 0.5, 0.35))
    pt = gpu.PathTracer(0).load_scene(desc)
    if light:
        pt.add_light(dict(type="spot", position=(-1.5, 1.5, 1.0), direction=(0.6, -1.0, -0.4), intensity=(6.0, 5.0, 4.0), cos_inner=0.9, cos_outer=0.5))
    img = pt.render(w, h, spp, seed=SEED, max_bounces=1)
    st, est = pt.stats(), pt.emissive_tex_stats()
    want, n_shadow, b1 = _hook_frame(pt, w, h, spp, SEED, light)
    assert _bits_equal(img[..., :3], want)
    assert (want > 0).any(2).mean() > 0.5 and b1 > 50                                  # light on most of the image; BSDF samples that found the emitter
    assert st["launches_trace_any"] == (2 if light else 1) and st["shadow_rays"] == n_shadow      # no emitters, no environment: the passes' own any-hit launches
    assert est["entries"] == 2 and est["shadow_records"] > 0 and est["hit_additions"] >= b1 and est["seconds_emissive_tex"] > 0
    assert st["seconds_shade"] >= est["seconds_emissive_tex"]
    pt.close()


def _masked_scene(pbr, opaque=False):
    """emitter_scene with a checkerboard MASK screen at y = 1.5 between the emitter and the floor, seen from a camera below it that looks down: no camera ray meets the
    screen or the emitter, the shadow segments of the floor's samples and the continuation rays that find the emitter all cross it."""
    S, Q = pbr.scene, pbr.scenes._quad
    desc = emitter_scene(pbr, factor=(3.0, 2.0, 1.0), floor_material=S.Material((0.9, 0.8, 0.7, 1.0), 0.5, 0.35))
    check = np.zeros((4, 4, 4), np.uint8)
    check[..., :3] = 200
    check[::2, ::2, 3] = 255
    check[1::2, 1::2, 3] = 255                                                             # alpha 0 | 255 in a checkerboard
    desc.textures.append(check)
    desc.materials.append(S.Material((0.8, 0.6, 0.4, 1.0), 0.0, 1.0, (0, 0, 0), 1, alpha_mode="opaque" if opaque else "mask", alpha_cutoff=0.5))
    sv, si = Q((-1.5, 1.5, 1.0), (1.5, 1.5, 1.0), (1.5, 1.5, -1.0), (-1.5, 1.5, -1.0))
    desc.meshes.append(S.MeshDesc(sv, si, 2))
    desc.instances.append(S.InstanceDesc(2, matrix=I16))
    desc.camera = S.CameraDesc((0.0, 1.2, 2.5), (0.0, 0.0, 0.0), math.radians(45.0), 1.5)
    return desc


def test_pipeline_equals_hooks_beside_alpha_and_a_light(gpu):
    """The pass beside the punctual pass and an alpha-mask material: the frame's shadow records take the alpha walk and its continuation rays the alpha resolution.  The
    48 x 32 image equals the sum rebuilt from the hooks, bit for bit."""
    w, h, spp = 48, 32, 3
    light = dict(type="point", position=(-0.5, 1.8, 0.3), intensity=(4.0, 4.0, 4.0))
    pt = gpu.PathTracer(0).load_scene(_masked_scene(gpu))
    twin = gpu.PathTracer(0).load_scene(_masked_scene(gpu, opaque=True))
    pt.add_light(light)
    o, d = pt.debug_camera_rays(w, h, SEED, 0, spp)
    _, prim, _, layers = pt.alpha_closest(o, d, np.zeros(len(o), np.uint32))
    assert not layers.any() and (prim < 2).all() and (prim >= 0).mean() > 0.8             # camera rays meet the floor or nothing: never the screen, never the emitter
    img = pt.render(w, h, spp, seed=SEED, max_bounces=1)
    st, est, ast = pt.stats(), pt.emissive_tex_stats(), pt.alpha_stats()
    want, n_shadow, b1 = _hook_frame(pt, w, h, spp, SEED, True, opaque_twin=twin)
    assert _bits_equal(img[..., :3], want)
    assert b1 > 20 and _hook_frame.blocked > 100                                           # continuation rays found the emitter through the holes; records ended on the screen
    assert ast["closest_passes"] >= b1 and ast["shadow_walked"] > 0 and st["launches_trace_any"] == 2
    assert est["shadow_records"] > _hook_frame.blocked and est["hit_additions"] >= b1
    assert (want > 0).any(2).mean() > 0.3
    twin.close()
    pt.close()


# ---- 3. equivalence with geometry -----------------------------------------------------------------------------------------------------------------------------
FACTOR = (3.0, 2.0, 1.0)
EQ_W, EQ_H, EQ_SEEDS, EQ_BOUNCES = 48, 32, 16, 3
# samples per pixel of one seed's frame.  Chosen on the CPU from the oracle's render of the plain-emitter side (16 seeds, 48 x 32, max_bounces 3): the standard error
# of the whole-image mean and of each quadrant mean over the seeds, relative to the mean, is at most EQ_SE_MEASURED at this spp — under the 1 % the comparison needs.
# `python tools/emissive_tex_spp.py` prints those figures for 32, 64 and 128 spp (CPU only, a few seconds)
EQ_SPP = {"lambert": 64, "metal": 64}
EQ_SE_MEASURED = {"lambert": 0.0008, "metal": 0.0024}


def _floor(pbr, kind):
    S = pbr.scene
    return S.Material((0.8, 0.8, 0.8, 1.0), 0.0, 1.0) if kind == "lambert" else S.Material((0.9, 0.9, 0.9, 1.0), 1.0, 0.05)


def _look_down(pbr, d):
    """The floor fills the image, and the camera aims at the mirror image of the lit half's centre (0.5, 2, 0): over the near-mirror floor every quadrant holds a
    quarter of the lit half's reflection, so no quadrant mean is a sum of rare bright samples."""
    d.camera = pbr.scene.CameraDesc((0.0, 1.9, 3.0), (0.5, -2.0, 0.0), math.radians(45.0), 1.5)
    return d


def plain_scene(pbr, kind, radiance=FACTOR, lit=(0.0, 1.0)):
    """emitter_scene's geometry with the quad cut at x = lit[0]: the part x in lit is a plain emitter of the given radiance, the rest a black surface."""
    S, Q = pbr.scene, pbr.scenes._quad
    d = emitter_scene(pbr, floor_material=_floor(pbr, kind))
    d.textures = []
    d.materials = [d.materials[0], S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, tuple(radiance)), S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0)]
    x0, x1 = lit
    parts = [(Q((x0, 2, -1), (x1, 2, -1), (x1, 2, 1), (x0, 2, 1)), 1)]
    if x0 > -1.0:
        parts.append((Q((-1, 2, -1), (x0, 2, -1), (x0, 2, 1), (-1, 2, 1)), 2))
    d.meshes = [d.meshes[0]] + [S.MeshDesc(v, i, m) for (v, i), m in parts]
    d.instances = [S.InstanceDesc(k, matrix=I16) for k in range(len(d.meshes))]
    return _look_down(pbr, d)


def _means(img):
    """Whole-image mean and the four quadrant means of the rgb sum."""
    y = img[..., :3].astype(F64).sum(2)
    h, w = y.shape
    return np.array([y.mean(), y[:h // 2, :w // 2].mean(), y[:h // 2, w // 2:].mean(), y[h // 2:, :w // 2].mean(), y[h // 2:, w // 2:].mean()])


def seed_means(render, spp):
    """(mean (5,), s.e. (5,)) of _means over EQ_SEEDS seeds: the s.e. from the spread over the seeds."""
    m = np.array([_means(render(EQ_W, EQ_H, spp, seed=1000 + s, max_bounces=EQ_BOUNCES)) for s in range(EQ_SEEDS)])
    return m.mean(0), m.std(0, ddof=1) / math.sqrt(EQ_SEEDS)


def _agree(a, b):
    (ma, sa), (mb, sb) = a, b
    return np.abs(ma - mb) <= 5.0 * np.sqrt(sa ** 2 + sb ** 2)


@pytest.mark.parametrize("kind", ["lambert", "metal"])
def test_texture_equals_geometry(gpu, kind):
    """u = 0.5 coincides with the cut, so under NEAREST the textured quad emits exactly where the plain half does.  The test has teeth: the same comparison fails
    against a plain emitter of 1.1 x the radiance, and fails for the texture with u flipped (white | black), which moves the light to the other half."""
    spp = EQ_SPP[kind]
    a = gpu.PathTracer(0).load_scene(_look_down(gpu, emitter_scene(gpu, factor=FACTOR, floor_material=_floor(gpu, kind))))
    b = gpu.PathTracer(0).load_scene(plain_scene(gpu, kind))
    c = gpu.PathTracer(0).load_scene(plain_scene(gpu, kind, tuple(1.1 * f for f in FACTOR)))
    A, B, Cc = seed_means(a.render, spp), seed_means(b.render, spp), seed_means(c.render, spp)
    print(kind, "textured", A[0], "rel se", A[1] / A[0], "\n plain", B[0], "rel se", B[1] / B[0], "\n z", np.abs(A[0] - B[0]) / np.sqrt(A[1] ** 2 + B[1] ** 2))
    assert (A[1] < 0.01 * A[0]).all() and (B[1] < 0.01 * B[0]).all()
    assert (B[1] <= 1.5 * EQ_SE_MEASURED[kind] * B[0]).all()                           # the plain side reproduces what the oracle measured (tools/emissive_tex_spp.py)
    assert _agree(A, B).all()
    assert not _agree(A, Cc).all()
    f = gpu.PathTracer(0).load_scene(_look_down(gpu, emitter_scene(gpu, tex=BW[:, ::-1], factor=FACTOR, floor_material=_floor(gpu, kind))))
    Fl = seed_means(f.render, spp)
    print(" 1.1 x: z", np.abs(A[0] - Cc[0]) / np.sqrt(A[1] ** 2 + Cc[1] ** 2), "\n flipped: z", np.abs(Fl[0] - B[0]) / np.sqrt(Fl[1] ** 2 + B[1] ** 2))
    assert not _agree(Fl, B).all()
    for p in (a, b, c, f):
        p.close()


def test_constant_texture_equals_a_plain_emitter(gpu):
    f = (1.5, 2.5, 0.5)
    white = np.full((3, 2, 4), 255, np.uint8)
    a = gpu.PathTracer(0).load_scene(_look_down(gpu, emitter_scene(gpu, tex=white, factor=f, floor_material=_floor(gpu, "lambert"))))
    b = gpu.PathTracer(0).load_scene(plain_scene(gpu, "lambert", f, lit=(-1.0, 1.0)))
    A, B = seed_means(a.render, EQ_SPP["lambert"]), seed_means(b.render, EQ_SPP["lambert"])
    print("constant: textured", A[0], "plain", B[0], "z", np.abs(A[0] - B[0]) / np.sqrt(A[1] ** 2 + B[1] ** 2))
    assert (A[1] < 0.01 * A[0]).all() and (B[1] < 0.01 * B[0]).all()
    assert _agree(A, B).all()
    a.close()
    b.close()


# ---- 4. invariance ------------------------------------------------------------------------------------------------------------------------------------------------
def test_no_cost_where_unused(gpu):
    """A scene with no emission texture, and the same scene after set-then-remove: image bits, launch counts and shadow rays of a context that never called the feature."""
    from test_emissive_tex_host import _describe
    w = h = 64
    desc = plain_scene(gpu, "metal")
    desc.textures = [BW]                                                                   # a texture nobody uses
    a = gpu.PathTracer(0).load_scene(desc)
    plain = a.render(w, h, 16, seed=1, max_bounces=6)
    st_a = a.stats()
    b = gpu.PathTracer(0)
    _describe(gpu, b, desc)
    b.set_material_emission_texture(2, 0, (1.0, 1.0, 1.0)).set_material_emission_texture(2, -1)
    assert b._L.ptc_scene_commit(b._h) == 0
    img = b.render(w, h, 16, seed=1, max_bounces=6)
    st = b.stats()
    assert _bits_equal(img, plain) and (plain[..., :3] > 0).any()
    for k in ("launches_trace_any", "launches_trace_closest", "shadow_rays", "segments", "hits"):
        assert st[k] == st_a[k], k
    for p in (a, b):
        assert p.emissive_tex_stats() == dict(entries=0, hit_additions=0, shadow_records=0, seconds_emissive_tex=0.0)
        p.close()


@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_refit_and_rebuild_equal_a_fresh_commit(gpu, builder):
    """The emitter instance scaled (2, 1, 0.5) and turned: after ptc_scene_refit and after ptc_scene_rebuild the table and the image are a fresh commit's, bit for bit."""
    w, h = 48, 32
    M2 = trs_matrix((0.2, 0.3, -0.1), 0.6, (2.0, 1.0, 0.5))
    kw = dict(tex=tex_5x3(), factor=(0.5, 2.0, 1.0), emitter=strip_mesh(gpu, 9), builder=builder)
    fresh = gpu.PathTracer(0).load_scene(emitter_scene(gpu, matrix=M2, **kw))
    want = fresh.render(w, h, 8, seed=SEED, max_bounces=3)
    want_table = fresh.emissive_tex_table()
    pt = gpu.PathTracer(0).load_scene(emitter_scene(gpu, **kw))
    first = pt.render(w, h, 8, seed=SEED, max_bounces=3)
    assert not _bits_equal(first, want)
    pt.update_instance(1, matrix=M2)
    for how in ("refit", "rebuild"):
        pt.scene_refit() if how == "refit" else pt.scene_rebuild()
        got = pt.emissive_tex_table()
        assert _bits_equal(got[0], want_table[0]) and _bits_equal(got[1], want_table[1]) and np.array_equal(got[2], want_table[2]) and got[3] == want_table[3], how
        assert _bits_equal(pt.render(w, h, 8, seed=SEED, max_bounces=3), want), how
    assert (want[..., :3] > 0).any(2).mean() > 0.5
    fresh.close()
    pt.close()


def test_a_morphed_emitter_follows_a_refit(gpu):
    """The emitter mesh has a morph target.  Weight 0 at the commit, 0.7 by ptc_update_mesh_pose + ptc_scene_refit (on the device: the host evaluates only the table's
    vertices): table and image are those of a commit in the posed state."""
    w, h = 48, 32
    def scene(weight):
        d = emitter_scene(gpu, tex=tex_5x3(), factor=(0.5, 2.0, 1.0), emitter=strip_mesh(gpu, 9))
        m = d.meshes[1]
        rng = np.random.default_rng(17)
        m.morph_dpos = rng.uniform(-0.3, 0.3, (1, m.vertices.size, 3)).astype(F32)
        m.morph_weights = np.array([weight], F32)
        return d
    fresh = gpu.PathTracer(0).load_scene(scene(0.7))
    want, want_table = fresh.render(w, h, 8, seed=SEED, max_bounces=3), fresh.emissive_tex_table()
    pt = gpu.PathTracer(0).load_scene(scene(0.0))
    rest = pt.emissive_tex_table()
    pt.update_mesh_pose(1, np.array([0.7], F32), None).scene_refit()
    got = pt.emissive_tex_table()
    assert not _bits_equal(got[0], rest[0])
    assert _bits_equal(got[0], want_table[0]) and _bits_equal(got[1], want_table[1]) and np.array_equal(got[2], want_table[2]) and got[3] == want_table[3]
    assert _bits_equal(pt.render(w, h, 8, seed=SEED, max_bounces=3), want)
    fresh.close()
    pt.close()


def test_a_medium_is_refused(gpu):
    desc = emitter_scene(gpu)
    pt = gpu.PathTracer(0).load_scene(desc)
    pt.set_medium(box_lo=(-3, 0, -3), box_hi=(3, 3, 3), sigma_t=0.3, albedo=(0.9, 0.9, 0.9), g=0.0)
    L, h = pt._L, pt._h
    assert L.ptc_frame_begin(h, 16, 16, 1, 1, 2, gpu.ptc.INTEGRATOR_PATH, 0, 1) == -2      # PTC_E_STATE
    err = L.ptc_last_error(h)
    assert b"medium" in err and b"emission texture" in err
    pt.clear_medium()
    assert np.isfinite(pt.render(16, 16, 1, seed=1, max_bounces=2)).all()
    pt.close()


def test_tile_shards_beside_alpha_and_a_light(gpu):
    """The pass beside the punctual pass and an alpha-mask material elsewhere in the scene (its shadow records take the alpha walk): tile shards merge to the whole frame."""
    S, Q = gpu.scene, gpu.scenes._quad
    w = h = 48
    desc = emitter_scene(gpu, factor=(3.0, 2.0, 1.0))
    check = np.zeros((4, 4, 4), np.uint8)
    check[..., :3] = 200
    check[::2, ::2, 3] = 255
    check[1::2, 1::2, 3] = 255                                                             # alpha 0 | 255 in a checkerboard
    desc.textures.append(check)
    desc.materials.append(S.Material((0.8, 0.6, 0.4, 1.0), 0.0, 1.0, (0, 0, 0), 1, alpha_mode="mask", alpha_cutoff=0.5))
    sv, si = Q((-1.5, 1.0, 1.0), (1.5, 1.0, 1.0), (1.5, 1.0, -1.0), (-1.5, 1.0, -1.0))        # a screen between the emitter and the floor
    desc.meshes.append(S.MeshDesc(sv, si, 2))
    desc.instances.append(S.InstanceDesc(2, matrix=I16))
    pt = gpu.PathTracer(0).load_scene(desc)
    pt.add_light(dict(type="point", position=(-1.5, 1.5, 1.0), intensity=(4.0, 4.0, 4.0)))
    whole = pt.render(w, h, 8, seed=SEED, max_bounces=3)
    est = pt.emissive_tex_stats()
    assert est["shadow_records"] > 0 and est["hit_additions"] > 0 and np.isfinite(whole).all()
    merged = np.zeros_like(whole)
    for rank in range(2):
        pt.frame_begin(w, h, 8, seed=SEED, max_bounces=3, tile_rank=rank, tile_count=2)
        pt.frame_add_samples(8)
        pt.frame_resolve()
        part = pt.read_radiance()
        assert (part[merged[..., 3] > 0] == 0).all()
        merged += part
    assert _bits_equal(merged, whole) and (whole[..., :3] > 0).any()
    # without the emission texture the floor under the screen is darker: the pass's light does pass the mask's holes
    desc.materials[1].emissive_texture = -1
    dark = gpu.PathTracer(0).load_scene(desc)
    dark.add_light(dict(type="point", position=(-1.5, 1.5, 1.0), intensity=(4.0, 4.0, 4.0)))
    d_img = dark.render(w, h, 8, seed=SEED, max_bounces=3)
    assert whole[..., :3].sum() > 1.2 * d_img[..., :3].sum()
    dark.close()
    pt.close()
