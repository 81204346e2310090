"""A frame's bits do not depend on how it was scheduled — for every optional pass of the path integrator, on a real MI355X.

run_batch (csrc/ptc_api.cpp) threads up to six passes through the core loop: alpha coverage, dielectric transmission, transparent shadows, the medium, punctual
lights and textured emission; beside them the thin-lens, probe and lightmap ray generators.  Each is a consumer of the segmented wavefront queues and right only if
it agrees with the core on the segment layout, the lane, the path numbering and the batch.  The per-pass modules hold the kernels to their restatements under the
default policy; this module holds every pass to ONE exact property under every launch policy (tests/pass_policies.py: ENV_POLICIES and the three policies without a
variable below): the image's bits, the nine counters and every per-record counter of the passes are those of a context created under the default environment.

1. test_policies_give_the_default_frame, per scene: the policy table, looped inside.  It prints the layouts it ran and the activity counters, and asserts that
   every feature of the scene ran.
2. test_probe_and_lightmap_frames_*: the same for frames without a camera, in the two composite scenes.
3. test_invisible_surfaces_in_probe_and_lightmap_frames: the one check here that pins WHAT such a frame computes: surfaces that let everything through change no bit.
4. test_lens_frame_is_the_reference_rays_through_the_hooks: the lens beside the passes, at max_bounces 0, rebuilt from the hooks."""
import dataclasses
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lens_reference as lref  # noqa: E402
import pass_policies as pp  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED, BOUNCES = pp.SEED, pp.BOUNCES
LENS = dict(aperture_radius=0.08, focus_distance=8.0, blades=6, aperture_rotation=0.1)
SURFACE_LIGHTS = [dict(type="point", position=(-1.0, 2.0, 1.0), intensity=(4.0, 4.0, 4.0)),
                  dict(type="spot", position=(1.5, 2.5, -1.0), direction=(-0.3, -1.0, 0.2), intensity=(6.0, 5.0, 4.0), cos_inner=0.9, cos_outer=0.5, sampling_weight=2.0)]
SUN = dict(type="directional", direction=(0.05, -1.0, 0.02), intensity=(3.0, 2.8, 2.5))
VOLUME_LIGHTS = [SUN, dict(type="point", position=(-0.8, 1.0, 0.5), intensity=(2.0, 2.0, 3.0))]
TEXTURED_LIGHTS = [dict(type="point", position=(0.0, 0.9, 0.3), intensity=(3.0, 3.0, 3.0)),
                   dict(type="spot", position=(-1.0, 1.2, 0.0), direction=(0.3, -1.0, 0.1), intensity=(5.0, 4.0, 3.0), cos_inner=0.9, cos_outer=0.6, sampling_weight=2.0)]


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


# ---- the scenes: name -> (description with its lights and lens, setup(pt), the counters that must be positive in the base frame, any-hit launches per bounce) ---
def _with(gpu, desc, lights=(), lens=None):
    desc.lights = [gpu.scene.LightDesc(**l) for l in lights]
    if lens:
        desc.camera = dataclasses.replace(desc.camera, **lens)
    return desc


def _shadows_on(pt):
    pt.set_glass_shadows(True)


def _surface(gpu, top="normal", lens=LENS):
    return _with(gpu, gpu.scenes.passes_surface(top=top), SURFACE_LIGHTS, lens)


def _volume(gpu):
    return _with(gpu, gpu.scenes.passes_volume(), VOLUME_LIGHTS, dict(LENS, focus_distance=5.0))


def _emission_beside_a_mask(gpu):
    from test_gpu_emissive_tex import _masked_scene
    return _masked_scene(gpu)


ALPHA = ["alpha.closest_passes", "alpha.shadow_walked", "alpha.shadow_passes"]
GLASS = ["glass.reflections", "glass.refractions", "glass.standing"]
GLASS_SHADOWS = ["glass_shadow.walked", "glass_shadow.passes", "glass_shadow.visible"]
MEDIUM = ["medium.crossed", "medium.scattered", "medium.attenuated"]
EMTEX = ["emissive_tex.hit_additions", "emissive_tex.shadow_records"]
SCENES = {
    "alpha_layers": (lambda g: g.scenes.alpha_layers(), None, ALPHA, 1),
    "glass_slab": (lambda g: g.scenes.glass_slab(thin=False, emitter=True), None, GLASS, 1),
    "glass_panes_shadows": (lambda g: g.scenes.glass_panes(emitter=True), _shadows_on, GLASS + GLASS_SHADOWS, 1),
    "fog_box_sun": (lambda g: _with(g, g.scenes.fog_box(), [SUN]), None, MEDIUM, 2),
    "shade_textured_lights": (lambda g: _with(g, g.scenes.shade_textured(), TEXTURED_LIGHTS), None, [], 2),
    "emission_beside_a_mask": (_emission_beside_a_mask, None, EMTEX + ALPHA[:2], 1),
    # in a frame with transparent shadows the alpha surfaces of a shadow record are passed by the glass walk: alpha's own shadow counters stay 0 (include/ptc_glass_shadows.h)
    "passes_surface": (_surface, _shadows_on, ALPHA[:1] + GLASS + GLASS_SHADOWS + EMTEX, 3),
    "passes_volume": (_volume, None, MEDIUM, 2),
}


def _frame(pt, w, h, spp, max_bounces=BOUNCES):
    return pp.frame_record(pt, pt.render(w, h, spp, seed=SEED, max_bounces=max_bounces))


def _capped_shape(gpu, desc):
    """(w, h, spp) of the capped frame, its height derived from the segment count a context has under PTC_SEGMENTS_PER_CU=1."""
    with pp.tracer(gpu, desc, **pp.CAPPED_ENV) as pt:
        segs = int(pp.policy_field(pt, "shade_segments"))
    return pp.CAPPED_W, pp.capped_height(segs), pp.CAPPED_SPP


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", list(SCENES))
def test_policies_give_the_default_frame(gpu, scene):
    build, setup, features, any_per_bounce = SCENES[scene]
    desc = build(gpu)
    shapes = {"ragged": pp.RAGGED, "capped": _capped_shape(gpu, desc)}
    assert desc.n_triangles < 100 and all(w * h * s < 160000 for w, h, s in shapes.values())
    t_start = time.time()
    base, ran = {}, []
    # the base: a context under the default environment per frame shape; the second goes on to the policy "queues that have grown" below
    with pp.tracer(gpu, desc, setup) as a:
        base["ragged"] = _frame(a, *pp.RAGGED)
        st = a.stats()
        assert st["launches_trace_closest"] == BOUNCES + 1 and st["launches_trace_any"] == any_per_bounce * BOUNCES, st      # one batch; every next-event pass of the scene ran
        assert pp.layout_of(a, 851, 5) == (1, 9, 512)
        acts = pp.activity(base["ragged"])
        print(f"\n{scene}: {desc.n_triangles} triangles; base frame {pp.RAGGED} layout (1, 9, 512); activity {acts}")
        assert acts["shadow_rays"] > 0 and all(acts.get(k, 0) > 0 for k in features), (features, acts)
        img = base["ragged"]["image"]
        assert np.isfinite(img).all() and (img[..., :3] > 0).any(-1).mean() > 0.2
    with pp.tracer(gpu, desc, setup) as b:
        w, h, spp = shapes["capped"]
        base["capped"] = _frame(b, w, h, spp)
        n_capped = w * h * spp
        cap = b.internals()["queue_cap"]
        ran.append(("default, capped-size frame", pp.layout_of(b, w * h, spp)))
        assert cap == n_capped and ran[-1][1][0] == 1 and ran[-1][1][2] == 512
        assert all(pp.activity(base["capped"]).get(k, 0) > 0 for k in features)
        # ---- no variable: one context, the capped-size frame, the ragged one, the capped-size one again: the lane's queues grew once and stayed
        pp.assert_same_frame(_frame(b, *pp.RAGGED), base["ragged"], f"{scene}, the ragged frame in queues grown for {n_capped} paths")
        assert b.internals()["queue_cap"] == cap
        pp.assert_same_frame(_frame(b, w, h, spp), base["capped"], f"{scene}, the capped-size frame again")
        assert b.internals()["queue_cap"] == cap
        ran.append(("grown queues: capped-size, ragged, capped-size", pp.layout_of(b, w * h, spp)))
    # ---- the policies that are a set of variables
    for name, env, shape, check in pp.ENV_POLICIES:
        w, h, spp = shapes[shape]
        with pp.tracer(gpu, desc, setup, **env) as pt:
            got = _frame(pt, w, h, spp)
            layout = pp.layout_of(pt, w * h, spp)
            ran.append((name, layout))
            check(pt, layout)
            pp.assert_same_frame(got, base[shape], f"{scene} under {name} {env}, layout {layout}")
    # ---- no variable: the frame as frame_add_samples(1, 3, 1)
    w, h, spp = pp.RAGGED
    with pp.tracer(gpu, desc, setup) as pt:
        pt.frame_begin(w, h, spp, seed=SEED, max_bounces=BOUNCES)
        for k in (1, 3, 1):
            pt.frame_add_samples(k)
        pt.frame_resolve()
        pp.assert_same_frame(pp.frame_record(pt, pt.read_radiance()), base["ragged"], f"{scene} as frame_add_samples(1, 3, 1)")
        ran.append(("add_samples(1, 3, 1)", pp.layout_of(pt, w * h, spp)))
    # ---- no variable: two halves.  Samples 0-1 as a frame of their own, checkpointed; samples 2-4 in another context, as a sample range on top of the restored sums
    with pp.tracer(gpu, desc, setup) as first, pp.tracer(gpu, desc, setup) as second:
        first.frame_begin(w, h, 2, seed=SEED, max_bounces=BOUNCES)
        first.frame_set_sample_range(0, 0)
        first.frame_add_samples(2)
        acc, done = first.frame_checkpoint()
        assert done == 2 and acc.shape == (w * h, 4)
        half1 = pp.frame_record(first, acc)
        second.frame_begin(w, h, 3, seed=SEED, max_bounces=BOUNCES)
        second.frame_set_sample_range(2, spp)
        second.frame_restore(acc, 0)
        second.frame_add_samples(3)
        second.frame_resolve()
        half2 = pp.frame_record(second, second.read_radiance())
        whole = {"image": half2["image"]}
        for k in half2:
            if k != "image":
                whole[k] = {f: half1[k][f] + half2[k][f] for f in half2[k]}
        for k in ("alpha_stats", "glass_stats", "glass_shadow_stats", "medium_stats", "emissive_tex_stats"):
            if "entries" in whole[k]:
                whole[k]["entries"] = half2[k]["entries"]      # the table's size, not a count of the frame
        pp.assert_same_frame(whole, base["ragged"], f"{scene} as samples [0, 2) + [2, 5) through a checkpoint")
        ran.append(("two halves", pp.layout_of(second, w * h, 3)))
    print(f"{scene}: layouts (batches, n_seg, seg_len): " + "; ".join(f"{n} {l}" for n, l in ran) + f"; {time.time() - t_start:.1f} s")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------------------
SURFACE_PROBES = np.array([(-2.5, 0.4, 2.0), (0.0, 0.3, 0.0), (2.6, 0.5, -2.2), (0.3, 0.8, -0.4), (-0.5, 1.6, 0.6), (1.8, 1.2, 1.9), (-2.4, 1.7, 0.1), (2.5, 2.0, 0.2)], F32)
VOLUME_PROBES = np.array([(-1.5, 0.3, 1.0), (0.0, 0.2, 0.0), (0.1, 1.3, -1.0), (1.2, 0.9, 0.1), (-0.6, 0.7, -1.5), (1.7, 0.4, 1.6), (0.0, 1.0, 0.4), (-1.8, 1.2, -0.2)], F32)
ENTRY_POLICIES = [("lanes2", dict(PTC_LANES="2", PTC_BATCH_PATHS="1024")), ("sort", dict(PTC_SHADE_SORT="1")), ("capped", dict(pp.CAPPED_ENV))]


def _entry_frames(gpu, desc, setup, n_entries, small_spp, bake, what):
    """bake(pt, spp) -> the arrays of a probe or lightmap frame of n_entries entries.  The default policy against ENTRY_POLICIES; the capped one at a sample count
    chosen by the layout, the others at small_spp."""
    segs = None
    with pp.tracer(gpu, desc, setup, **pp.CAPPED_ENV) as pt:
        segs = int(pp.policy_field(pt, "shade_segments"))
    capped_spp = -(-pp.capped_paths(segs) // n_entries)
    assert n_entries * capped_spp < 160000
    base = {}
    with pp.tracer(gpu, desc, setup) as pt:
        for spp in (small_spp, capped_spp):
            base[spp] = pp.frame_record(pt, bake(pt, spp))
            assert np.isfinite(base[spp]["image"]).all() and (base[spp]["image"] != 0).any()
        print(f"\n{what}: {n_entries} entries; activity at {small_spp} spp {pp.activity(base[small_spp])}")
    for name, env in ENTRY_POLICIES:
        spp = capped_spp if name == "capped" else small_spp
        with pp.tracer(gpu, desc, setup, **env) as pt:
            got = pp.frame_record(pt, bake(pt, spp))
            layout = pp.layout_of(pt, n_entries, spp)
            if name == "capped":
                pp._capped(pt, layout)
            if name == "lanes2":
                assert pp.policy_field(pt, "lanes") == "2" and layout[0] >= 4, layout
            print(f"{what} under {name}: {spp} spp, layout (batches, n_seg, seg_len) {layout}")
            pp.assert_same_frame(got, base[spp], f"{what} under {name} {env}, layout {layout}")
    return base[small_spp]


def _bake_probes(positions):
    def bake(pt, spp):
        return pt.render_probes(positions, spp, seed=SEED, max_bounces=BOUNCES).reshape(1, -1, 3)
    return bake


def _bake_lightmap(pt, spp):
    """The atlas (its alpha is the validity: 1 baked, 0 empty or invalid) and, appended as rows, the back-face fraction per entry."""
    atlas = pt.render_lightmap(0, 24, 20, spp, seed=SEED, max_bounces=BOUNCES, dilate=0)
    _, frac = pt.read_lightmap(dilate=0, with_backface=True)
    assert frac.size == 480
    return np.concatenate([atlas.reshape(1, -1, 4), np.repeat(frac[None, :, None], 4, 2)], 1)


def test_probe_and_lightmap_frames_in_passes_surface(gpu):
    desc = _surface(gpu, lens=None)
    rec = _entry_frames(gpu, desc, _shadows_on, 8, 300, _bake_probes(SURFACE_PROBES), "passes_surface probes")
    acts = pp.activity(rec)
    assert all(acts.get(k, 0) > 0 for k in ALPHA[:1] + GLASS + GLASS_SHADOWS + EMTEX), acts
    rec = _entry_frames(gpu, desc, _shadows_on, 480, 9, _bake_lightmap, "passes_surface lightmap of the floor")
    acts = pp.activity(rec)
    assert all(acts.get(k, 0) > 0 for k in ALPHA[:1] + GLASS + GLASS_SHADOWS + EMTEX), acts
    valid = rec["image"][0, :480, 3] == 1                                                # both kinds occur, so the validity compared above is no constant: texels under the
    assert 0.0 < valid.mean() < 1.0                                                       # patches and many under the BLEND and MASK sheets see back faces (9 samples, threshold 0.1)


def test_probe_frames_in_passes_volume(gpu):
    rec = _entry_frames(gpu, _volume(gpu), None, 8, 300, _bake_probes(VOLUME_PROBES), "passes_volume probes")
    acts = pp.activity(rec)
    assert all(acts.get(k, 0) > 0 for k in MEDIUM), acts


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_invisible_surfaces_in_probe_and_lightmap_frames(gpu):
    """passes_surface with its MASK sheet's alpha all zero and its panes the invisible pane of test_gpu_glass.py::test_an_invisible_pane_changes_nothing (thin, ior 1,
    white, transmission 1), against the scene without the three.  That test compares means: a ray that passes a surface goes on from a point one ray epsilon off it,
    so what it meets next is met with other barycentrics.  Here bit equality holds by construction (scenes.passes_surface): the three lie above everything else, so
    a ray of a frame without a camera that passes them meets nothing afterwards — its radiance is the environment's along a direction and a throughput that the
    passes leave bit for bit, and, with transparent shadows on, its pdf word stays as well; a shadow record that passes them is added with transmittance (1, 1, 1),
    the products skipped; the primitives were added last and the floor sets the ray epsilon, so everything else is the same scene."""
    out = {}
    for top in ("invisible", "none"):
        with pp.tracer(gpu, _surface(gpu, top=top, lens=None), _shadows_on) as pt:
            sh = pt.render_probes(SURFACE_PROBES, 64, seed=SEED, max_bounces=BOUNCES)
            p_stats = (pt.alpha_stats(), pt.glass_stats(), pt.glass_shadow_stats())
            lm = _bake_lightmap(pt, 4)
            l_stats = (pt.alpha_stats(), pt.glass_stats(), pt.glass_shadow_stats())
            out[top] = (sh, lm, p_stats, l_stats)
    for k, what in ((2, "probes"), (3, "lightmap")):
        (a_i, g_i, s_i), (a_n, g_n, s_n) = out["invisible"][k], out["none"][k]
        print(f"\n{what}: invisible: alpha {a_i}\n glass {g_i}\n shadow walk {s_i}\n without: alpha {a_n}\n glass {g_n}\n shadow walk {s_n}")
        # the walks happened: rays passed the zero-alpha sheet and the panes, shadow records were walked through them
        assert a_i["closest_passes"] > a_n["closest_passes"] and g_i["refractions"] > g_n["refractions"] and s_i["walked"] > 0 and s_i["passes"] > 0
        assert a_i["exhausted"] == a_n["exhausted"] and g_i["exhausted"] == g_n["exhausted"] and g_i["reflections"] == g_n["reflections"] and s_i["exhausted"] == 0
        assert s_n["walked"] == 0 and a_n["shadow_walked"] > 0                          # without a thin pane the shadow records take alpha's own walk
    sh_i, sh_n = out["invisible"][0], out["none"][0]
    differ = (sh_i.view(np.uint32) != sh_n.view(np.uint32)).any((1, 2))
    assert not differ.any(), f"SH coefficients of probes {np.flatnonzero(differ).tolist()} differ"
    lm_i, lm_n = out["invisible"][1], out["none"][1]
    differ = (lm_i.view(np.uint32) != lm_n.view(np.uint32)).any(-1)[0]
    assert not differ.any(), f"{int(differ[:480].sum())} texels and {int(differ[480:].sum())} back-face fractions differ"
    assert (sh_i != 0).any() and 0.0 < (lm_i[0, :480, 3] == 1).mean() < 1.0          # valid and invalid texels both occur


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_lens_frame_is_the_reference_rays_through_the_hooks(gpu):
    """passes_surface through a bladed lens at max_bounces 0: the image of the reference's lens rays (tests/lens_reference.py) pushed through the hooks for bounce 0,
    as test_gpu_lens.py::test_rendered_image_is_the_reference_rays_image builds it.  A path of such a frame is: the camera ray, the alpha and glass resolutions of
    bounce 0 (ptc_debug_glass_closest runs both, with the frame's settings), then k_shade — T x the environment along the final direction for a ray that left the
    scene (ptc_debug_medium_env serves the lookup), nothing for a surface: the camera sees the two emitters from behind, and emission is one-sided.  Each pixel is the
    binary32 sum of its samples in sample order, divided by spp.  The lens under every policy at max_bounces 4 is test_policies_give_the_default_frame[passes_surface]."""
    w, h, spp = pp.RAGGED
    desc = _surface(gpu)
    cam = desc.camera
    lens = (cam.aperture_radius, cam.focus_distance, cam.blades, cam.aperture_rotation)
    with pp.tracer(gpu, desc, _shadows_on) as pt:
        img = pt.render(w, h, spp, seed=SEED, max_bounces=0)
        pinhole = dataclasses.replace(cam, aperture_radius=0.0)
        o, d, _ = lref.camera_rays(lref.camera_basis(cam), lens, w, h, SEED, 0, spp, np.arange(w * h))
        do, dd = pt.debug_camera_rays(w, h, SEED, 0, spp)
        assert pp.bits_equal(o, do) and pp.bits_equal(d, dd)
        assert not pp.bits_equal(o, lref.camera_rays(lref.camera_basis(pinhole), (0.0, 1.0, 0, 0.0), w, h, SEED, 0, spp, np.arange(w * h))[0])      # the lens is on
        pix = np.tile(np.arange(w * h, dtype=np.uint64), spp)
        smp = np.repeat(np.arange(spp, dtype=np.uint64), w * h)
        keys = lref.path_key(lref.seed_hash(SEED), pix, smp).astype(np.uint32)
        t, prim, uv, o2, d2, T, pdf, j = pt.glass_closest(o, d, keys, 0)
        miss = prim < 0
        on_emitter = np.isin(prim, (2, 3, 8, 9))
        assert (d2[on_emitter, 1] < 0).all() and on_emitter.sum() > 20                   # both face down, the rays come from above
        assert miss.sum() > 50 and (j[miss] > 0).sum() > 20 and (j[~miss] > 0).sum() > 500      # rays the panes or the slab sent back to the sky; rays that went through
        L = np.zeros((w * h * spp, 3), F32)
        zeros = np.zeros(int(miss.sum()), F32)
        _, Le, _ = pt.medium_env(zeros, zeros, d2[miss])
        L[miss] = T[miss] * Le
        acc = np.zeros((w * h, 3), F32)
        for s in range(spp):
            acc = acc + L.reshape(spp, w * h, 3)[s]
        want = np.ones((h, w, 4), F32)
        want[..., :3] = (acc / F32(spp)).reshape(h, w, 3)
        differ = (img.view(np.uint32) != want.view(np.uint32)).any(-1)
        print(f"\nlens beside the passes: {int(miss.sum())} of {miss.size} paths end in the sky, {int((j > 0).sum())} had a glass event; {int(differ.sum())} of {w * h} pixels differ")
        assert not differ.any()
        assert (want[..., :3] > 0).any(-1).mean() > 0.05
