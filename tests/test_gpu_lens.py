"""The thin-lens camera on a real MI355X (include/ptc.h: ptc_set_camera_lens, ptc_focus_distance_at_pixel, ptc_debug_camera_rays; csrc/pt_lens.hip).

Everything here is equality of bits.  The rays k_raygen (R = 0) and k_raygen_lens (R > 0) write are the numpy restatement's (tests/lens_reference.py); the
rendered image of a scene of emitters at max_bounces = 0 is rebuilt from those rays and ptc_debug_trace_closest; tile shares, checkpoint / restore and
adaptive frames give the frames they give without a lens; guides, denoiser and the raster integrators do not see the lens.

The shapes are small on purpose: 33 x 17 x 5 samples = 2,805 paths is no multiple of 256, crosses block and wave boundaries, and 33 is no multiple of the
32-pixel tile."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lens_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, FIRST, NS, SEED = 33, 17, 3, 5, 0x1234567890ABCDEF
FOCUS = 3.5
LENSES = {"pinhole": (0.0, FOCUS, 0, 0.0), "disk": (0.15, FOCUS, 0, 0.0), "hexagon": (0.15, FOCUS, 6, 0.3)}
EMISSION = ((3.1, 0.2, 0.7), (0.3, 2.7, 0.4), (0.5, 0.6, 4.3))
E_ARG, E_STATE = -1, -2


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _scene(pbr, aspect=W / H):
    """Three emissive quads of distinct colours facing the camera — in front of (view depth 2), at (3.5) and behind (6) the plane of focus — and nothing
    else.  They overlap in the image, so that a blurred edge lies over a sharp one and over the background.  The camera is not axis-aligned."""
    S = pbr.scene
    cam = S.CameraDesc((3.1, -1.7, 2.3), (0.4, 0.2, -0.9), 0.9, aspect)
    pos, f, s, u, _, _ = (np.asarray(v, np.float64) for v in ref.camera_basis(cam))
    mats = [S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, e) for e in EMISSION]
    meshes = []
    for m, (z, cx, cy, half) in enumerate(((2.0, -0.45, 0.1, 0.4), (FOCUS, 0.2, -0.15, 0.9), (6.0, 1.6, 0.5, 2.2))):
        c = pos + z * f + cx * s + cy * u
        corners = [c - half * s - half * u, c + half * s - half * u, c + half * s + half * u, c - half * s + half * u]      # s x u = -f: the front faces the camera
        v, i = pbr.scenes._quad(*corners)
        meshes.append(S.MeshDesc(v, i, m))
    inst = [S.InstanceDesc(k) for k in range(3)]
    return S.SceneDesc(mats, meshes, inst, cam, "lens_quads")


_state = {}


def _tracer(gpu):
    if "pt" not in _state:
        d = _scene(gpu)
        _state["desc"], _state["pt"] = d, gpu.PathTracer(0).load_scene(d)
    return _state["desc"], _state["pt"]


def _render(pt, w, h, spp, lens, seed=SEED, max_bounces=0, **kw):
    pt.set_camera_lens(*lens)
    return pt.render(w, h, spp, seed=seed, max_bounces=max_bounces, **kw)


# ---- 1. the rays ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LENSES))
def test_device_camera_rays_equal_reference_bit_for_bit(gpu, name):
    """The launcher a batch would choose — k_raygen for R = 0, k_raygen_lens otherwise — into lane 0's queue, read back."""
    desc, pt = _tracer(gpu)
    lens = LENSES[name]
    pt.set_camera_lens(*lens)
    basis = ref.camera_basis(desc.camera)
    scattered = np.random.default_rng(5).permutation(W * H)[:97]
    for pixels in (np.arange(W * H), scattered):
        o, d = pt.debug_camera_rays(W, H, SEED, FIRST, NS, pixels)
        ro, rd, _ = ref.camera_rays(basis, lens, W, H, SEED, FIRST, NS, pixels)
        assert _bits_equal(o, ro) and _bits_equal(d, rd), name
    host = gpu.PathTracer(gpu.ptc.DEVICE_NONE)                                            # and the host evaluation of the same header
    host.set_camera(desc.camera.position, desc.camera.target, desc.camera.fov_y, desc.camera.aspect)
    host.set_camera_lens(*lens)
    ho, hd = host.debug_camera_rays(W, H, SEED, FIRST, NS, scattered)
    assert _bits_equal(o, ho) and _bits_equal(d, hd)


# ---- 2. the rendered image --------------------------------------------------------------------------------------------------------------------------------
def _expected_image(pt, desc, lens, w, h, spp, seed):
    """The image from the reference's rays: emission of the first hit's quad (the front faces the camera: emission is one-sided) or 0, summed per pixel in
    sample order in float32, divided by (float)spp."""
    basis = ref.camera_basis(desc.camera)
    o, d, _ = ref.camera_rays(basis, lens, w, h, seed, 0, spp, np.arange(w * h))
    _, prim, _ = pt.trace_closest(o, d)
    _, _, tri_mat = pt.flat_scene()
    Le = np.concatenate([np.asarray(EMISSION, F32), np.zeros((1, 3), F32)])             # row 3: a miss
    which = np.where(prim >= 0, tri_mat[np.maximum(prim, 0)], 3).reshape(spp, h, w)      # the quad every sample saw; 3: none
    L = Le[which]
    acc = np.zeros((h, w, 3), F32)
    for k in range(spp):
        acc = (acc + L[k]).astype(F32)
    img = np.ones((h, w, 4), F32)
    img[..., :3] = acc / F32(spp)
    return img, which


def test_rendered_image_is_the_reference_rays_image(gpu):
    desc, pt = _tracer(gpu)
    images, mixed = {}, {}
    for name in ("pinhole", "disk", "hexagon"):      # the pinhole first: it validates this test's model of the integrator before the model judges the lens
        want, which = _expected_image(pt, desc, LENSES[name], W, H, NS, SEED)
        got = _render(pt, W, H, NS, LENSES[name])
        assert {int(m) for m in np.unique(which)} == {0, 1, 2, 3}, "the image shows all three quads and the background"
        assert _bits_equal(got, want), name
        images[name] = got
        mixed[name] = int((which.min(0) != which.max(0)).sum())      # pixels whose samples saw more than one quad: edges, and the blur
    assert not _bits_equal(images["disk"], images["pinhole"]) and not _bits_equal(images["hexagon"], images["disk"])
    assert mixed["disk"] > mixed["pinhole"]


# ---- 3. - 5. the lens under the frame machinery -------------------------------------------------------------------------------------------------------------
def test_tile_shares_sum_to_the_unsharded_lens_frame(gpu):
    desc, pt = _tracer(gpu)
    w, h, spp = 70, 40, 3
    lens = LENSES["hexagon"]
    full = _render(pt, w, h, spp, lens)
    total = np.zeros_like(full)
    for r in range(2):
        pt.frame_begin(w, h, spp, SEED, 0, 0, r, 2)
        pt.frame_add_samples(spp)
        pt.frame_resolve()
        share = pt.read_radiance()
        assert (share[..., 3] > 0).any() and not (share[..., 3] > 0).all()
        total += share
    assert _bits_equal(total, full)
    assert not _bits_equal(full, _render(pt, w, h, spp, LENSES["pinhole"]))


def test_checkpoint_and_restore_give_the_uninterrupted_lens_frame(gpu):
    desc, pt = _tracer(gpu)
    lens = LENSES["disk"]
    full = _render(pt, W, H, 5, lens)
    pt.frame_begin(W, H, 5, SEED, 0, 0)
    pt.frame_add_samples(2)
    acc, done = pt.frame_checkpoint()
    assert done == 2
    other = gpu.PathTracer(0).load_scene(desc)
    other.set_camera_lens(*lens)
    other.frame_begin(W, H, 5, SEED, 0, 0)
    other.frame_restore(acc, done)
    other.frame_add_samples(3)
    other.frame_resolve()
    assert _bits_equal(other.read_radiance(), full)


def test_adaptive_lens_frame_holds_the_uniform_frames_bits(gpu):
    """max_bounces = 0 and emitters only: a pixel is noisy exactly where the lens blurs an edge, so sharp pixels stop at the first decision and blurred ones go on."""
    desc, pt = _tracer(gpu)
    lens = LENSES["disk"]
    pt.set_camera_lens(*lens)
    img = pt.render_adaptive(W, H, 24, seed=SEED, max_bounces=0, threshold=0.05, radius=0, min_samples=8, step_samples=8)
    counts = pt.read_sample_counts()
    present = sorted(int(n) for n in np.unique(counts))
    assert len(present) >= 2 and present[0] == 8, present                                # some pixels stopped early, some did not
    for n in (present[0], present[-1]):
        uniform = _render(pt, W, H, n, lens)
        sel = counts == n
        assert sel.any() and _bits_equal(img[sel], uniform[sel]), n


# ---- 6. - 8. what does not see the lens ---------------------------------------------------------------------------------------------------------------------
def test_guides_ignore_the_lens_and_stay_valid(gpu):
    desc, pt = _tracer(gpu)
    guides = {}
    for name in ("pinhole", "disk"):
        _render(pt, W, H, 2, LENSES[name])
        pt.frame_guides()
        guides[name] = (pt.read_guide(gpu.ptc.GUIDE_ALBEDO), pt.read_guide(gpu.ptc.GUIDE_NORMAL_DEPTH)) + pt.read_guide_hit()
    for a, b in zip(guides["pinhole"], guides["disk"]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    assert (guides["disk"][0][..., 3] == 2).any() and (guides["disk"][0][..., 3] == 0).any()      # emitters and background
    pt.set_camera_lens(*LENSES["hexagon"])                                               # leaves guides_valid alone ...
    assert _bits_equal(pt.read_guide(gpu.ptc.GUIDE_NORMAL_DEPTH), guides["disk"][1])
    pt.denoise()                                                                         # ... so the denoiser still has its guides
    pt.select_output(gpu.ptc.OUTPUT_DENOISED)
    assert np.isfinite(pt.read_radiance()).all()


def test_focus_distance_at_pixel(gpu):
    desc, pt = _tracer(gpu)
    L = gpu.load_library()
    out = C.c_float(-1.0)
    pt.set_camera_lens(*LENSES["disk"])
    pt.frame_begin(W, H, 1, SEED, 0, 0)
    assert L.ptc_focus_distance_at_pixel(pt._h, 3, 3, C.byref(out)) == E_STATE          # no guides yet
    pt.frame_guides()
    nz = pt.read_guide(gpu.ptc.GUIDE_NORMAL_DEPTH)
    basis = ref.camera_basis(desc.camera)
    hit = miss = 0
    for y in range(H):
        for x in range(0, W, 2):
            got = pt.focus_distance_at_pixel(x, y)
            assert _bits_equal(F32(got), ref.focus_distance(basis, W, H, x, y, nz[y, x, 3])), (x, y)
            if nz[y, x, 3] == 0:
                assert got == 0.0                                                        # a miss
                miss += 1
            else:
                hit += 1
    assert hit and miss
    for x, y in ((-1, 0), (W, 0), (0, H), (0, -1)):
        assert L.ptc_focus_distance_at_pixel(pt._h, x, y, C.byref(out)) == E_ARG
    assert L.ptc_focus_distance_at_pixel(pt._h, 0, 0, None) == E_ARG
    pt.set_camera(desc.camera.position, desc.camera.target, desc.camera.fov_y, desc.camera.aspect)      # a new camera: its guides are gone
    assert L.ptc_focus_distance_at_pixel(pt._h, 3, 3, C.byref(out)) == E_STATE


@pytest.mark.parametrize("integrator", ["INTEGRATOR_RASTER_COMPAT", "INTEGRATOR_RASTER_GBUFFER16"])
def test_raster_integrators_ignore_the_lens(gpu, integrator):
    d = gpu.scenes.cornell_box()
    pt = gpu.PathTracer(0).load_scene(d)
    kind = getattr(gpu.ptc, integrator)
    plain = pt.render(W, H, 1, seed=1, integrator=kind)
    pt.set_camera_lens(0.2, 3.0, 5, 0.1)
    assert _bits_equal(pt.render(W, H, 1, seed=1, integrator=kind), plain)
    assert (plain[..., :3] > 0).any()


# ---- 9. the command-line renderer ---------------------------------------------------------------------------------------------------------------------------
def _read_pfm(path, w, h):
    head, body = open(path, "rb").read().split(b"-1.0\n", 1)
    assert head.startswith(b"PF\n%d %d" % (w, h))
    return np.ascontiguousarray(np.frombuffer(body, "<f4").reshape(h, w, 3)[::-1])        # PFM rows are bottom-up


def test_cpp_host_cli_renders_through_the_lens(gpu, tmp_path):
    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    w, h = 48, 40
    out = str(tmp_path / "lens.pfm")
    common = [exe, "--scene", "cornell", "--width", str(w), "--height", str(h), "--spp", "4", "--seed", "5", "--bounces", "3"]
    r = subprocess.run(common + ["--aperture", "0.125", "--focus", "2.75", "--blades", "5", "--aperture-rotation", "0.25", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    d = gpu.scenes.cornell_box()
    d.camera.aspect = 1.0
    d.camera.aperture_radius, d.camera.focus_distance, d.camera.blades, d.camera.aperture_rotation = 0.125, 2.75, 5, 0.25
    pt = gpu.PathTracer(0).load_scene(d)                                                 # the scene camera's lens fields are applied with the camera
    assert pt.get_camera_lens() == dict(aperture_radius=0.125, focus_distance=2.75, blades=5, rotation=0.25)
    img = pt.render(w, h, 4, seed=5, max_bounces=3)
    assert _bits_equal(_read_pfm(out, w, h), np.ascontiguousarray(img[..., :3]))
    pt.set_camera_lens()
    assert not _bits_equal(pt.render(w, h, 4, seed=5, max_bounces=3), img)
    # --focus-pixel: the guides once, then the depth of what the pixel sees
    r = subprocess.run(common + ["--aperture", "0.125", "--focus-pixel", "24,20", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    pt.frame_begin(w, h, 1, 5, 3, 0)
    pt.frame_guides()
    focus = pt.focus_distance_at_pixel(24, 20)
    assert focus > 0
    pt.set_camera_lens(0.125, focus)
    assert _bits_equal(_read_pfm(out, w, h), np.ascontiguousarray(pt.render(w, h, 4, seed=5, max_bounces=3)[..., :3]))
    bad = subprocess.run(common + ["--aperture", "0.1", "--focus", "3", "--focus-pixel", "2,2"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "exclude each other" in bad.stderr
    bad = subprocess.run(common + ["--aperture", "-1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--aperture" in bad.stderr
