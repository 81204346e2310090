"""First-hit guide buffers, the variance-guided à-trous denoiser and the output selector on a real MI355X (include/ptc.h: ptc_frame_guides,
ptc_read_guide_*, ptc_denoise, ptc_select_output).  The guides are checked as functions of the hit against the flattened scene and the scalar
oracle's closest hit; the filter against the specification evaluated in numpy (tests/denoise_reference.py), in float64, with the float32-float64
gap of that same evaluation as the yardstick; the rest are exact properties: pass-through classes, an untouched frame, the selected output."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "segments", "shadow_rays", "hits", "node_visits_closest", "tri_tests_closest", "node_visits_any", "tri_tests_any", "algorithmic_bytes")
SCENES = ("cornell", "sphere10k", "textured_objects")
EXPLICIT = dict(iterations=4, sigma_l=4.0, sigma_n=128.0, sigma_p=1.0, demodulate=1)


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _load(gpu, name):
    d = gpu.scenes.by_name(name)
    return d, gpu.PathTracer(0).load_scene(d)


def _frame_with_guides(pt, w, h, spp=4, seed=1, **kw):
    pt.frame_begin(w, h, spp, seed=seed, max_bounces=8, **kw)
    pt.frame_guides()
    prim, uv = pt.read_guide_hit()
    return pt.read_guide(0), pt.read_guide(1), prim, uv


@pytest.mark.parametrize("name", SCENES)
def test_guides_are_functions_of_the_hit(gpu, name):
    """Class from the hit's material, normal from the vertex normals at the barycentrics, albedo = colour factor (x the NEAREST texel of the colour texture)."""
    d, pt = _load(gpu, name)
    w = h = 128
    ak, nz, prim, uv = _frame_with_guides(pt, w, h)
    verts, idx, tm = pt.flat_scene()
    mats, texs = pt.description()
    factors = np.array([m[0] for m in mats], np.float32)
    tex_color = np.array([m[1][0] for m in mats])
    hit = prim >= 0
    pr = np.where(hit, prim, 0)
    mat = tm[pr]
    K = np.where(hit, np.where((factors[mat][..., 6:9] != 0).any(-1), 2, 1), 0)
    assert np.array_equal(ak[..., 3], K.astype(np.float32))
    surf = K == 1
    assert surf.mean() > 0.2
    # misses and emitters: albedo 1, normal 0; depth 0 on a miss only
    assert (ak[~surf][:, :3] == 1).all() and (nz[~surf][:, :3] == 0).all() and (nz[~hit][:, 3] == 0).all() and (nz[hit][:, 3] > 0).all()
    assert (prim[~hit] == -1).all() and (uv[~hit] == 0).all()
    hu, hv = uv[..., 0:1].astype(np.float64), uv[..., 1:2].astype(np.float64)
    wgt = (1 - hu - hv, hu, hv)
    n = sum(verts[idx[pr, k], 3:6].astype(np.float64) * wgt[k] for k in range(3))
    n /= np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-30)
    err_n = float(np.abs(nz[..., :3] - n)[surf].max())
    print(f"{name}: classes miss/surface/emitter {[round(float((K == k).mean()), 4) for k in (0, 1, 2)]}, normal max abs error {err_n:.3g}")
    assert err_n <= 1e-5
    plain = surf & (tex_color[mat] < 0)
    assert np.array_equal(ak[plain][:, :3], factors[mat][plain][:, :3])
    textured = surf & (tex_color[mat] >= 0)
    if name == "textured_objects":
        assert textured.mean() > 0.2
        tc = sum(verts[idx[pr, k], 10:12].astype(np.float64) * wgt[k] for k in range(3))
        checked = np.zeros((h, w), bool)
        for t in np.unique(tex_color[mat][textured]):
            img = texs[t]
            th, tw = img.shape[:2]
            sel = textured & (tex_color[mat] == t)
            f = tc - np.floor(tc)
            xs, ys = f[..., 0] * tw, f[..., 1] * th
            near = lambda v: np.minimum(v - np.floor(v), np.ceil(v) - v) < 1e-3
            ok = sel & ~near(xs) & ~near(ys)
            x, y = np.minimum(xs.astype(np.int64), tw - 1), np.minimum(ys.astype(np.int64), th - 1)
            texel = img[y, x, :3].astype(np.float32) / np.float32(255.0)
            want = (factors[mat][..., :3] * texel).astype(np.float32)
            assert np.array_equal(ak[ok][:, :3], want[ok]), t
            checked |= ok
        left_out = (textured & ~checked).sum() / (w * h)
        print(f"{name}: textured pixels {textured.mean():.3f} of the frame, left out at texel borders {left_out:.5f}")
        assert left_out <= 0.01
    else:
        assert not textured.any()


@pytest.mark.parametrize("name", SCENES)
def test_guide_hit_is_the_closest_hit(gpu, ora, name):
    """The guide ray is k_raygen's camera ray with the jitter at (0.5, 0.5); its hit is the oracle's closest hit of the float32 mirror of that ray."""
    d, pt = _load(gpu, name)
    w, h = 160, 96
    ak, nz, prim, uv = _frame_with_guides(pt, w, h)
    dirs, pos = ref.guide_dirs(d.camera, w, h)
    t, oprim, ouv = ora.Oracle().load_scene(d).trace_closest(np.broadcast_to(pos, dirs.shape).reshape(-1, 3), dirs.reshape(-1, 3))
    t, oprim, ouv = t.reshape(h, w), oprim.reshape(h, w), ouv.reshape(h, w, 2)
    agree = prim == oprim
    both = agree & (prim >= 0)
    print(f"{name}: primitive ids agree on {agree.mean():.5f} of the pixels, max |Z - t| / t {float((np.abs(nz[..., 3] - t) / np.maximum(t, 1e-30))[both].max()):.3g}, "
          f"max barycentric difference {float(np.abs(uv - ouv)[both].max()):.3g}")
    assert agree.mean() >= 0.999
    assert (np.abs(nz[..., 3] - t)[both] <= 1e-5 * t[both]).all()
    assert np.abs(uv - ouv)[both].max() <= 1e-4


def _synthetic(ak, seed):
    """albedo x a smooth ramp + seeded noise, alpha 1"""
    h, w = ak.shape[:2]
    rng = np.random.default_rng(seed)
    ramp = 0.2 + 0.8 * (np.arange(w)[None, :, None] / w) * (0.5 + 0.5 * np.arange(h)[:, None, None] / h)
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = np.maximum(ak[..., :3] * ramp + 0.15 * rng.standard_normal((h, w, 3)), 0.0)
    return img


@pytest.mark.parametrize("name,w,h", [("cornell", 128, 128), ("sphere10k", 128, 128), ("textured_objects", 128, 128), ("sphere10k", 200, 72)])
def test_filter_is_the_specified_one(gpu, name, w, h):
    """The library's image lies within 16 x E32 of the float64 evaluation of the specification, E32 = the gap between the float32 and the float64
    evaluation of the same input over the image maximum.  16 covers library exp / pow a few ulp off numpy's and another summation order.
    Iterations 1, 4 and 5 (steps through LDS tiles and gathered), demodulation on and off, a rendered and a synthetic input, a non-square frame."""
    d, pt = _load(gpu, name)
    noisy = pt.render(w, h, 4, seed=3)
    ak, nz, prim, uv = _frame_with_guides(pt, w, h)
    dirs, pos = ref.guide_dirs(d.camera, w, h)
    worst = 0.0
    for label, img in (("rendered 4 spp", noisy), ("synthetic", _synthetic(ak, 11))):
        pt.write_radiance(img)
        for iters in (1, 4, 5):
            for demod in (1, 0):
                p = dict(iterations=iters, sigma_l=4.0, sigma_n=128.0, sigma_p=1.0, demodulate=demod)
                pt.denoise(**p)
                pt.select_output(gpu.ptc.OUTPUT_DENOISED)
                got = pt.read_radiance()
                pt.select_output(gpu.ptc.OUTPUT_RADIANCE)
                e64, e32 = (ref.atrous(img[..., :3], ak, nz, dirs, pos, d.camera.fov_y, dt=dt, **p) for dt in (np.float64, np.float32))
                top = float(e64.max())
                E32 = float(np.abs(e32.astype(np.float64) - e64).max()) / top
                err = float(np.abs(got[..., :3].astype(np.float64) - e64).max()) / top
                print(f"{name} {w}x{h} {label}, {iters} iterations, demodulate {demod}: E32 {E32:.3g}, library error {err:.3g}, ratio {err / E32:.2f}")
                worst = max(worst, err / E32)
                assert np.array_equal(got[..., 3], img[..., 3])            # alpha from the radiance
                assert err <= 16 * E32, (label, iters, demod, err, E32)
    print(f"{name} {w}x{h}: worst library error / E32 = {worst:.2f} (bound 16)")


@pytest.mark.parametrize("name", ("cornell", "sphere10k"))
def test_exact_properties(gpu, name):
    """iterations = 0 copies; misses and emitters pass through bit for bit at any iteration count; the radiance buffer is not modified."""
    d, pt = _load(gpu, name)
    w, h = 144, 80
    pt.frame_begin(w, h, 4, seed=5, max_bounces=8)
    pt.frame_add_samples(4)
    pt.frame_guides()
    pt.frame_resolve()
    rad = pt.read_radiance()
    K = pt.read_guide(0)[..., 3]
    assert (K != 1).any() and (K == 1).any()
    for iters in (0, 1, 3, 6):
        pt.denoise(**dict(EXPLICIT, iterations=iters))
        assert _bits_equal(pt.read_radiance(), rad)                          # still the radiance: the output was not selected, the buffer not touched
        pt.select_output(1)
        dn = pt.read_radiance()
        pt.select_output(0)
        if iters == 0:
            assert _bits_equal(dn, rad)
        else:
            assert _bits_equal(dn[K != 1], rad[K != 1])
            assert not _bits_equal(dn[K == 1], rad[K == 1])
        assert _bits_equal(pt.read_radiance(), rad)
    with pytest.raises(gpu.PtcError, match="ptc error -1"):
        pt.denoise(iterations=9)
    for bad in (dict(sigma_l=-1.0), dict(sigma_n=float("nan")), dict(sigma_p=float("inf")), dict(iterations=-1)):
        with pytest.raises(gpu.PtcError, match="ptc error -1"):
            pt.denoise(**bad)


def test_guides_and_denoise_leave_the_frame_alone(gpu):
    """A progressive frame with ptc_frame_guides and ptc_denoise in its middle accumulates the same bytes and counts the same rays."""
    d, pt = _load(gpu, "sphere10k")
    w, h = 128, 96

    def frame(with_calls):
        pt.frame_begin(w, h, 6, seed=21, max_bounces=6)
        pt.frame_add_samples(2)
        if with_calls:
            pt.frame_guides()
        pt.frame_add_samples(3)
        if with_calls:
            pt.denoise(**EXPLICIT)
        pt.frame_add_samples(1)
        pt.frame_resolve()
        st = pt.stats()
        return pt.read_radiance(), [st[k] for k in COUNTERS]

    img0, c0 = frame(False)
    img1, c1 = frame(True)
    assert _bits_equal(img0, img1)
    assert c0 == c1 and c0[0] == w * h * 6
    # the guides cover every pixel whatever the frame's tile share
    whole = _frame_with_guides(pt, w, h)
    half = _frame_with_guides(pt, w, h, tile_rank=0, tile_count=2)
    for a, b in zip(whole, half):
        assert _bits_equal(a, b) if a.dtype == np.float32 else np.array_equal(a, b)


def test_guides_of_a_frame_larger_than_the_queues_are_traced_in_chunks(gpu):
    """A lane's queues hold at most 2 M guide rays unless the frame's batches made them larger: a 2.25 M-pixel frame is traced in two chunks, and gives
    what a context whose queues hold the whole frame gives in one."""
    w, h = 2048, 1100
    d, pt = _load(gpu, "cornell")
    chunked = _frame_with_guides(pt, w, h, spp=1)
    assert pt.internals()["queue_cap"] < w * h
    pt2 = gpu.PathTracer(0).load_scene(d)
    pt2.frame_begin(w, h, 1, seed=1, max_bounces=8)
    pt2.frame_reserve()
    assert pt2.internals()["queue_cap"] >= w * h
    pt2.frame_guides()
    prim, uv = pt2.read_guide_hit()
    for a, b in zip(chunked, (pt2.read_guide(0), pt2.read_guide(1), prim, uv)):
        assert _bits_equal(a, b) if a.dtype == np.float32 else np.array_equal(a, b)
    assert (chunked[2][-1] >= 0).any()                                       # the last rows (the second chunk) hold hits


def test_output_selection_and_state_errors(gpu, ora):
    d, pt = _load(gpu, "cornell")
    w, h = 96, 64
    pt.frame_begin(w, h, 4, seed=2, max_bounces=8)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise(**EXPLICIT)                                               # no guides yet
    pt.frame_add_samples(4)
    pt.frame_guides()
    pt.frame_resolve()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.select_output(gpu.ptc.OUTPUT_DENOISED)                            # nothing denoised yet
    with pytest.raises(gpu.PtcError, match="ptc error -1"):
        pt.select_output(7)
    rad = pt.read_radiance()
    pt.denoise(**EXPLICIT)
    pt.select_output(gpu.ptc.OUTPUT_DENOISED)
    dn = pt.read_radiance()
    assert not _bits_equal(dn, rad)
    assert np.array_equal(pt.tonemap(), ora.tonemap_rgba8(dn))
    want16 = np.array([ora.f32_to_f16(v) for v in dn.ravel()], np.uint16).reshape(h, w, 4)
    assert np.array_equal(pt.read_radiance_f16().view(np.uint16), want16)
    assert pt.radiance_f16_device_ptr() != 0
    g_s, d_s = pt.denoise_seconds()
    assert 0 < g_s < 1 and 0 < d_s < 1
    # the next frame serves the plain radiance again, and its guides have to be traced again
    pt.frame_begin(w, h, 4, seed=2, max_bounces=8)
    pt.frame_add_samples(4)
    pt.frame_resolve()
    assert _bits_equal(pt.read_radiance(), rad)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise(**EXPLICIT)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.read_guide(0)
    # a moved camera or a refitted scene ends the guides' validity
    pt.frame_guides()
    c = d.camera
    pt.set_camera(c.position, c.target, c.fov_y, c.aspect)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise(**EXPLICIT)
    pt.frame_guides()
    pt.denoise(**EXPLICIT)
    pt.scene_refit()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.frame_guides()                                                    # the refit ended the frame
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise(**EXPLICIT)
    # the raster integrators are noise-free: no guides for them
    pt.frame_begin(w, h, 1, seed=2, max_bounces=8, integrator=gpu.ptc.INTEGRATOR_RASTER_COMPAT)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.frame_guides()


def _relmse(a, b):
    a, b = a[..., :3].astype(np.float64), b[..., :3].astype(np.float64)
    return float((((a - b) ** 2) / (b ** 2 + 1e-2)).mean())


@pytest.mark.parametrize("name", SCENES)
def test_it_denoises(gpu, name):
    """4 spp, the explicit parameters (4, 4, 128, 1, demodulate on), against the library's own 1024-spp render with another seed:
    relMSE(denoised) <= 0.5 relMSE(noisy) on cornell and sphere10k (the float64 prototype: 0.13 and 0.18).  textured_objects: recorded, not asserted."""
    d, pt = _load(gpu, name)
    w = h = 128
    converged = pt.render(w, h, 1024, seed=7)
    pt.frame_begin(w, h, 4, seed=1, max_bounces=8)
    pt.frame_add_samples(4)
    pt.frame_guides()
    pt.frame_resolve()
    noisy = pt.read_radiance()
    ratios = {}
    for demod in (1, 0):
        pt.denoise(**dict(EXPLICIT, demodulate=demod))
        pt.select_output(1)
        ratios[demod] = _relmse(pt.read_radiance(), converged) / _relmse(noisy, converged)
        pt.select_output(0)
    print(f"{name}: relMSE noisy {_relmse(noisy, converged):.4g}, denoised / noisy = {ratios[1]:.3f} with demodulation, {ratios[0]:.3f} without")
    if name != "textured_objects":
        assert ratios[1] <= 0.5


def _read_pfm(path, w, h):
    head, body = open(path, "rb").read().split(b"-1.0\n", 1)
    assert head.startswith(b"PF\n%d %d" % (w, h))
    return np.ascontiguousarray(np.frombuffer(body, "<f4").reshape(h, w, 3)[::-1])        # PFM rows are bottom-up


def test_cpp_host_cli_denoises_and_writes_guides(gpu, tmp_path):
    """ptc_render --denoise --guides PREFIX (host/pbr_pt.hpp over the same C-ABI): the image and the guide files equal what the Python binding reads."""
    import subprocess

    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    w, h = 96, 64
    out, pre = str(tmp_path / "dn.pfm"), str(tmp_path / "g")
    r = subprocess.run([exe, "--scene", "cornell", "--width", str(w), "--height", str(h), "--spp", "4", "--seed", "5", "--bounces", "4", "--denoise-iters", "3", "--guides", pre, "--out", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    d = gpu.scenes.cornell_box()
    d.camera.aspect = 1.0
    pt = gpu.PathTracer(0).load_scene(d)
    noisy = pt.render(w, h, 4, seed=5, max_bounces=4)
    pt.frame_guides()                                                          # ptc_render leaves its frame open
    pt.denoise(iterations=3)
    pt.select_output(gpu.ptc.OUTPUT_DENOISED)
    dn = pt.read_radiance()
    assert not _bits_equal(dn, noisy)
    assert _bits_equal(_read_pfm(out, w, h), np.ascontiguousarray(dn[..., :3]))
    ak, nz = pt.read_guide(gpu.ptc.GUIDE_ALBEDO), pt.read_guide(gpu.ptc.GUIDE_NORMAL_DEPTH)
    assert _bits_equal(_read_pfm(pre + "_albedo.pfm", w, h), np.ascontiguousarray(ak[..., :3]))
    assert _bits_equal(_read_pfm(pre + "_normal.pfm", w, h), np.ascontiguousarray(nz[..., :3]))
    assert _bits_equal(_read_pfm(pre + "_depth.pfm", w, h), np.ascontiguousarray(np.repeat(nz[..., 3:4], 3, axis=-1)))
    bad = subprocess.run([exe, "--scene", "cornell", "--raster", "--denoise"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "path integrator" in bad.stderr
