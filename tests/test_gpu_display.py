"""The display transform on a real MI355X (include/ptc.h: ptc_meter_exposure ... ptc_display_rgba16f; csrc/pt_display.hip).

1. k_meter_hist + k_meter_reduce against the numpy restatement (tests/display_reference.py): histogram, N, M, rejected, Q and the adaptation state, exact.
2. k_display_rgba8 (every operator x transfer function) and k_display_half against it, bit for bit; a metering and a display queued back to back.
3. Parity with k_tonemap and k_to_half.
4. The frame in progress, its statistics and the other read-backs are not disturbed; the select_output choice is followed.
5. The adaptation state's lifetime.
6. A sun of 100 000 lx: ptc_tonemap_rgba8 is white, the metered display is an image; ptc_render's PNG is the Python path's.

Images are put in place with a 1-spp Cornell frame of the shape and ptc_write_radiance_rgba32f.  The shapes: a single pixel, less than a wave, a wave and one more, one
block, an odd count over several blocks, and one pixel row more than a pass of k_meter_hist's grid covers, so that its grid-stride loop runs a second, partial pass."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import display_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
SMALL = [(1, 1), (7, 3), (64, 1), (65, 1), (16, 16), (257, 3)]
SHAPES = SMALL + ["two passes"]
COUNTERS = ("paths", "segments", "shadow_rays", "hits", "node_visits_closest", "tri_tests_closest", "node_visits_any", "tri_tests_any", "launches_trace_closest",
            "launches_trace_any")


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


@pytest.fixture(scope="module")
def pt(gpu):
    p = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    yield p
    p.close()


@pytest.fixture(scope="module")
def colours():
    return ref.colours()


def _shape(pt, shape):
    if shape != "two passes":
        return shape
    P = pt.display_internals()[0]
    w, h = 1031, (P + 1 + 1030) // 1031
    assert P < w * h < P + 2 * w and w * h < 2 ** 22
    return w, h


def _frame(pt, shape):
    w, h = _shape(pt, shape)
    pt.render(w, h, 1, seed=1, max_bounces=0)
    return w, h


def _put(pt, px, w, h):
    pt.write_radiance(np.ascontiguousarray(px, F32).reshape(h, w, 4))


def _tiled(px, n, shift=0):
    """n pixels that walk through px again and again (from `shift` on): an index into px, so that a reference computed on px once serves every shape."""
    return (np.arange(n) + shift) % len(px)


def _check_metering(pt, px, p, A_before, what):
    want = ref.meter(px, p, A_before)
    got = pt.exposure_state()
    for k in ("A", "Q", "N", "M", "rejected"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(pt.luminance_histogram(), want["hist"]), what
    e = pt.exposure()
    assert e["metered"] == want["N"] and e["rejected"] == want["rejected"], what
    assert F32(e["scale"]) == ref.scale(p, want["A"]) and F32(e["metered_luminance"]).view(U32) == want["Q"] and F32(e["adapted_luminance"]).view(U32) == want["A"], what
    return want["A"]


# ---- 1. metering ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_metering_equals_reference(pt, shape):
    w, h = _frame(pt, shape)
    n = w * h
    keys, special = ref.all_keys_image(), ref.special_pixels()
    rng = np.random.default_rng(n)
    contents = {"constant": np.tile(np.array([[0.3, 0.2, 0.1, 1.0]], F32), (n, 1)),                  # every lane adds to one LDS address
                "all keys": keys[rng.permutation(_tiled(keys, n))], "random": ref.random_image(n, n), "special": special[_tiled(special, n, 3)],
                "nothing": np.zeros((n, 4), F32)}
    fields = dict(auto_exposure=1, adapt_rate=0.5, percentile_lo=0.05, percentile_hi=0.95, gain=1.25)
    p = ref.params(**fields)
    pt.set_display(**fields)
    pt.exposure_reset()
    assert pt.exposure_state()["A"] == 0
    A = 0
    for name, px in contents.items():
        _put(pt, px, w, h)
        pt.meter_exposure()
        A = _check_metering(pt, px, p, A, (shape, name))
        if name == "all keys" and n >= len(keys):
            assert (pt.luminance_histogram()[:4080] >= 1).all()                                       # every key that can be metered
    # two meterings in a row: the histogram is the second one's, the state has taken two steps
    _put(pt, contents["random"], w, h)
    pt.meter_exposure()
    pt.meter_exposure()
    A = ref.meter(contents["random"], p, A)["A"]
    _check_metering(pt, contents["random"], p, A, (shape, "twice"))
    m, _ = pt.display_seconds()
    assert 0.0 < m < 0.1
    pt.set_display()


# ---- 2. display ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def display_reference(colours):
    """The reference's bytes for the colours, per (operator, transfer function), at the gain the test uses: computed once, indexed by every shape."""
    E = F32(3.7)
    out = {(op, oe): ref.display_rgba8(colours, E, ref.params(tonemap=op, oetf=oe, white=3.0)) for op in range(4) for oe in range(2)}
    out["half"] = ref.display_rgba16f(colours, E)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_display_equals_reference(pt, colours, display_reference, shape):
    w, h = _frame(pt, shape)
    n = w * h
    idx = _tiled(colours, n, 0 if n > 4000 else 3195)          # the small shapes start among the special values
    px = colours[idx]
    _put(pt, px, w, h)
    pt.exposure_reset()
    for op in range(4):
        for oe in range(2):
            pt.set_display(gain=3.7, tonemap=op, oetf=oe, white=3.0)
            got = pt.display().reshape(n, 4)
            want = display_reference[(op, oe)][idx]
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (shape, op, oe, px[bad[:4]], got[bad[:4]], want[bad[:4]])
    got = pt.display_f16().view(np.uint16).reshape(n, 4)
    want = display_reference["half"][idx]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (shape, px[bad[:4]], got[bad[:4]], want[bad[:4]])
    _, d = pt.display_seconds()
    assert 0.0 < d < 0.1
    # a metering and a display queued back to back, nothing that waits in between: the display uses the exposure that metering found
    fields = dict(auto_exposure=1, gain=1.5, key=0.18, tonemap="neutral", oetf="srgb", percentile_lo=0.1, percentile_hi=0.9)
    p = ref.params(**dict(fields, tonemap=ref.NEUTRAL, oetf=ref.SRGB))
    pt.set_display(**fields)
    pt.meter_exposure()
    got = pt.display().reshape(n, 4)
    A = ref.meter(px, p, 0)["A"]
    E = ref.scale(p, A)
    assert A != 0 and E != F32(1.5)
    want = ref.display_rgba8(colours, E, p)[idx]
    assert np.array_equal(got, want), shape
    got16 = pt.display_f16().view(np.uint16).reshape(n, 4)
    assert np.array_equal(got16, ref.display_rgba16f(colours, E)[idx]), shape
    assert pt.exposure_state()["A"] == A
    pt.set_display()


# ---- 3. parity with the existing kernels ---------------------------------------------------------------------------------------------------------------------
def test_defaults_are_the_existing_tonemapper_and_half_conversion(pt):
    w = h = 48
    pt.set_display()
    pt.exposure_reset()
    img = pt.render(w, h, 8, seed=3, max_bounces=4)
    assert (img[..., :3] > 0).mean() > 0.5
    assert np.array_equal(pt.display(), pt.tonemap())
    assert np.array_equal(pt.display_f16().view(np.uint16), pt.read_radiance_f16().view(np.uint16))
    special = ref.special_pixels()
    px = special[_tiled(special, w * h)]
    _put(pt, px, w, h)
    assert np.array_equal(pt.display(), pt.tonemap())                                                 # NaN and inf included
    finite_or_inf = ~np.isnan(px).any(axis=1)                                                          # the header fixes half(NaN) = 0x7e00; k_to_half takes the hardware's
    a, b = pt.display_f16().view(np.uint16).reshape(-1, 4), pt.read_radiance_f16().view(np.uint16).reshape(-1, 4)
    assert np.array_equal(a[finite_or_inf], b[finite_or_inf]) and finite_or_inf.sum() > w * h // 4
    # auto exposure is on but nothing was metered: E = gain
    pt.set_display(auto_exposure=1)
    assert pt.exposure()["scale"] == 1.0
    assert np.array_equal(pt.display(), pt.tonemap())
    pt.set_display()


# ---- 4. non-interference -------------------------------------------------------------------------------------------------------------------------------------
def test_display_calls_do_not_disturb_the_frame(gpu):
    w, h = 40, 24
    desc = gpu.scenes.cornell_box()

    def run(with_display):
        t = gpu.PathTracer(0).load_scene(desc)
        t.frame_begin(w, h, 16, seed=9, max_bounces=4)
        t.frame_add_samples(8)
        t.frame_resolve()
        first = t.read_radiance()
        if with_display:
            t.set_display(auto_exposure=1, tonemap="reinhard", oetf="srgb", gain=2.0)
            t.meter_exposure()
            t.display()
            t.display_f16()
            assert t.display_f16_device_ptr() != 0
            assert np.array_equal(t.read_radiance().view(U32), first.view(U32))
        mid_tm, mid_st = t.tonemap(), t.stats()
        t.frame_add_samples(8)
        t.frame_resolve()
        out = (first, mid_tm, {k: mid_st[k] for k in COUNTERS}, t.read_radiance(), t.tonemap(), t.read_radiance_f16().view(np.uint16), {k: t.stats()[k] for k in COUNTERS})
        return t, out

    a, plain = run(False)
    b, shown = run(True)
    for x, y in zip(plain, shown):
        if isinstance(x, dict):
            assert x == y
        else:
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    # the image select_output serves is the one metered and displayed
    b.set_display()
    b.exposure_reset()
    b.frame_guides()
    b.denoise()
    radiance_bytes = b.display()
    b.select_output(gpu.ptc.OUTPUT_DENOISED)
    den = b.read_radiance()
    assert np.array_equal(b.display(), b.tonemap()) and not np.array_equal(b.display(), radiance_bytes)
    b.meter_exposure()
    assert np.array_equal(b.luminance_histogram(), ref.histogram(den)[0])
    b.temporal_accumulate()
    b.select_output(gpu.ptc.OUTPUT_ACCUMULATED)
    acc = b.read_radiance()
    b.meter_exposure()
    assert np.array_equal(b.luminance_histogram(), ref.histogram(acc)[0])
    assert np.array_equal(b.display(), ref.display_rgba8(acc, 1.0, ref.params()))
    b.select_output(gpu.ptc.OUTPUT_RADIANCE)
    assert np.array_equal(b.display(), radiance_bytes)
    assert np.array_equal(b.read_radiance().view(U32), plain[3].view(U32))
    a.close()
    b.close()


def test_display_needs_an_image(gpu):
    t = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    L = gpu.load_library()
    assert L.ptc_meter_exposure(t._h) == -2 and "nothing rendered" in L.ptc_last_error(t._h).decode()     # PTC_E_STATE
    with pytest.raises(gpu.ptc.PtcError):
        t._w, t._h_px = 4, 4
        t.display()
    assert t.exposure_state() == {"A": 0, "Q": 0, "N": 0, "M": 0, "rejected": 0} and t.exposure()["scale"] == 1.0
    t.close()


# ---- 5. the adaptation state's lifetime ----------------------------------------------------------------------------------------------------------------------
def test_adaptation_state_lifetime(gpu):
    w, h = 24, 16
    desc = gpu.scenes.cornell_box()
    t = gpu.PathTracer(0).load_scene(desc)
    L = gpu.load_library()
    fields = dict(auto_exposure=1, adapt_rate=0.25)
    p = ref.params(**fields)
    t.set_display(**fields)
    A = 0

    def step(level):
        nonlocal A
        px = np.tile(np.array([[level, level, level, 1.0]], F32), (w * h, 1))
        _put(t, px, w, h)
        t.meter_exposure()
        A = ref.meter(px, p, A)["A"]
        assert t.exposure_state()["A"] == A and A != 0

    t.render(w, h, 1, seed=1, max_bounces=0)
    step(0.2)
    first = A
    step(900.0)
    assert A != first and A != ref.meter(np.array([[900.0, 900.0, 900.0, 1.0]], F32), p, 0)["A"]          # on its way: the integer recurrence, not a jump
    t.frame_begin(w, h, 4, seed=2, max_bounces=1)                                                        # a new frame
    t.frame_add_samples(1)
    t.frame_resolve()
    step(900.0)
    c = desc.camera
    t.set_camera((0.3, 0.1, 3.0), c.target, c.fov_y, c.aspect)                                           # a new camera
    t.render(w, h, 1, seed=3, max_bounces=0)
    step(5.0)
    t.update_instance(0, (0.0, -0.05, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))                      # a refit
    t.scene_refit()
    t.render(w, h, 1, seed=4, max_bounces=0)
    step(5.0)
    t.scene_rebuild()                                                                                    # a rebuild
    t.render(w, h, 1, seed=5, max_bounces=0)
    step(0.01)
    t._ck(L.ptc_scene_commit(t._h))                                                                      # a commit of the same description
    t.render(w, h, 1, seed=6, max_bounces=0)
    step(0.01)
    t.exposure_reset()                                                                                   # the reset drops it ...
    assert t.exposure_state()["A"] == 0 and t.exposure()["scale"] == 1.0
    A = 0
    step(40.0)
    assert A == ref.meter(np.array([[40.0, 40.0, 40.0, 1.0]], F32), p, 0)["Q"]                            # ... and the next metering is taken at once
    t.load_scene(desc)                                                                                   # ... and so does ptc_scene_begin; the parameters stay
    assert t.exposure_state()["A"] == 0 and t.get_display()["auto_exposure"] == 1 and t.get_display()["adapt_rate"] == 0.25
    t.close()


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------------------------
SUN = dict(type="directional", direction=(0.2, -0.4, -1.0), intensity=(100000.0, 100000.0, 100000.0))


def test_a_sun_in_physical_units_becomes_an_image(gpu, tmp_path):
    w = h = 64
    t = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    t.add_light(**SUN)
    t.render(w, h, 8, seed=5, max_bounces=4)
    white = t.tonemap()
    # saturated: a colour channel has hit 255 and holds no detail any more.  (All three cannot be asked for: k_tonemap's output matrix sends a grey of any brightness to
    # (1.50, 0.50, 1.00) x rrt_odt's asymptote 1.0165 — the green byte of an arbitrarily bright grey stays at 188.)
    saturated = float((white[..., :3] == 255).any(axis=-1).mean())
    print(f"tonemap(): {saturated:.3f} of the pixels are saturated")
    assert saturated > 0.9                                                # the premise: without exposure there is no image
    t.set_display(auto_exposure=1, tonemap="neutral", oetf="srgb")
    t.meter_exposure()
    shown = t.display()
    lum = 0.2126 * shown[..., 0] + 0.7152 * shown[..., 1] + 0.0722 * shown[..., 2]
    e = t.exposure()
    print(f"display(): median luminance byte {np.median(lum):.1f}, E = {e['scale']:.4g}, metered luminance {e['metered_luminance']:.4g}")
    assert 32 < np.median(lum) < 224
    # every pixel of the frame is owned (alpha 1), so each is metered or rejected; a pixel whose eight paths all ended black has luminance 0 and is rejected
    assert e["metered"] + e["rejected"] == w * h and e["metered"] > 0.99 * w * h and e["scale"] < 1e-2
    # the command-line renderer writes the same bytes
    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    out, png = str(tmp_path / "s.pfm"), str(tmp_path / "s.png")
    r = subprocess.run([exe, "--scene", "cornell", "--width", str(w), "--height", str(h), "--spp", "8", "--seed", "5", "--bounces", "4", "--light",
                        "sun:0.2,-0.4,-1:100000,100000,100000", "--auto-exposure", "--tonemap", "neutral", "--srgb", "--out", out, "--png", png],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[0])
    assert F32(info["exposure_scale"]) == F32(e["scale"]) and info["metered_pixels"] == e["metered"] and info["rejected_pixels"] == e["rejected"]
    from PIL import Image

    assert np.array_equal(np.asarray(Image.open(png)), shown)
    t.close()
