"""The thin-lens camera without a GPU (include/ptc.h: ptc_set_camera_lens, ptc_get_camera_lens, ptc_debug_lens_sample, ptc_debug_camera_rays): symbols,
defaults, the validation table, the lens's lifetime, the host evaluation of csrc/pt_lens.h against its numpy restatement (tests/lens_reference.py) bit for
bit, and — in float64 — the geometry the specification promises: every ray of a pixel sample goes through one point of the plane of focus, a point off
that plane spreads over a disk (polygon) of radius R |1 - z / F| with the second moment of a uniform disk (polygon), polygon samples lie in the polygon."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lens_reference as ref  # noqa: E402

NEW = ("ptc_lens_default_params", "ptc_set_camera_lens", "ptc_get_camera_lens", "ptc_focus_distance_at_pixel", "ptc_debug_lens_sample", "ptc_debug_camera_rays")
E_ARG, E_STATE, E_DEVICE = -1, -2, -3
F32, F64 = np.float32, np.float64
W, H, FIRST, NS, SEED = 33, 17, 3, 5, 0x1234567890ABCDEF
BLADES = (0, 3, 4, 5, 6, 7, 8, 16)
ROTATIONS = (0.0, 0.25, 0.999)
ONE_M = float(F32(1.0) - F32(2.0 ** -24))      # the largest float32 below 1: what rng_f can return at most


def _camera(pbr):
    return pbr.scene.CameraDesc((3.1, -1.7, 2.3), (0.4, 0.2, -0.9), 0.9, W / H)      # no axis of the basis is a world axis; |pos| = 4.2


def _ctx(pbr, cam=None):
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    L = pbr.load_library()
    assert L.ptc_scene_begin(pt._h) == 0
    cam = cam or _camera(pbr)
    pt.set_camera(cam.position, cam.target, cam.fov_y, cam.aspect)
    return pt


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def test_symbols_abi_and_defaults(pbr):
    header = open(os.path.join(ROOT, "include", "ptc.h")).read()
    L = pbr.load_library()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in pbr.ptc.ABI_SYMBOLS and hasattr(L, sym) and getattr(L, sym).argtypes is not None, sym
    assert re.search(r"typedef struct ptc_lens_params \{", header)
    assert "#define PTC_ABI_VERSION 4" in header and L.ptc_abi_version() == 4            # additive: the ABI version stays
    assert C.sizeof(pbr.ptc.PtcLensParams) == 16
    assert pbr.ptc.lens_default_params() == dict(aperture_radius=0.0, focus_distance=1.0, blades=0, rotation=0.0)
    L.ptc_lens_default_params(None)                                                       # a NULL pointer is ignored
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    assert pt.get_camera_lens() == pbr.ptc.lens_default_params()                          # a new context has the pinhole
    for m in ("set_camera_lens", "get_camera_lens", "focus_distance_at_pixel", "debug_camera_rays"):
        assert callable(getattr(pbr.PathTracer, m)), m
    assert callable(pbr.ptc.lens_sample)
    cam = pbr.scene.CameraDesc((0, 0, 1), (0, 0, 0), 1.0, 1.0)
    assert (cam.aperture_radius, cam.focus_distance, cam.blades, cam.aperture_rotation) == (0.0, 1.0, 0, 0.0)      # a scene's camera is a pinhole by default
    assert L.ptc_set_camera_lens(None, None) == E_ARG and L.ptc_get_camera_lens(None, None) == E_ARG
    out = C.c_float(0)
    assert L.ptc_focus_distance_at_pixel(pt._h, 0, 0, C.byref(out)) == E_DEVICE          # reads the guides: needs the device


def test_validation_table_changes_nothing(pbr):
    L = pbr.load_library()
    pt = _ctx(pbr)
    good = dict(aperture_radius=float(F32(0.125)), focus_distance=float(F32(3.5)), blades=6, rotation=float(F32(0.25)))
    pt.set_camera_lens(**good)
    assert pt.get_camera_lens() == good
    inf, nan = float("inf"), float("nan")
    bad = [("aperture_radius", -0.5), ("aperture_radius", inf), ("aperture_radius", nan),
           ("focus_distance", 0.0), ("focus_distance", -1.0), ("focus_distance", inf), ("focus_distance", nan),
           ("blades", 1), ("blades", 2), ("blades", 17), ("blades", -3),
           ("rotation", -0.25), ("rotation", 1.0), ("rotation", 1.5), ("rotation", inf), ("rotation", nan)]
    for field, value in bad:
        p = pbr.ptc.PtcLensParams(**dict(good, **{field: value}))
        assert L.ptc_set_camera_lens(pt._h, C.byref(p)) == E_ARG, (field, value)
        assert b"set_camera_lens" in L.ptc_last_error(pt._h)
        assert pt.get_camera_lens() == good, (field, value)
        with pytest.raises(pbr.PtcError, match="ptc error -1"):
            pt.set_camera_lens(**dict(good, **{field: value}))
    for blades in (0, 3, 16):                                                            # the edges of what is accepted
        pt.set_camera_lens(0.0, 1e-3, blades, ONE_M)
        assert pt.get_camera_lens()["blades"] == blades
    assert L.ptc_set_camera_lens(pt._h, None) == 0                                       # NULL: the defaults
    assert pt.get_camera_lens() == pbr.ptc.lens_default_params()


def test_lifetime_is_the_cameras(pbr):
    L = pbr.load_library()
    lens = dict(aperture_radius=0.25, focus_distance=2.0, blades=5, rotation=0.5)
    pt = _ctx(pbr)
    pt.set_camera_lens(**lens)
    pt.set_camera((0, 0, 5), (0, 0, 0), 1.0, 1.0)
    assert pt.get_camera_lens() == lens                                                  # kept across ptc_set_camera
    assert L.ptc_scene_begin(pt._h) == 0
    assert pt.get_camera_lens() == pbr.ptc.lens_default_params()                         # reset with the camera
    desc = pbr.scenes.cornell_box()
    desc.camera.aperture_radius, desc.camera.focus_distance, desc.camera.blades, desc.camera.aperture_rotation = 0.25, 2.0, 5, 0.5
    g = pbr.Group([pbr.ptc.DEVICE_NONE, pbr.ptc.DEVICE_NONE])
    assert g.ctx(1).get_camera_lens() == pbr.ptc.lens_default_params()
    g.load_scene(desc)                                                                   # the description's camera carries the lens; the group commit copies it
    assert g.ctx(0).get_camera_lens() == lens and g.ctx(1).get_camera_lens() == lens
    g.close()


def test_rng_and_sincos_restatements_match_the_reference(pbr):
    """pcg, path_key, rng_f and sincos2pi of csrc/pt_lens.h through what exposes them: the disk sample (sqrt, sincos2pi) and the pinhole and lens rays
    (path_key, rng_f dimensions 0..3) are the reference's bit for bit — here on inputs chosen for the hash and the polynomial's branches."""
    u = np.concatenate([np.arange(0, 64, dtype=F32) / F32(64), F32([0.125, 0.375, 0.625, 0.875, ONE_M, 0.5 - 2.0 ** -25, 0.25 + 2.0 ** -24])])      # every octant, both sides of each swap
    got = pbr.ptc.lens_sample(np.full_like(u, 0.81), u, aperture_radius=1.0)
    lx, ly = ref.lens_point(1.0, 0, 0.0, np.full_like(u, 0.81), u)
    assert _same_bits(got[:, 0], lx) and _same_bits(got[:, 1], ly)
    s, c = ref.sincos2pi(u)
    assert np.abs(s - np.sin(2 * np.pi * u.astype(F64))).max() < 3e-7 and np.abs(c - np.cos(2 * np.pi * u.astype(F64))).max() < 3e-7
    for seed in (0, 1, 0xFFFFFFFF, 1 << 32, SEED):                                        # both halves of the seed reach the hash
        pt = _ctx(pbr)
        pt.set_camera_lens(0.3, 2.0)
        o, d = pt.debug_camera_rays(7, 5, seed, 0xFFFFFFF0, 4, [0, 34, 6])
        ro, rd, _ = ref.camera_rays(ref.camera_basis(_camera(pbr)), (0.3, 2.0, 0, 0.0), 7, 5, seed, 0xFFFFFFF0, 4, [0, 34, 6])
        assert _same_bits(o, ro) and _same_bits(d, rd), seed


def test_lens_sample_equals_reference_bit_for_bit(pbr):
    rng = np.random.default_rng(11)
    u = (rng.integers(0, 1 << 24, (4096, 2)).astype(F32) * F32(2.0 ** -24)).astype(F32)      # what rng_f returns: multiples of 2^-24 in [0, 1)
    corners = np.array([(a, b) for a in (0.0, ONE_M) for b in (0.0, ONE_M)], F32)        # the k = n - 1 clamp and quadrant 3 of sincos2pi
    u = np.concatenate([u, corners])
    for blades in BLADES:
        for rot in ROTATIONS if blades else (0.0,):
            for R in (1.0, 0.0371):
                got = pbr.ptc.lens_sample(u[:, 0], u[:, 1], aperture_radius=R, blades=blades, rotation=rot)
                lx, ly = ref.lens_point(R, blades, rot, u[:, 0], u[:, 1])
                assert _same_bits(got[:, 0], lx) and _same_bits(got[:, 1], ly), (blades, rot, R)
    L = pbr.load_library()
    xy = (C.c_float * 2)()
    p = pbr.ptc.PtcLensParams(1.0, 1.0, 0, 0.0)
    assert L.ptc_debug_lens_sample(C.byref(p), 1.0, 0.0, xy) == E_ARG and L.ptc_debug_lens_sample(C.byref(p), 0.0, -0.1, xy) == E_ARG
    assert L.ptc_debug_lens_sample(None, 0.5, 0.5, xy) == E_ARG and L.ptc_debug_lens_sample(C.byref(pbr.ptc.PtcLensParams(1.0, 1.0, 2, 0.0)), 0.5, 0.5, xy) == E_ARG


LENSES = {"pinhole": (0.0, 3.5, 0, 0.0), "disk": (0.15, 3.5, 0, 0.0), "hexagon": (0.15, 3.5, 6, 0.3)}


@pytest.mark.parametrize("name", list(LENSES))
def test_camera_rays_equal_reference_bit_for_bit(pbr, name):
    lens = LENSES[name]
    pt = _ctx(pbr)
    pt.set_camera_lens(*lens)
    basis = ref.camera_basis(_camera(pbr))
    scattered = np.random.default_rng(5).permutation(W * H)[:97]
    for pixels in (np.arange(W * H), scattered):
        o, d = pt.debug_camera_rays(W, H, SEED, FIRST, NS, pixels)
        ro, rd, _ = ref.camera_rays(basis, lens, W, H, SEED, FIRST, NS, pixels)
        assert o.shape == (NS * len(pixels), 3)
        assert _same_bits(o, ro) and _same_bits(d, rd), name
        assert np.abs(np.linalg.norm(d.astype(F64), axis=1) - 1).max() < 3e-7
    if lens[0] > 0:
        assert not _same_bits(o, np.broadcast_to(basis[0], o.shape))                     # the origins left the pinhole
    L = pbr.load_library()
    px = np.array([W * H], np.uint32)
    buf = np.zeros(3, F32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.ptc_debug_camera_rays(pt._h, W, H, 1, 0, 1, px.ctypes.data_as(C.POINTER(C.c_uint32)), 1, fp(buf), fp(buf)) == E_ARG      # pixel outside the frame
    assert L.ptc_debug_camera_rays(pt._h, W, H, 1, 0, 0, px.ctypes.data_as(C.POINTER(C.c_uint32)), 1, fp(buf), fp(buf)) == E_ARG
    nocam = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    px[0] = 0
    assert L.ptc_debug_camera_rays(nocam._h, W, H, 1, 0, 1, px.ctypes.data_as(C.POINTER(C.c_uint32)), 1, fp(buf), fp(buf)) == E_STATE


# ---- the geometry of the specification, in float64 ------------------------------------------------------------------------------------------------------
def _plane_points(basis, o, d, target):
    """Where the rays (o, d) meet the plane through `target` perpendicular to the forward axis, in float64."""
    f = basis[1].astype(F64)
    o, d = o.astype(F64), d.astype(F64)
    t = ((target - o) @ f) / (d @ f)
    return o + t[:, None] * d


@pytest.mark.parametrize("name", ["disk", "hexagon"])
def test_every_ray_of_a_sample_meets_the_focus_plane_in_the_pinhole_point(pbr, name):
    """F = 3.5, |pos| = 4.2.  The point is pos + F (s dvx + u dvy + f) whatever the lens point; the yardstick is the distance between where the float32 and
    the float64 evaluation of the reference meet the plane (about 7e-7 here), and the float32 rays may miss the exact point by 4x that."""
    lens = LENSES[name]
    basis = ref.camera_basis(_camera(pbr))
    pos, f, s, u = (basis[k].astype(F64) for k in range(4))
    pixels = np.arange(W * H)
    o32, d32, key = ref.camera_rays(basis, lens, W, H, SEED, FIRST, NS, pixels)
    o64, d64, _ = ref.camera_rays(basis, lens, W, H, SEED, FIRST, NS, pixels, dt=F64)
    pix = np.tile(pixels, NS)
    dvx, dvy = ref.slopes(basis, W, H, (pix % W).astype(F64), (pix // W).astype(F64), ref.rng_f(key, 0, 0), ref.rng_f(key, 0, 1), dt=F64)
    target = pos + F64(F32(lens[1])) * (dvx[:, None] * s + dvy[:, None] * u + f)
    p32, p64 = _plane_points(basis, o32, d32, target), _plane_points(basis, o64, d64, target)
    yard = np.linalg.norm(p32 - p64, axis=1).max()
    spec = np.linalg.norm(p64 - target, axis=1).max()
    err = np.linalg.norm(p32 - target, axis=1).max()
    print(f"{name}: float32 vs float64 on the focus plane {yard:.3e} ({yard / lens[1] * 2 ** 24:.2f} x 2^-24 F); float64 vs the pinhole point {spec:.3e}; float32 vs it {err:.3e}")
    assert spec <= 1e-12                                                                  # the specification itself: exact up to float64 rounding
    assert err <= 4 * yard
    assert np.linalg.norm(o32.astype(F64) - pos, axis=1).max() > 0.5 * lens[0]           # and the rays do start all over the aperture


def _second_moment(blades):
    return 0.5 if blades == 0 else (2.0 + math.cos(2 * math.pi / blades)) / 6.0


@pytest.mark.parametrize("blades", [0, 3, 6, 16])
@pytest.mark.parametrize("z", [1.5, 9.0])
def test_circle_of_confusion_off_the_focus_plane(pbr, blades, z):
    """One pixel centre, 65,536 lens samples: at view depth z the rays lie within R |1 - z / F| of the pinhole ray's point, and their mean squared distance
    from it is that radius squared times 1/2 (disk) or (2 + cos(2 pi / n)) / 6 (n-gon), within four standard errors of the sample mean.  Slack of the
    radius bound: 4x the float32-float64 gap of the reference on this plane, plus 2^-22 of the radius for the sincos polynomial (its unit vectors are
    unit to 2.5e-8 truncation + float32 rounding)."""
    R, F = 0.2, 3.5
    lens = (R, F, blades, 0.3 if blades else 0.0)
    basis = ref.camera_basis(_camera(pbr))
    pos, f, s, u = (basis[k].astype(F64) for k in range(4))
    n = 65536
    key = ref.path_key(ref.seed_hash(SEED), np.full(n, 5 * W + 11, np.uint64), np.arange(n, dtype=np.uint64))
    u1, u2 = ref.rng_f(key, 0, 2), ref.rng_f(key, 0, 3)
    dvx32, dvy32 = ref.slopes(basis, W, H, F32(11), F32(5), F32(0.5), F32(0.5))
    o32, d32 = ref.lens_ray(basis, lens, np.full(n, dvx32), np.full(n, dvy32), u1, u2)
    o64, d64 = ref.lens_ray(basis, lens, np.full(n, F64(dvx32)), np.full(n, F64(dvy32)), u1, u2, dt=F64)
    centre = pos + z * (F64(dvx32) * s + F64(dvy32) * u + f)                              # the pinhole ray at view depth z
    p32, p64 = _plane_points(basis, o32, d32, centre), _plane_points(basis, o64, d64, centre)
    yard = np.linalg.norm(p32 - p64, axis=1).max()
    rad = R * abs(1.0 - z / F)
    r = np.linalg.norm(p32 - centre, axis=1)
    print(f"blades {blades} z {z}: radius {rad:.6f}, largest distance {r.max():.9f}, float32 vs float64 {yard:.3e}")
    assert r.max() <= rad + 4 * yard + rad * 2.0 ** -22
    assert r.max() >= 0.97 * rad                                                          # the samples reach the rim (a vertex, for a polygon)
    sq = r * r
    want = rad * rad * _second_moment(blades)
    se = sq.std(ddof=1) / math.sqrt(n)
    print(f"   mean squared distance {sq.mean():.9e}, expected {want:.9e}, standard error {se:.3e}")
    assert abs(sq.mean() - want) <= 4 * se


@pytest.mark.parametrize("blades", [b for b in BLADES if b])
def test_polygon_samples_lie_inside_the_polygon(pbr, blades):
    """Apothem test per edge, slack one ulp of R.  The polygon is the one the specification draws: the union of its n fan triangles (centre, V_k, V_k+1)
    with the vertices at the turns t_k and t_k+1 AS THE SPECIFICATION ROUNDS THEM to float32 (a rotation is realised to about 2^-24 turn, 3.7e-7 rad: that
    is the resolution of the parameter, not an error of the sampling).  Edge k is held against the exact line through exact vertices at those turns
    (float64 sines and cosines): a sample of fan triangle k satisfies n_k . p <= R n_k . V_k + ulp(R); the two other sides of the triangle are radii.  No
    sample is further than R + ulp(R) from the centre either."""
    rng = np.random.default_rng(blades)
    u = (rng.integers(0, 1 << 24, (65536, 2)).astype(F32) * F32(2.0 ** -24)).astype(F32)
    u = np.concatenate([u, np.array([(a, b) for a in (0.0, ONE_M) for b in (0.0, ONE_M)], F32)])
    k = np.minimum((u[:, 0] * F32(blades)).astype(np.int32), blades - 1)
    for rot in ROTATIONS:
        t = [F32(rot) + (k + j).astype(F32) / F32(blades) for j in (0, 1)]
        V = [np.stack([np.cos(2 * np.pi * (tj - np.floor(tj)).astype(F64)), np.sin(2 * np.pi * (tj - np.floor(tj)).astype(F64))], -1) for tj in t]
        e = V[1] - V[0]
        normal = np.stack([e[:, 1], -e[:, 0]], -1) / np.linalg.norm(e, axis=1)[:, None]      # outward: the vertices run counter-clockwise
        assert ((normal * V[0]).sum(-1) > 0).all()
        for R in (1.0, 0.15):
            lx, ly = ref.lens_point(R, blades, rot, u[:, 0], u[:, 1])
            p = np.stack([lx, ly], -1).astype(F64)
            over = ((normal * p).sum(-1) - F64(F32(R)) * (normal * V[0]).sum(-1)).max()
            far = np.linalg.norm(p, axis=1).max()
            print(f"blades {blades} rotation {rot} R {R}: furthest outside its edge {over:.3e}, furthest from the centre {far - F64(F32(R)):.3e}, one ulp of R {np.spacing(F32(R)):.3e}")
            assert over <= np.spacing(F32(R))
            assert far <= F64(F32(R)) + np.spacing(F32(R))
            assert far >= 0.98 * R                                                        # and they reach the vertices


def test_cli_refuses_bad_lens_arguments_before_any_device_work(pbr):
    """ptc_render --focus with --focus-pixel, and values ptc_set_camera_lens would refuse: exit code 1 and the reason, on a machine without a GPU too."""
    import subprocess

    exe = os.path.join(os.path.dirname(pbr.ptc.LIB_PATH), "ptc_render")
    for args, text in ((["--aperture", "0.1", "--focus", "3", "--focus-pixel", "2,2"], "exclude each other"), (["--aperture", "-1"], "--aperture"),
                       (["--aperture", "0.1", "--focus", "0"], "--focus"), (["--aperture", "0.1", "--blades", "2"], "--blades"),
                       (["--aperture", "0.1", "--blades", "5", "--aperture-rotation", "1"], "--aperture-rotation"),
                       (["--aperture", "0.1", "--focus-pixel", "64,3", "--width", "64", "--height", "64"], "--focus-pixel"),
                       (["--aperture", "0.1", "--raster"], "path integrator")):
        r = subprocess.run([exe, "--scene", "cornell"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and text in r.stderr and "ptc_create" not in r.stderr, (args, r.stderr)
