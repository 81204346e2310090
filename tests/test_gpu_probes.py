"""Light probes on a real MI355X (include/ptc.h: ptc_probes_begin, ptc_probes_read_sh, ptc_render_probes; csrc/pt_probes.hip).

1. The kernels against the definition: k_raygen_probe and k_accumulate_sh through the debug hooks against tests/probes_reference.py, bit for bit.
2. The frame against its own samples: a 16-sample frame returns exactly the projection, in sample order, of the 16 one-sample frames' radiance.
3. However the samples are cut — calls, batches, lanes, probe shards — the coefficients are bit for bit the same.
4. Closed forms at 4096 samples within 5 standard errors (float64, computed here): a furnace, one emitting face of a cube per axis and sign, a half-lit sky.
5. Neighbours: camera frames around a probe frame, punctual lights, the refusals of a probe frame, the kernel hash."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probes_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
E_ARG, E_STATE = -1, -2
SEED = 0x5EED0FC0FFEE1234
N_CF = 4096      # samples of the closed-form tests


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _grid_probes():
    """65 probes on a jittered 5 x 13 grid well inside the Cornell box [-1, 1]^3."""
    rng = np.random.default_rng(65)
    gx, gz = np.meshgrid(np.linspace(-0.7, 0.7, 13), np.linspace(-0.6, 0.6, 5))
    P = np.stack([gx.ravel(), np.linspace(-0.7, 0.7, 65), gz.ravel()], -1) + rng.uniform(-0.05, 0.05, (65, 3))
    return P.astype(F32)


@pytest.fixture(scope="module")
def cornell(gpu):
    pt = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    yield pt
    pt.close()


@pytest.fixture(scope="module")
def whole(cornell):
    """The 65 probes of the Cornell box, 16 samples, 3 bounces, in one call: the result everything in 2 and 3 must reproduce.  Computed once, never written to."""
    sh = cornell.render_probes(_grid_probes(), 16, seed=SEED, max_bounces=3)
    sh.setflags(write=False)
    return sh


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 513])
def test_kernels_equal_reference_bit_for_bit(cornell, n):
    """One thread per path (raygen); a block per 8 probes that walks the samples 32 at a time (projection).  The probe counts sit on and around a wave and are no
    multiples of 8 (513 probes: 65 blocks, the last with one probe); 1, 2 and 5 samples are partial tiles, 32 is one whole tile, 70 is two and a partial one.  The
    projection starts once from zero and once from the sums of an earlier batch."""
    pt = cornell
    rng = np.random.default_rng(n)
    P = rng.uniform(-3, 3, (n, 3)).astype(F32)
    for ns in (1, 2, 5) + ((32, 70) if n in (1, 65) else ()):
        first, base = 7 * ns, 1000 * (ns - 1)
        o, d, key = pt.debug_probe_rays(P, SEED, first, ns, index_base=base)
        ro, rd, rkey = ref.probe_rays(P, base, SEED, first, ns)
        assert _bits_equal(o, ro) and _bits_equal(d, rd) and np.array_equal(key, rkey), (n, ns)
        L = rng.normal(0, 2, (n * ns, 4)).astype(F32)
        L[::5, :3] = 0
        L[1::7, :3] *= F32(1e-41)                                      # denormals
        acc = pt.debug_probe_project(n, SEED, first, ns, L, index_base=base)
        assert _bits_equal(acc, ref.project(n, base, SEED, first, ns, L)), (n, ns)
        L2 = rng.normal(0, 2, (n * ns, 4)).astype(F32)
        acc2 = pt.debug_probe_project(n, SEED, first + ns, ns, L2, acc=acc, index_base=base)      # from a non-zero acc: accumulation continues across batches
        assert _bits_equal(acc2, ref.project(n, base, SEED, first, 2 * ns, np.concatenate([L, L2]))), (n, ns)


# ---- 2. the frame against its own samples -------------------------------------------------------------------------------------------------------------------
def test_frame_is_the_projection_of_its_samples(cornell, whole):
    """A one-sample frame at sample index s resolves to that sample (x / 1 = x), so its n x 1 radiance image is L_s of every probe."""
    pt, P = cornell, _grid_probes()
    n = len(P)
    Ls = []
    for s in range(16):
        pt.probes_begin(P, 1, seed=SEED, max_bounces=3)
        pt.frame_set_sample_range(s, 0)
        pt.frame_add_samples(1)
        pt.frame_resolve()
        img = pt.read_radiance()
        assert img.shape == (1, n, 4)
        Ls.append(img[0])
    Ls = np.concatenate(Ls)                                                # path order: sample-major
    assert np.isfinite(Ls).all() and (Ls[:, :3] > 0).mean() > 0.5         # the box is lit
    want = ref.resolve(ref.project(n, 0, SEED, 0, 16, Ls), 16)
    assert _bits_equal(whole, want)
    # and the plain per-probe mean of the 16-sample frame is the sum of those samples in order, over 16
    pt.probes_begin(P, 16, seed=SEED, max_bounces=3)
    pt.frame_add_samples(16)
    pt.frame_resolve()
    mean = pt.read_radiance()[0, :, :3]
    acc = np.zeros((n, 3), F32)
    for s in range(16):
        acc = acc + Ls[s * n:(s + 1) * n, :3]
    assert _bits_equal(mean, acc / F32(16))
    assert _bits_equal(pt.read_probes_sh(), whole)                         # reading the image did not disturb the sums


# ---- 3. however the samples are cut -------------------------------------------------------------------------------------------------------------------------
def _bake_in_steps(pt, P, steps, sync):
    pt.probes_begin(P, 16, seed=SEED, max_bounces=3)
    for k in steps:
        pt.frame_add_samples(k)
        if sync:
            pt.sync()
    return pt.read_probes_sh()


def test_sample_splits_leave_the_result_unchanged(cornell, whole):
    P = _grid_probes()
    assert _bits_equal(_bake_in_steps(cornell, P, [16], False), whole)
    assert _bits_equal(_bake_in_steps(cornell, P, [5, 11], False), whole)          # a held-back remainder merges with the next call
    assert _bits_equal(_bake_in_steps(cornell, P, [1] * 16, True), whole)          # sixteen batches of one sample
    # partial results are the projection so far: N is the samples accumulated
    cornell.probes_begin(P, 16, seed=SEED, max_bounces=3)
    cornell.frame_add_samples(4)
    part = cornell.read_probes_sh()
    cornell.frame_add_samples(12)
    assert _bits_equal(cornell.read_probes_sh(), whole) and not _bits_equal(part, whole)


@pytest.mark.parametrize("env", [dict(PTC_BATCH_PATHS="1024"), dict(PTC_LANES="2"), dict(PTC_LANES="2", PTC_BATCH_PATHS="1024")], ids=["small_batches", "two_lanes", "two_lanes_small_batches"])
def test_batches_and_lanes_leave_the_result_unchanged(gpu, whole, env):
    """PTC_BATCH_PATHS=1024: 15 samples of 65 probes per batch on one lane, 7 on each of two — the frame spans two or three batches, which alternate between
    the lanes; the SH sums stay in sample order behind the same event as k_accumulate's."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pt = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    got = pt.render_probes(_grid_probes(), 16, seed=SEED, max_bounces=3)
    pt.close()
    assert _bits_equal(got, whole)


def test_probe_shards_concatenate_to_the_whole(cornell, whole):
    P = _grid_probes()
    a = cornell.render_probes(P[:40], 16, seed=SEED, max_bounces=3, index_base=0)
    b = cornell.render_probes(P[40:], 16, seed=SEED, max_bounces=3, index_base=40)
    assert a.shape == (40, 9, 3) and b.shape == (25, 9, 3)
    assert _bits_equal(np.concatenate([a, b]), whole)
    assert not _bits_equal(cornell.render_probes(P[40:], 16, seed=SEED, max_bounces=3), whole[40:])      # the base is what makes them equal
    # sample-range shards: partial coefficients with the whole frame's divisor; the first is what the whole frame held after 8 samples
    cornell.probes_begin(P, 8, seed=SEED, max_bounces=3)
    cornell.frame_set_sample_range(0, 16)
    cornell.frame_add_samples(8)
    lo = cornell.read_probes_sh()
    cornell.probes_begin(P, 16, seed=SEED, max_bounces=3)
    cornell.frame_add_samples(8)
    assert _bits_equal(lo, (cornell.read_probes_sh() * F32(0.5)).astype(F32))       # 4 pi / 16 is half of 4 pi / 8, exactly


# ---- 4. closed forms ----------------------------------------------------------------------------------------------------------------------------------------
def _cube(pbr, emit, Le=(2.0, 1.0, 0.5)):
    """[-1, 1]^3 of 12 triangles, every face's front towards the inside, albedo 0; the faces whose name is in `emit` ('+x', '-y', ...) emit Le."""
    S = pbr.scene
    mats = [S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0), S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, tuple(Le))]
    meshes = []
    for axis in range(3):
        for sign in (1, -1):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            c = []
            for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = [0.0, 0.0, 0.0]
                p[axis], p[u], p[v] = float(sign), float(su), float(sv)
                c.append(p)
            nrm = np.cross(np.subtract(c[1], c[0]), np.subtract(c[2], c[0]))
            if nrm[axis] * sign > 0:                                       # the front must look at the centre
                c = c[::-1]
            vq, iq = pbr.scenes._quad(*c)
            assert vq["normal"][0][axis] * sign < 0
            meshes.append(S.MeshDesc(vq, iq, 1 if ("+-"[sign < 0] + "xyz"[axis]) in emit else 0))
    cam = S.CameraDesc((0.0, 0.0, 0.5), (0.0, 0.0, 0.0), 1.0, 1.0)
    return S.SceneDesc(mats, meshes, [S.InstanceDesc(k) for k in range(6)], cam, "probe_cube")


ALL_FACES = ("+x", "-x", "+y", "-y", "+z", "-z")


def test_furnace(gpu):
    """Every direction sees Le: each sample's L is Le exactly, coef_0 is a float32 running sum of N equal terms (worst case (N + 2) 2^-24 relative with the two
    roundings of the term and the resolve), every other coefficient estimates 0 with the variance 4 pi Le^2 int Y_k^2 / N = 4 pi Le^2 / N."""
    Le = np.array([2.0, 1.0, 0.5])
    pt = gpu.PathTracer(0).load_scene(_cube(gpu, ALL_FACES, Le))
    P = np.random.default_rng(1).uniform(-0.9, 0.9, (8, 3)).astype(F32)
    sh = pt.render_probes(P, N_CF, seed=SEED, max_bounces=0).astype(F64)
    pt.frame_resolve()
    assert np.array_equal(pt.read_radiance()[0, :, :3].astype(F64), np.broadcast_to(Le, (8, 3)))       # the mean of N equal samples
    pt.close()
    want0 = 2 * math.sqrt(math.pi) * Le
    err0 = np.abs(sh[:, 0] - want0).max(0)
    rest = np.abs(sh[:, 1:]).max((0, 1))
    print(f"furnace: |coef_0 - 2 sqrt(pi) Le| / (2 sqrt(pi) Le) = {err0 / want0} (bound {(N_CF + 2) * 2.0 ** -24:.3e}); max |coef_k| / (Le sqrt(4 pi / N)) = {rest / (Le * math.sqrt(4 * math.pi / N_CF))} (bound 5)")
    assert (err0 <= want0 * (N_CF + 2) * 2.0 ** -24).all()
    assert (rest <= 5 * Le * math.sqrt(4 * math.pi / N_CF)).all()


def _face_quadrature(axis, sign, m=768):
    """int Y_k dw and int Y_k^2 dw over the face `sign axis = 1` of the cube seen from its centre, float64, midpoint rule on m x m cells:
    dw = du dv / (1 + u^2 + v^2)^(3/2)."""
    t = (np.arange(m) + 0.5) / m * 2 - 1
    u, v = np.meshgrid(t, t, indexing="ij")
    r2 = 1 + u * u + v * v
    dw = (2.0 / m) ** 2 / r2 ** 1.5
    d = np.zeros(u.shape + (3,))
    d[..., axis], d[..., (axis + 1) % 3], d[..., (axis + 2) % 3] = sign, u, v
    d /= np.sqrt(r2)[..., None]
    Y = ref.basis64(d)
    return (Y * dw[..., None]).sum((0, 1)), (Y * Y * dw[..., None]).sum((0, 1)), dw.sum()


@pytest.mark.parametrize("face", ALL_FACES)
def test_one_emitting_face(gpu, face):
    """The estimator of coef_k is the mean of X = 4 pi L(w) Y_k(w) over uniform w: E X = Le int_face Y_k, E X^2 = 4 pi Le^2 int_face Y_k^2.  The linear coefficient
    of the face's axis has the face's sign, the two others are 0, and the band-2 terms have the signs of the axis: which coefficient is which axis, and every sign."""
    Le = np.array([2.0, 1.0, 0.5])
    axis, sign = "xyz".index(face[1]), 1 if face[0] == "+" else -1
    pt = gpu.PathTracer(0).load_scene(_cube(gpu, (face,), Le))
    sh = pt.render_probes(np.zeros((1, 3), F32), N_CF, seed=SEED, max_bounces=0)[0].astype(F64)
    pt.close()
    I1, I2, area = _face_quadrature(axis, sign)
    assert abs(area - 4 * math.pi / 6) < 1e-6
    mean = I1[:, None] * Le
    se = np.sqrt(np.maximum(4 * math.pi * I2[:, None] * Le ** 2 - mean ** 2, 0) / N_CF)
    z = np.abs(sh - mean) / se
    print(f"face {face}: coefficients (red) {sh[:, 0] / Le[0]}\n   expected {I1}\n   |error| / standard error {z.max(1)}")
    assert (z <= 5).all()
    k_axis = {1: 1, 2: 2, 0: 3}[axis]                                     # band 1 is ordered y, z, x
    assert sign * I1[k_axis] > 0.6                                         # 0.4886 int_face |axis| dw
    assert (sign * sh[k_axis] > 0.5 * Le).all()                            # the right axis, the right sign, many standard errors from 0
    for k in (1, 2, 3):
        if k != k_axis:
            assert abs(I1[k]) < 1e-12


def _sphere_moments(Lfun, weights, my=512, mphi=1024):
    """Mean and standard deviation over uniform directions of X = 4 pi L(w) sum_k weights_k Y_k(w), float64, on an equal-area grid whose polar axis is y (the
    boundary y = 0 of the half-lit sky is a cell boundary)."""
    y = ((np.arange(my) + 0.5) / my * 2 - 1)[:, None]
    phi = ((np.arange(mphi) + 0.5) / mphi * 2 * math.pi)[None, :]
    s = np.sqrt(1 - y * y)
    d = np.stack([s * np.cos(phi), np.broadcast_to(y, (my, mphi)), s * np.sin(phi)], -1)
    X = 4 * math.pi * Lfun(d) * (ref.basis64(d) @ np.asarray(weights, F64))
    return X.mean(), math.sqrt(max((X * X).mean() - X.mean() ** 2, 0.0))


def test_half_lit_sky(gpu):
    """A 1 x 2 lat-long map (the upper row L, the lower row 0) is the radiance 'L for y > 0, else 0' exactly.  coef_0 = sqrt(pi) L, coef_1 = 0.4886025 pi L, the
    rest 0; int_{y>0} Y_k^2 = 1/2 for every k, so E X^2 = 2 pi L^2.  The irradiance is linear in the samples: its standard error comes from the same quadrature."""
    S = gpu.scene
    Lr = np.array([3.0, 1.5, 0.75])
    tri = gpu.scenes._verts([(-1, -50, -1), (1, -50, -1), (0, -50, 1)], [(0, 1, 0)] * 3, [(1, 0, 0)] * 3, [(0, 0), (1, 0), (0, 1)])
    desc = S.SceneDesc([S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0)], [S.MeshDesc(tri, np.array([0, 1, 2], np.uint32), 0)], [S.InstanceDesc(0)],
                       S.CameraDesc((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), 1.0, 1.0), "half_lit_sky")
    desc.env = np.array([[Lr], [np.zeros(3)]], F32)                        # (h, w, 3) = (2, 1, 3), row 0 = +y
    pt = gpu.PathTracer(0).load_scene(desc)
    P = np.random.default_rng(2).uniform(-1, 1, (8, 3)).astype(F32)
    sh = pt.render_probes(P, N_CF, seed=SEED, max_bounces=0)
    pt.close()
    pi = math.pi
    mean = np.zeros((9, 3))
    mean[0], mean[1] = math.sqrt(pi) * Lr, 0.5 * math.sqrt(3 * pi) * Lr
    se = np.sqrt((2 * pi * Lr ** 2 - mean ** 2) / N_CF)
    z = np.abs(sh.astype(F64) - mean) / se
    print(f"half-lit sky: largest |error| / standard error per coefficient {z.max((0, 2))}")
    assert (z <= 5).all()
    half = lambda d: (d[..., 1] > 0).astype(F64)
    for nrm, want in (((0, 1, 0), pi), ((0, -1, 0), 0.0)):
        w = ref.BAND_A.astype(F64) * ref.basis64(np.array(nrm, F64))
        m, sd = _sphere_moments(half, w)
        assert abs(m - want) < 2e-3                                        # the quadrature reproduces pi L and 0 (band-limited to l <= 2: exact up to the grid)
        E = gpu.ptc.sh9_irradiance(sh, np.array(nrm, F32)).astype(F64)
        print(f"   irradiance for n = {nrm}: {E[:, 0] / Lr[0]} (expected {want:.6f}, standard error {sd / math.sqrt(N_CF):.4f})")
        assert (np.abs(E - want * Lr) <= 5 * sd / math.sqrt(N_CF) * Lr).all()


# ---- 5. neighbours ------------------------------------------------------------------------------------------------------------------------------------------
def test_camera_frames_around_a_probe_frame(gpu, cornell, whole):
    before = cornell.render(48, 32, 4, seed=9, max_bounces=3)
    assert _bits_equal(cornell.render_probes(_grid_probes(), 16, seed=SEED, max_bounces=3), whole)
    after = cornell.render(48, 32, 4, seed=9, max_bounces=3)
    assert after.shape == (32, 48, 4) and _bits_equal(before, after)
    fresh = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())             # a context that never baked
    assert _bits_equal(fresh.render(48, 32, 4, seed=9, max_bounces=3), after)
    fresh.close()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):                    # the camera frame left probe mode
        cornell.read_probes_sh()


def test_punctual_light_reaches_the_probes_and_leaves_again(cornell, whole):
    P = _grid_probes()
    cornell.add_light(type="point", position=(0.3, 0.2, 0.1), intensity=(4.0, 3.0, 2.0))
    lit = cornell.render_probes(P, 16, seed=SEED, max_bounces=3)
    cornell.clear_lights()
    assert not _bits_equal(lit, whole) and (lit[:, 0] >= whole[:, 0]).all() and (lit[:, 0] > whole[:, 0]).mean() > 0.9      # bounced light only adds
    assert _bits_equal(cornell.render_probes(P, 16, seed=SEED, max_bounces=3), whole)


def test_refusals_in_a_probe_frame(gpu, cornell, whole):
    """PTC_E_STATE, and the frame goes on as if nothing had been called."""
    L, pt, P = gpu.load_library(), cornell, _grid_probes()
    h = pt._h
    out = np.zeros((65, 9, 3), F32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    pt.render(16, 16, 1, seed=1, max_bounces=1)
    assert L.ptc_probes_read_sh(h, fp) == E_STATE and b"probes_read_sh" in L.ptc_last_error(h)      # outside a probe frame
    assert L.ptc_probes_begin(h, P.ctypes.data_as(C.POINTER(C.c_float)), 0, 0, 16, 1, 3) == E_ARG
    pt.frame_resolve()                                                         # PTC_E_ARG changed nothing: the camera frame is still the frame
    pt.probes_begin(P, 16, seed=SEED, max_bounces=3)
    pt.frame_add_samples(5)
    n64, u32, f1 = C.c_uint64(0), C.c_uint32(0), C.c_float(0)
    px = np.zeros(1, np.uint32)
    calls = {
        "frame_guides": lambda: L.ptc_frame_guides(h),
        "set_sample_covariance": lambda: L.ptc_set_sample_covariance(h, 1),
        "frame_set_adaptive": lambda: L.ptc_frame_set_adaptive(h, None),
        "frame_adapt": lambda: L.ptc_frame_adapt(h, C.byref(n64)),
        "denoise": lambda: L.ptc_denoise(h, None),
        "denoise_sampled": lambda: L.ptc_denoise_sampled(h, None),
        "denoise_accumulated": lambda: L.ptc_denoise_accumulated(h, None),
        "temporal_accumulate": lambda: L.ptc_temporal_accumulate(h, None),
        "frame_checkpoint": lambda: L.ptc_frame_checkpoint(h, None, C.byref(n64), C.byref(u32)),
        "frame_restore": lambda: L.ptc_frame_restore(h, fp, 65, 0),
        "comm_reduce_radiance": lambda: L.ptc_comm_reduce_radiance(h, 0),
        "focus_distance_at_pixel": lambda: L.ptc_focus_distance_at_pixel(h, 0, 0, C.byref(f1)),
        "debug_camera_rays": lambda: L.ptc_debug_camera_rays(h, 4, 4, 1, 0, 1, px.ctypes.data_as(C.POINTER(C.c_uint32)), 1, fp, fp),
    }
    for name, call in calls.items():
        assert call() == E_STATE, name
    assert L.ptc_set_sample_covariance(h, 0) == 0                              # switching it off is no request for statistics
    pt.frame_add_samples(11)
    assert _bits_equal(pt.read_probes_sh(), whole) and not out.any()
    assert L.ptc_frame_add_samples(h, 1) == E_ARG                              # the budget of ptc_probes_begin holds, as in any frame
    st = pt.stats()
    assert st["paths"] == 65 * 16
    # the refused ptc_set_sample_covariance(1) left the setting off: an adaptive frame begun now keeps no covariance
    assert L.ptc_probes_begin(h, None, 65, 0, 16, 1, 3) == E_ARG and b"probes_begin" in L.ptc_last_error(h)
    pt.frame_begin(16, 16, 4, seed=1, max_bounces=1)
    pt.frame_set_adaptive()
    assert L.ptc_read_sample_covariance(h, fp) == E_STATE


def test_kernel_hash_is_the_profiled_one(gpu):
    """The hashed kernel sources are untouched: ptc_build_info reports the hash the committed kernel models were measured on."""
    sha = gpu.load_library().ptc_build_info().decode().split()[-1]
    for f in ("r04_kernel_model.json", "r04_textured_kernel_model.json"):      # the two models bench.py uses (tests/test_profiles.py)
        assert json.load(open(os.path.join(ROOT, "profiles", f)))["kernel_source_sha256"] == sha, f


def test_cli_bakes_a_probe_grid(gpu, tmp_path):
    """ptc_render --probe-grid 2,2,2 on the Cornell box [-1, 1]^3: the cell centres are (+-0.5, +-0.5, +-0.5), x fastest; a 9 x 8 RGB PFM whose row j is probe j —
    the bytes ptc_render_probes returns for those positions."""
    import subprocess

    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    out = str(tmp_path / "sh.pfm")
    r = subprocess.run([exe, "--scene", "cornell", "--probe-grid", "2,2,2", "--probes-out", out, "--spp", "16", "--seed", "7", "--bounces", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    head = json.loads(r.stdout.splitlines()[0])
    assert head["probe_grid"] == [2, 2, 2] and np.allclose(head["origin"], [-1, -1, -1], atol=1e-6) and np.allclose(head["cell"], [1, 1, 1], atol=1e-6)
    raw = open(out, "rb").read()
    magic, size, scale, body = raw.split(b"\n", 3)
    assert magic == b"PF" and size == b"9 8" and float(scale) < 0 and len(body) == 9 * 8 * 12
    sh = np.frombuffer(body, "<f4").reshape(8, 9, 3)[::-1]                 # PFM stores the bottom row first
    assert np.isfinite(sh).all() and (sh[:, 0] > 0).all()
    lo, cell = np.array(head["origin"], F32), np.array(head["cell"], F32)   # %.9g round-trips a float32; the positions as the CLI forms them
    P = np.array([lo + (np.array([x, y, z], F32) + F32(0.5)) * cell for z in range(2) for y in range(2) for x in range(2)], F32)
    assert np.array_equal(P, np.array([(x, y, z) for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], F32))
    pt = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    assert _bits_equal(sh, pt.render_probes(P, 16, seed=7, max_bounces=3))
    pt.close()


CPP_MIRROR = r"""
#include "pbr_pt.hpp"
#include <cstdio>
#include <cstring>
int main() {
  pbr::PathTraceRenderSystem rs(0);
  rs.beginScene();
  const int white = rs.addMaterial({{0.7f, 0.7f, 0.7f, 1}, 0, 1, {0, 0, 0}}), light = rs.addMaterial({{0, 0, 0, 1}, 0, 1, {5, 5, 5}});
  pbr::MeshBuilder mb;
  auto quad = [](float y, float e, int m) {
    pbr::MeshBuilder::Primitive p;
    const float P[4][3] = {{-e, y, -e}, {e, y, -e}, {e, y, e}, {-e, y, e}};
    for (auto& q : P) { pbr::MeshVertex v{}; v.position = {q[0], q[1], q[2]}; v.normal = {0, y > 0 ? -1.0f : 1.0f, 0}; v.tangent = {1, 0, 0, 1}; p.vertices.push_back(v); }
    p.indices = y > 0 ? std::vector<std::uint32_t>{0, 1, 2, 0, 2, 3} : std::vector<std::uint32_t>{0, 2, 1, 0, 3, 2};
    p.material = m;
    return p;
  };
  mb.addPrimitive(quad(-1.0f, 2.0f, white));
  mb.addPrimitive(quad(1.0f, 0.5f, light));
  for (int m : rs.addMesh(mb.build())) rs.addInstance(m, pbr::Transform{});
  rs.setCamera({0, 0, 3}, {0, 0, 0}, 1.0f, 1.0f);
  rs.commitScene();
  bool threw = false;
  try { rs.readProbesSh(); } catch (std::exception const&) { threw = true; }      // nothing begun: no guess at a size
  std::vector<float> few(3 * 10, 0.0f), many(3 * 1000, 0.0f);
  for (std::size_t i = 0; i < 1000; ++i) many[i * 3] = -0.9f + 0.0018f * (float)i;
  rs.beginProbes(few, 4, 9, 2);
  const std::vector<float> a = rs.renderProbes(many, 4, 9, 2);      // leaves a 1000-probe frame in progress
  const std::vector<float> b = rs.readProbesSh();                   // ... which this must be sized for
  const bool same = a.size() == 27000 && b.size() == a.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
  std::printf("threw %d sizes %zu %zu same %d coef0 %g\n", (int)threw, a.size(), b.size(), (int)same, (double)a[0]);
  return threw && same && a[0] > 0.0f ? 0 : 1;
}
"""


def test_cpp_mirror_sizes_the_read_by_the_frame_in_progress(gpu, tmp_path):
    """host/pbr_pt.hpp: readProbesSh() after renderProbes(1000 probes), with an earlier beginProbes(10 probes): 27,000 floats, the bytes renderProbes returned;
    and it throws before anything was begun."""
    import subprocess

    src, exe = tmp_path / "mirror.cpp", str(tmp_path / "mirror")
    src.write_text(CPP_MIRROR)
    lib = os.path.dirname(gpu.ptc.LIB_PATH)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "physically-based-renderer_amd", "host"), str(src), "-o", exe,
                        "-L" + lib, "-lptc", "-Wl,-rpath," + lib], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "threw 1 sizes 27000 27000 same 1" in r.stdout, r.stdout + r.stderr
