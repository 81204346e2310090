"""Temporal accumulation on a real MI355X (include/ptc.h: ptc_temporal_accumulate, ptc_temporal_reset, ptc_read_temporal_rgba32f,
ptc_denoise_accumulated, PTC_OUTPUT_ACCUMULATED).  Every step is held against the specification evaluated in numpy (tests/temporal_reference.py) FROM THE
LIBRARY'S OWN PREVIOUS STATE, in float64, with the float32-float64 gap of that same evaluation as the yardstick; the rest are exact properties (the copies
the specification asks for), the lifetime of the history, an untouched frame, and that sixteen accumulated frames are worth sixteen samples."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dref  # noqa: E402
import temporal_reference as tref  # noqa: E402
from test_temporal_host import CASES, FRAGILE_CAP, MOVED_Q, MOVED_T, moved_camera  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "segments", "shadow_rays", "hits", "node_visits_closest", "tri_tests_closest", "node_visits_any", "tri_tests_any", "algorithmic_bytes")
BUFFERS = ("history", "moments", "motion")


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _load(gpu, name, w, h):
    d = gpu.scenes.by_name(name)
    d.camera.aspect = w / h
    return d, gpu.PathTracer(0).load_scene(d)


def _frame(pt, w, h, seed, noise=None, spp=1):
    """A resolved frame with guides; `noise`: a generator whose white noise replaces the radiance.  Returns (radiance, (albedo_class, normal_depth, prim, uv))."""
    pt.frame_begin(w, h, spp, seed=seed, max_bounces=6)
    pt.frame_add_samples(spp)
    pt.frame_guides()
    pt.frame_resolve()
    if noise is not None:
        img = np.ones((h, w, 4), np.float32)
        img[..., :3] = 2.0 * noise.random((h, w, 3), np.float32)
        pt.write_radiance(img)
    prim, uv = pt.read_guide_hit()
    return pt.read_radiance(), (pt.read_guide(0), pt.read_guide(1), prim, uv)


def _read_state(pt):
    return {k: pt.read_temporal(i) for i, k in enumerate(BUFFERS)}


def _accumulated(pt):
    pt.select_output(2)
    img = pt.read_radiance()
    pt.select_output(0)
    return img


def _positions(pt):
    """(n_tris, 3, 3): the first three float4 of every shading record as they lie in HBM."""
    shade = pt.shading_tables()[0]
    return np.ascontiguousarray(shade.reshape(shade.shape[0], -1, 4)[:, :3, :3])


def _hold_step(label, pt, rad, guides, prev, params):
    """One accumulate against the reference.  Returns (the new previous-state ingredients, worst ratio, the float64 evaluation)."""
    ak, nz, prim, uv = guides
    pt.temporal_accumulate(**params)
    got = _read_state(pt)
    got["accumulated"] = _accumulated(pt)
    e64, e32 = (tref.accumulate(rad[..., :3], ak, nz, prim, uv, prev, dt=dt, **params) for dt in (np.float64, np.float32))
    surf = ak[..., 3] == 1
    left_out = (e64["fragile"] | e32["fragile"]) & surf
    share = float(left_out.sum()) / surf.sum()
    keep = surf & ~left_out
    worst = 0.0
    line = []
    for k in BUFFERS + ("accumulated",):
        g = got[k][..., :3] if k == "accumulated" else got[k]
        top = 1.0 if k == "motion" else float(np.abs(e64[k]).max())                       # motion: the unit is the pixel
        E32 = float(np.abs(e32[k].astype(np.float64) - e64[k])[keep].max()) / top
        err = float(np.abs(g.astype(np.float64) - e64[k])[keep].max()) / top
        ratio = err / E32 if E32 > 0 else (0.0 if err == 0 else math.inf)
        line.append(f"{k} E32 {E32:.3g} error {err:.3g} ratio {ratio:.2f}")
        worst = max(worst, ratio)
        assert err <= 16 * E32, (label, k, err, E32)
    print(f"{label}: left out {share:.5f}, valid history {float(e64['valid'].sum()) / surf.sum():.3f}; " + "; ".join(line))
    assert share <= FRAGILE_CAP, (label, share)
    assert np.array_equal(got["accumulated"][..., 3], rad[..., 3])                        # alpha from the radiance
    return got, worst, e64


@pytest.mark.parametrize("name,w,h,how", [c + ("refit",) for c in CASES] + [("sphere10k", 96, 64, "rebuild")])
def test_steps_are_the_specified_ones(gpu, name, w, h, how):
    """Three accumulates — first frame, unmoved, moved (camera, and instance 3 of the sphere scenes through a refit or a rebuild) — of a rendered 1-spp
    radiance and of seeded white noise, with demodulation on and off: over the class-1 pixels outside the fragile mask all four channels of HISTORY,
    MOMENTS, MOTION and of the accumulated image lie within 16 x E32 of the float64 evaluation, E32 = the float32-float64 gap of the reference over the
    same pixels relative to the buffer's maximum (MOTION: in pixels).  At most 1 % of the class-1 pixels are left out."""
    d, pt = _load(gpu, name, w, h)
    cam0, cam1 = d.camera, moved_camera(d.camera)
    it = d.instances[3] if name != "cornell" else None
    worst = 0.0
    for noise in (False, True):
        for demod in (1, 0):
            params = dict(max_history=32, sigma_z=1.0, demodulate=demod)
            rng = np.random.default_rng(17) if noise else None
            pt.temporal_reset()
            pt.set_camera(cam0.position, cam0.target, cam0.fov_y, cam0.aspect)
            if it is not None:
                pt.update_instance(3, it.t, it.q_wxyz, it.s).scene_refit()
            tri = _positions(pt)
            prev = None
            for step, seed in (("first", 1), ("unmoved", 2), ("moved", 3)):
                cam = cam0
                if step == "moved":
                    cam = cam1
                    pt.set_camera(cam1.position, cam1.target, cam1.fov_y, cam1.aspect)
                    if it is not None:
                        pt.update_instance(3, MOVED_T, MOVED_Q, (1.0, 1.0, 1.0))
                        getattr(pt, "scene_" + how)()
                rad, guides = _frame(pt, w, h, seed, rng)
                label = f"{name} {w}x{h} {how} {'noise' if noise else 'rendered'} demodulate {demod} {step}"
                got, ratio, e64 = _hold_step(label, pt, rad, guides, prev, params)
                worst = max(worst, ratio)
                surf = guides[0][..., 3] == 1
                if step == "first":
                    assert (got["history"][..., 3][surf] == 1).all()
                if step == "moved":
                    assert e64["valid"].any()
                    assert (name == "cornell") == bool(e64["valid"][surf].all())            # the moved sphere scenes have class-1 pixels without valid history
                    assert (got["motion"][..., 2][surf & ~e64["valid"] & ~e64["fragile"]] < tref.W_MIN).all()
                prev = tref.previous_state(got["history"], got["moments"], guides[1], guides[0], cam, tri)
    print(f"{name} {w}x{h} {how}: worst library error / E32 = {worst:.2f} (bound 16)")


@pytest.mark.parametrize("name", ("cornell", "sphere10k"))
def test_exact_properties(gpu, name):
    """The copies of the specification are copies: other classes, the first frame without demodulation, the history's guides; n stops at max_history; the
    radiance buffer and the guides are not written."""
    w, h = 100, 60
    d, pt = _load(gpu, name, w, h)
    rad, guides = _frame(pt, w, h, 5)
    K = guides[0][..., 3]
    assert (K != 1).any() and (K == 1).any()
    pt.temporal_accumulate(demodulate=0, max_history=2)
    acc = _accumulated(pt)
    assert _bits_equal(acc, rad)                                                     # no history, no demodulation: D_new = C
    st = _read_state(pt)
    assert (st["history"][..., 3][K == 1] == 1).all() and (st["history"][..., 3][K != 1] == 0).all()
    assert _bits_equal(pt.read_temporal(gpu.ptc.TEMPORAL_NORMAL_DEPTH), guides[1])
    assert _bits_equal(pt.read_temporal(gpu.ptc.TEMPORAL_POSITION_CLASS)[..., 3], K)
    for seed in (6, 7, 8):
        rad_k, guides_k = _frame(pt, w, h, seed)
        pt.temporal_accumulate(demodulate=0, max_history=2)
        n = pt.read_temporal(0)[..., 3]
        assert (n[K == 1] == 2).all() and (n[K != 1] == 0).all()                     # never more than max_history
        acc = _accumulated(pt)
        assert _bits_equal(acc[K != 1], rad_k[K != 1])
        assert not _bits_equal(acc[K == 1], rad_k[K == 1])
        # nothing the step reads is written: the radiance, the four guide read-backs
        assert _bits_equal(pt.read_radiance(), rad_k)
        prim, uv = pt.read_guide_hit()
        for a, b in zip((pt.read_guide(0), pt.read_guide(1), prim, uv), guides_k):
            assert _bits_equal(a, b) if a.dtype == np.float32 else np.array_equal(a, b)
        assert _bits_equal(pt.read_temporal(gpu.ptc.TEMPORAL_NORMAL_DEPTH), guides_k[1])      # the history's (N, Z) is this frame's guide, bit for bit
    # with demodulation the other classes still are the radiance's bits
    pt.temporal_accumulate(demodulate=1)
    acc = _accumulated(pt)
    assert _bits_equal(acc[K != 1], rad_k[K != 1])
    assert (pt.read_temporal(0)[..., 3][K == 1] == 1).all()                          # another `demodulate`: the history was dropped


def test_denoise_accumulated_is_the_specified_filter(gpu):
    """On a first frame (n = 1 everywhere: the 7x7 estimate, D_new = D) ptc_denoise_accumulated is ptc_denoise bit for bit.  After four unmoved frames and a move
    — n_new about 5 where the history is valid, 1 where it is not: both variance sources in one image — it lies within 16 x E32 of the float64 evaluation of
    the filter with the variance rule, evaluated from the library's own HISTORY and MOMENTS (E32 as in tests/test_gpu_denoise.py)."""
    w, h = 96, 64
    d, pt = _load(gpu, "sphere10k", w, h)
    params = dict(sigma_l=4.0, sigma_n=128.0, sigma_p=1.0, demodulate=1)
    rad, guides = _frame(pt, w, h, 1)
    pt.temporal_accumulate()
    for iters in (1, 4):
        pt.denoise(iterations=iters, **params)
        pt.select_output(1)
        plain = pt.read_radiance()
        pt.denoise_accumulated(iterations=iters, **params)
        assert _bits_equal(pt.read_radiance(), plain)
        pt.select_output(0)
    for seed in (2, 3, 4):
        _frame(pt, w, h, seed)
        pt.temporal_accumulate()
    cam1 = moved_camera(d.camera)
    pt.set_camera(cam1.position, cam1.target, cam1.fov_y, cam1.aspect)
    pt.update_instance(3, MOVED_T, MOVED_Q, (1.0, 1.0, 1.0)).scene_refit()
    rad, (ak, nz, prim, uv) = _frame(pt, w, h, 5)
    pt.temporal_accumulate()
    hist, mom = pt.read_temporal(0), pt.read_temporal(1)
    surf = ak[..., 3] == 1
    long_, short = surf & (hist[..., 3] >= 4), surf & (hist[..., 3] < 4)
    assert long_.mean() > 0.3 and short.sum() > 50                                   # both variance sources occur
    dirs, pos = dref.guide_dirs(cam1, w, h)
    for iters in (1, 4):
        pt.denoise_accumulated(iterations=iters, **params)
        pt.select_output(1)
        got = pt.read_radiance()
        pt.select_output(0)
        e64, e32 = (tref.denoise_accumulated(hist, mom, rad[..., :3], ak, nz, dirs, pos, cam1.fov_y, iterations=iters, dt=dt, **params) for dt in (np.float64, np.float32))
        top = float(e64.max())
        E32 = float(np.abs(e32.astype(np.float64) - e64).max()) / top
        err = float(np.abs(got[..., :3].astype(np.float64) - e64).max()) / top
        print(f"sphere10k {w}x{h} denoise_accumulated, {iters} iterations: n >= 4 on {long_.sum()} pixels, n < 4 on {short.sum()}; E32 {E32:.3g}, library error {err:.3g}, ratio {err / E32:.2f}")
        assert np.array_equal(got[..., 3], rad[..., 3])
        assert _bits_equal(got[~surf], rad[~surf])
        assert err <= 16 * E32, (iters, err, E32)


def test_accumulate_and_denoise_leave_the_frame_alone(gpu):
    """A progressive frame with guides, ptc_temporal_accumulate and ptc_denoise_accumulated in its middle accumulates the same bytes and counts the same rays."""
    w, h = 128, 96
    d, pt = _load(gpu, "sphere10k", w, h)

    def frame(with_calls):
        pt.frame_begin(w, h, 6, seed=21, max_bounces=6)
        pt.frame_add_samples(2)
        if with_calls:
            pt.frame_guides()
        pt.frame_resolve()                                                           # both ways: what the accumulate reads
        if with_calls:
            pt.temporal_accumulate()
        pt.frame_add_samples(3)
        pt.frame_resolve()
        if with_calls:
            pt.temporal_accumulate()
            pt.denoise_accumulated()
        pt.frame_add_samples(1)
        pt.frame_resolve()
        st = pt.stats()
        return pt.read_radiance(), [st[k] for k in COUNTERS]

    img0, c0 = frame(False)
    img1, c1 = frame(True)
    assert _bits_equal(img0, img1)
    assert c0 == c1 and c0[0] == w * h * 6


def test_lifetime_and_refusals(gpu, ora):
    w, h = 96, 64
    d, pt = _load(gpu, "sphere10k", w, h)
    cam = d.camera
    pt.frame_begin(w, h, 1, seed=2, max_bounces=6)
    pt.frame_add_samples(1)
    pt.frame_resolve()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.temporal_accumulate()                                                     # no guides yet
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.read_temporal(0)                                                          # no history yet
    pt.frame_guides()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.select_output(gpu.ptc.OUTPUT_ACCUMULATED)                                 # nothing accumulated yet
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise_accumulated()
    for bad in (dict(max_history=0), dict(max_history=1025), dict(sigma_z=-1.0), dict(sigma_z=float("nan")), dict(sigma_z=float("inf"))):
        with pytest.raises(gpu.PtcError, match="ptc error -1"):
            pt.temporal_accumulate(**bad)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.select_output(gpu.ptc.OUTPUT_ACCUMULATED)                                 # a refused accumulate changed nothing
    pt.temporal_accumulate()
    K = pt.read_guide(0)[..., 3]
    surf = K == 1
    n = lambda: pt.read_temporal(0)[..., 3][surf]
    assert (n() == 1).all()
    with pytest.raises(gpu.PtcError, match="ptc error -1"):
        pt.denoise_accumulated(demodulate=0)                                         # the accumulate demodulated
    with pytest.raises(gpu.PtcError, match="ptc error -1"):
        pt.denoise_accumulated(iterations=9)
    with pytest.raises(gpu.PtcError, match="ptc error -1"):
        pt.read_temporal(5)
    assert 0 < pt.temporal_seconds() < 1
    # the served image: the accumulated output through the read-backs ptc_select_output governs
    pt.select_output(gpu.ptc.OUTPUT_ACCUMULATED)
    acc = pt.read_radiance()
    assert np.array_equal(pt.tonemap(), ora.tonemap_rgba8(acc))
    want16 = np.array([ora.f32_to_f16(v) for v in acc.ravel()], np.uint16).reshape(h, w, 4)
    assert np.array_equal(pt.read_radiance_f16().view(np.uint16), want16)
    assert pt.radiance_f16_device_ptr() != 0
    pt.denoise_accumulated(iterations=0)
    pt.select_output(gpu.ptc.OUTPUT_DENOISED)
    assert _bits_equal(pt.read_radiance(), acc)                                      # no iterations: a copy of the accumulated image
    pt.denoise_accumulated()
    assert not _bits_equal(pt.read_radiance()[surf], acc[surf]) and _bits_equal(pt.read_radiance()[~surf], acc[~surf])

    def again(seed=3):
        _frame(pt, w, h, seed)
        with pytest.raises(gpu.PtcError, match="ptc error -2"):
            pt.select_output(gpu.ptc.OUTPUT_ACCUMULATED)                             # every frame_begin selects the radiance again and ends the accumulated image
        pt.temporal_accumulate()
        return pt.read_temporal(0)[..., 3][pt.read_guide(0)[..., 3] == 1]

    # the history survives a new frame, a new camera, a refit and a rebuild
    near = lambda n, k: np.abs(n - k).max() < 1e-4                                   # n is a weighted mean of the taps' n: k up to rounding
    assert near(again(), 2)
    pt.set_camera(cam.position, cam.target, cam.fov_y, cam.aspect)
    assert near(again(), 3)
    pt.update_instance(3, MOVED_T, MOVED_Q, (1.0, 1.0, 1.0)).scene_refit()
    got = again()
    assert abs(got.max() - 4) < 1e-4 and (got > 1).mean() > 0.9
    pt.scene_refit()                                                                 # two refits between two accumulates: the positions kept are the history's
    pt.update_instance(3, d.instances[3].t, d.instances[3].q_wxyz, d.instances[3].s).scene_rebuild()
    got = again()
    assert abs(got.max() - 5) < 1e-4 and (got > 1).mean() > 0.9
    pt.update_instance(3, MOVED_T, MOVED_Q, (1.0, 1.0, 1.0)).scene_refit()           # a refit of a tree the device built
    got = again()
    assert abs(got.max() - 6) < 1e-4 and (got > 1).mean() > 0.9
    # ... and is gone after a reset, a commit, another size
    pt.temporal_reset()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.read_temporal(0)
    assert (again() == 1).all()
    assert near(again(), 2)
    pt.load_scene(d)
    assert (again() == 1).all()
    assert near(again(), 2)
    w, h = 80, 64
    assert (again() == 1).all()


def test_read_back_is_refused_while_the_history_has_another_size(gpu):
    """The history survives a frame_begin with another size until the next accumulate drops it; in between its buffers are not the size the caller's are."""
    d, pt = _load(gpu, "cornell", 96, 64)
    _frame(pt, 96, 64, 1)
    pt.temporal_accumulate()
    assert pt.read_temporal(0).shape == (64, 96, 4)
    for w, h in ((48, 32), (128, 96)):
        pt.frame_begin(w, h, 1, seed=2, max_bounces=6)
        for which in range(5):
            with pytest.raises(gpu.PtcError, match="ptc error -2"):
                pt.read_temporal(which)
    _frame(pt, 96, 64, 3)
    assert np.abs(pt.read_temporal(0)[..., 3].max() - 1) == 0                         # the old size again, before any accumulate: served, still the first frame's
    _frame(pt, 48, 32, 4)
    pt.temporal_accumulate()
    hist = pt.read_temporal(0)
    assert hist.shape == (32, 48, 4) and hist[..., 3].max() == 1


def test_group_commit_drops_the_history_on_every_context(gpu):
    """ptc_group_scene_commit is a commit on every context of the group, also on those that do not pass through ptc_scene_commit: after it every context starts
    from a first frame, although a history and a position snapshot of the smaller scene before it were live.  Two devices where the machine has them (context 1
    is the one that takes the other way); one otherwise."""
    import torch

    w, h = 96, 64
    small, big = gpu.scenes.by_name("textured_objects"), gpu.scenes.by_name("sphere10k")
    g = gpu.Group([0, 1] if torch.cuda.device_count() >= 2 else [0]).load_scene(small)
    try:
        def accumulate_everywhere():
            out = []
            for i in range(len(g)):
                pt = g.ctx(i)
                _, guides = _frame(pt, w, h, 7)
                pt.temporal_accumulate()
                out.append(pt.read_temporal(0)[..., 3][guides[0][..., 3] == 1])
            return out

        assert all((n == 1).all() for n in accumulate_everywhere())
        assert all(np.abs(n - 2).max() < 1e-4 for n in accumulate_everywhere())
        g.ctx(0).update_instance(3, MOVED_T, MOVED_Q, (1.0, 1.0, 1.0))
        g.scene_refit()                                                              # every context now keeps a snapshot of the small scene's positions
        assert g.ctx(0).stats()["n_triangles"] < len(big.meshes[0].indices) // 3
        g.load_scene(big)
        assert all((n == 1).all() for n in accumulate_everywhere())
        assert all(np.abs(n - 2).max() < 1e-4 for n in accumulate_everywhere())
    finally:
        g.close()


def _relmse(a, b):
    a, b = a[..., :3].astype(np.float64), b[..., :3].astype(np.float64)
    return float((((a - b) ** 2) / (b ** 2 + 1e-2)).mean())


@pytest.mark.parametrize("name", ("cornell", "sphere10k"))
def test_it_accumulates(gpu, name):
    """Unmoved, sixteen 1-spp frames with seeds 1..16, max_history 32, against the library's own 1024-spp render with another seed:
    relMSE(accumulated) <= 1/8 of the frames' mean relMSE (independent frames: 1/16 + 1/1024), and accumulate + ptc_denoise_accumulated beats ptc_denoise
    of the last frame alone."""
    w = h = 128
    d, pt = _load(gpu, name, w, h)
    converged = pt.render(w, h, 1024, seed=77)
    pt.temporal_reset()
    frames = []
    for seed in range(1, 17):
        pt.frame_begin(w, h, 1, seed=seed, max_bounces=8)
        pt.frame_add_samples(1)
        pt.frame_guides()
        pt.frame_resolve()
        frames.append(_relmse(pt.read_radiance(), converged))
        pt.temporal_accumulate(max_history=32)
    surf = pt.read_guide(0)[..., 3] == 1
    assert np.abs(pt.read_temporal(0)[..., 3][surf] - 16).max() < 1e-4
    acc = _relmse(_accumulated(pt), converged)
    pt.denoise_accumulated()
    pt.select_output(gpu.ptc.OUTPUT_DENOISED)
    acc_dn = _relmse(pt.read_radiance(), converged)
    pt.denoise()
    last_dn = _relmse(pt.read_radiance(), converged)
    print(f"{name}: relMSE of a 1-spp frame {np.mean(frames):.4g} (mean of 16), accumulated {acc:.4g} = {acc / np.mean(frames):.4f} of it (bound 0.125), "
          f"accumulated + denoise_accumulated {acc_dn:.4g}, ptc_denoise of the last frame alone {last_dn:.4g}")
    assert acc / np.mean(frames) <= 1 / 8
    assert acc_dn < last_dn


def test_viewer_shim_temporal_path(gpu):
    """examples/viewer_shim.cpp with its `temporal` argument: a 1-spp frame per displayed frame, accumulated across the node's turn (a refit, or a refit and a
    rebuild) and filtered; the scene is the same either way, so is the picture."""
    import json
    import subprocess

    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "viewer_shim")
    sums = []
    for ratio, rebuilds in (("1e9", 0), ("0", 1)):
        r = subprocess.run([exe, "0", "6", ratio, "temporal"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        info = json.loads(r.stdout.strip().splitlines()[0])
        assert info["rendered"] is True and info["frames"] == 6 and info["staging_sum"] > 0 and info["rebuilds"] == rebuilds
        sums.append(info["staging_sum"])
    assert sums[0] == sums[1]
    plain = json.loads(subprocess.run([exe, "0", "6", "1e9"], capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[0])
    assert plain["staging_sum"] != sums[0]                                           # the argument does select another path
