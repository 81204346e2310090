"""Denoising from per-sample statistics on a real MI355X (include/ptc.h: ptc_set_sample_covariance, ptc_read_sample_covariance, ptc_denoise_sampled,
ptc_read_sampled_variance).

The six sums and the variance are IEEE binary32 in the order written, so they are compared bit for bit with the numpy mirror (tests/sampled_reference.py):
the sums on the per-sample radiances of one-sample frames (ptc_frame_set_sample_range(k, 0), as tests/test_gpu_adaptive.py obtains them), the variance on the
library's own sums, counts and albedo guide.  The filter is held to tests/temporal_reference.denoise_accumulated in float64, evaluated from the library's own
read-backs, with the float32-float64 gap of that evaluation as the yardstick (the bound and factor of §8a / §8c).  The rest: the frame is the frame it is
without the covariance, the refusals, and that the filter is better fed by the samples' variance than by the 7x7 window at 32 spp."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dref  # noqa: E402
import sampled_reference as sref  # noqa: E402
import temporal_reference as tref  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "segments", "shadow_rays", "hits", "node_visits_closest", "tri_tests_closest", "node_visits_any", "tri_tests_any", "algorithmic_bytes")
CASES = (("cornell", 64, 64), ("sphere10k", 64, 64), ("textured_objects", 64, 64), ("sphere10k", 75, 50))      # 75 x 50: no multiple of the tile or the block
SEED, MAX_SPP, BOUNCES = 7, 64, 8
ADAPTIVE = dict(threshold=0.1, radius=1)
FILTER = dict(sigma_l=4.0, sigma_n=128.0, sigma_p=1.0)
E_ARG, E_STATE = -1, -2


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_tracers, _samples = {}, {}


def _tracer(gpu, name, w, h):
    key = (name, w, h)
    if key not in _tracers:
        d = gpu.scenes.by_name(name)
        d.camera.aspect = w / h
        _tracers[key] = (d, gpu.PathTracer(0).load_scene(d))
    return _tracers[key]


def _per_sample(gpu, name, w, h):
    """L[k] (MAX_SPP, h, w, 3): the radiance of sample k alone, from calls that exist without the feature."""
    key = (name, w, h)
    if key not in _samples:
        _, pt = _tracer(gpu, name, w, h)
        L = np.empty((MAX_SPP, h, w, 3), np.float32)
        for k in range(MAX_SPP):
            pt.frame_begin(w, h, 1, seed=SEED, max_bounces=BOUNCES)
            pt.frame_set_sample_range(k, 0)
            pt.frame_add_samples(1)
            pt.frame_resolve()
            L[k] = pt.read_radiance()[..., :3]
        _samples[key] = L
    return _samples[key]


def _frame(pt, w, h, covariance, first=8, step=8, max_spp=MAX_SPP, decide=True, seed=SEED, params=ADAPTIVE, **tiles):
    """An adaptive frame through the caller-driven calls: `first` samples, then a decision step every `step` samples (decide = False: no decision step at all,
    max_spp samples for every pixel).  Leaves the frame resolved.  Returns (image, counts, the nine counters)."""
    pt.set_sample_covariance(covariance)
    pt.frame_begin(w, h, max_spp, seed=seed, max_bounces=BOUNCES, **tiles)
    pt.frame_set_adaptive(**params)
    if decide:
        pt.frame_add_samples(min(first, max_spp))
        done = min(first, max_spp)
        while pt.frame_adapt():
            k = min(step, max_spp - done)
            pt.frame_add_samples(k)
            done += k
    else:
        pt.frame_add_samples(max_spp)
    pt.frame_resolve()
    st = pt.stats()
    return pt.read_radiance(), pt.read_sample_counts(), [st[k] for k in COUNTERS]


def _denoised(pt):
    pt.select_output(1)
    img = pt.read_radiance()
    pt.select_output(0)
    return img


@pytest.mark.parametrize("name,w,h", CASES)
def test_sums_and_variance_are_exact(gpu, name, w, h):
    """The sums equal the float32 mirror fed the per-sample frames in sample order, wherever the count is n, on an adaptive frame with decision steps every 8
    samples and on a frame with none; image, counts and counters are those of the same frame without the covariance.  Then ptc_read_sampled_variance equals the
    mirror evaluated from the library's own sums, counts and albedo guide, with demodulation on and off, on every pixel."""
    _, pt = _tracer(gpu, name, w, h)
    L = _per_sample(gpu, name, w, h)
    for decide in (True, False):
        img0, cnt0, st0 = _frame(pt, w, h, 0, decide=decide)
        with pytest.raises(gpu.PtcError, match="ptc error -2"):
            pt.read_sample_covariance()                                                   # this frame does not keep it
        img1, cnt1, st1 = _frame(pt, w, h, 1, decide=decide)
        assert _bits_equal(img0, img1) and np.array_equal(cnt0, cnt1) and st0 == st1
        got = pt.read_sample_covariance()
        assert got.shape == (h, w, 6)
        s, q = sref.accumulate(L, cnt1)
        distinct = sorted(int(n) for n in np.unique(cnt1))
        print(f"{name} {w}x{h} {'decision steps every 8' if decide else 'no decision step'}: counts {distinct}; {int((got.view(np.uint32) != q.view(np.uint32)).sum())} of {got.size} sums differ")
        if decide:
            assert len(distinct) >= 4 and distinct[0] >= 8 and distinct[-1] == MAX_SPP
        else:
            assert distinct == [MAX_SPP]
            assert _bits_equal(img1, pt.render(w, h, MAX_SPP, seed=SEED, max_bounces=BOUNCES))     # a uniform frame with statistics IS the uniform frame
            _frame(pt, w, h, 1, decide=False)
        assert _bits_equal(got, q)
        fn = np.maximum(cnt1, 1).astype(np.float32)[..., None]
        assert _bits_equal(img1[..., :3], np.where(cnt1[..., None] > 0, s / fn, 0))        # the mirror's sums are the frame's
        # the variance, from the library's own read-backs
        pt.frame_guides()
        ak = pt.read_guide(0)
        for demodulate in (1, 0):
            pt.denoise_sampled(iterations=1, demodulate=demodulate, **FILTER)
            sv = pt.read_sampled_variance()
            assert sv.shape == (h, w, 2)
            V = sref.variance_of_mean(img1[..., :3], got, cnt1, ak, demodulate)
            want = sref.sampled_variance(V, cnt1)
            print(f"  demodulate {demodulate}: V < 0 before the clamp on {float((V < 0).mean()):.5f} of the pixels; {int((sv.view(np.uint32) != want.view(np.uint32)).sum())} of {sv.size} values differ")
            assert _bits_equal(sv, want)
            assert np.isfinite(sv).all() and (sv[..., 0] >= 0).all()


def _hold_filter(gpu, label, d, pt, w, h, counts, iterations, demodulate):
    """ptc_denoise_sampled against the float64 evaluation from the library's own read-backs; returns (n >= 4, n < 4) class-1 pixel counts."""
    rad = pt.read_radiance()
    ak, nz = pt.read_guide(0), pt.read_guide(1)
    dirs, pos = dref.guide_dirs(d.camera, w, h)
    surf = ak[..., 3] == 1
    out = None
    for iters in iterations:
        p = dict(FILTER, iterations=iters, demodulate=demodulate)
        pt.denoise_sampled(**p)
        got = _denoised(pt)
        sv = pt.read_sampled_variance()
        D = sref.demodulated(rad, ak, demodulate)                                         # one correctly rounded division: the library's bits
        hist = np.concatenate([D, counts.astype(np.float32)[..., None]], -1)
        mom = np.concatenate([np.zeros((h, w, 2), np.float32), sv], -1)
        e64, e32 = (tref.denoise_accumulated(hist, mom, rad[..., :3], ak, nz, dirs, pos, d.camera.fov_y, dt=dt, **p) for dt in (np.float64, np.float32))
        top = float(e64.max())
        E32 = float(np.abs(e32.astype(np.float64) - e64).max()) / top
        err = float(np.abs(got[..., :3].astype(np.float64) - e64).max()) / top
        out = int((surf & (counts >= 4)).sum()), int((surf & (counts < 4)).sum())
        print(f"{label}, {iters} iterations, demodulate {demodulate}: n >= 4 on {out[0]} surface pixels, n < 4 on {out[1]}; E32 {E32:.3g}, library error {err:.3g}, ratio {err / E32:.2f} (bound 16)")
        assert np.array_equal(got[..., 3], rad[..., 3])                                   # alpha from the radiance
        assert _bits_equal(got[~surf], rad[~surf])                                        # classes 0 and 2 pass through
        assert err <= 16 * E32, (label, iters, demodulate, err, E32)
    return out


@pytest.mark.parametrize("name,w,h", CASES)
def test_filter_is_the_specified_one(gpu, name, w, h):
    """Within 16 x E32 of temporal_reference.denoise_accumulated in float64, fed (D, n), (Var_s, 1 / n), the guides and the radiance as the library reads them
    back; E32 = the float32-float64 gap of that evaluation.  An adaptive frame (counts 8..64), iterations 1 and 4, demodulation on and off."""
    d, pt = _tracer(gpu, name, w, h)
    _, counts, _ = _frame(pt, w, h, 1)
    pt.frame_guides()
    for demodulate in (1, 0):
        _hold_filter(gpu, f"{name} {w}x{h}", d, pt, w, h, counts, (1, 4), demodulate)


def test_filter_with_both_variance_sources(gpu):
    """A caller-driven frame whose first decision comes after 2 samples: pixels that stop there have n < 4 and take the 7x7 estimate, the others the samples'
    variance.  n >= 4 compares integers: no pixel is left out."""
    name, w, h = "sphere10k", 64, 64
    d, pt = _tracer(gpu, name, w, h)
    _, counts, _ = _frame(pt, w, h, 1, first=2, step=8, max_spp=34, params=dict(threshold=0.3, radius=0))
    pt.frame_guides()
    long_, short = _hold_filter(gpu, f"{name} {w}x{h}, first decision after 2 samples", d, pt, w, h, counts, (1, 4), 1)
    assert long_ >= 50 and short >= 50                                                    # both variance sources occur


def test_filter_on_a_tile_share(gpu):
    """Tile share 0 of 2: the pixels of the other share take n = 0 (the 7x7 estimate over what the radiance buffer holds there) and zeros."""
    name, w, h = "sphere10k", 75, 50
    d, pt = _tracer(gpu, name, w, h)
    img, counts, _ = _frame(pt, w, h, 1, decide=False, max_spp=8, tile_rank=0, tile_count=2)
    owned = counts > 0
    assert 0 < owned.sum() < w * h and (counts[owned] == 8).all()
    pt.frame_guides()
    _hold_filter(gpu, f"{name} {w}x{h}, tile share 0 of 2", d, pt, w, h, counts, (1, 4), 1)
    sv, cov = pt.read_sampled_variance(), pt.read_sample_covariance()
    assert (sv[~owned] == 0).all() and (cov[~owned] == 0).all()
    assert (sv[..., 1][owned] == np.float32(1) / np.float32(8)).all()


def test_frame_is_untouched_and_refusals(gpu):
    name, w, h = "sphere10k", 75, 50
    d, pt = _tracer(gpu, name, w, h)
    L = pt._L

    def rc(call, *a):
        return call(pt._h, *a)

    # the parent's ptc_denoise of the same frame, begun without the covariance
    img0, cnt0, st0 = _frame(pt, w, h, 0)
    pt.frame_guides()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise_sampled()                                                              # an adaptive frame, but it does not keep the covariance
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.read_sampled_variance()
    pt.denoise(iterations=4, **FILTER)
    plain = _denoised(pt)

    # the setter only acts from the next ptc_frame_set_adaptive
    pt.set_sample_covariance(1)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise_sampled()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.read_sample_covariance()
    assert rc(L.ptc_set_sample_covariance, 2) == E_ARG                                    # refused, the setting stays on

    pt.frame_begin(w, h, MAX_SPP, seed=SEED, max_bounces=BOUNCES)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.read_sample_covariance()                                                       # a uniform frame
    pt.frame_set_adaptive(**ADAPTIVE)
    pt.set_sample_covariance(0)                                                           # ... and switching it off does not reach the frame in progress
    assert (pt.read_sample_covariance() == 0).all()
    pt.frame_add_samples(8)
    done = 8
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise_sampled()                                                              # no guides
    pt.frame_guides()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise_sampled()                                                              # samples added, not resolved
    while pt.frame_adapt():
        pt.frame_add_samples(8)
        done += 8
    pt.frame_resolve()
    img1, cnt1 = pt.read_radiance(), pt.read_sample_counts()
    st1 = [pt.stats()[k] for k in COUNTERS]
    assert _bits_equal(img0, img1) and np.array_equal(cnt0, cnt1) and st0 == st1
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.read_sampled_variance()                                                        # before the frame's first ptc_denoise_sampled
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.select_output(1)
    for bad in (dict(iterations=9), dict(iterations=-1), dict(sigma_l=-1.0), dict(sigma_n=float("nan")), dict(sigma_p=float("inf"))):
        with pytest.raises(gpu.PtcError, match="ptc error -1"):
            pt.denoise_sampled(**bad)
    assert rc(L.ptc_read_sample_covariance, None) == E_ARG and rc(L.ptc_read_sampled_variance, None) == E_ARG

    cov = pt.read_sample_covariance()
    assert rc(L.ptc_denoise_sampled, None) == 0                                           # NULL: the defaults
    sampled = _denoised(pt)
    pt.denoise_sampled(iterations=4, demodulate=1, **FILTER)
    assert _bits_equal(_denoised(pt), sampled)
    assert not _bits_equal(sampled, plain)
    g, t = pt.denoise_seconds()
    assert g > 0 and t > 0                                                                # reported as ptc_denoise_accumulated's time is
    pt.denoise_sampled(iterations=0)
    assert _bits_equal(_denoised(pt), img1)                                               # iterations = 0 copies the radiance
    # radiance, counts, sums and counters are unchanged; ptc_denoise still gives the parent's result
    assert _bits_equal(pt.read_radiance(), img1) and np.array_equal(pt.read_sample_counts(), cnt1) and _bits_equal(pt.read_sample_covariance(), cov)
    assert [pt.stats()[k] for k in COUNTERS] == st1
    pt.denoise(iterations=4, **FILTER)
    assert _bits_equal(_denoised(pt), plain)

    # everything an adaptive frame refuses stays refused
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.frame_checkpoint()
    # samples after the resolve: refused until the next resolve (a frame with budget left: no decision step, so every pixel stays active)
    pt.set_sample_covariance(1)
    pt.frame_begin(w, h, 8, seed=SEED, max_bounces=BOUNCES)
    pt.frame_set_adaptive(**ADAPTIVE)
    pt.frame_add_samples(4)
    pt.frame_resolve()
    pt.frame_guides()
    pt.denoise_sampled()
    pt.frame_add_samples(4)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise_sampled()
    pt.frame_resolve()
    pt.denoise_sampled()
    assert (pt.read_sampled_variance()[..., 1] == np.float32(0.125)).all()
    # a new camera ends the guides; a new frame ends the variance
    cam = d.camera
    pt.set_camera(cam.position, cam.target, cam.fov_y, cam.aspect)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.denoise_sampled()
    pt.render(w, h, 1, seed=1, max_bounces=BOUNCES)
    for call in (pt.read_sampled_variance, pt.read_sample_covariance, pt.denoise_sampled):
        with pytest.raises(gpu.PtcError, match="ptc error -2"):
            call()
    pt.set_sample_covariance(0)


def _relmse(a, b):
    a, b = a[..., :3].astype(np.float64), b[..., :3].astype(np.float64)
    return float((((a - b) ** 2) / (b ** 2 + 1e-2)).mean())


@pytest.mark.parametrize("name", ("cornell", "sphere10k"))
def test_it_is_worth_it(gpu, name):
    """128 x 128, 32 spp with no decision step, against the library's own 1024-spp render with another seed: ptc_denoise_sampled is better than the noisy frame,
    and better than ptc_denoise of the same frame.  Both are conditions (the float64 prototype: ratios 0.68 / 0.55 on cornell, 0.58 / 0.17 on sphere10k)."""
    w = h = 128
    d, pt = _tracer(gpu, name, w, h)
    converged = pt.render(w, h, 1024, seed=7)
    noisy, _, _ = _frame(pt, w, h, 1, decide=False, max_spp=32, seed=1, params={})
    pt.frame_guides()
    p = dict(FILTER, iterations=4, demodulate=1)
    pt.denoise(**p)
    e_plain = _relmse(_denoised(pt), converged)
    pt.denoise_sampled(**p)
    e_sampled = _relmse(_denoised(pt), converged)
    e_noisy = _relmse(noisy, converged)
    pt.set_sample_covariance(0)
    print(f"{name} 32 spp: relMSE noisy {e_noisy:.4g}, ptc_denoise {e_plain:.4g}, ptc_denoise_sampled {e_sampled:.4g}: sampled / noisy {e_sampled / e_noisy:.3f}, sampled / ptc_denoise {e_sampled / e_plain:.3f}")
    assert e_sampled < e_noisy
    assert e_sampled < e_plain


def _read_pfm(path, w, h):
    head, body = open(path, "rb").read().split(b"-1.0\n", 1)
    assert head.startswith(b"PF\n%d %d" % (w, h))
    return np.ascontiguousarray(np.frombuffer(body, "<f4").reshape(h, w, 3)[::-1])        # PFM rows are bottom-up


def test_cpp_host_cli_denoise_sampled(gpu, tmp_path):
    """ptc_render --denoise-sampled (host/pbr_pt.hpp over the same C-ABI): without --adaptive the frame is the uniform frame with statistics, and the image is
    what the Python binding's denoise_sampled gives for it."""
    import subprocess

    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    w, h = 96, 64
    out = str(tmp_path / "dn.pfm")
    r = subprocess.run([exe, "--scene", "cornell", "--width", str(w), "--height", str(h), "--spp", "8", "--seed", "5", "--bounces", "4", "--denoise-sampled", "--out", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    d = gpu.scenes.cornell_box()
    d.camera.aspect = 1.0
    pt = gpu.PathTracer(0).load_scene(d)
    uniform = pt.render(w, h, 8, seed=5, max_bounces=4)
    pt.set_sample_covariance(1)
    pt.frame_begin(w, h, 8, seed=5, max_bounces=4)
    pt.frame_set_adaptive()
    pt.frame_add_samples(8)
    pt.frame_resolve()
    assert _bits_equal(pt.read_radiance(), uniform)
    pt.frame_guides()
    pt.denoise_sampled()
    dn = _denoised(pt)
    assert not _bits_equal(dn, uniform)
    assert _bits_equal(_read_pfm(out, w, h), np.ascontiguousarray(dn[..., :3]))
