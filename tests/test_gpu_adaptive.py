"""Adaptive sampling on a real MI355X (include/ptc.h: ptc_frame_set_adaptive, ptc_frame_adapt, ptc_read_sample_counts, ptc_render_adaptive).

The RNG is counter-based and a pixel's sum is taken in sample order, so everything here is exact.  The per-sample radiances L[k] come from one-sample
frames through calls that exist without the feature (ptc_frame_set_sample_range(k, 0)); they are validated against the scalar oracle; the schedule is then
evaluated on them in numpy float32 (tests/adaptive_reference.py) and the device's count map has to equal that, pixel for pixel, and its image the oracle's
n-spp image wherever the count is n."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "segments", "shadow_rays", "hits", "node_visits_closest", "tri_tests_closest", "node_visits_any", "tri_tests_any", "algorithmic_bytes")
SCENES = ("cornell", "sphere10k", "textured_objects")
SIZES = ((64, 64), (75, 50))          # whole tiles; partial tiles
SEED, MAX_SPP, BOUNCES = 7, 64, 8
PARAMS = dict(threshold=0.1, min_samples=8, step_samples=8)
# (scene, w, h, radius) -> threshold, for a combination whose reference count map misses the condition on the inputs at 0.1 (none so far)
THRESHOLD = {}
E_ARG, E_STATE = -1, -2


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_tracers, _samples, _oracle = {}, {}, {}


def _tracer(gpu, name):
    if name not in _tracers:
        d = gpu.scenes.by_name(name)
        _tracers[name] = (d, gpu.PathTracer(0).load_scene(d))
    return _tracers[name]


def _per_sample(gpu, name, w, h):
    """L[k] (MAX_SPP, h, w, 3): the radiance of sample k alone, from behaviour the library has without adaptive sampling."""
    key = (name, w, h)
    if key not in _samples:
        _, pt = _tracer(gpu, name)
        L = np.empty((MAX_SPP, h, w, 3), np.float32)
        for k in range(MAX_SPP):
            pt.frame_begin(w, h, 1, seed=SEED, max_bounces=BOUNCES)
            pt.frame_set_sample_range(k, 0)
            pt.frame_add_samples(1)
            pt.frame_resolve()
            L[k] = pt.read_radiance()[..., :3]
        _samples[key] = L
    return _samples[key]


def _oracle_image(gpu, ora, name, w, h, n):
    key = (name, w, h, n)
    if key not in _oracle:
        if name not in _oracle:
            _oracle[name] = ora.Oracle().load_scene(_tracer(gpu, name)[0])
        _oracle[key] = _oracle[name].render(w, h, n, seed=SEED, max_bounces=BOUNCES)
    return _oracle[key]


def _drive(pt, w, h, max_spp, tile_rank=0, tile_count=1, **params):
    """ptc_render_adaptive's loop through the caller-driven calls (a tile share has no convenience call)."""
    pt.frame_begin(w, h, max_spp, seed=SEED, max_bounces=BOUNCES, tile_rank=tile_rank, tile_count=tile_count)
    pt.frame_set_adaptive(**params)
    pt.frame_add_samples(min(params["min_samples"], max_spp))
    done = min(params["min_samples"], max_spp)
    while pt.frame_adapt():
        k = min(params["step_samples"], max_spp - done)
        pt.frame_add_samples(k)
        done += k
    pt.frame_resolve()
    return pt.read_radiance(), pt.read_sample_counts()


def _assert_image_is_the_oracles(gpu, ora, name, w, h, img, counts):
    for n in np.unique(counts):
        if n == 0:
            continue
        sel = counts == n
        want = _oracle_image(gpu, ora, name, w, h, int(n))
        assert _bits_equal(img[sel][:, :3], want[sel][:, :3]), f"{name} {w}x{h}: pixels with count {n} differ from the oracle's {n}-spp frame"
        assert (img[sel][:, 3] == 1).all()
    assert (img[counts == 0] == 0).all()


@pytest.mark.parametrize("radius", (0, 1, 2))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", SCENES)
def test_exact_schedule_and_exact_image(gpu, ora, name, size, radius):
    w, h = size
    _, pt = _tracer(gpu, name)
    L = _per_sample(gpu, name, w, h)
    for n in (8, MAX_SPP):            # the inputs: the sample-order float32 mean of the one-sample frames IS the oracle's n-spp frame
        assert _bits_equal(ref.sample_order_mean(L, n), _oracle_image(gpu, ora, name, w, h, n)[..., :3]), f"per-sample frames of {name} do not sum to the oracle's {n}-spp frame"
    params = dict(PARAMS, radius=radius, threshold=THRESHOLD.get((name, w, h, radius), PARAMS["threshold"]))
    sched = ref.Schedule(L, params["threshold"], radius, MAX_SPP)
    want = sched.run(params["min_samples"], params["step_samples"])
    shares = ref.distinct_counts(want)
    print(f"{name} {w}x{h} r={radius} threshold={params['threshold']}: reference counts " + ", ".join(f"{n}: {100 * s:.1f} %" for n, s in sorted(shares.items())) +
          f"; mean {want.mean():.2f} spp, {sched.passes} decision steps")
    assert sum(1 for s in shares.values() if s >= 0.01) >= 4, "the inputs do not exercise the schedule: fewer than four counts held by 1 % of the pixels"
    img = pt.render_adaptive(w, h, MAX_SPP, seed=SEED, max_bounces=BOUNCES, **params)
    counts = pt.read_sample_counts()
    print(f"  device: {int((counts != want).sum())} of {w * h} counts differ from the reference")
    assert np.array_equal(counts, want)
    _assert_image_is_the_oracles(gpu, ora, name, w, h, img, counts)
    st, ad = pt.stats(), pt.adaptive_stats()
    assert ad["samples_total"] == st["paths"] == int(counts.sum()) and ad["owned_pixels"] == w * h and ad["active_pixels"] == 0
    assert ad["passes"] == sched.passes and ad["max_count"] == int(counts.max())


def test_zero_threshold_is_the_uniform_frame(gpu, ora):
    """Cornell box with radius 2: the only pixels whose samples are all alike are the directly seen emitter's, and each has a noisy pixel of the ceiling within 2."""
    name, w, h, radius = "cornell", 64, 64, 2
    _, pt = _tracer(gpu, name)
    L = _per_sample(gpu, name, w, h)
    sched = ref.Schedule(L, 0.0, radius, MAX_SPP)
    assert (sched.run(8, 8) == MAX_SPP).all(), "the scene is not noisy enough for this test: the reference stops pixels at threshold 0"
    uniform = pt.render(w, h, MAX_SPP, seed=SEED, max_bounces=BOUNCES)
    st_uniform = pt.stats()
    img = pt.render_adaptive(w, h, MAX_SPP, seed=SEED, max_bounces=BOUNCES, threshold=0.0, radius=radius, min_samples=8, step_samples=8)
    st = pt.stats()
    assert (pt.read_sample_counts() == MAX_SPP).all()
    assert _bits_equal(img, uniform) and _bits_equal(img[..., :3], _oracle_image(gpu, ora, name, w, h, MAX_SPP)[..., :3])
    for k in COUNTERS:
        assert st[k] == st_uniform[k], k
    assert st["paths"] == w * h * MAX_SPP


@pytest.mark.parametrize("name", SCENES)
def test_huge_threshold_stops_at_min_samples(gpu, ora, name):
    w, h = 75, 50
    _, pt = _tracer(gpu, name)
    img = pt.render_adaptive(w, h, MAX_SPP, seed=SEED, max_bounces=BOUNCES, threshold=1e30, radius=2, min_samples=8, step_samples=8)
    assert (pt.read_sample_counts() == 8).all()
    assert _bits_equal(img[..., :3], _oracle_image(gpu, ora, name, w, h, 8)[..., :3])
    ad = pt.adaptive_stats()
    assert ad["passes"] == 1 and ad["active_pixels"] == 0 and ad["samples_total"] == 8 * w * h == pt.stats()["paths"]
    pt.frame_add_samples(8)               # nothing is active: accepted, nothing happens
    assert pt.frame_adapt() == 0 and (pt.read_sample_counts() == 8).all() and pt.stats()["paths"] == 8 * w * h


@pytest.mark.parametrize("ranks", (2, 3))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_tile_shares_sum_to_the_whole_frame(gpu, ora, ranks, size):
    name, (w, h) = "cornell", size
    _, pt = _tracer(gpu, name)
    params = dict(PARAMS, radius=1)
    whole = pt.render_adaptive(w, h, MAX_SPP, seed=SEED, max_bounces=BOUNCES, **params)
    whole_counts = pt.read_sample_counts()
    assert len(np.unique(whole_counts)) >= 4
    img_sum, cnt_sum = np.zeros_like(whole), np.zeros_like(whole_counts)
    for r in range(ranks):
        img, cnt = _drive(pt, w, h, MAX_SPP, tile_rank=r, tile_count=ranks, **params)
        owner = np.array([[ora.tile_owner(w, h, x, y, ranks) for x in range(w)] for y in range(h)])
        assert (cnt[owner != r] == 0).all() and (cnt[owner == r] > 0).all() and (img[owner != r] == 0).all()
        assert pt.adaptive_stats()["owned_pixels"] == int((owner == r).sum())
        img_sum += img
        cnt_sum += cnt
    assert np.array_equal(cnt_sum, whole_counts) and _bits_equal(img_sum, whole)


def test_caller_driven_form(gpu, ora):
    """add_samples(3) with decision steps at irregular points; a resolve in mid-frame; the totals."""
    name, w, h, budget = "cornell", 64, 64, 30
    _, pt = _tracer(gpu, name)
    L = _per_sample(gpu, name, w, h)
    sched = ref.Schedule(L, 0.12, 1, budget)
    pt.frame_begin(w, h, budget, seed=SEED, max_bounces=BOUNCES)
    pt.frame_set_adaptive(threshold=0.12, radius=1)
    calls = "aaDaDaaaDaRaDaD"         # a: add 3 samples, D: decision step, R: resolve + check in mid-frame
    for op in calls:
        if op == "a":
            pt.frame_add_samples(3)
            sched.add(3)
        elif op == "D":
            assert pt.frame_adapt() == sched.adapt()
        else:
            pt.frame_resolve()
            img, cnt = pt.read_radiance(), pt.read_sample_counts()
            assert np.array_equal(cnt, sched.count)
            assert (cnt[sched.active] == sched.done).all() and (cnt[~sched.active] < sched.done).all() and sched.active.any() and not sched.active.all()
            for n in np.unique(cnt):      # active pixels are divided by the samples so far, stopped ones by their own count
                assert _bits_equal(img[cnt == n][:, :3], ref.sample_order_mean(L, int(n))[cnt == n])
    pt.frame_resolve()
    img, cnt = pt.read_radiance(), pt.read_sample_counts()
    shares = ref.distinct_counts(sched.count)
    print("caller-driven: reference counts " + ", ".join(f"{n}: {100 * s:.1f} %" for n, s in sorted(shares.items())))
    assert sum(1 for s in shares.values() if s >= 0.01) >= 3
    assert np.array_equal(cnt, sched.count)
    assert _bits_equal(img[..., :3], sched.image()[..., :3])
    _assert_image_is_the_oracles(gpu, ora, name, w, h, img, cnt)
    ad = pt.adaptive_stats()
    assert ad["samples_total"] == pt.stats()["paths"] == int(cnt.sum())
    assert ad["passes"] == sched.passes == calls.count("D") and ad["active_pixels"] == int(sched.active.sum()) and ad["max_count"] == int(cnt.max())


def test_two_lanes_and_small_batches_give_the_same_bits(gpu):
    """PTC_LANES=2 with a batch budget that cuts every pass into several batches: the accumulation stays in sample order."""
    name, w, h = "textured_objects", 75, 50
    _, pt = _tracer(gpu, name)
    params = dict(PARAMS, radius=1)
    img = pt.render_adaptive(w, h, MAX_SPP, seed=SEED, max_bounces=BOUNCES, **params)
    counts = pt.read_sample_counts()
    old = {k: os.environ.get(k) for k in ("PTC_LANES", "PTC_BATCH_PATHS")}
    os.environ.update(PTC_LANES="2", PTC_BATCH_PATHS="16384")
    try:
        pt2 = gpu.PathTracer(0).load_scene(gpu.scenes.by_name(name))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert "lanes=2" in pt2.launch_policy() and "batch_paths=16384" in pt2.launch_policy()
    img2 = pt2.render_adaptive(w, h, MAX_SPP, seed=SEED, max_bounces=BOUNCES, **params)
    assert np.array_equal(pt2.read_sample_counts(), counts) and _bits_equal(img2, img)
    assert pt2.stats()["paths"] == int(counts.sum())
    pt2.close()


def test_neighbours_are_not_disturbed(gpu):
    name, w, h = "cornell", 75, 50
    _, pt = _tracer(gpu, name)
    params = dict(PARAMS, radius=1)
    img = pt.render_adaptive(w, h, MAX_SPP, seed=SEED, max_bounces=BOUNCES, **params)
    counts = pt.read_sample_counts()
    pt.frame_guides()
    pt.denoise(iterations=3)
    pt.select_output(gpu.ptc.OUTPUT_DENOISED)
    den = pt.read_radiance()
    assert np.isfinite(den).all() and not _bits_equal(den, img)
    half, ldr = pt.read_radiance_f16(), pt.tonemap()
    assert np.isfinite(half.astype(np.float32)).all() and ldr.shape == (h, w, 4)
    pt.select_output(gpu.ptc.OUTPUT_RADIANCE)
    assert _bits_equal(pt.read_radiance(), img) and np.array_equal(pt.read_sample_counts(), counts)
    # a frame without set_adaptive right after an adaptive one, on the same context, is a fresh context's
    after = pt.render(w, h, 16, seed=SEED, max_bounces=BOUNCES)
    st_after = pt.stats()
    fresh_pt = gpu.PathTracer(0).load_scene(gpu.scenes.by_name(name))
    fresh = fresh_pt.render(w, h, 16, seed=SEED, max_bounces=BOUNCES)
    st_fresh = fresh_pt.stats()
    assert _bits_equal(after, fresh)
    for k in COUNTERS:
        assert st_after[k] == st_fresh[k], k
    fresh_pt.close()


def test_refusals(gpu):
    L = gpu.load_library()
    _, pt = _tracer(gpu, "cornell")
    h = pt._h
    P = gpu.ptc.PtcAdaptiveParams

    def params(**kw):
        p = P()
        L.ptc_adaptive_default_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    n = C.c_uint64()
    counts = np.zeros((16, 16), np.uint32)
    st = gpu.ptc.PtcAdaptiveStats()
    acc = np.zeros((256, 4), np.float32)
    accp = acc.ctypes.data_as(C.POINTER(C.c_float))
    # state: no frame (a refused ptc_frame_begin ends the one before); a raster frame; after a sample
    assert L.ptc_frame_begin(h, 0, 16, 8, 1, 4, 0, 0, 1) == E_ARG
    assert L.ptc_frame_set_adaptive(h, None) == E_STATE and L.ptc_frame_adapt(h, None) == E_STATE
    pt.frame_begin(16, 16, 8, integrator=gpu.ptc.INTEGRATOR_RASTER_COMPAT)
    assert L.ptc_frame_set_adaptive(h, None) == E_STATE
    pt.frame_begin(16, 16, 8)
    pt.frame_add_samples(1)
    assert L.ptc_frame_set_adaptive(h, None) == E_STATE
    # a frame that is not adaptive
    assert L.ptc_frame_adapt(h, C.byref(n)) == E_STATE
    assert L.ptc_read_sample_counts(h, counts.ctypes.data_as(C.POINTER(C.c_uint32))) == E_STATE
    assert L.ptc_get_adaptive_stats(h, C.byref(st)) == E_STATE
    # a resolve divisor and adaptivity exclude each other, in either order
    pt.frame_begin(16, 16, 8)
    pt.frame_set_sample_range(0, 8)
    assert L.ptc_frame_set_adaptive(h, None) == E_STATE
    # arguments: refused, and the frame stays as it was (not adaptive)
    pt.frame_begin(16, 16, 8)
    for bad in (dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(radius=-1), dict(radius=3), dict(min_samples=0), dict(step_samples=0)):
        assert L.ptc_frame_set_adaptive(h, C.byref(params(**bad))) == E_ARG, bad
        assert L.ptc_frame_adapt(h, None) == E_STATE, bad
        assert L.ptc_render_adaptive(h, 16, 16, 8, 1, 4, C.byref(params(**bad))) == E_ARG, bad
    # the refused ptc_render_adaptive calls began no frame of their own either: this one is still open and takes the switch
    assert L.ptc_frame_set_adaptive(h, C.byref(params(radius=0, threshold=0.0))) == 0
    assert L.ptc_frame_set_adaptive(h, None) == E_STATE                          # once per frame
    assert L.ptc_frame_adapt(h, None) == E_STATE                                 # no sample yet
    assert L.ptc_frame_set_sample_range(h, 0, 8) == E_STATE
    assert L.ptc_frame_set_sample_range(h, 5, 0) == 0                            # a first sample index alone is fine
    n_owned, done = C.c_uint64(), C.c_uint32()
    assert L.ptc_frame_checkpoint(h, None, C.byref(n_owned), C.byref(done)) == E_STATE
    assert L.ptc_frame_restore(h, accp, 256, 0) == E_STATE
    pt.frame_add_samples(4)
    assert L.ptc_frame_checkpoint(h, accp, C.byref(n_owned), C.byref(done)) == E_STATE
    assert L.ptc_frame_adapt(h, C.byref(n)) == 0 and 0 < n.value <= 256           # threshold 0: every pixel with any noise stays
    assert L.ptc_read_sample_counts(h, None) == E_ARG and L.ptc_get_adaptive_stats(h, None) == E_ARG
    assert L.ptc_frame_add_samples(h, 5) == E_ARG                                # beyond the budget (4 + 5 > 8) while pixels are active
    pt.frame_add_samples(4)
    assert L.ptc_frame_adapt(h, C.byref(n)) == 0 and n.value == 0                # the budget is spent: everything stops
    assert L.ptc_frame_add_samples(h, 5) == 0                                    # nothing is active: accepted, nothing happens
    assert pt.read_sample_counts().max() == 8 and pt.stats()["paths"] == int(pt.read_sample_counts().sum())
    # ptc_render_adaptive needs a committed scene and sane sizes like ptc_render
    assert L.ptc_render_adaptive(h, 0, 16, 8, 1, 4, None) == E_ARG
    assert L.ptc_render_adaptive(h, 16, 16, 8, 1, 4, None) == 0
