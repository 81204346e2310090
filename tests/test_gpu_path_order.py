"""The numbering of a batch's paths on a real MI355X (csrc/pt_device.h: pt_path_id / pt_path_entry; PTC_PATH_ORDER=sample|pixel).

Pixel-major numbering (p = j S + s) changes which rays share a wave and how k_accumulate / k_ad_accumulate read the per-path radiance (a transpose through
LDS, a tile of samples at a time); it changes no value.  So everything here is equality of bits: images, the nine counters and the per-pixel sums of
ptc_frame_checkpoint, against the scalar oracle and against a context created under the other order.

The shapes are where a mapping or a transpose goes wrong: 37 x 23 = 851 pixels is no multiple of 64 or 256; 1, 5, 64 and 67 samples are below a transpose
tile, a ragged tile, whole tiles, and whole tiles plus a ragged rest; a tile share owns a strict subset of the frame; an adaptive frame's active list shrinks.

What the oracle has no call for is checked through what it does have: it renders n-spp frames, so the per-pixel SUMS are rebuilt from one-sample frames
(ptc_frame_set_sample_range(k, 0): a batch of one sample is the same batch under both orders) whose sample-order float32 mean is first shown to be the oracle's
frame; it has no lens, so the thin-lens frame is held to the numpy restatement of the lens rays (tests/lens_reference.py), as tests/test_gpu_lens.py does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_reference as aref  # noqa: E402
import sampled_reference as sref  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "segments", "shadow_rays", "hits", "node_visits_closest", "tri_tests_closest", "node_visits_any", "tri_tests_any", "algorithmic_bytes")
W, H, SEED, BOUNCES = 37, 23, 7, 3
SPPS = (1, 5, 64, 67)
F32 = np.float32


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_ctx, _ora, _cache = {}, {}, {}


def _context(gpu, order, desc=None, key="cornell", **env):
    """A context created under PTC_PATH_ORDER=order (and whatever else `env` sets), with the scene loaded; one per (scene, order, env)."""
    k = (key, order, tuple(sorted(env.items())))
    if k not in _ctx:
        want = dict(env, PTC_PATH_ORDER=order)
        old = {n: os.environ.get(n) for n in want}
        os.environ.update(want)
        try:
            pt = gpu.PathTracer(0).load_scene(desc if desc is not None else gpu.scenes.cornell_box())
        finally:
            for n, v in old.items():
                os.environ.pop(n, None) if v is None else os.environ.__setitem__(n, v)
        assert f"path_order={order}" in pt.launch_policy()
        _ctx[k] = pt
    return _ctx[k]


def _oracle(gpu, ora, w, h, spp, mb=BOUNCES, **tiles):
    """(image, the nine counters) of the oracle's frame of the Cornell box."""
    k = (w, h, spp, mb, tuple(sorted(tiles.items())))
    if k not in _ora:
        if "o" not in _ora:
            _ora["o"] = ora.Oracle().load_scene(gpu.scenes.cornell_box())
        img = _ora["o"].render(w, h, spp, seed=SEED, max_bounces=mb, **tiles)
        st = _ora["o"].stats()
        _ora[k] = (img, [st[c] for c in COUNTERS])
    return _ora[k]


def _counters(pt):
    st = pt.stats()
    return [st[c] for c in COUNTERS]


def _per_sample(gpu, w, h, n, mb):
    """L[k] (n, h, w, 3): sample k alone.  One sample per batch: both orders number such a batch alike, so these frames do not depend on what is tested here."""
    k = ("L", w, h, n, mb)
    if k not in _cache:
        pt = _context(gpu, "sample")
        L = np.empty((n, h, w, 3), F32)
        for s in range(n):
            pt.frame_begin(w, h, 1, seed=SEED, max_bounces=mb)
            pt.frame_set_sample_range(s, 0)
            pt.frame_add_samples(1)
            pt.frame_resolve()
            L[s] = pt.read_radiance()[..., :3]
        _cache[k] = L
    return _cache[k]


def _owned_order(pt, w, h, spp_total, **tiles):
    """index into the frame's owned list per pixel (-1: not owned), read through the library: a restored checkpoint that holds j resolves to j at owned[j]."""
    pt.frame_begin(w, h, spp_total, seed=SEED, max_bounces=BOUNCES, **tiles)
    acc, _ = pt.frame_checkpoint()
    n = acc.shape[0]
    ramp = np.zeros((n, 4), F32)
    ramp[:, 0] = np.arange(1, n + 1)
    pt.frame_begin(w, h, spp_total, seed=SEED, max_bounces=BOUNCES, **tiles)
    pt.frame_restore(ramp, 1)
    pt.frame_resolve()
    return pt.read_radiance()[..., 0].astype(np.int64) - 1


def _sums(L, n):
    acc = np.zeros(L.shape[1:], F32)
    for k in range(n):
        acc = acc + L[k]
    return acc


# ---- 1. odd size, varied sample counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", SPPS)
def test_pixel_major_frame_is_the_oracles(gpu, ora, spp):
    pt = _context(gpu, "pixel")
    img = pt.render(W, H, spp, seed=SEED, max_bounces=BOUNCES)
    want, counters = _oracle(gpu, ora, W, H, spp)
    print(f"{W}x{H}x{spp}: {int((img != want).any(-1).sum())} of {W * H} pixels differ from the oracle")
    assert _bits_equal(img, want)
    assert _counters(pt) == counters


# ---- 2. several batches and resolves ---------------------------------------------------------------------------------------------------------------------
def test_batches_and_resolves_keep_the_sums(gpu, ora):
    pt = _context(gpu, "pixel")
    L = _per_sample(gpu, W, H, 69, BOUNCES)
    for n in (3, 67, 69):      # the inputs: the one-sample frames sum to the oracle's frames
        assert _bits_equal(aref.sample_order_mean(L, n), _oracle(gpu, ora, W, H, n)[0][..., :3]), n
    order = _owned_order(pt, W, H, 69)
    assert sorted(order.ravel()) == list(range(W * H))

    def check(n):
        acc, done = pt.frame_checkpoint()
        assert done == n and acc.shape == (W * H, 4)
        assert _bits_equal(acc[order][..., :3], _sums(L, n)), f"sums after {n} samples"

    pt.frame_begin(W, H, 69, seed=SEED, max_bounces=BOUNCES)
    pt.frame_add_samples(3)
    check(3)                    # a checkpoint issues what was accepted: the 3 samples are a batch of their own
    pt.frame_add_samples(64)
    pt.frame_resolve()
    assert _bits_equal(pt.read_radiance(), _oracle(gpu, ora, W, H, 67)[0])
    check(67)
    pt.frame_add_samples(2)
    pt.frame_resolve()
    assert _bits_equal(pt.read_radiance(), _oracle(gpu, ora, W, H, 69)[0])
    check(69)
    assert _counters(pt) == _oracle(gpu, ora, W, H, 69)[1]
    # and without the checkpoint in between: add(3) and add(64) may travel as one batch of 67
    pt.frame_begin(W, H, 69, seed=SEED, max_bounces=BOUNCES)
    pt.frame_add_samples(3)
    pt.frame_add_samples(64)
    pt.frame_resolve()
    check(67)
    pt.frame_add_samples(2)
    pt.frame_resolve()
    check(69)
    assert _bits_equal(pt.read_radiance(), _oracle(gpu, ora, W, H, 69)[0])


# ---- 3. a tile share ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,ragged", [(64, 40, False), (75, 50, True)])
def test_tile_share(gpu, ora, w, h, ragged):
    """tile_rank 1 of 3: the owned list is a strict subset of the frame.  75 x 50 adds an owned count that is no multiple of 64 (partial tiles)."""
    pt = _context(gpu, "pixel")
    tiles = dict(tile_rank=1, tile_count=3)
    pt.frame_begin(w, h, 67, seed=SEED, max_bounces=BOUNCES, **tiles)
    pt.frame_add_samples(67)
    pt.frame_resolve()
    img = pt.read_radiance()
    n_owned = pt.frame_checkpoint()[0].shape[0]
    print(f"{w}x{h} rank 1 of 3 owns {n_owned} pixels")
    assert 0 < n_owned < w * h
    if ragged:
        assert n_owned % 64 != 0
    want, counters = _oracle(gpu, ora, w, h, 67, **tiles)
    assert _bits_equal(img, want)
    assert _counters(pt) == counters


# ---- 4. an adaptive frame whose active list shrinks ------------------------------------------------------------------------------------------------------
def test_adaptive_frame_with_covariance(gpu, ora):
    w, h, max_spp, mb = 64, 64, 64, 8
    params = dict(threshold=0.1, radius=1, min_samples=8, step_samples=8)
    L = _per_sample(gpu, w, h, max_spp, mb)
    for n in (8, max_spp):
        assert _bits_equal(aref.sample_order_mean(L, n), _oracle(gpu, ora, w, h, n, mb)[0][..., :3]), n
    sched = aref.Schedule(L, params["threshold"], params["radius"], max_spp)
    want = sched.run(params["min_samples"], params["step_samples"])
    assert len(set(sched.history)) >= 3 and sched.history[0] < w * h, "the active list does not shrink between passes"
    results = {}
    for order in ("pixel", "sample"):
        pt = _context(gpu, order)
        for cov in (0, 1):
            pt.set_sample_covariance(cov)
            img = pt.render_adaptive(w, h, max_spp, seed=SEED, max_bounces=mb, **params)
            counts = pt.read_sample_counts()
            print(f"{order} covariance={cov}: {int((counts != want).sum())} of {w * h} counts differ from the reference")
            assert np.array_equal(counts, want)
            assert _bits_equal(img, sched.image())
            assert pt.adaptive_stats()["passes"] == sched.passes
            results[order, cov] = (img, _counters(pt))
            if cov:
                got = pt.read_sample_covariance()
                s, q = sref.accumulate(L, counts)
                assert _bits_equal(got, q), "covariance sums"
                results[order, "q"] = got
        pt.set_sample_covariance(0)
    assert results["pixel", 0][1] == results["sample", 0][1] == results["pixel", 1][1]
    assert _bits_equal(results["pixel", "q"], results["sample", "q"])


# ---- 5. a thin-lens frame ---------------------------------------------------------------------------------------------------------------------------------
def test_thin_lens_frame(gpu):
    import lens_reference as lref
    import test_gpu_lens as tl

    desc = tl._scene(gpu)
    pt = _context(gpu, "pixel", desc=desc, key="lens_quads")
    w, h, spp = tl.W, tl.H, tl.NS
    assert (w, h, spp) == (33, 17, 5)
    for name in ("pinhole", "disk", "hexagon"):      # aperture_radius 0 first: it validates the model of the integrator the two lenses are then held to
        lens = tl.LENSES[name]
        want, which = tl._expected_image(pt, desc, lens, w, h, spp, tl.SEED)
        assert {int(m) for m in np.unique(which)} == {0, 1, 2, 3}
        assert _bits_equal(tl._render(pt, w, h, spp, lens), want), name
        # the debug entry's rays keep their documented order (sample-major) while the device numbers them pixel-major
        pixels = np.random.default_rng(5).permutation(w * h)[:97]
        o, d = pt.debug_camera_rays(w, h, tl.SEED, tl.FIRST, spp, pixels)
        ro, rd, _ = lref.camera_rays(lref.camera_basis(desc.camera), lens, w, h, tl.SEED, tl.FIRST, spp, pixels)
        assert _bits_equal(o, ro) and _bits_equal(d, rd), name
    pt.set_camera_lens(*tl.LENSES["pinhole"])


# ---- 6. two lanes -----------------------------------------------------------------------------------------------------------------------------------------
def test_two_lanes_keep_the_sample_order(gpu, ora):
    """PTC_LANES=2, and a batch budget of 8 samples per batch so that the 67 samples alternate over the lanes in nine batches."""
    pt = _context(gpu, "pixel", PTC_LANES="2", PTC_BATCH_PATHS=str(W * H * 8 * 2))
    assert "lanes=2" in pt.launch_policy()
    img = pt.render(W, H, 67, seed=SEED, max_bounces=BOUNCES)
    want, counters = _oracle(gpu, ora, W, H, 67)
    assert _bits_equal(img, want) and _counters(pt) == counters
    assert pt.stats()["launches_trace_closest"] == 9 * (BOUNCES + 1)
    plain = _context(gpu, "pixel", PTC_LANES="2")      # and the whole frame as one batch on one of two lanes
    assert _bits_equal(plain.render(W, H, 67, seed=SEED, max_bounces=BOUNCES), want)


# ---- 7. both orders ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", SPPS)
def test_both_orders_give_the_same_sums_and_counters(gpu, spp):
    got = {}
    for order in ("sample", "pixel"):
        pt = _context(gpu, order)      # _context asserts that ptc_launch_policy names the order the context was created with
        pt.frame_begin(W, H, spp, seed=SEED, max_bounces=BOUNCES)
        pt.frame_add_samples(spp)
        acc, done = pt.frame_checkpoint()
        assert done == spp
        got[order] = (acc, _counters(pt))
    assert _bits_equal(got["sample"][0], got["pixel"][0]) and got["sample"][1] == got["pixel"][1]
    defaults = gpu.load_library().ptc_launch_policy(None).decode().split(" | ")[1]
    assert "path_order=sample" in defaults or "path_order=pixel" in defaults
