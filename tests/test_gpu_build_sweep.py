"""The device BVH builders (csrc/pt_build.hip: pt_build_lbvh, pt_build_sah) on a real MI355X over tests/build_sweep.py: triangle counts on either side of every
constant at which a kernel changes path (64 lanes, 512-key sort tiles and 2048-key blocks, kSahBig = 1024, kSahChunk = 4096, 256 tiles per scan round, the
262,144-triangle grid of k_bld_prims) and soups that leave a builder nothing to decide by (one triangle N times, an outlier, runs of equal Morton keys across sort
tiles, zero-area triangles, duplicates, signed zeros).  tests/test_gpu_parity.py and tests/test_gpu_device_sah.py hold the same contract on the named scenes: 2, 12,
302, 640, a few thousand and 249,936 triangles.

The contract is the one of every device build: the bytes of the host's build of the same description (tests/test_build_sweep_host.py holds that build against the
oracle's tree on these inputs) — after the commit and after a rebuild, which makes the spare tree set the live one.  Up to 8,193 triangles the trees are traced too:
the oracle's bits and traversal counters on the rays of the CPU anchor, and for the generic kinds the float64 search of all triangles (tests/trace_reference.py,
its own 16 x E32).  The three large counts are held to their bytes and, in a test of their own, to 128 rays (64 at 262,445 triangles) against that float64 search.

One context that builds a small tree after a large one (grow-only scratch, swapped tree sets), the 40 random soups of test_gpu_parity through both device
builders, and a move followed by a refit and a rebuild at the SAH builder's thresholds complete the file."""
import copy
import functools
import hashlib
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import build_sweep as bs  # noqa: E402
import trace_reference as tr  # noqa: E402
from test_build_sweep_host import CLASSES, oracle_answers, rays_of  # noqa: E402

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_gpu_parity", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_parity.py"))
tg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tg)
_scene_bytes = tg._scene_bytes

STATS = ("n_triangles", "n_bvh_nodes", "n_emitters", "bvh_max_depth", "bvh_sa_cost", "bvh_sa_cost_built")
# rays per large soup: 128, and 64 at 262,445 triangles, where the float64 search of 128 rays alone takes as long as the whole of
# test_gpu_device_sah's full-size atrium commit, the slowest builder test before this file
N_RAYS_LARGE = {131072: 128, 131073: 128, 262445: 64}


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _same_bytes(want, got, what=""):
    for key in want:
        assert want[key].shape == got[key].shape and np.array_equal(want[key], got[key]), \
            f"{what}{key} differs in {int((want[key] != got[key]).sum()) if want[key].shape == got[key].shape else -1} words"


def _desc(pbr, kind, n, builder):
    d = bs.desc(pbr, kind, n)
    d.bvh_builder = builder
    return d


def _host(pbr, d):
    """(bytes, statistics) of the host's commit of `d` on a description-only context."""
    pt = pbr.PathTracer(pbr.DEVICE_NONE).load_scene(d)
    s = pt.stats()
    return _scene_bytes(pt), {k: s[k] for k in STATS}


@functools.lru_cache(maxsize=16)
def _want(kind, n, builder):
    import pbr_amd

    return _host(pbr_amd, _desc(pbr_amd, kind, n, builder))


def _on_the_device(dev, builder, what=""):
    it = dev.internals()
    assert it["commit_on_device"] == 1 and it["device_build_sah"] == (1 if builder == "sah" else 0), what + "not built on the device by the %s builder" % builder


def _hold_traced(tag, pt, kind, n, builder):
    """The tree in HBM answers the case's rays with the oracle's bits and traversal counters; the generic kinds are right against the float64 search as well."""
    c = rays_of(kind, n)
    org, dirs, tmax = c["rays"][:3]
    t0, prim0, uv0, occ0, counters = oracle_answers(kind, n, builder)
    t, prim, uv = pt.trace_closest(org, dirs)
    s = pt.stats()
    assert _bits(t, t0) and np.array_equal(prim, prim0) and _bits(uv, uv0), tag + ": closest hit differs from the oracle's"
    for k in ("node_visits_closest", "tri_tests_closest"):
        assert s[k] == counters[k], (tag, k)
    occ = pt.trace_any(org, dirs, tmax)
    s = pt.stats()
    assert np.array_equal(occ, occ0), tag + ": any-hit differs from the oracle's"
    for k in ("node_visits_any", "tri_tests_any"):
        assert s[k] == counters[k], (tag, k)
    if c["truth"] is not None:
        v, i, _ = pt.flat_scene()
        assert _bits(v, c["verts"]) and np.array_equal(i, c["idx"]), tag + ": the reference is not that of this context's flat_scene()"
        tr.assert_true(tag, c["verts"], c["idx"], c["rays"], c["truth"], c["e32"], t, prim, uv, occ)


_LARGE = {}


def _large_case(kind, n, flat):
    """Rays at one of the large soups (the classes of the CPU anchor's table; there is no oracle tree, so no origin lies on a box plane) and their float64 truth,
    computed once per soup from `flat` = flat_scene() of the first context that asks; a later context must hold the same vertices, bit for bit."""
    verts, idx, _ = flat
    digest = hashlib.sha1(np.ascontiguousarray(verts).tobytes() + np.ascontiguousarray(idx).tobytes()).hexdigest()
    if (kind, n) not in _LARGE:
        none = (np.zeros(0, np.int64), np.zeros(0, np.float32))
        rays = tr.make_rays(verts, idx, none, 256, seed=2000 + bs.CASES.index((kind, n)))
        keep = np.nonzero(np.isin(rays[3], CLASSES[kind]))[0][:N_RAYS_LARGE[n]]
        rays = tuple(np.ascontiguousarray(x[keep]) for x in rays)
        assert len(rays[0]) == N_RAYS_LARGE[n]
        truth = tr.closest_all(verts, idx, rays[0], rays[1])          # chunked over the rays: (1 << 22) / n of them at a time
        _LARGE[kind, n] = dict(rays=rays, truth=truth, e32=tr.e32_of(verts, idx, rays[0], rays[1], truth)[:2], digest=digest)
    assert _LARGE[kind, n]["digest"] == digest, "the flattened scene differs from the one the truth was computed for"
    return _LARGE[kind, n]


@pytest.mark.parametrize("builder", bs.BUILDERS)
@pytest.mark.parametrize("case", bs.CASES, ids=bs.case_id)
def test_device_build_writes_the_bytes_of_the_host_build(gpu, ora, case, builder):
    """Commit on the device with the builder's own scene builder, then ptc_scene_rebuild: both leave the bytes of the host's commit, and the tree traces right."""
    kind, n = case
    tag = "%s %d %s" % (kind, n, builder)
    dev = gpu.PathTracer(0).set_device_builder(builder).load_scene(_desc(gpu, kind, n, builder))
    _on_the_device(dev, builder)
    want, want_stats = _want(kind, n, builder)
    sd = dev.stats()
    for k in STATS:
        assert sd[k] == want_stats[k], k
    assert sd["n_triangles"] == n
    _same_bytes(want, _scene_bytes(dev), "commit: ")
    if n <= bs.TRACED:
        _hold_traced(tag + " commit", dev, kind, n, builder)
    dev.scene_rebuild()
    _on_the_device(dev, builder, "rebuild: ")
    _same_bytes(want, _scene_bytes(dev), "rebuild: ")
    if n <= bs.TRACED:
        _hold_traced(tag + " rebuild", dev, kind, n, builder)
    print(f"{tag}: commit on the device {sd['seconds_commit'] * 1e3:.2f} ms, rebuild {dev.stats()['seconds_rebuild'] * 1e3:.2f} ms")
    dev.close()


@pytest.mark.parametrize("builder", bs.BUILDERS)
@pytest.mark.parametrize("case", bs.LARGE_CASES, ids=bs.case_id)
def test_large_device_builds_trace_right(gpu, case, builder):
    """The three large soups (their bytes are held above; a test of their own keeps each within the time of the existing builder tests): the tree a rebuild on the
    device leaves answers closest-hit rays right against the float64 search of all triangles.  No oracle, no image."""
    kind, n = case
    dev = gpu.PathTracer(0).set_device_builder(builder).load_scene(_desc(gpu, kind, n, builder))
    _on_the_device(dev, builder)
    dev.scene_rebuild()
    verts, idx, _ = flat = dev.flat_scene()
    c = _large_case(kind, n, flat)
    t, prim, uv = dev.trace_closest(c["rays"][0], c["rays"][1])
    tr.assert_true("%s %d %s rebuild" % (kind, n, builder), verts, idx, c["rays"], c["truth"], c["e32"], t, prim, uv, None)
    dev.close()


@pytest.mark.parametrize("mode", ["lbvh", "sah", "alternating"])
def test_a_small_tree_after_a_large_one_on_the_same_context(gpu, mode):
    """The build scratch only grows and the two tree sets swap on every rebuild: one context commits and rebuilds build_sweep.WALK in order — 262,445 triangles,
    then 65, then soups of one triangle repeated, ... — so that whatever an earlier, larger build left behind (scratch beyond the new count, records beyond the new
    unit count, counters of levels the new tree does not have) lies under the smaller one.  `alternating` changes the device builder between the commits."""
    dev = gpu.PathTracer(0)
    for step, (kind, n) in enumerate(bs.WALK):
        builder = bs.BUILDERS[step % 2] if mode == "alternating" else mode
        tag = "step %d, %s %d %s: " % (step, kind, n, builder)
        dev.set_device_builder(builder).load_scene(_desc(gpu, kind, n, builder))
        _on_the_device(dev, builder, tag)
        want, want_stats = _want(kind, n, builder)
        sd = dev.stats()
        for k in STATS:
            assert sd[k] == want_stats[k], (tag, k)
        _same_bytes(want, _scene_bytes(dev), tag + "commit: ")
        dev.scene_rebuild()
        _on_the_device(dev, builder, tag + "rebuild: ")
        _same_bytes(want, _scene_bytes(dev), tag + "rebuild: ")
    dev.close()


@functools.lru_cache(maxsize=None)
def _soups():
    """The 40 soups of test_gpu_parity.test_random_scenes_are_bit_exact (the same generator and draws), each with a frame of at most 48 x 48."""
    import pbr_amd

    rng = np.random.default_rng(2024)
    out = []
    for k in range(40):
        d = tg._random_scene(pbr_amd.scene, rng, k)
        w, h = int(rng.integers(8, 70)), int(rng.integers(8, 70))
        _, mb, seed = int(rng.integers(1, 6)), int(rng.integers(0, 9)), int(rng.integers(0, 1 << 40))
        out.append((d, min(w, 48), min(h, 48), mb, seed))
    return out


@pytest.mark.parametrize("builder", bs.BUILDERS)
def test_random_soups_through_the_device_builders(gpu, ora, builder):
    """Degenerate and duplicate triangles, mirrored and sheared instances: committed and rebuilt on the device, the bytes of the host's commit; a small frame has
    the oracle's bits."""
    dev = gpu.PathTracer(0).set_device_builder(builder)
    for k, (d0, w, h, mb, seed) in enumerate(_soups()):
        d = copy.copy(d0)
        d.bvh_builder = builder
        tag = "soup %d %s: " % (k, builder)
        want, want_stats = _host(gpu, d)
        dev.load_scene(d)
        if want_stats["n_triangles"] >= 2:
            _on_the_device(dev, builder, tag)
        else:
            assert dev.internals()["commit_on_device"] == 0, tag
        sd = dev.stats()
        for key in STATS:
            assert sd[key] == want_stats[key], (tag, key)
        ref = ora.Oracle().load_scene(d).render(w, h, 2, seed=seed, max_bounces=mb)
        assert _bits(dev.render(w, h, 2, seed=seed, max_bounces=mb), ref), tag + "the frame differs from the oracle's"
        _same_bytes(want, _scene_bytes(dev), tag + "commit: ")
        dev.scene_rebuild()
        _same_bytes(want, _scene_bytes(dev), tag + "rebuild: ")
        assert _bits(dev.render(w, h, 2, seed=seed, max_bounces=mb), ref), tag + "the frame after the rebuild differs from the oracle's"
    dev.close()


@pytest.mark.parametrize("builder", bs.BUILDERS)
@pytest.mark.parametrize("case", [("uniform", 1024), ("uniform", 4097), ("same", 4097)], ids=bs.case_id)
def test_move_refit_then_rebuild_at_the_thresholds(gpu, case, builder):
    """One instance turned and scaled non-uniformly, a refit on the device, then the rebuild: the bytes of a fresh host commit of the moved description."""
    kind, n = case
    d = _desc(gpu, kind, n, builder)
    dev = gpu.PathTracer(0).set_device_builder(builder).load_scene(d)
    _on_the_device(dev, builder)
    a = 0.7
    ax = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    it = d.instances[0]
    it.t, it.q_wxyz, it.s = (0.05, -0.02, 0.03), (math.cos(a / 2), *(math.sin(a / 2) * ax)), (1.2, 0.8, 1.1)
    dev.update_instance(0, it.t, it.q_wxyz, it.s)
    dev.scene_refit()
    assert dev.internals()["refit_on_device"] == 1
    dev.scene_rebuild()
    _on_the_device(dev, builder, "rebuild: ")
    want, _ = _host(gpu, d)
    _same_bytes(want, _scene_bytes(dev), "after the move: ")
    assert not np.array_equal(want["verts"], _want(kind, n, builder)[0]["verts"])
    dev.close()
