"""Adaptive sampling without a GPU: the symbols are declared, exported and bound, the defaults are the documented ones, a description-only context refuses
every new call with PTC_E_DEVICE, and the numpy mirror of the schedule (tests/adaptive_reference.py) has the properties the specification promises."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_reference as ref  # noqa: E402

NEW = ("ptc_adaptive_default_params", "ptc_frame_set_adaptive", "ptc_frame_adapt", "ptc_read_sample_counts", "ptc_render_adaptive", "ptc_get_adaptive_stats")
E_ARG, E_DEVICE = -1, -3


def test_symbols_are_declared_exported_and_bound(pbr):
    header = open(os.path.join(ROOT, "include", "ptc.h")).read()
    L = pbr.load_library()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in pbr.ptc.ABI_SYMBOLS and hasattr(L, sym), sym
    for struct in ("ptc_adaptive_params", "ptc_adaptive_stats"):
        assert re.search(r"typedef struct %s \{" % struct, header), struct
    assert "#define PTC_ABI_VERSION 4" in header and L.ptc_abi_version() == 4            # additive: the ABI version stays
    for m in ("adaptive_default_params", "frame_set_adaptive", "frame_adapt", "read_sample_counts", "render_adaptive", "adaptive_stats"):
        assert callable(getattr(pbr.PathTracer, m)), m
    assert C.sizeof(pbr.ptc.PtcStats) == 176                                              # ptc_stats keeps its layout


def test_default_parameters(pbr):
    d = pbr.PathTracer.adaptive_default_params()
    assert d == dict(threshold=float(np.float32(0.05)), radius=1, min_samples=16, step_samples=16)
    assert C.sizeof(pbr.ptc.PtcAdaptiveParams) == 16 and C.sizeof(pbr.ptc.PtcAdaptiveStats) == 40
    pbr.load_library().ptc_adaptive_default_params(None)                                  # a NULL pointer is ignored


def test_description_only_context_refuses_with_e_device(pbr):
    L = pbr.load_library()
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(pbr.scenes.cornell_box())
    h = pt._h
    p = pbr.ptc.PtcAdaptiveParams()
    L.ptc_adaptive_default_params(C.byref(p))
    n = C.c_uint64()
    counts = np.zeros((4, 4), np.uint32)
    st = pbr.ptc.PtcAdaptiveStats()
    calls = {
        "ptc_frame_set_adaptive": lambda c: L.ptc_frame_set_adaptive(c, C.byref(p)),
        "ptc_frame_set_adaptive (NULL parameters)": lambda c: L.ptc_frame_set_adaptive(c, None),
        "ptc_frame_adapt": lambda c: L.ptc_frame_adapt(c, C.byref(n)),
        "ptc_frame_adapt (NULL count)": lambda c: L.ptc_frame_adapt(c, None),
        "ptc_read_sample_counts": lambda c: L.ptc_read_sample_counts(c, counts.ctypes.data_as(C.POINTER(C.c_uint32))),
        "ptc_render_adaptive": lambda c: L.ptc_render_adaptive(c, 4, 4, 8, 1, 2, C.byref(p)),
        "ptc_get_adaptive_stats": lambda c: L.ptc_get_adaptive_stats(c, C.byref(st)),
    }
    for name, call in calls.items():
        assert call(h) == E_DEVICE, name
        assert b"PTC_DEVICE_NONE" in L.ptc_last_error(h), name
        assert call(None) == E_ARG, name
    with pytest.raises(pbr.PtcError, match="ptc error -3"):
        pt.render_adaptive(4, 4, 8)
    with pytest.raises(pbr.PtcError, match="ptc error -3"):
        pt.frame_adapt()
    with pytest.raises(TypeError):
        pt.frame_set_adaptive(sigma=1.0)


# ---- properties of the reference schedule on synthetic per-sample radiances ----------------------------------------------------------------------------
def _synthetic(h, w, K, seed=3):
    """A noisy image whose noise level varies over the frame: flat and quiet on the left, rough on the right, one dark band"""
    rng = np.random.default_rng(seed)
    xs = np.linspace(0.0, 1.0, w)[None, :, None]
    base = 0.2 + 0.8 * rng.random((h, w, 3))
    sigma = (0.02 + 1.5 * xs ** 3) * base
    L = base[None] + sigma[None] * rng.standard_normal((K, h, w, 3))
    L = np.maximum(L, 0.0)
    L[:, h // 3: h // 3 + 4] *= 0.01
    return L.astype(np.float32)


@pytest.mark.parametrize("radius", (0, 1, 2))
def test_active_set_only_shrinks(radius):
    h, w, K = 50, 75, 64
    s = ref.Schedule(_synthetic(h, w, K), 0.05, radius, K)
    s.add(8)
    prev = s.active.copy()
    while True:
        n = s.adapt()
        assert not (s.active & ~prev).any()                    # nothing comes back
        assert n == int(s.active.sum()) <= int(prev.sum())
        assert (s.count[s.active] == s.done).all()             # every active pixel has count = samples added
        prev = s.active.copy()
        if not n:
            break
        s.add(min(8, K - s.done))
    assert sorted(s.history, reverse=True) == s.history
    shares = ref.distinct_counts(s.count)
    assert len(shares) >= 3 and min(s.count.ravel()) >= 8 and max(s.count.ravel()) == K
    assert np.array_equal(s.image()[..., :3][s.count == K], ref.sample_order_mean(s.L, K)[s.count == K])


def test_wider_radius_keeps_more():
    L = _synthetic(64, 64, 32)
    counts = [ref.Schedule(L, 0.05, r, 32).run(8, 8) for r in (0, 1, 2)]
    assert (counts[0] <= counts[1]).all() and (counts[1] <= counts[2]).all()
    assert counts[0].sum() < counts[2].sum()


def test_zero_threshold_never_stops_before_the_budget():
    L = _synthetic(40, 40, 24)
    assert (luminance_spread(L) > 0).all()                     # noisy everywhere: every pixel's estimate has a positive variance
    s = ref.Schedule(L, 0.0, 0, 24)
    assert (s.run(5, 7) == 24).all() and s.history[:-1] == [1600] * (len(s.history) - 1) and s.history[-1] == 0
    assert np.array_equal(s.image()[..., :3], ref.sample_order_mean(L, 24))


def luminance_spread(L):
    l = ref.luminance(L[:5])
    return l.max(0) - l.min(0)


def test_huge_threshold_stops_everything_at_the_first_step():
    L = _synthetic(40, 40, 24)
    s = ref.Schedule(L, 1e30, 2, 24)
    assert (s.run(6, 6) == 6).all() and s.history == [0] and s.passes == 1
    s.add(6)                                                   # nothing is active: accepted, nothing happens
    assert (s.count == 6).all() and s.done == 6 and s.adapt() == 0


@pytest.mark.parametrize("ranks", (2, 3))
@pytest.mark.parametrize("radius", (0, 1, 2))
def test_tile_owners_compute_the_whole_frames_counts(ora, ranks, radius):
    """The neighbourhood stops at the ownership tile, so every rank of a tile-sharded frame decides exactly as the whole frame does."""
    h, w, K = 50, 75, 48
    L = _synthetic(h, w, K, seed=5)
    whole = ref.Schedule(L, 0.05, radius, K).run(8, 8)
    owner = np.array([[ora.tile_owner(w, h, x, y, ranks) for x in range(w)] for y in range(h)])
    assert set(np.unique(owner)) == set(range(ranks))
    total = np.zeros_like(whole)
    for r in range(ranks):
        part = ref.Schedule(L, 0.05, radius, K, owned=owner == r).run(8, 8)
        assert (part[owner != r] == 0).all()
        total += part
    assert np.array_equal(total, whole)
    assert len(ref.distinct_counts(whole)) >= 3
