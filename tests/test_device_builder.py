"""ptc_set_device_builder (include/ptc.h): the tree a build ON THE DEVICE makes — the LBVH by default, or the host's binned-SAH tree.  What can be held without
a GPU: the symbol is exported and bound, the setting takes PTC_BVH_SAH / PTC_BVH_LBVH and refuses anything else with PTC_E_ARG (the setting and the context
unharmed), and a description-only context takes the setting and still commits on the host, the bytes of the default context's commit with either scene builder.
The device side is tests/test_gpu_device_sah.py."""
import copy

import numpy as np
import pytest

PTC_E_ARG = -1


def _scene_bytes(pt):
    units, nn, nt, grid = pt.bvh()
    shade, lights, cdf = pt.shading_tables()
    v, i, m = pt.flat_scene()
    return {"units": units.view(np.uint32), "grid": np.asarray(grid), "shade": shade.view(np.uint32), "lights": lights.view(np.uint32), "cdf": cdf.view(np.uint32),
            "verts": v.view(np.uint32), "idx": i, "mat": m, "counts": np.array([nn, nt])}


def test_set_device_builder_is_exported_and_bound(pbr):
    L = pbr.load_library()
    assert hasattr(L, "ptc_set_device_builder")
    assert "ptc_set_device_builder" in pbr.ptc.ABI_SYMBOLS
    assert L.ptc_abi_version() == 4
    assert hasattr(pbr.PathTracer, "set_device_builder")


def test_set_device_builder_accepts_the_two_builders_and_refuses_the_rest(pbr):
    L = pbr.load_library()
    pt = pbr.PathTracer(pbr.DEVICE_NONE)
    h = pt._h
    assert L.ptc_set_device_builder(h, 0) == 0 and L.ptc_set_device_builder(h, 1) == 0
    for bad in (2, -1, 7):
        assert L.ptc_set_device_builder(h, bad) == PTC_E_ARG
        assert b"set_device_builder" in L.ptc_last_error(h)
    assert L.ptc_set_device_builder(None, 0) == PTC_E_ARG
    with pytest.raises(KeyError):
        pt.set_device_builder("ploc")
    # the context is still usable after the refusals
    pt.set_device_builder("sah").set_device_builder("lbvh")
    pt.load_scene(pbr.scenes.cornell_box())
    assert pt.stats()["n_triangles"] > 0


@pytest.mark.parametrize("builder", ["sah", "lbvh"])
@pytest.mark.parametrize("name,kw", [("cornell", {}), ("sphere10k", {}), ("atrium", {"scale": 0.02})])
def test_description_only_context_commits_on_the_host_with_either_device_builder(pbr, name, kw, builder):
    d = copy.deepcopy(pbr.scenes.by_name(name, **kw))
    d.bvh_builder = builder
    want = _scene_bytes(pbr.PathTracer(pbr.DEVICE_NONE).load_scene(d))
    for dev_builder in ("sah", "lbvh"):
        pt = pbr.PathTracer(pbr.DEVICE_NONE).set_device_builder(dev_builder)
        pt.load_scene(d)
        got = _scene_bytes(pt)
        for key in want:
            assert want[key].shape == got[key].shape and np.array_equal(want[key], got[key]), f"{dev_builder}: {key} differs"
        it = pt.internals()
        assert it["commit_on_device"] == 0 and it["device_build_sah"] == 0 and it["refit_on_device"] == 0
