"""The CPU anchor of the builder sweep (tests/build_sweep.py), without a GPU: what tests/test_gpu_build_sweep.py holds the device builders to is sound on these inputs.

For every case of at most 8,193 triangles and both builders, the host's build on a description-only context is a valid partition whose boxes contain their
triangles (tests/test_host_logic.py::_check_partition) and is the oracle's tree.  The three larger counts (131,072, 131,073 and 262,445 triangles; the last crosses
the host's threshold of 32,768 for splitting a range in parallel) are left out here: decoding and comparing the two structures in Python takes 10 to 30 s each.  They
were compared once when these cases were chosen: both builders' trees were the oracle's at all three counts, and _check_partition passed for all but `uniform` 131,073
with the SAH builder, where one leaf's lower y plane, taken exactly, lies 2^-30 (an eighth of an ulp of the coordinate) above a vertex at y = 0.0633...: quantize_planes
(csrc/pt_scene_rules.h) compares org + q * scale as rounded to float32.  Host and device share that rule, so it is no difference between them.

For every generic case the oracle's closest-hit and any-hit answers on 256 seeded rays (tests/trace_reference.py::make_rays with the box planes of both oracle trees:
interior, edge and vertex targets, misses, secondary rays) are right against the float64 search of all triangles, within trace_reference's own caps: the rays the
device answers in tests/test_gpu_build_sweep.py are rays for which the reference alone stays inside those caps.

  kind      classes of make_rays the case keeps
  uniform   interior, edge, vertex, miss.  No secondary rays: the scene is sparse, so a ray that leaves a surface point, like a ray to an edge or a vertex, mostly
            has nothing solid behind it and stays undecided; with all five classes 55 to 62 % of the rays are decided, on either side of the cap of 60 %
  line      all five
  geom      all five"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import build_sweep as bs  # noqa: E402
import trace_reference as tr  # noqa: E402
from test_host_logic import _canon, _check_partition, _decode_oracle, _decode_product  # noqa: E402

N_RAYS = 256
CLASSES = {"uniform": (tr.INTERIOR, tr.EDGE, tr.VERTEX, tr.MISS), "line": tuple(range(5)), "geom": tuple(range(5))}


def _desc(kind, n, builder):
    import pbr_amd

    d = bs.desc(pbr_amd, kind, n)
    d.bvh_builder = builder
    return d


@functools.lru_cache(maxsize=None)
def oracle_of(kind, n, builder):
    """The oracle holding the case with that builder's tree; shared, never changed."""
    from oracle import ora

    return ora.Oracle().load_scene(_desc(kind, n, builder))


@functools.lru_cache(maxsize=None)
def rays_of(kind, n):
    """One set of rays per case for both builders.  Generic kinds: make_rays, the float64 truth and E32.  Tie-heavy kinds (coincident triangles: the reference has
    nothing to say about which of them is hit): rays from around the camera, no truth."""
    from golden.make_golden import fixed_rays

    seed = 1000 + bs.CASES.index((kind, n))
    if kind not in bs.GENERIC:
        return dict(rays=fixed_rays(_desc(kind, n, None), n=N_RAYS + 37, seed=11), truth=None)
    oracles = [oracle_of(kind, n, b) for b in bs.BUILDERS]
    verts, idx, _ = oracles[0].flat_scene()
    pl = [tr.box_planes(o.bvh()[0]) for o in oracles]
    rays = tr.make_rays(verts, idx, (np.concatenate([p[0] for p in pl]), np.concatenate([p[1] for p in pl])), N_RAYS + N_RAYS // 2, seed)
    keep = np.nonzero(np.isin(rays[3], CLASSES[kind]))[0][:N_RAYS]
    rays = tuple(np.ascontiguousarray(x[keep]) for x in rays)
    assert len(rays[0]) == N_RAYS
    truth = tr.any_all(verts, idx, rays[0], rays[1], rays[2])
    return dict(rays=rays, truth=truth, verts=verts, idx=idx, e32=tr.e32_of(verts, idx, rays[0], rays[1], truth)[:2])


@functools.lru_cache(maxsize=None)
def oracle_answers(kind, n, builder):
    """(t, prim, uv, occluded, {the four traversal counters}) of the oracle on the case's rays."""
    o, r = oracle_of(kind, n, builder), rays_of(kind, n)["rays"]
    t, prim, uv = o.trace_closest(r[0], r[1])
    s = o.stats()
    counters = {k: s[k] for k in ("node_visits_closest", "tri_tests_closest")}
    occ = o.trace_any(r[0], r[1], r[2])
    s = o.stats()
    counters.update({k: s[k] for k in ("node_visits_any", "tri_tests_any")})
    return t, prim, uv, occ, counters


@pytest.mark.parametrize("builder", bs.BUILDERS)
@pytest.mark.parametrize("case", bs.SMALL_CASES, ids=bs.case_id)
def test_host_build_is_a_partition_and_the_oracles_tree(ora, pbr, case, builder):
    kind, n = case
    pt = pbr.PathTracer(pbr.DEVICE_NONE).load_scene(_desc(kind, n, builder))
    assert pt.stats()["n_triangles"] == n
    _check_partition(pt, "%s %d %s" % (kind, n, builder), n, None)
    o = oracle_of(kind, n, builder)
    v1, i1, m1 = pt.flat_scene()
    v2, i2, m2 = o.flat_scene()
    assert np.array_equal(v1.view(np.uint32), v2.view(np.uint32)) and np.array_equal(i1, i2) and np.array_equal(m1, m2)
    units, nn, nt, grid = pt.bvh()
    nodes, tris = o.bvh()
    assert nn == nodes.shape[0] and np.array_equal(_canon(_decode_product(units, nn, nt, grid)), _canon(_decode_oracle(nodes, tris)))
    s1, s2 = pt.stats(), o.stats()
    for k in ("n_triangles", "n_bvh_nodes", "n_emitters", "bvh_max_depth"):
        assert s1[k] == s2[k], k
    if kind != "degdupzero":                                                      # (whose last triangles are copies of zero-area ones)
        assert s1["n_emitters"] == max(1, n // 16)


@pytest.mark.parametrize("builder", bs.BUILDERS)
@pytest.mark.parametrize("case", [c for c in bs.SMALL_CASES if c[0] in bs.GENERIC], ids=bs.case_id)
def test_the_reference_decides_the_rays_of_the_generic_cases(ora, pbr, case, builder):
    """The oracle on the case's rays: 0 lost, 0 ghost, any-hit never wrong, the three caps held, every solid hit within 16 x E32."""
    kind, n = case
    c = rays_of(kind, n)
    rays = c["rays"]
    assert len(rays[0]) == N_RAYS and all((rays[3] == k).sum() > 0.04 * N_RAYS for k in CLASSES[kind])
    tr.assert_true("%s %d %s" % (kind, n, builder), c["verts"], c["idx"], rays, c["truth"], c["e32"], *oracle_answers(kind, n, builder)[:4])
