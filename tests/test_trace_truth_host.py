"""The oracle's closest-hit and any-hit answers against a float64 search of all triangles (tests/trace_reference.py), without a GPU: scenes x builders x
(after the commit, after a refit of moved instances); and the checker itself against answers with one thing altered at a time.  The kernels reproduce
the oracle bit for bit (tests/test_gpu_parity.py), and tests/test_gpu_trace_truth.py holds them to the same reference on the device."""
import copy
import dataclasses
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deform_reference as dref  # noqa: E402
import trace_reference as tr  # noqa: E402

SCENES = ("cornell", "sphere10k", "atrium", "textured_objects", "deform")
N_RAYS = {"cornell": 3000}


def scene_desc(pbr, name):
    if name == "deform":                                     # tests/deform_reference.scene in pose "a", as the plain meshes a commit of the posed scene is
        sc = dref.scene(pbr)
        return dref.plain_desc(sc.desc, dref.posed_vertices(sc.desc, sc.poses["a"]))
    return pbr.scenes.by_name(name, **({"scale": 0.05} if name == "atrium" else {}))


def shear_matrix(k, t):
    """column-major 4x4 with rotation, non-uniform scale AND shear: no (t, q, s) gives it"""
    a = 0.5 + k
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    m = np.eye(4)
    m[:3, :3] = R @ np.diag([1.2, 0.8, 1.1]) @ np.array([[1, 0.3, 0], [0, 1, 0], [0, 0.2, 1]])
    m[:3, 3] = t
    return m.T.reshape(16).astype(np.float32)


def instance_moves(desc):
    """[(instance, keywords of update_instance)]: about seven instances of the scene rotated, scaled non-uniformly and shifted, the last of them given by a
    matrix with shear."""
    ni = len(desc.instances)
    picks = list(range(0, ni, max(1, ni // 7)))
    moves = []
    for k in picks:
        t0 = np.asarray(desc.instances[k].t, np.float64)
        t = tuple(float(x) for x in t0 + (0.07 * (k % 5) - 0.1, 0.05, -0.08))
        if k == picks[-1]:
            moves.append((k, dict(matrix=shear_matrix(k, t))))
        else:
            moves.append((k, dict(t=t, q_wxyz=(math.cos(0.15 + 0.1 * k), 0.0, math.sin(0.15 + 0.1 * k), 0.0), s=(1.2, 0.8, 1.1))))
    return moves


def move_instances(ctx, desc, how="scene_refit"):
    """instance_moves applied to a committed Oracle or PathTracer (the same calls), then the refit (or `how`)."""
    for k, kw in instance_moves(desc):
        ctx.update_instance(k, **kw)
    getattr(ctx, how)()
    return ctx


def moved_desc(desc):
    """The description a fresh commit of the moved scene takes."""
    d = copy.copy(desc)
    d.instances = list(desc.instances)
    for k, kw in instance_moves(desc):
        d.instances[k] = dataclasses.replace(desc.instances[k], **kw)
    return d


@functools.lru_cache(maxsize=None)
def _case(scene, state):
    """Both builders' oracles of the scene in that state, ONE set of rays (box planes of both trees) and its truth, computed once."""
    import pbr_amd as pbr
    from oracle import ora

    oracles = {}
    for builder in ("sah", "lbvh"):
        d = scene_desc(pbr, scene)
        d.bvh_builder = builder
        o = ora.Oracle().load_scene(d)
        if state == "refit":
            move_instances(o, d)
        oracles[builder] = o
    verts, idx, _ = oracles["sah"].flat_scene()
    v2, i2, _ = oracles["lbvh"].flat_scene()
    assert np.array_equal(verts.view(np.uint32), v2.view(np.uint32)) and np.array_equal(idx, i2)
    pl = [tr.box_planes(o.bvh()[0]) for o in oracles.values()]
    planes = (np.concatenate([p[0] for p in pl]), np.concatenate([p[1] for p in pl]))
    rays = tr.make_rays(verts, idx, planes, N_RAYS.get(scene, 1500), seed=SCENES.index(scene) * 2 + (state == "refit") + 100)
    truth = tr.any_all(verts, idx, rays[0], rays[1], rays[2])
    e32 = tr.e32_of(verts, idx, rays[0], rays[1], truth)
    return dict(oracles=oracles, verts=verts, idx=idx, rays=rays, truth=truth, e32=e32)


def _answers(o, rays):
    t, prim, uv = o.trace_closest(rays[0], rays[1])
    return t, prim, uv, o.trace_any(rays[0], rays[1], rays[2])


@pytest.mark.parametrize("state", ["commit", "refit"])
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
@pytest.mark.parametrize("scene", SCENES)
def test_oracle_against_all_triangles(ora, pbr, scene, builder, state):
    """0 lost, 0 ghost, any-hit never wrong, the three caps held, every solid hit within 16 x E32."""
    c = _case(scene, state)
    rays = c["rays"]
    assert ((rays[1] == 0).any(1)).sum() > 0.1 * len(rays[0]) and (np.abs(rays[1]) < 1e-20).any() and np.signbit(rays[1][rays[1] == 0]).any()
    assert all((rays[3] == k).sum() > 0.05 * len(rays[0]) for k in range(5))
    tr.assert_true("%s %s %s" % (scene, builder, state), c["verts"], c["idx"], rays, c["truth"], c["e32"][:2], *_answers(c["oracles"][builder], rays))


def test_the_refit_moved_the_triangles_and_the_matrix_instance_is_sheared(ora, pbr):
    a, b = _case("sphere10k", "commit"), _case("sphere10k", "refit")
    assert not np.array_equal(a["verts"][:, :3], b["verts"][:, :3])
    m = shear_matrix(4, (0, 0, 0)).reshape(4, 4).T[:3, :3].astype(np.float64)
    g = m.T @ m                                                 # R S has orthogonal columns; a sheared matrix has not
    assert abs(g[0, 1]) > 0.1 * math.sqrt(g[0, 0] * g[1, 1])


# ---- the checker has teeth ---------------------------------------------------------------------------------------------------------------
def _altered(c, answers, pick, change):
    """`change(t, prim, uv, occ, rows)` alters copies of the oracle's answers on the rays `pick`; returns (reported per ray, rows)."""
    rows = np.nonzero(pick)[0]
    assert len(rows) >= 20, "too few decided rays to alter: %d" % len(rows)
    t, prim, uv, occ = (x.copy() for x in answers)
    change(t, prim, uv, occ, rows)
    lost, ghost, wrong = tr.check("altered", c["verts"], c["idx"], c["rays"], c["truth"], c["e32"][:2], t, prim, uv, occ, caps=False)
    return lost, ghost, wrong, rows


@pytest.mark.parametrize("scene", ["sphere10k", "atrium"])
def test_every_altered_answer_is_reported(ora, pbr, scene):
    c = _case(scene, "commit")
    ans = _answers(c["oracles"]["sah"], c["rays"])
    t0, prim0, uv0, occ0 = ans
    truth, rays = c["truth"], c["rays"]
    lost, ghost, wrong = tr.check("unaltered", c["verts"], c["idx"], rays, truth, c["e32"][:2], *ans)
    assert not lost.any() and not ghost.any() and not wrong.any()
    t64, _, _, m, g, mg = tr.pair_at(c["verts"], c["idx"], rays[0], rays[1], prim0)
    own_solid = tr._classes(t64, m, g, mg)[0] & (prim0 >= 0)                 # the oracle's own hit is a solid pair: the accuracy rule applies to it
    assert c["e32"][0] * tr.ACCURACY < 1e-3 / 4                              # what the accuracy rule allows is well below the alteration of t

    def drop(t, prim, uv, occ, r):
        t[r], prim[r], uv[r] = -1.0, -1, 0.0
    lost, ghost, wrong, r = _altered(c, ans, truth.prim >= 0, drop)
    assert lost[r].all() and lost.sum() == len(r) and not ghost.any()

    for f in (1 - 1e-3, 1 + 1e-3):
        def scale(t, prim, uv, occ, r, f=f):
            t[r] = (t[r].astype(np.float64) * f).astype(np.float32)
        lost, ghost, wrong, r = _altered(c, ans, own_solid, scale)
        assert (lost | ghost)[r].all() and ghost[r].all() and (lost | ghost).sum() == len(r)

    # the next solid hit behind, reported consistently (its own float32 t, u, v): nothing is wrong with that pair, it is just not the closest
    behind = (truth.prim2 >= 0) & (truth.t2 > truth.t * 1.01)
    t2, u2, v2, _, _, _ = tr.pair_at(c["verts"], c["idx"], rays[0], rays[1], truth.prim2, np.float32)

    def swap_prim(t, prim, uv, occ, r):
        t[r], prim[r], uv[r, 0], uv[r, 1] = t2[r], truth.prim2[r], u2[r], v2[r]
    lost, ghost, wrong, r = _altered(c, ans, behind, swap_prim)
    assert lost[r].all() and lost.sum() == len(r)

    def swap_uv(t, prim, uv, occ, r):
        uv[r] = uv[r][:, ::-1]
    lost, ghost, wrong, r = _altered(c, ans, own_solid & (np.abs(uv0[:, 0] - uv0[:, 1]) > max(1e-2, 4 * tr.ACCURACY * c["e32"][1])), swap_uv)
    assert ghost[r].all() and ghost.sum() == len(r) and not lost.any()

    def flip(t, prim, uv, occ, r):
        occ[r] = 1 - occ[r]
    for pick in (truth.must_block, ~truth.may_block):
        lost, ghost, wrong, r = _altered(c, ans, pick, flip)
        assert wrong[r].all() and wrong.sum() == len(r) and not lost.any() and not ghost.any()


def test_a_scene_that_lacks_a_triangle_is_reported(ora, pbr):
    """The oracle's answers for the Cornell box WITHOUT one triangle of its back wall, held against the truth of the whole box: every ray whose nearest
    solid hit is that triangle is reported, by closest hit (nothing lies behind the wall) and by any-hit."""
    full = pbr.scenes.cornell_box()
    verts, idx, _ = ora.Oracle().load_scene(full).flat_scene()
    a, b, c3 = tr.triangles(verts, idx)
    back = [k for k in range(len(a)) if (a[k, 2], b[k, 2], c3[k, 2]) == (-1.0, -1.0, -1.0)]
    gone = back[0]
    part = copy.deepcopy(full)
    mesh = [m for m, me in enumerate(part.meshes) if (np.asarray(me.vertices["position"])[:, 2] == -1.0).all()][0]
    part.meshes[mesh] = dataclasses.replace(part.meshes[mesh], indices=np.asarray(part.meshes[mesh].indices)[3:])
    o = ora.Oracle().load_scene(part)
    assert o.stats()["n_triangles"] == len(a) - 1
    first = sum(len(me.indices) // 3 for me in part.meshes[:mesh])
    assert gone == first                                                     # the removed triangle was the mesh's first: later ids shift by one
    rng = np.random.default_rng(3)
    bary = rng.dirichlet((2.0, 2.0, 2.0), 40)
    tgt = a[gone] * bary[:, 0:1] + b[gone] * bary[:, 1:2] + c3[gone] * bary[:, 2:3]
    org = rng.uniform((-0.8, -0.8, 0.0), (0.8, 0.8, 3.0), (40, 3)).astype(np.float32)
    d = tgt - org
    length = np.linalg.norm(d, axis=1)
    rays = (org, (d / length[:, None]).astype(np.float32), (2 * length).astype(np.float32), np.zeros(40, np.int64))
    truth = tr.any_all(verts, idx, *rays[:3])
    e32 = tr.e32_of(verts, idx, rays[0], rays[1], truth)
    aimed = truth.prim == gone
    assert aimed.sum() >= 20
    t, prim, uv, occ = _answers(o, rays)
    prim = np.where(prim >= gone, prim + 1, prim)
    lost, ghost, wrong = tr.check("cornell less one triangle", verts, idx, rays, truth, e32[:2], t, prim, uv, occ, caps=False)
    assert lost[aimed].all() and wrong[aimed].all() and not lost[~aimed].any() and not ghost.any() and not wrong[~aimed].any()
