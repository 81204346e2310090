"""The binned-SAH tree built ON THE DEVICE (ptc_set_device_builder(PTC_BVH_SAH); csrc/pt_build.hip pt_build_sah) on a real MI355X.

The contract is the one of every device build here: the bytes of the host's build.  A SAH commit with the SAH device builder leaves in HBM the unit array, origin grid,
shading records, emitter table, cdf and world vertices of the host's SAH commit (which tests/test_host_logic.py holds against the oracle, tree for tree); a rebuild with it
leaves the bytes of a fresh host SAH commit of the geometry as it lies; images and all nine traversal counters are the oracle's SAH.  The LBVH default is unchanged, a
group commit keeps its host build.  The scenes here have 2, 12, 302, 640, a few thousand and 249,936 triangles; tests/test_gpu_build_sweep.py holds the same bytes at the
counts where the kernels change path and on soups of coincident triangles."""
import copy
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("_gpu_parity", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_parity.py"))
tg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tg)
COUNTERS, _scene_bytes = tg.COUNTERS, tg._scene_bytes


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _same_bytes(want, got, what=""):
    for key in want:
        assert want[key].shape == got[key].shape and np.array_equal(want[key], got[key]), \
            f"{what}{key} differs in {int((want[key] != got[key]).sum()) if want[key].shape == got[key].shape else -1} words"


def _planar_scene(gpu):
    """640 triangles in the plane z = -0.5, one to a cell of a 32 x 20 grid (no two overlap: closest hit has no ties), the last 40 emissive: the z axis takes part
    in no cut."""
    sc = gpu.scene
    d = gpu.scenes.cornell_box()
    rng = np.random.default_rng(11)
    cells = [(i, j) for j in range(20) for i in range(32)]
    meshes = []
    for part, mat in ((cells[:600], 0), (cells[600:], 3)):
        n = len(part)
        pos = np.zeros((3 * n, 3), np.float32)
        for t, (i, j) in enumerate(part):
            u = rng.uniform(0.1, 0.9, (3, 2))
            pos[3 * t:3 * t + 3, 0] = -0.9 + (i + u[:, 0]) * (1.8 / 32)
            pos[3 * t:3 * t + 3, 1] = -0.9 + (j + u[:, 1]) * (1.8 / 20)
        pos[:, 2] = -0.5
        v = np.zeros(3 * n, sc.MESH_VERTEX)
        v["position"], v["normal"], v["tangent"] = pos, (0, 0, 1), (1, 0, 0, 1)
        meshes.append(sc.MeshDesc(v, np.arange(3 * n, dtype=np.uint32), mat))
    return sc.SceneDesc(d.materials, meshes, [sc.InstanceDesc(0, (0, 0, 0), (1, 0, 0, 0), (1, 1, 1)), sc.InstanceDesc(1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 1))],
                        d.camera, "planar")


def _scene(gpu, name, kw):
    if name == "coincident":
        return copy.deepcopy(tg._coincident_scene(gpu))
    if name == "planar":
        return copy.deepcopy(_planar_scene(gpu))
    return copy.deepcopy(gpu.scenes.by_name(name, **kw))


def _two_triangle_scene(gpu):
    sc = gpu.scene
    d = gpu.scenes.cornell_box()
    m = d.meshes[5]
    return sc.SceneDesc([d.materials[3]], [sc.MeshDesc(m.vertices.copy(), np.asarray(m.indices, np.uint32).copy(), 0)],
                        [sc.InstanceDesc(0, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))], d.camera, "two")


COMMIT_CASES = [("cornell", {}), ("sphere10k", {}), ("atrium", {"scale": 0.05}), ("textured_atrium", {"scale": 0.05, "tex_size": 64, "env_size": (64, 32)}),
                ("textured_objects", {}), ("coincident", {}), ("planar", {}), ("atrium", {})]


@pytest.mark.parametrize("name,kw", COMMIT_CASES)
def test_sah_commit_on_the_device_writes_the_bytes_of_the_host_sah_commit(gpu, ora, name, kw):
    """A SAH scene committed with the SAH device builder: flattened, shaded and built on the device; every array in HBM is the host SAH commit's (on the same device and on a
    description-only context); statistics, image bits and the nine counters agree, the counters with the oracle's SAH tree."""
    d = _scene(gpu, name, kw)
    d.bvh_builder = "sah"
    dev = gpu.PathTracer(0).set_device_builder("sah").load_scene(d)
    it = dev.internals()
    assert it["commit_on_device"] == 1 and it["device_build_sah"] == 1
    host = gpu.PathTracer(0).load_scene(d)                       # the default device builder: the SAH commit stays on the host
    assert host.internals()["commit_on_device"] == 0 and host.internals()["device_build_sah"] == 0
    sd, sh = dev.stats(), host.stats()
    for key in ("n_triangles", "n_bvh_nodes", "n_emitters", "bvh_max_depth", "bvh_sa_cost", "bvh_sa_cost_built"):
        assert sd[key] == sh[key], key
    for key in ("trace_blocks_per_cu", "stack_lds"):
        assert dev.internals()[key] == host.internals()[key], key
    w, h = 96, 54
    gd, gh = dev.render(w, h, 2, seed=7, max_bounces=4), host.render(w, h, 2, seed=7, max_bounces=4)
    assert _bits_equal(gd, gh)
    o = ora.Oracle().load_scene(d)
    assert _bits_equal(gd, o.render(w, h, 2, seed=7, max_bounces=4))
    sg, so = dev.stats(), o.stats()
    for key in COUNTERS:
        assert sg[key] == so[key], key
    a, b, c = _scene_bytes(dev), _scene_bytes(host), _scene_bytes(gpu.PathTracer(gpu.DEVICE_NONE).load_scene(d))
    _same_bytes(b, a)
    _same_bytes(c, a, "against the description-only context: ")
    # the same context commits again: the first commit is released, the second is the same tree
    dev.load_scene(d)
    assert dev.internals()["commit_on_device"] == 1 and dev.internals()["device_build_sah"] == 1
    _same_bytes(b, _scene_bytes(dev), "second commit: ")
    print(f"{name}: {sd['n_triangles']} triangles, SAH commit on the device {sd['seconds_commit'] * 1e3:.2f} ms (replacing {dev.stats()['seconds_commit'] * 1e3:.2f} ms), "
          f"on the host {sh['seconds_commit'] * 1e3:.2f} ms")


def _move(dev, d, rng):
    """Moves a third of the instances of `d` (in place) and of the context."""
    for i, it in enumerate(d.instances):
        if i % 3 == 0:
            a = 1.3 + 0.1 * i
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            if getattr(it, "matrix", None) is not None:
                r = np.eye(4, dtype=np.float32); r[0, 0] = r[2, 2] = math.cos(a); r[0, 2] = -math.sin(a); r[2, 0] = math.sin(a)
                it.matrix = (np.asarray(it.matrix, np.float32).reshape(4, 4) @ r).astype(np.float32).reshape(16)
                dev.update_instance(i, matrix=it.matrix)
            else:
                it.q_wxyz = (math.cos(a / 2), *(math.sin(a / 2) * ax))
                it.s = tuple(np.float32(x) * np.float32(1.0 + 0.2 * (k == 1)) for k, x in enumerate(it.s))
                dev.update_instance(i, it.t, it.q_wxyz, it.s)


@pytest.mark.parametrize("name,kw,commit_builder", [("atrium", {"scale": 0.05}, "sah"), ("atrium", {"scale": 0.05}, "lbvh"), ("textured_objects", {}, "sah"),
                                                     ("coincident", {}, "lbvh"), ("planar", {}, "sah"), ("atrium", {}, "sah")])
def test_sah_rebuild_on_the_device_writes_the_bytes_of_a_fresh_host_sah_commit(gpu, ora, name, kw, commit_builder):
    """ptc_scene_rebuild with the SAH device builder, whatever builder the commit used: the bytes of a fresh host SAH commit — right after the commit and after a third of the
    instances moved (counters then the oracle's SAH of the moved scene).  A refit after it runs on the device; PTC_REBUILD=host builds the same SAH tree on the host; a host-path
    refit renders the same image.  Set back to the LBVH, the same context commits a SAH scene on the host and rebuilds the LBVH, as before."""
    d = _scene(gpu, name, kw)
    d.bvh_builder = commit_builder
    dev = gpu.PathTracer(0).set_device_builder("sah").load_scene(d)
    assert dev.internals()["device_build_sah"] == (1 if commit_builder == "sah" else 0)
    d_s = copy.deepcopy(d); d_s.bvh_builder = "sah"
    w, h = 96, 54
    img0 = dev.render(w, h, 2, seed=7, max_bounces=4)
    dev.scene_rebuild()
    assert dev.internals()["device_build_sah"] == 1
    _same_bytes(_scene_bytes(gpu.PathTracer(gpu.DEVICE_NONE).load_scene(d_s)), _scene_bytes(dev))
    st = dev.stats()
    assert st["seconds_rebuild"] > 0.0 and st["bvh_sa_cost"] == st["bvh_sa_cost_built"] > 0.0
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), img0)
    first_rebuild_ms = st["seconds_rebuild"] * 1e3
    _move(dev, d_s, np.random.default_rng(3))
    dev.scene_refit()
    assert dev.internals()["refit_on_device"] == 1 and dev.internals()["device_build_sah"] == 1
    o = ora.Oracle().load_scene(d_s)
    ref = o.render(w, h, 2, seed=7, max_bounces=4)
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), ref)
    dev.scene_rebuild()
    want = _scene_bytes(gpu.PathTracer(gpu.DEVICE_NONE).load_scene(d_s))
    _same_bytes(want, _scene_bytes(dev), "after the move: ")
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), ref)
    sg, so = dev.stats(), o.stats()
    for key in COUNTERS:
        assert sg[key] == so[key], key
    moved_rebuild_ms = sg["seconds_rebuild"] * 1e3
    dev.scene_refit()
    assert dev.internals()["refit_on_device"] == 1
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), ref)
    os.environ["PTC_REFIT"] = "host"
    try:
        dev.scene_refit()
    finally:
        del os.environ["PTC_REFIT"]
    assert dev.internals()["refit_on_device"] == 0
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), ref)
    os.environ["PTC_REBUILD"] = "host"
    try:
        dev.scene_rebuild()
    finally:
        del os.environ["PTC_REBUILD"]
    assert dev.internals()["device_build_sah"] == 0
    _same_bytes(want, _scene_bytes(dev), "PTC_REBUILD=host: ")
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), ref)
    dev.scene_rebuild()                                          # the device again, over the host's build
    _same_bytes(want, _scene_bytes(dev), "device rebuild after a host build: ")
    print(f"{name} ({commit_builder} commit): {st['n_triangles']} triangles, SAH rebuild on the device {first_rebuild_ms:.2f} ms, after the move {moved_rebuild_ms:.2f} ms")
    # the default again: a SAH commit goes to the host, the rebuild makes the LBVH
    dev.set_device_builder("lbvh")
    dev.load_scene(d_s)
    assert dev.internals()["commit_on_device"] == 0 and dev.internals()["device_build_sah"] == 0
    _same_bytes(want, _scene_bytes(dev), "host SAH commit: ")
    dev.scene_rebuild()
    assert dev.internals()["device_build_sah"] == 0
    d_l = copy.deepcopy(d_s); d_l.bvh_builder = "lbvh"
    _same_bytes(_scene_bytes(gpu.PathTracer(gpu.DEVICE_NONE).load_scene(d_l)), _scene_bytes(dev), "LBVH rebuild: ")


def test_sah_device_builder_edges(gpu, ora):
    """A single triangle commits on the host, two on the device; an instance whose positions overflow is refused with the host path's words and the context commits again;
    two lanes; a scene lit by its environment alone; the LBVH scene builder still commits the LBVH on the device."""
    sc = gpu.scene
    one = copy.deepcopy(tg._single_triangle_scene(gpu)); one.bvh_builder = "sah"
    pt, o = gpu.PathTracer(0).set_device_builder("sah").load_scene(one), ora.Oracle().load_scene(one)
    assert pt.internals()["commit_on_device"] == 0
    assert _bits_equal(pt.render(32, 32, 2, seed=1, max_bounces=2), o.render(32, 32, 2, seed=1, max_bounces=2))
    two = _two_triangle_scene(gpu); two.bvh_builder = "sah"
    pt, o = gpu.PathTracer(0).set_device_builder("sah").load_scene(two), ora.Oracle().load_scene(two)
    assert pt.internals()["commit_on_device"] == 1 and pt.internals()["device_build_sah"] == 1
    assert _bits_equal(pt.render(32, 32, 2, seed=1, max_bounces=2), o.render(32, 32, 2, seed=1, max_bounces=2))
    _same_bytes(_scene_bytes(gpu.PathTracer(gpu.DEVICE_NONE).load_scene(two)), _scene_bytes(pt))
    bad = copy.deepcopy(gpu.scenes.by_name("cornell")); bad.bvh_builder = "sah"
    big = np.eye(4, dtype=np.float32); big[0, 0] = 3e38; big[3, 0] = 3e38
    bad.instances[2] = sc.InstanceDesc(bad.instances[2].mesh, matrix=big.reshape(16))
    ctx = gpu.PathTracer(0).set_device_builder("sah")
    with pytest.raises(gpu.PtcError, match="non-finite"):
        ctx.load_scene(bad)
    ok = copy.deepcopy(gpu.scenes.by_name("cornell")); ok.bvh_builder = "sah"
    ref = ora.Oracle().load_scene(ok).render(48, 48, 2, seed=4, max_bounces=4)
    assert _bits_equal(ctx.load_scene(ok).render(48, 48, 2, seed=4, max_bounces=4), ref) and ctx.internals()["device_build_sah"] == 1
    ok.bvh_builder = "lbvh"
    assert _bits_equal(ctx.load_scene(ok).render(48, 48, 2, seed=4, max_bounces=4), ref)
    assert ctx.internals()["commit_on_device"] == 1 and ctx.internals()["device_build_sah"] == 0      # an LBVH scene commits the LBVH
    d = copy.deepcopy(gpu.scenes.by_name("textured_objects")); d.bvh_builder = "sah"
    d.materials = [copy.copy(m) for m in d.materials]
    for m in d.materials:
        m.emissive = (0.0, 0.0, 0.0)
    if getattr(d, "env", None) is None:
        d.env = np.random.default_rng(2).uniform(0.0, 2.0, (16, 32, 3)).astype(np.float32)
    pt, o = gpu.PathTracer(0).set_device_builder("sah").load_scene(d), ora.Oracle().load_scene(d)
    assert pt.internals()["device_build_sah"] == 1 and pt.stats()["n_emitters"] == 0
    c = o.render(64, 48, 2, seed=5, max_bounces=3)
    assert _bits_equal(pt.render(64, 48, 2, seed=5, max_bounces=3), c) and all(pt.stats()[k] == o.stats()[k] for k in COUNTERS)
    os.environ["PTC_LANES"] = "2"
    try:
        lanes2 = gpu.PathTracer(0)
    finally:
        del os.environ["PTC_LANES"]
    lanes2.set_device_builder("sah").load_scene(d)
    assert lanes2.internals()["device_build_sah"] == 1 and _bits_equal(lanes2.render(64, 48, 2, seed=5, max_bounces=3), c)
    os.environ["PTC_DEVICE_BVH"] = "sah"
    try:
        from_env = gpu.PathTracer(0)
    finally:
        del os.environ["PTC_DEVICE_BVH"]
    assert from_env.load_scene(d).internals()["device_build_sah"] == 1


def test_group_commit_keeps_its_host_build_with_the_sah_device_builder(gpu, ora):
    """ptc_group_scene_commit shares one host build: with the SAH device builder set on device 0, the group's commit is made on the host."""
    d = copy.deepcopy(gpu.scenes.cornell_box()); d.bvh_builder = "sah"
    g = gpu.Group([0])
    g.ctx(0).set_device_builder("sah")
    g.load_scene(d)
    assert g.ctx(0).internals()["commit_on_device"] == 0 and g.ctx(0).internals()["device_build_sah"] == 0
    img = g.render(64, 48, 2, seed=3, max_bounces=4)
    assert _bits_equal(img, ora.Oracle().load_scene(d).render(64, 48, 2, seed=3, max_bounces=4))
    g.close()
