"""Parity of the HIP path (through the C-ABI) against the oracle on a real MI355X.

Bar (BASELINE.json north_star): relative L2 <= 1e-4 on the HDR radiance buffer with identical scene +
seed.  Because both sides follow one arithmetic contract the tests demand more: identical
bits for hit records, counters, images and RGBA8 output; the 1e-4 bound is asserted as well so that a
future relaxation of bit-equality still has the contractual gate.

Sizes: oracle-checked cases finish in seconds on the host; BASELINE's full sizes are covered through
size-independent properties (tile-sharded sum == whole frame, batch split invariance, run-to-run
determinism, counter identities)."""
import hashlib
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN, rel_l2, run_torchrun  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-4  # north_star tolerance on the fp32 radiance buffer
COUNTERS = ("paths", "segments", "shadow_rays", "hits", "node_visits_closest", "tri_tests_closest", "node_visits_any", "tri_tests_any", "algorithmic_bytes")


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _pair(gpu, ora, desc):
    return gpu.PathTracer(0).load_scene(desc), ora.Oracle().load_scene(desc)


CASES = [
    ("cornell", {}, 96, 96, 16, 1, 8),            # config 1 geometry (12 tris, Lambert + emitter)
    ("sphere10k", {}, 128, 128, 8, 2, 8),         # config 2 geometry (10 k tris, GGX metal, instanced non-uniform scale)
    ("atrium", {"scale": 0.05}, 160, 90, 4, 3, 8),  # config 3 at reduced tessellation
    ("atrium", {}, 240, 135, 2, 3, 8),            # config 3 geometry, 249,936 tris
    ("two_tris_sphere", {}, 64, 64, 2, 5, 3),     # no emitters: NEE disabled, background 0
    # config 5: RGBA8 NEAREST/REPEAT textures (albedo, tangent-space normal map, metal-rough) + lat-long env light
    ("textured_objects", {}, 128, 128, 8, 5, 6),                                                          # environment NEE only
    ("textured_atrium", {"scale": 0.05, "tex_size": 128, "env_size": (128, 64)}, 160, 90, 4, 5, 8),      # env + emissive panels
    ("textured_atrium", {"scale": 0.05, "tex_size": 64, "env_size": (64, 32), "keep_panels": False}, 120, 68, 4, 6, 4),
]


@pytest.mark.parametrize("name,kw,w,h,spp,seed,mb", CASES)
def test_path_tracer_image_and_counters(gpu, ora, name, kw, w, h, spp, seed, mb):
    pt, o = _pair(gpu, ora, gpu.scenes.by_name(name, **kw))
    g = pt.render(w, h, spp, seed=seed, max_bounces=mb)
    c = o.render(w, h, spp, seed=seed, max_bounces=mb)
    assert np.isfinite(g).all()
    assert rel_l2(g, c) <= TOL
    assert _bits_equal(g, c), f"{int((g != c).any(-1).sum())} pixels differ"
    sg, so = pt.stats(), o.stats()
    for k in COUNTERS:                                  # counted, and the two sides must agree exactly
        assert sg[k] == so[k], k
    # a small batch runs closest(b + 1) beside any(b): it carries the batch's span only (per-kernel spans would include each other; PTC_TIMING=2 records them all the same)
    assert sg["seconds_render"] > 0 and sg["launches_trace_closest"] == mb + 1


@pytest.mark.parametrize("name,kw,w,h,spp,seed,mb", [("sphere10k", {}, 96, 96, 4, 2, 6), ("atrium", {}, 160, 90, 2, 3, 8)])
def test_lbvh_builder(gpu, ora, name, kw, w, h, spp, seed, mb):
    """PTC_BVH_LBVH (BASELINE north_star's literal "flattened LBVH"): image and all counters bit-exact against the oracle's LBVH;
    the image is also the SAH tree's image, bit for bit (closest hit and occlusion do not depend on the tree), with more node visits."""
    d = gpu.scenes.by_name(name, **kw)
    d.bvh_builder = "lbvh"
    pt, o = _pair(gpu, ora, d)
    g = pt.render(w, h, spp, seed=seed, max_bounces=mb)
    c = o.render(w, h, spp, seed=seed, max_bounces=mb)
    assert _bits_equal(g, c)
    sg, so = pt.stats(), o.stats()
    for k in COUNTERS:
        assert sg[k] == so[k], k
    d.bvh_builder = "sah"
    g2 = pt.load_scene(d).render(w, h, spp, seed=seed, max_bounces=mb)
    s2 = pt.stats()
    assert _bits_equal(g, g2)
    assert s2["node_visits_closest"] < sg["node_visits_closest"] and s2["segments"] == sg["segments"]


@pytest.mark.parametrize("name,kw,w,h", [("two_tris_sphere", {}, 64, 64), ("atrium", {"scale": 0.05}, 160, 90), ("sphere10k", {}, 101, 67),
                                         ("textured_objects", {}, 96, 96), ("textured_atrium", {"scale": 0.05, "tex_size": 128, "env_size": (64, 32)}, 160, 90)])
def test_raster_compat(gpu, ora, name, kw, w, h):
    pt, o = _pair(gpu, ora, gpu.scenes.by_name(name, **kw))
    g = pt.render(w, h, 1, integrator=gpu.INTEGRATOR_RASTER_COMPAT)
    c = o.render(w, h, 1, integrator=1)
    assert _bits_equal(g, c)
    assert pt.stats()["node_visits_closest"] == o.stats()["node_visits_closest"]
    assert np.array_equal(pt.tonemap(), ora.tonemap_rgba8(c))          # R9, byte-exact


@pytest.mark.parametrize("name,kw", [("cornell", {}), ("sphere10k", {}), ("atrium", {})])
def test_hit_records(gpu, ora, name, kw):
    from golden.make_golden import fixed_rays

    d = gpu.scenes.by_name(name, **kw)
    pt, o = _pair(gpu, ora, d)
    org, dirs, tmax = fixed_rays(d, n=8192 + 37, seed=11)              # ragged: not a multiple of 64
    t1, p1, uv1 = pt.trace_closest(org, dirs)
    s1 = pt.stats()
    t2, p2, uv2 = o.trace_closest(org, dirs)
    s2 = o.stats()
    assert _bits_equal(t1, t2) and np.array_equal(p1, p2) and _bits_equal(uv1, uv2)
    assert (s1["node_visits_closest"], s1["tri_tests_closest"]) == (s2["node_visits_closest"], s2["tri_tests_closest"])
    assert np.array_equal(pt.trace_any(org, dirs, tmax), o.trace_any(org, dirs, tmax))
    assert pt.stats()["node_visits_any"] == o.stats()["node_visits_any"]


def test_golden_fixtures(gpu):
    from golden.make_golden import DIGEST_CASES, fixed_rays

    pt = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    gold = np.load(os.path.join(GOLDEN, "cornell_256x256x64_seed1.npy"))      # BASELINE config 1 in full
    img = pt.render(256, 256, 64, seed=1, max_bounces=8)
    assert rel_l2(img, gold) <= TOL and _bits_equal(img, gold)
    pt.load_scene(gpu.scenes.two_triangles_and_sphere())
    assert _bits_equal(pt.render(64, 64, 1, integrator=1), np.load(os.path.join(GOLDEN, "raster_two_tris_sphere_64.npy")))
    d = gpu.scenes.sphere_scene()
    pt.load_scene(d)
    org, dirs, tmax = fixed_rays(d)
    g = np.load(os.path.join(GOLDEN, "sphere10k_rays4096.npz"))
    t, prim, uv = pt.trace_closest(org, dirs)
    assert _bits_equal(t, g["t"]) and np.array_equal(prim, g["prim"]) and _bits_equal(uv, g["uv"])
    assert np.array_equal(pt.trace_any(org, dirs, tmax), g["occ"])
    dig = json.load(open(os.path.join(GOLDEN, "digests.json")))
    for name, (scene, kw, w, h, spp, seed, mb) in DIGEST_CASES.items():
        pt.load_scene(gpu.scenes.by_name(scene, **kw))
        img = pt.render(w, h, spp, seed=seed, max_bounces=mb)
        assert hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == dig[name]["sha256"], name
        st = pt.stats()
        assert {k: int(st[k]) for k in dig[name]["stats"]} == dig[name]["stats"]


def test_tonemap_bytes(gpu, ora):
    pt = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    img = pt.render(64, 48, 4, seed=2)
    assert np.array_equal(pt.tonemap(), ora.tonemap_rgba8(img))
    rnd = np.random.default_rng(1).uniform(-0.1, 20.0, (48, 64, 4)).astype(np.float32)   # write → tonemap round trip
    pt.write_radiance(rnd)
    assert _bits_equal(pt.read_radiance(), rnd)
    assert np.array_equal(pt.tonemap(), ora.tonemap_rgba8(rnd))


def test_edge_cases(gpu, ora):
    sc = gpu.scene
    v, i = gpu.scenes._quad((-1, -1, -3), (1, -1, -3), (1, 1, -3), (-1, 1, -3))
    cam = sc.CameraDesc((0, 0, 0), (0, 0, -1), math.pi / 2, 1.0)
    emis = sc.Material((0.5, 0.5, 0.5, 1), 0.0, 1.0, (2.0, 3.0, 4.0))
    # 1 triangle (single-node BVH), an emitter seen directly, odd sizes, max_bounces 0, 1x1 frame
    for ntri, w, h, spp, mb in [(1, 33, 17, 2, 0), (2, 1, 1, 3, 2), (2, 65, 31, 1, 1)]:
        d = sc.SceneDesc([emis], [sc.MeshDesc(v, i[: 3 * ntri], 0)], [sc.InstanceDesc(0, (0, 0, 0), (1, 0, 0, 0), (1, 1, 1))], cam)
        pt, o = _pair(gpu, ora, d)
        assert _bits_equal(pt.render(w, h, spp, seed=4, max_bounces=mb), o.render(w, h, spp, seed=4, max_bounces=mb))
        assert _bits_equal(pt.render(w, h, 1, integrator=1), o.render(w, h, 1, integrator=1))
    # degenerate (zero-area) triangles and a ray-parallel triangle are never hit, on either side
    vv = v.copy()
    vv["position"][2] = vv["position"][1]
    d = sc.SceneDesc([emis, sc.Material()], [sc.MeshDesc(vv, i, 0), sc.MeshDesc(v, i, 1)],
                     [sc.InstanceDesc(0, (0, 0, 0.5), (1, 0, 0, 0), (1, 1, 1)), sc.InstanceDesc(1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 1)),
                      sc.InstanceDesc(1, (0, 0, -1), (math.cos(math.pi / 4), 0, math.sin(math.pi / 4), 0), (1, 1, 1))], cam)
    pt, o = _pair(gpu, ora, d)
    g, c = pt.render(40, 40, 4, seed=1, max_bounces=3), o.render(40, 40, 4, seed=1, max_bounces=3)
    assert np.isfinite(g).all() and _bits_equal(g, c)
    # API misuse on a live context
    with pytest.raises(gpu.PtcError):
        pt.render(0, 8, 1)
    with pytest.raises(gpu.PtcError):
        pt.frame_begin(8, 8, 1, tile_rank=2, tile_count=2)
    with pytest.raises(gpu.PtcError):
        gpu.PathTracer(0).render(8, 8, 1)                                   # no scene


def test_deep_tree_uses_stack_overflow(gpu, ora):
    """6000 coincident triangles (every box overlaps every other: a ray through them enters all children of
    all nodes, so a group of pending children waits at every level of the tree) plus triangles at exponentially
    spaced distances, traversed with only 2 stack entries in LDS and with the default stack, so that most pushes go
    through the global overflow slab —
    still bit-exact, path tracer and raster-compat alike.  The second camera sits in front of the cluster."""
    sc = gpu.scene
    cents = [(1024.0, 1024.0, 1024.0)]
    for k in range(10):
        x = float(2 ** (9 - k))
        cents += [(x, 0, 0), (0, x, 0), (0, 0, x)]
    cents += [(0.0, 0.0, 0.0)] * 6000
    c = np.asarray(cents, np.float64)
    n, e = len(c), 0.05
    pos = np.zeros((3 * n, 3), np.float32)
    pos[0::3], pos[1::3], pos[2::3] = c + (-e, -e, 0), c + (e, -e, 0), c + (0, e, 0)
    v = np.zeros(3 * n, sc.MESH_VERTEX)
    v["position"], v["normal"], v["tangent"] = pos, (0, 0, 1), (1, 0, 0, 1)
    emis = sc.Material((0.6, 0.6, 0.6, 1), 0.0, 1.0, (1.0, 1.0, 1.0))
    for cam_z, stack_lds in ((3.0, "2"), (0.9, "2"), (0.9, None)):
        d = sc.SceneDesc([emis], [sc.MeshDesc(v, np.arange(3 * n, dtype=np.uint32), 0)], [sc.InstanceDesc(0, (0, 0, 0), (1, 0, 0, 0), (1, 1, 1))],
                         sc.CameraDesc((0.0, 0.0, cam_z), (0, 0, 0), 0.2, 1.0))
        if stack_lds:
            os.environ["PTC_STACK_LDS"] = stack_lds
        try:
            pt, o = _pair(gpu, ora, d)
        finally:
            os.environ.pop("PTC_STACK_LDS", None)
        assert pt.stats()["bvh_max_depth"] >= 6 and pt.stats()["bvh_max_depth"] == o.stats()["bvh_max_depth"]
        # default: as many entries as leave the register limit of 8 trace blocks per CU room in the 160 KiB of LDS (3 beside the round-4 ring of prepared rays)
        assert pt.internals()["stack_lds"] == 2 if stack_lds else 3 <= pt.internals()["stack_lds"] <= 6
        for integ, spp in ((1, 1), (0, 2)):
            g, c2 = pt.render(64, 64, spp, seed=2, max_bounces=2, integrator=integ), o.render(64, 64, spp, seed=2, max_bounces=2, integrator=integ)
            assert _bits_equal(g, c2)
            assert pt.stats()["node_visits_closest"] == o.stats()["node_visits_closest"] and pt.stats()["node_visits_any"] == o.stats()["node_visits_any"]
            if cam_z < 1.0:
                assert o.stats()["tri_tests_closest"] > 6000 * 500      # the cluster really is traversed exhaustively


def test_sharding_and_batching_do_not_change_bits(gpu):
    """tile-sharded partial frames sum to the undivided frame bit for bit; splitting the
    samples into different wavefront batches (and a smaller queue) changes nothing either."""
    pt = gpu.PathTracer(0).load_scene(gpu.scenes.atrium(0.05))
    w, h, spp = 200, 120, 6
    full = pt.render(w, h, spp, seed=7)
    acc = np.zeros_like(full)
    for n in (2, 3):
        acc[:] = 0
        for r in range(n):
            pt.frame_begin(w, h, spp, 7, 8, 0, tile_rank=r, tile_count=n)
            pt.frame_add_samples(spp)
            pt.frame_resolve()
            part = pt.read_radiance()
            assert (part[~gpu.dist.owned_mask(w, h, r, n)] == 0).all()
            acc += part
        assert _bits_equal(acc, full)
    for split in ([1, 2, 3], [5, 1], [2, 2, 2]):
        pt.frame_begin(w, h, spp, 7, 8, 0)
        for k in split:
            pt.frame_add_samples(k)
        pt.frame_resolve()
        assert _bits_equal(pt.read_radiance(), full)
    for lanes in (1, 2, 3):                                                        # batches on one stream, and alternating over 2 and 3
        os.environ["PTC_BATCH_PATHS"] = str(15000 * lanes)                         # forces ~5 internal batches of 1 spp
        os.environ["PTC_LANES"] = str(lanes)
        try:
            small = gpu.PathTracer(0).load_scene(gpu.scenes.atrium(0.05))
            assert _bits_equal(small.render(w, h, spp, seed=7), full)
            assert small.stats()["launches_trace_closest"] >= 5 * 9
        finally:
            del os.environ["PTC_BATCH_PATHS"], os.environ["PTC_LANES"]


def test_full_size_properties(gpu):
    """BASELINE's full size (1920x1080, 249,936 triangles) at 2 spp: determinism, counter identities,
    tile-shard sum == whole frame, radiance-buffer device pointer usable by torch (the RCCL reduce's input)."""
    import torch

    pt = gpu.PathTracer(0).load_scene(gpu.scenes.atrium())
    w, h, spp = 1920, 1080, 2
    a = pt.render(w, h, spp, seed=3)
    sa = pt.stats()
    assert np.isfinite(a).all() and (a[..., 3] == 1).all() and a[..., :3].min() >= 0
    assert sa["paths"] == w * h * spp and sa["hits"] <= sa["segments"] and sa["shadow_rays"] <= sa["hits"]
    assert sa["segments"] >= sa["paths"] and sa["node_visits_closest"] >= sa["segments"]
    t = gpu.dist.radiance_tensor(pt, w, h)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), a)
    b = pt.render(w, h, spp, seed=3)
    assert _bits_equal(a, b) and all(pt.stats()[k] == sa[k] for k in COUNTERS)    # scheduling-independent
    acc = torch.zeros_like(t)
    for r in range(4):
        pt.frame_begin(w, h, spp, 3, 8, 0, tile_rank=r, tile_count=4)
        pt.frame_add_samples(spp)
        pt.frame_resolve()
        pt.sync()
        acc += gpu.dist.radiance_tensor(pt, w, h)
    assert np.array_equal(acc.cpu().numpy(), a)


def test_cpp_host_cli(gpu, ora, tmp_path):
    """The C++ host (host/pbr_pt.hpp + ptc_render.cpp, mirroring the reference's MeshBuilder/Transform/camera
    interface) drives the same C-ABI: its Cornell box must equal the oracle's render of the Python-built scene."""
    import subprocess

    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    assert os.path.exists(exe), "ptc_render not built"
    out, ppm, png = str(tmp_path / "c.pfm"), str(tmp_path / "c.ppm"), str(tmp_path / "c.png")
    r = subprocess.run([exe, "--scene", "cornell", "--width", "96", "--height", "64", "--spp", "8", "--seed", "5", "--bounces", "4", "--out", out, "--ppm", ppm, "--png", png],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["paths"] == 96 * 64 * 8
    raw = open(out, "rb").read()
    head, body = raw.split(b"-1.0\n", 1)
    assert head.startswith(b"PF\n96 64")
    img = np.frombuffer(body, "<f4").reshape(64, 96, 3)[::-1]                 # PFM rows are bottom-up
    d = gpu.scenes.cornell_box()
    d.camera.aspect = 1.0                                                     # the CLI keeps Cornell's aspect 1 like scenes.cornell_box()
    ref = ora.Oracle().load_scene(d).render(96, 64, 8, seed=5, max_bounces=4)
    assert _bits_equal(np.ascontiguousarray(img), np.ascontiguousarray(ref[..., :3]))
    ldr = np.frombuffer(open(ppm, "rb").read().split(b"255\n", 1)[1], np.uint8).reshape(64, 96, 3)
    assert np.array_equal(ldr, ora.tonemap_rgba8(ref)[..., :3])
    from PIL import Image                                                      # the stored-deflate PNG writer (host/image_io.hpp)

    assert np.array_equal(np.asarray(Image.open(png)), ora.tonemap_rgba8(ref))
    bad = subprocess.run([exe, "--scene", "nope"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "unknown scene" in bad.stderr


def test_textured_gltf_renders_identically(gpu, ora, tmp_path):
    """§8f-1 + §8f-3 together: textures that travelled as PNG images inside a GLB (deflate → own decoder → RGBA8,
    like the reference's stb path) give the same picture, bit for bit, as the oracle fed with the arrays."""
    d = gpu.scenes.by_name("textured_objects")
    p = str(tmp_path / "t.glb")
    gpu.gltf.write_glb(d, p)
    pt = gpu.PathTracer(0)
    n, _, _ = gpu.gltf.load_into(pt, p, camera=d.camera, env=d.env)   # a GLB carries no environment: handed over beside it
    assert n == d.n_triangles
    a = pt.render(96, 96, 4, seed=11, max_bounces=4)
    ref = ora.Oracle().load_scene(d).render(96, 96, 4, seed=11, max_bounces=4)
    assert _bits_equal(a, ref) and float(ref[..., :3].sum()) > 0.0
    # the CLI with the same environment from a PFM file (top row = up = -y = the map's last row: the CLI flips it back)
    import subprocess

    env_pfm, out = str(tmp_path / "env.pfm"), str(tmp_path / "t.pfm")
    eh, ew, _ = d.env.shape
    with open(env_pfm, "wb") as f:
        f.write(f"PF\n{ew} {eh}\n-1.0\n".encode() + np.ascontiguousarray(d.env, "<f4").tobytes())   # PFM rows run bottom-up
    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    cam = d.camera
    r = subprocess.run([exe, "--gltf", p, "--env", env_pfm, "--width", "96", "--height", "96", "--spp", "4", "--seed", "11", "--bounces", "4", "--out", out,
                        "--cam-pos", *map(str, cam.position), "--cam-target", *map(str, cam.target), "--fov", str(np.degrees(cam.fov_y))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = np.frombuffer(open(out, "rb").read().split(b"-1.0\n", 1)[1], "<f4").reshape(96, 96, 3)[::-1]
    assert rel_l2(np.ascontiguousarray(img), ref[..., :3]) <= 5e-3          # the CLI rounds fov through degrees in float: a few paths differ
    r = subprocess.run([exe, "--gltf", p, "--sky", "--width", "64", "--height", "64", "--spp", "4", "--png", str(tmp_path / "s.png"), "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and gpu.gltf.png_decode(open(tmp_path / "s.png", "rb").read())[..., :3].mean() > 5


def test_gltf_loaded_scene_renders_identically(gpu, ora, tmp_path):
    """§8f-1: a scene that went through the GLB writer and the C++ glTF loader renders bit for bit like the same
    SceneDesc handed to the C-ABI directly (and like the oracle); the CLI takes the same file."""
    import subprocess

    d = gpu.scenes.sphere_scene(32, 17)
    p = str(tmp_path / "s.glb")
    gpu.gltf.write_glb(d, p)
    pt = gpu.PathTracer(0)
    n, lo, hi = gpu.gltf.load_into(pt, p, camera=d.camera)
    assert n == d.n_triangles
    a = pt.render(96, 96, 4, seed=9, max_bounces=4)
    ref = ora.Oracle().load_scene(d).render(96, 96, 4, seed=9, max_bounces=4)
    assert _bits_equal(a, ref)
    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    out = str(tmp_path / "g.pfm")
    cam = d.camera
    r = subprocess.run([exe, "--gltf", p, "--width", "96", "--height", "96", "--spp", "4", "--seed", "9", "--bounces", "4", "--out", out,
                        "--cam-pos", *map(str, cam.position), "--cam-target", *map(str, cam.target), "--fov", "45"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = np.frombuffer(open(out, "rb").read().split(b"-1.0\n", 1)[1], "<f4").reshape(96, 96, 3)[::-1]
    assert rel_l2(np.ascontiguousarray(img), ref[..., :3]) <= TOL          # the CLI rounds fov from degrees in float: not bit-identical inputs


def test_bench_two_rank_rehearsal(gpu):
    """bench.py's N > 1 path (tile sharding, framebuffer reduce, max-over-ranks timing, whole-job sums) rehearsed with
    two ranks sharing this box's one GPU over gloo; the driver's real runs use RCCL with one GPU per rank."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--spp-per-step", "2", "--width", "256", "--height", "192",
            "--scene-scale", "0.05", "--backend", "gloo", "--share-device", "--no-cpu-baseline"]
    r = run_torchrun(2, args, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, r.stdout
    d = json.loads(line[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["steps"] == 2       # the default: the frame is fixed, ranks split its pixels
    assert d["config"]["paths"] == 256 * 192 * 2 * 2 and d["value"] > 0              # 2 spp per step, 2 steps, whole frame
    assert d["per_path"]["segments"] > 1.0 and "torch.distributed.reduce" in d["config"]["sharding"]
    pr = d["per_rank"]                                                             # what makes a scaling point readable: per-rank kernel sums, wall, paths
    assert len(pr["wall"]["ranks"]) == 2 and 0 < pr["wall"]["min"] <= pr["wall"]["max"] and sum(pr["paths"]["ranks"]) == d["config"]["paths"]
    assert "reduce_ms" in pr and "written from the generator by rank 0" in d["config"]["scene_source"]
    # small batches: closest(b + 1) beside any(b) — flagged, and no per-kernel seconds are recorded for them (they would include each other)
    assert pr["reduce_impl"] == "torch.distributed.reduce" and pr["batches_per_rank"] >= 1 and pr["kernel_seconds_overlap"] is True and pr["seconds_trace_closest"]["max"] == 0.0
    assert "trace_blocks_per_cu=" in d["launch_policy"] and d["launch_policy"].startswith(d["launch_policy_defaults"].split(" | ")[0])
    r = run_torchrun(2, args + ["--scaling", "weak"], cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert d["scaling"] == "weak" and d["config"]["paths"] == 256 * 192 * 2 * 2 * 2  # weak (opt-in): 2 spp x 2 ranks per step, 2 steps


def test_plain_c_client_renders(gpu, tmp_path):
    """examples/c_client.c (C99, nothing but include/ptc.h) renders on GPU 0 through the C-ABI."""
    import subprocess

    import test_cabi

    r = subprocess.run([test_cabi._build_c_client(tmp_path), "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rendered 65536 paths" in r.stdout


def test_contexts_release_their_device_memory(gpu):
    """create → commit → render → re-commit → destroy, several times: the free device memory comes back (queues, scene
    buffers, overflow slabs, per-lane allocations, events)."""
    import gc

    import torch

    def cycle(k):
        pt = gpu.PathTracer(0).load_scene(gpu.scenes.atrium(0.05))
        pt.render(320, 200, 8, seed=k)
        pt.load_scene(gpu.scenes.sphere_scene(32, 17))          # re-commit on a live context frees the old scene
        pt.render(64, 64, 4, seed=k)
        del pt
        gc.collect()

    cycle(99)                                                   # the first use loads code objects and runtime pools that stay
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    for k in range(4):
        cycle(k)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    assert free0 - free1 < 64 << 20, (free0, free1, (free0 - free1) >> 20)


@pytest.mark.parametrize("world", [2, 3])
def test_render_sharded_two_ranks_on_one_gpu(gpu, world):
    """pbr_amd.dist.render_sharded end to end on the GPU: ranks share the card, gloo carries the reduce of the
    library-owned device buffers, the assembled frame equals the undivided one bit for bit."""
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    r = run_torchrun(world, [os.path.join(here, "_dist_gpu_worker.py")])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "DIST_GPU_OK" in r.stdout


@pytest.mark.parametrize("name,kw,w,h", [("textured_objects", {}, 112, 80), ("textured_atrium", {"scale": 0.05, "tex_size": 64, "env_size": (64, 32)}, 160, 90)])
def test_bilinear_texture_filter_is_bit_exact(gpu, ora, name, kw, w, h):
    """PTC_FILTER_LINEAR (option beyond the reference's NEAREST samplers): HIP and oracle agree bit for bit, in the path
    tracer and in raster-compat, and the result differs from NEAREST."""
    d = gpu.scenes.by_name(name, **kw)
    near = gpu.PathTracer(0).load_scene(d).render(w, h, 4, seed=8, max_bounces=4)
    d.texture_filter = "linear"
    pt, o = _pair(gpu, ora, d)
    g, c = pt.render(w, h, 4, seed=8, max_bounces=4), o.render(w, h, 4, seed=8, max_bounces=4)
    assert _bits_equal(g, c) and not np.array_equal(g, near)
    for k in COUNTERS:
        assert pt.stats()[k] == o.stats()[k], k
    assert _bits_equal(pt.render(w, h, 1, integrator=gpu.INTEGRATOR_RASTER_COMPAT), o.render(w, h, 1, integrator=1))


def _random_scene(sc, rng, k):
    """Random triangle soup: degenerate and coincident triangles, mirrored / sheared instances, emissive, metallic and textured
    materials, a camera somewhere inside.  Everything that could make the two implementations take different branches."""
    n_mat = int(rng.integers(1, 6))
    tex = [rng.integers(0, 256, (int(rng.integers(1, 9)), int(rng.integers(1, 9)), 4), dtype=np.uint8) for _ in range(int(rng.integers(0, 3)))]
    mats = []
    for _ in range(n_mat):
        emissive = tuple(float(x) for x in rng.uniform(0, 8, 3)) if rng.random() < 0.35 else (0.0, 0.0, 0.0)
        t = lambda: int(rng.integers(0, len(tex))) if tex and rng.random() < 0.5 else -1
        mats.append(sc.Material((*[float(x) for x in rng.uniform(0.05, 1.0, 3)], 1.0), float(rng.choice([0.0, 0.0, 1.0, rng.random()])),
                                float(rng.choice([1.0, 1.0, rng.uniform(0.02, 1.0)])), emissive, t(), t(), t()))
    if not any(max(m.emissive) > 0 for m in mats):
        mats[0].emissive = (4.0, 4.0, 4.0)
    meshes = []
    for _ in range(int(rng.integers(1, 5))):
        nv = int(rng.integers(3, 40))
        v = np.zeros(nv, sc.MESH_VERTEX)
        v["position"] = rng.uniform(-1, 1, (nv, 3)).astype(np.float32)
        if rng.random() < 0.3:
            v["position"][: nv // 2] = np.round(v["position"][: nv // 2] * 2) / 2          # coincident vertices, axis-aligned faces
        nrm = rng.normal(0, 1, (nv, 3))
        v["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        tan = np.cross(nrm, rng.normal(0, 1, (nv, 3)))
        v["tangent"][:, :3] = (tan / np.linalg.norm(tan, axis=1, keepdims=True)).astype(np.float32)
        v["tangent"][:, 3] = rng.choice([-1.0, 1.0], nv)
        v["texCoords"] = rng.uniform(-2, 3, (nv, 2)).astype(np.float32)
        nt = int(rng.integers(1, 60))
        idx = rng.integers(0, nv, (nt, 3)).astype(np.uint32)                                  # includes degenerate (repeated-index) triangles
        if rng.random() < 0.4:
            idx = np.concatenate([idx, idx[: nt // 3]])                                       # exact duplicates: ties in t resolved by primitive id
        meshes.append(sc.MeshDesc(v, idx.reshape(-1), int(rng.integers(0, n_mat))))
    insts = []
    for _ in range(int(rng.integers(1, 7))):
        m = np.eye(4, dtype=np.float32)
        a = rng.normal(0, 1, (3, 3)).astype(np.float32) * float(rng.uniform(0.3, 2.0))      # general affine: shear, mirror (det < 0), anisotropic
        if rng.random() < 0.3:
            a = np.diag(rng.choice([-1.0, 1.0], 3) * rng.uniform(0.2, 2.0, 3)).astype(np.float32)
        m[:3, :3] = a
        m[:3, 3] = rng.uniform(-1.5, 1.5, 3)
        insts.append(sc.InstanceDesc(int(rng.integers(0, len(meshes))), matrix=np.ascontiguousarray(m.T).reshape(16)))   # column-major
    cam = sc.CameraDesc(tuple(float(x) for x in rng.uniform(-3, 3, 3)), tuple(float(x) for x in rng.uniform(-0.5, 0.5, 3)), float(rng.uniform(0.3, 2.0)), float(rng.uniform(0.5, 2.0)))
    env = rng.uniform(0, 2, (int(rng.integers(1, 6)), int(rng.integers(1, 9)), 3)).astype(np.float32) if rng.random() < 0.4 else None
    d = sc.SceneDesc(mats, meshes, insts, cam, f"random{k}", textures=tex, env=env)
    d.texture_filter = "linear" if rng.random() < 0.3 else "nearest"
    return d


def test_random_scenes_are_bit_exact(gpu, ora):
    """Differential fuzzing of the whole path: 40 seeded random scenes through both implementations — images, raster-compat,
    counters and the BVH statistics must agree exactly."""
    rng = np.random.default_rng(2024)
    for k in range(40):
        d = _random_scene(gpu.scene, rng, k)
        pt, o = _pair(gpu, ora, d)
        w, h = int(rng.integers(8, 70)), int(rng.integers(8, 70))
        spp, mb, seed = int(rng.integers(1, 6)), int(rng.integers(0, 9)), int(rng.integers(0, 1 << 40))
        g, c = pt.render(w, h, spp, seed=seed, max_bounces=mb), o.render(w, h, spp, seed=seed, max_bounces=mb)
        assert np.isfinite(c).all(), k
        assert _bits_equal(g, c), (k, int((g != c).any(-1).sum()))
        sg, so = pt.stats(), o.stats()
        for key in COUNTERS + ("n_bvh_nodes", "bvh_max_depth", "n_emitters", "n_triangles"):
            assert sg[key] == so[key], (k, key)
        assert _bits_equal(pt.render(w, h, 1, integrator=gpu.INTEGRATOR_RASTER_COMPAT), o.render(w, h, 1, integrator=1)), k


def test_full_resolution_frame_is_bit_exact(gpu, ora):
    """BASELINE config 3 at its real resolution: 1920x1080 on the 249,936-triangle atrium, 2 spp (the oracle needs a few
    seconds for 4 M paths on the box's host cores) — image, counters and tone-mapped bytes identical."""
    d = gpu.scenes.atrium()
    d.camera.aspect = 1920 / 1080
    pt, o = _pair(gpu, ora, d)
    g = pt.render(1920, 1080, 2, seed=3, max_bounces=8)
    c = o.render(1920, 1080, 2, seed=3, max_bounces=8, n_threads=ora.hw_threads())
    assert _bits_equal(g, c), int((g != c).any(-1).sum())
    for k in COUNTERS:
        assert pt.stats()[k] == o.stats()[k], k
    assert np.array_equal(pt.tonemap(), ora.tonemap_rgba8(c))


def test_camera_change_without_recommit(gpu, ora):
    """Viewer-style use: the camera moves between frames of a committed scene — no BVH rebuild, and each
    frame equals a fresh context (and the oracle) with that camera; progressive accumulation restarts with frame_begin."""
    sc = gpu.scene
    d = gpu.scenes.sphere_scene(32, 17)
    pt = gpu.PathTracer(0).load_scene(d)
    commit_s = pt.stats()["seconds_commit"]
    for k, (pos, tgt, fov) in enumerate((((0.0, 1.0, 6.0), (0.0, 0.0, 0.0), 0.8), ((3.0, 2.0, 3.0), (0.0, -0.2, 0.0), 1.1), ((-4.0, 0.5, 1.0), (0.5, 0.0, 0.0), 0.6))):
        pt.set_camera(pos, tgt, fov, 1.5)
        g = pt.render(96, 64, 3, seed=k, max_bounces=4)
        d2 = sc.SceneDesc(d.materials, d.meshes, d.instances, sc.CameraDesc(pos, tgt, fov, 1.5))
        c = ora.Oracle().load_scene(d2).render(96, 64, 3, seed=k, max_bounces=4)
        assert _bits_equal(g, c), k
        assert pt.stats()["seconds_commit"] == commit_s                      # the scene was not committed again
    # progressive: 1 + 2 samples added to one frame = the 3-sample frame
    pt.frame_begin(96, 64, 3, 2, 4, 0)
    pt.frame_add_samples(1)
    pt.frame_resolve()
    first = pt.read_radiance().copy()
    pt.frame_add_samples(2)
    pt.frame_resolve()
    assert _bits_equal(pt.read_radiance(), g) and not np.array_equal(first, g)


@pytest.mark.parametrize("name,kw,w,h,spp,seed,mb", [("sphere10k", {}, 96, 96, 4, 2, 6), ("atrium", {}, 160, 90, 2, 3, 8),
                                                      ("textured_atrium", {"scale": 0.05, "tex_size": 64, "env_size": (64, 32)}, 120, 68, 4, 5, 6)])
def test_scene_dynamics_refit(gpu, ora, name, kw, w, h, spp, seed, mb):
    """The viewer turns its nodes every frame (src/gltf_viewer/App.cpp:306-313).  ptc_update_instance + ptc_scene_refit: the image is, bit for
    bit, that of a fresh commit of the same transforms (closest hit and occlusion do not depend on the tree) and that of the oracle's refit;
    the traversal counters are those of the oracle's refitted tree; a second turn refits the refitted tree again."""
    import copy
    import math
    d = gpu.scenes.by_name(name, **kw)
    pt, o = _pair(gpu, ora, d)
    pt.render(w, h, 1, seed=seed, max_bounces=mb)                                        # something was rendered before the scene moves
    d2 = copy.deepcopy(d)
    for k in (1, 2):
        for i, it in enumerate(d2.instances):
            if i % 3 or getattr(it, "matrix", None) is not None:
                continue
            a = 0.07 * k + 0.013 * i
            w1, x1, y1, z1 = math.cos(a / 2), 0.0, math.sin(a / 2), 0.0
            w2, x2, y2, z2 = d.instances[i].q_wxyz
            q = (w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2)
            t = (d.instances[i].t[0], d.instances[i].t[1] + 0.03 * k, d.instances[i].t[2])
            it.t, it.q_wxyz = t, q
            pt.update_instance(i, t, q, it.s)
            o.update_instance(i, t, q, it.s)
        pt.scene_refit()
        o.scene_refit()
        g = pt.render(w, h, spp, seed=seed, max_bounces=mb)
        c = o.render(w, h, spp, seed=seed, max_bounces=mb)
        assert _bits_equal(g, c), f"turn {k}: {int((g != c).any(-1).sum())} pixels differ from the oracle's refit"
        sg, so = pt.stats(), o.stats()
        for key in COUNTERS:
            assert sg[key] == so[key], (k, key)
        fresh = gpu.PathTracer(0).load_scene(d2)
        f = fresh.render(w, h, spp, seed=seed, max_bounces=mb)
        assert _bits_equal(g, f), f"turn {k}: {int((g != f).any(-1).sum())} pixels differ from a fresh commit"
        sf = fresh.stats()
        assert sf["segments"] == sg["segments"] and sf["shadow_rays"] == sg["shadow_rays"] and sf["hits"] == sg["hits"]
        assert 0.0 < sg["seconds_refit"]
    # the refit is cheaper than the commit it replaces (no build), and the numbers are there to be read
    print(f"{name}: commit {pt.stats()['seconds_commit'] * 1e3:.1f} ms, refit {pt.stats()['seconds_refit'] * 1e3:.1f} ms")


def test_tables_beyond_the_lds_copies(gpu, ora):
    """k_shade keeps the emitter table, the material table and the environment's row cdf in LDS when they fit (64 emitters, 64 materials, 2048
    rows) and runs a variant without any fallback then; a scene beyond every one of the three limits takes the other variant, which reads them from
    global memory: 90 materials, 120 emitters, an environment 2100 rows high — image and counters are the oracle's, and so are those of the same
    scene cut down to fit."""
    sc = gpu.scene
    rng = np.random.default_rng(5)
    base = gpu.scenes.cornell_box()
    for n_quads, env_rows in ((90, 2100), (12, 16)):
        mats, meshes, insts = [], [], []
        for k in range(n_quads):
            em = (float(rng.uniform(1, 6)),) * 3 if k % 3 == 0 or k >= 30 and k < 60 else (0.0, 0.0, 0.0)
            mats.append(sc.Material((*[float(x) for x in rng.uniform(0.2, 0.9, 3)], 1.0), float(rng.choice([0.0, 1.0])), float(rng.uniform(0.1, 1.0)), em))
            c = rng.uniform(-0.9, 0.9, 3); e1 = rng.normal(0, 0.25, 3); e2 = rng.normal(0, 0.25, 3)
            v, i = gpu.scenes._quad(tuple(c), tuple(c + e1), tuple(c + e1 + e2), tuple(c + e2))
            meshes.append(sc.MeshDesc(v, i, k))
            insts.append(sc.InstanceDesc(k, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
        env = rng.uniform(0.0, 1.5, (env_rows, 4, 3)).astype(np.float32)
        d = sc.SceneDesc(mats, meshes, insts, base.camera, f"tables{n_quads}", env=env)
        pt, o = _pair(gpu, ora, d)
        assert pt.stats()["n_emitters"] > 64 or n_quads < 64
        g, c = pt.render(40, 40, 3, seed=9, max_bounces=4), o.render(40, 40, 3, seed=9, max_bounces=4)
        assert _bits_equal(g, c), f"{n_quads} quads: {int((g != c).any(-1).sum())} pixels differ"
        sg, so = pt.stats(), o.stats()
        for key in COUNTERS:
            assert sg[key] == so[key], (n_quads, key)


def _single_triangle_scene(gpu):
    sc = gpu.scene
    d = gpu.scenes.cornell_box()
    v = d.meshes[5].vertices[:3].copy()
    return sc.SceneDesc([d.materials[3]], [sc.MeshDesc(v, np.array([0, 1, 2], np.uint32), 0)], [sc.InstanceDesc(0, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))], d.camera, "one")


def _scene_bytes(pt):
    units, nn, nt, grid = pt.bvh()
    shade, lights, cdf = pt.shading_tables()
    v, i, m = pt.flat_scene()
    return {"units": units.view(np.uint32), "grid": np.asarray(grid), "shade": shade.view(np.uint32), "lights": lights.view(np.uint32), "cdf": cdf.view(np.uint32),
            "verts": v.view(np.uint32), "idx": i, "mat": m, "counts": np.array([nn, nt])}


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,builder", [("cornell", {}, None), ("sphere10k", {}, None), ("atrium", {"scale": 0.05}, None), ("atrium", {"scale": 0.02}, "lbvh"),
                                             ("textured_objects", {}, None), ("textured_atrium", {"scale": 0.05, "tex_size": 64, "env_size": (64, 32)}, None),
                                             ("one", {}, None)])
def test_refit_on_the_device_writes_the_bytes_of_the_host_refit(gpu, name, kw, builder):
    """csrc/pt_refit.hip against ptc_refit_scene: after the same moves the BVH units (nodes + triangle records), the origin grid, the shading
    records, the emitter table and its cdf and the flattened vertices read back from HBM are, byte for byte, what the host refit computes on a
    description-only context (which tests/test_host_logic.py holds against the oracle's refit) — over SAH and LBVH trees, textured (192-byte)
    and plain (80-byte) shading records, the single-triangle tree, rotations, translations, non-uniform scales and matrix instances."""
    import copy
    d = _single_triangle_scene(gpu) if name == "one" else gpu.scenes.by_name(name, **kw)
    if builder:
        d = copy.deepcopy(d)
        d.bvh_builder = builder
    dev = gpu.PathTracer(0).load_scene(d)
    host = gpu.PathTracer(gpu.DEVICE_NONE).load_scene(d)
    before = _scene_bytes(dev)
    dev.scene_refit()                                             # nothing moved: the committed bytes come back
    assert dev.internals()["refit_on_device"] == 1
    same = _scene_bytes(dev)
    for key, val in before.items():
        assert np.array_equal(val, same[key]), f"refit without a move changed {key}"
    rng = np.random.default_rng(11)
    for turn in (1, 2, 3):
        for i, it in enumerate(d.instances):
            if i % 2 and len(d.instances) > 2:
                continue
            a = 0.11 * turn + 0.017 * i
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            q = (math.cos(a / 2), *(math.sin(a / 2) * ax))
            if getattr(it, "matrix", None) is not None or turn == 3:       # the third turn moves everything by matrices (shear included)
                m = np.eye(4, dtype=np.float32)
                m[:3, :3] += 0.05 * rng.normal(size=(3, 3)).astype(np.float32)
                m[3, :3] = 0.02 * rng.normal(size=3)                       # column-major: row 3 of the array is the translation column
                if getattr(it, "matrix", None) is not None:
                    m = (np.asarray(it.matrix, np.float32).reshape(4, 4) @ m).astype(np.float32)
                dev.update_instance(i, matrix=m.reshape(16)); host.update_instance(i, matrix=m.reshape(16))
            else:
                t = tuple(np.float32(x) + np.float32(0.03 * turn) for x in it.t)
                s = tuple(np.float32(x) * np.float32(1.0 + 0.1 * k * turn) for k, x in enumerate(it.s))
                dev.update_instance(i, t, q, s); host.update_instance(i, t, q, s)
        dev.scene_refit(); host.scene_refit()
        assert dev.internals()["refit_on_device"] == 1 and host.internals()["refit_on_device"] == 0
        a, b = _scene_bytes(dev), _scene_bytes(host)
        for key in a:
            assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), f"turn {turn}: {key} differs in {int((a[key] != b[key]).sum())} words"
        # the tree's surface-area cost (one fixed-point reduction inside k_refit_nodes) is the host's sum, to the bit, in the unit of the commit
        assert dev.stats()["bvh_sa_cost"] == host.stats()["bvh_sa_cost"] > 0.0 and dev.stats()["bvh_sa_cost_built"] == host.stats()["bvh_sa_cost_built"]
    print(f"{name}: commit {dev.stats()['seconds_commit'] * 1e3:.1f} ms, refit on the device {dev.stats()['seconds_refit'] * 1e3:.2f} ms")


def _coincident_scene(gpu):
    """300 triangles of which 200 share one box centre (one Morton code): the LBVH tells them apart by their sorted position."""
    sc = gpu.scene
    d = gpu.scenes.cornell_box()
    rng = np.random.default_rng(5)
    cents = np.concatenate([np.tile([[0.1, 0.2, -0.3]], (200, 1)), rng.uniform(-0.8, 0.8, (100, 3))])
    n, e = len(cents), 0.04
    pos = np.zeros((3 * n, 3), np.float32)
    pos[0::3], pos[1::3], pos[2::3] = cents + (-e, -e, 0), cents + (e, -e, 0), cents + (0, e, 0)
    v = np.zeros(3 * n, sc.MESH_VERTEX)
    v["position"], v["normal"], v["tangent"] = pos, (0, 0, 1), (1, 0, 0, 1)
    return sc.SceneDesc(d.materials, [sc.MeshDesc(v, np.arange(3 * n, dtype=np.uint32), 0), d.meshes[5]],
                        [sc.InstanceDesc(0, (0, 0, 0), (1, 0, 0, 0), (1, 1, 1)), sc.InstanceDesc(1, (0, 0, 0), (1, 0, 0, 0), (1, 1, 1))], d.camera, "coincident")


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [("cornell", {}), ("sphere10k", {}), ("atrium", {"scale": 0.05}), ("textured_atrium", {"scale": 0.05, "tex_size": 64, "env_size": (64, 32)}),
                                     ("textured_objects", {}), ("coincident", {}), ("atrium", {})])
def test_commit_on_the_device_writes_the_bytes_of_the_host_lbvh_commit(gpu, ora, name, kw):
    """ptc_scene_commit with the LBVH builder on a device context (csrc/ptc_api_scene.cpp device_commit): the host only describes — indices, materials, the emitter table from
    the emissive primitives, textures —, the device flattens the vertices, writes the shading records around their two seeded indices and builds the tree.  What then lies in
    HBM — unit array, origin grid, shading records (padding included), emitters, cdf, world vertices — is byte for byte what the host's commit of the same description
    (PTC_COMMIT=host on the same device, and a description-only context) computes; statistics, launch configuration, image and traversal counters agree, the counters with the
    oracle's LBVH.  A refit of the device-committed scene runs on the device and writes the bytes of the host's refit.  The SAH builder commits on the host, as before."""
    import copy
    d = copy.deepcopy(_coincident_scene(gpu) if name == "coincident" else gpu.scenes.by_name(name, **kw))
    d.bvh_builder = "lbvh"
    dev = gpu.PathTracer(0).load_scene(d)
    assert dev.internals()["commit_on_device"] == 1
    os.environ["PTC_COMMIT"] = "host"
    try:
        host = gpu.PathTracer(0).load_scene(d)
    finally:
        del os.environ["PTC_COMMIT"]
    assert host.internals()["commit_on_device"] == 0
    sd, sh = dev.stats(), host.stats()
    for key in ("n_triangles", "n_bvh_nodes", "n_emitters", "bvh_max_depth", "bvh_sa_cost", "bvh_sa_cost_built"):
        assert sd[key] == sh[key], key
    for key in ("trace_blocks_per_cu", "stack_lds"):
        assert dev.internals()[key] == host.internals()[key], key
    w, h = 96, 54
    gd, gh = dev.render(w, h, 2, seed=7, max_bounces=4), host.render(w, h, 2, seed=7, max_bounces=4)      # rendered BEFORE the arrays are read back: the scene in HBM is what is judged
    assert _bits_equal(gd, gh)
    o = ora.Oracle().load_scene(d)
    assert _bits_equal(gd, o.render(w, h, 2, seed=7, max_bounces=4))
    sg, so = dev.stats(), o.stats()
    for key in COUNTERS:
        assert sg[key] == so[key], key
    a, b, c = _scene_bytes(dev), _scene_bytes(host), _scene_bytes(gpu.PathTracer(gpu.DEVICE_NONE).load_scene(d))
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), f"{key} differs in {int((a[key] != b[key]).sum()) if a[key].shape == b[key].shape else -1} words"
        assert np.array_equal(a[key], c[key]), key
    print(f"{name}: commit on the device {sd['seconds_commit'] * 1e3:.2f} ms, on the host {sh['seconds_commit'] * 1e3:.2f} ms")
    # a second commit of the same context (everything of the first is released), then moves + refit: on the device, the bytes of the host path's refit
    dev.load_scene(d)
    assert dev.internals()["commit_on_device"] == 1
    print(f"{name}: second commit on the device {dev.stats()['seconds_commit'] * 1e3:.2f} ms")
    for i, it in enumerate(d.instances):
        if i % 2 == 0 and getattr(it, "matrix", None) is None:
            a_ = 0.4 + 0.05 * i
            q = (math.cos(a_ / 2), 0.0, math.sin(a_ / 2), 0.0)
            dev.update_instance(i, it.t, q, it.s); host.update_instance(i, it.t, q, it.s)
    dev.scene_refit()
    os.environ["PTC_REFIT"] = "host"
    try:
        host.scene_refit()
    finally:
        del os.environ["PTC_REFIT"]
    assert dev.internals()["refit_on_device"] == 1 and host.internals()["refit_on_device"] == 0
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), host.render(w, h, 2, seed=7, max_bounces=4))
    a, b = _scene_bytes(dev), _scene_bytes(host)
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), f"after the refit: {key} differs"
    d.bvh_builder = "sah"
    assert gpu.PathTracer(0).load_scene(d).internals()["commit_on_device"] == 0


@pytest.mark.gpu
def test_commit_on_the_device_edges(gpu, ora):
    """What the device commit does not take, refuses, and keeps apart: a single triangle goes to the host builder (the device build needs two); a scene lit by its environment
    alone (no emitter table) and a scene on two lanes commit on the device; an instance whose matrix overflows to non-finite positions is refused with the host path's words, after
    which the context commits again; and a context that committed on the device can be re-described and committed with the SAH builder (everything of the device commit released)."""
    import copy
    sc = gpu.scene
    one = copy.deepcopy(_single_triangle_scene(gpu)); one.bvh_builder = "lbvh"
    pt, o = gpu.PathTracer(0).load_scene(one), ora.Oracle().load_scene(one)
    assert pt.internals()["commit_on_device"] == 0
    assert _bits_equal(pt.render(32, 32, 2, seed=1, max_bounces=2), o.render(32, 32, 2, seed=1, max_bounces=2))
    d = copy.deepcopy(gpu.scenes.by_name("textured_objects")); d.bvh_builder = "lbvh"
    d.materials = [copy.copy(m) for m in d.materials]
    for m in d.materials:
        m.emissive = (0.0, 0.0, 0.0)                                                # the environment is the only light
    if getattr(d, "env", None) is None:
        rng = np.random.default_rng(2)
        d.env = rng.uniform(0.0, 2.0, (16, 32, 3)).astype(np.float32)
    pt, o = gpu.PathTracer(0).load_scene(d), ora.Oracle().load_scene(d)
    assert pt.internals()["commit_on_device"] == 1 and pt.stats()["n_emitters"] == 0
    g, c = pt.render(64, 48, 2, seed=5, max_bounces=3), o.render(64, 48, 2, seed=5, max_bounces=3)
    assert _bits_equal(g, c) and all(pt.stats()[k] == o.stats()[k] for k in COUNTERS)
    os.environ["PTC_LANES"] = "2"
    try:
        two = gpu.PathTracer(0)
    finally:
        del os.environ["PTC_LANES"]
    two.load_scene(d)
    assert two.internals()["commit_on_device"] == 1 and _bits_equal(two.render(64, 48, 2, seed=5, max_bounces=3), c)
    bad = copy.deepcopy(gpu.scenes.by_name("cornell")); bad.bvh_builder = "lbvh"
    big = np.eye(4, dtype=np.float32); big[0, 0] = 3e38; big[3, 0] = 3e38          # finite entries, positions overflow in the flatten
    good_matrix = getattr(bad.instances[2], "matrix", None)
    bad.instances[2] = sc.InstanceDesc(bad.instances[2].mesh, matrix=big.reshape(16))
    ctx = gpu.PathTracer(0)
    with pytest.raises(gpu.PtcError, match="non-finite"):
        ctx.load_scene(bad)
    os.environ["PTC_COMMIT"] = "host"
    try:
        with pytest.raises(gpu.PtcError, match="non-finite"):
            gpu.PathTracer(0).load_scene(bad)
    finally:
        del os.environ["PTC_COMMIT"]
    ok = copy.deepcopy(gpu.scenes.by_name("cornell")); ok.bvh_builder = "lbvh"
    oo = ora.Oracle().load_scene(ok)
    ref = oo.render(48, 48, 2, seed=4, max_bounces=4)
    assert _bits_equal(ctx.load_scene(ok).render(48, 48, 2, seed=4, max_bounces=4), ref) and ctx.internals()["commit_on_device"] == 1      # the refused commit left a usable context
    ok.bvh_builder = "sah"
    assert _bits_equal(ctx.load_scene(ok).render(48, 48, 2, seed=4, max_bounces=4), ref) and ctx.internals()["commit_on_device"] == 0
    ok.bvh_builder = "lbvh"
    assert _bits_equal(ctx.load_scene(ok).render(48, 48, 2, seed=4, max_bounces=4), ref) and ctx.internals()["commit_on_device"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,commit_builder", [("cornell", {}, "lbvh"), ("sphere10k", {}, "lbvh"), ("atrium", {"scale": 0.05}, "lbvh"), ("atrium", {"scale": 0.05}, "sah"),
                                                     ("textured_atrium", {"scale": 0.05, "tex_size": 64, "env_size": (64, 32)}, "lbvh"), ("textured_objects", {}, "sah"),
                                                     ("coincident", {}, "lbvh"), ("atrium", {}, "lbvh")])
def test_rebuild_on_the_device_writes_the_bytes_of_the_host_lbvh_build(gpu, ora, name, kw, commit_builder):
    """csrc/pt_build.hip against the host's LBVH builder (which tests/test_host_logic.py holds against the oracle's, tree for tree): ptc_scene_rebuild —
    Morton keys, LDS radix sort, radix tree, bottom-up boxes and collapse costs, 8-wide collapse, octant slots, layout, then the refit kernels for the
    planes — leaves in HBM, byte for byte, the unit array, origin grid, shading records, emitter table and vertices that a fresh ptc_scene_commit of
    the same geometry with PTC_BVH_LBVH computes on the host: right after the commit (whatever builder the commit used), and after the instances
    have moved.  The 249,936-triangle atrium is in the list at full size; `coincident` has 200 triangles with one Morton code."""
    import copy
    d = copy.deepcopy(_coincident_scene(gpu) if name == "coincident" else gpu.scenes.by_name(name, **kw))
    d.bvh_builder = commit_builder
    dev = gpu.PathTracer(0).load_scene(d)
    d_l = copy.deepcopy(d); d_l.bvh_builder = "lbvh"
    want = _scene_bytes(gpu.PathTracer(gpu.DEVICE_NONE).load_scene(d_l))
    w, h = 96, 54
    img0 = dev.render(w, h, 2, seed=7, max_bounces=4)
    dev.scene_rebuild()
    got = _scene_bytes(dev)
    for key in want:
        assert want[key].shape == got[key].shape and np.array_equal(want[key], got[key]), f"{key} differs in {int((want[key] != got[key]).sum()) if want[key].shape == got[key].shape else -1} words"
    st = dev.stats()
    assert st["seconds_rebuild"] > 0.0 and st["bvh_sa_cost"] == st["bvh_sa_cost_built"] > 0.0
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), img0), "the image does not depend on the tree"
    # move, refit (the cost figure follows the refitted boxes), rebuild: the bytes of a fresh LBVH commit of the moved scene
    rng = np.random.default_rng(3)
    for i, it in enumerate(d_l.instances):
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
    dev.scene_refit()
    refit_cost, built_cost = dev.stats()["bvh_sa_cost"], dev.stats()["bvh_sa_cost_built"]
    assert built_cost == st["bvh_sa_cost_built"] and refit_cost > 0.0
    o = ora.Oracle().load_scene(d_l)
    ref = o.render(w, h, 2, seed=7, max_bounces=4)
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), ref)
    dev.scene_rebuild()
    want = _scene_bytes(gpu.PathTracer(gpu.DEVICE_NONE).load_scene(d_l))
    got = _scene_bytes(dev)
    for key in want:
        assert want[key].shape == got[key].shape and np.array_equal(want[key], got[key]), f"after the move: {key} differs"
    g = dev.render(w, h, 2, seed=7, max_bounces=4)
    assert _bits_equal(g, ref)
    sg, so = dev.stats(), o.stats()
    for key in COUNTERS:
        assert sg[key] == so[key], key                       # the rebuilt tree IS the oracle's LBVH of the moved scene: its traversal counters too
    # and a refit after the rebuild runs on the device over the new tree
    dev.scene_refit()
    assert dev.internals()["refit_on_device"] == 1
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), ref)
    # the host has no topology of a tree the device built: a host-path refit builds from scratch (with the description's builder), PTC_REBUILD=host likewise (LBVH)
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
    got = _scene_bytes(dev)
    for key in want:
        assert want[key].shape == got[key].shape and np.array_equal(want[key], got[key]), f"PTC_REBUILD=host: {key} differs"
    assert _bits_equal(dev.render(w, h, 2, seed=7, max_bounces=4), ref)
    dev.scene_rebuild()                                      # and the device again, over the host's build
    got = _scene_bytes(dev)
    for key in want:
        assert want[key].shape == got[key].shape and np.array_equal(want[key], got[key]), f"device rebuild after a host build: {key} differs"
    print(f"{name}: {st['n_triangles']} triangles, rebuild on the device {dev.stats()['seconds_rebuild'] * 1e3:.2f} ms (commit, {'on the device' if commit_builder == 'lbvh' else 'SAH on the host'}, {st['seconds_commit'] * 1e3:.1f} ms); "
          f"SA cost built {built_cost:.2f}, refitted after the move {refit_cost:.2f}, rebuilt {sg['bvh_sa_cost_built']:.2f}")


@pytest.mark.gpu
def test_refit_paths_agree_and_fall_back(gpu, ora):
    """PTC_REFIT=host takes the host refit + upload; a move that changes WHICH triangles are emitters (an emitter scaled to zero area) cannot keep
    the emitter indices of the shading records and takes the host path by itself; a non-finite matrix is refused and leaves the scene in HBM as
    it was.  Images: the oracle's, bit for bit, every time."""
    d = gpu.scenes.by_name("cornell")
    pt, o = _pair(gpu, ora, d)
    ref = pt.render(48, 48, 2, seed=4, max_bounces=4)
    t, q = (0.1, 0.0, 0.05), (math.cos(0.2), 0.0, math.sin(0.2), 0.0)
    os.environ["PTC_REFIT"] = "host"
    try:
        pt.update_instance(0, t, q, (1.0, 1.0, 1.0)); o.update_instance(0, t, q, (1.0, 1.0, 1.0))
        pt.scene_refit(); o.scene_refit()
    finally:
        del os.environ["PTC_REFIT"]
    assert pt.internals()["refit_on_device"] == 0
    assert _bits_equal(pt.render(48, 48, 2, seed=4, max_bounces=4), o.render(48, 48, 2, seed=4, max_bounces=4))
    pt.update_instance(5, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 1.0)); o.update_instance(5, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 1.0))
    pt.scene_refit(); o.scene_refit()                      # the light collapsed to a segment: no emitter left
    assert pt.internals()["refit_on_device"] == 0 and pt.stats()["n_emitters"] == 0
    assert _bits_equal(pt.render(48, 48, 2, seed=4, max_bounces=4), o.render(48, 48, 2, seed=4, max_bounces=4))
    pt.update_instance(5, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0)); o.update_instance(5, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    pt.update_instance(0, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0)); o.update_instance(0, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    pt.scene_refit(); o.scene_refit()                      # and back: the emitters return (host path again: the set changed), the image is the first one
    assert pt.stats()["n_emitters"] == 2
    back = pt.render(48, 48, 2, seed=4, max_bounces=4)
    assert _bits_equal(back, ref) and _bits_equal(back, o.render(48, 48, 2, seed=4, max_bounces=4))
    pt.update_instance(1, (0.0, 0.01, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0)); o.update_instance(1, (0.0, 0.01, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    pt.scene_refit(); o.scene_refit()
    assert pt.internals()["refit_on_device"] == 1
    moved = pt.render(48, 48, 2, seed=4, max_bounces=4)
    assert _bits_equal(moved, o.render(48, 48, 2, seed=4, max_bounces=4))
    big = np.eye(4, dtype=np.float32); big[0, 0] = 3e38; big[3, 0] = 3e38          # finite entries, positions overflow on the device
    pt.update_instance(2, matrix=big.reshape(16))
    with pytest.raises(gpu.PtcError, match="non-finite"):
        pt.scene_refit()
    assert _bits_equal(pt.render(48, 48, 2, seed=4, max_bounces=4), moved), "a refused refit must leave the committed scene alone"


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["device", "host"])
def test_refit_refuses_a_description_that_changed_since_the_commit(gpu, path):
    """An instance added after the commit, then ptc_scene_refit: refused on the device path and on the host path alike, before any upload or
    launch (the refit kernels would read and write past the committed arrays), with and without a refit plan already built; the committed scene
    still renders what it rendered."""
    import ctypes as C
    d = gpu.scenes.by_name("cornell")
    pt = gpu.PathTracer(0).load_scene(d)
    ref = pt.render(48, 48, 2, seed=4, max_bounces=4)
    f3 = lambda *v: (C.c_float * len(v))(*v)
    if path == "host":
        os.environ["PTC_REFIT"] = "host"
    try:
        for plan_first in (False, True):
            if plan_first:
                pt = gpu.PathTracer(0).load_scene(d)
                pt.scene_refit()                                                        # builds the refit plan of the committed scene
            assert pt._L.ptc_add_instance(pt._h, 0, f3(0.0, 0.1, 0.0), f3(1.0, 0.0, 0.0, 0.0), f3(1.0, 1.0, 1.0)) >= 0
            with pytest.raises(gpu.PtcError, match="changed since the commit"):
                pt.scene_refit()
            assert _bits_equal(pt.render(48, 48, 2, seed=4, max_bounces=4), ref)
    finally:
        os.environ.pop("PTC_REFIT", None)


@pytest.mark.parametrize("name,kw,w,h,spp,seed,mb", [("atrium", {"scale": 0.05}, 160, 90, 4, 3, 8), ("textured_atrium", {"scale": 0.05, "tex_size": 64, "env_size": (64, 32)}, 120, 68, 4, 5, 6),
                                                      ("two_tris_sphere", {}, 64, 64, 2, 5, 3)])
def test_material_sort_is_an_option_that_changes_nothing_but_time(gpu, ora, name, kw, w, h, spp, seed, mb):
    """P9's per-wave material sort (PTC_SHADE_SORT=1: class rings in LDS by ballot + mbcnt, class-uniform batches of 64) is off by default — k_shade is
    bound by the CUs' memory path, the sort costs 11 % of its time — and either way the image and every counter are the oracle's, bit for bit."""
    d = gpu.scenes.by_name(name, **kw)
    c = ora.Oracle().load_scene(d).render(w, h, spp, seed=seed, max_bounces=mb)
    imgs = []
    for sort in ("1", "0"):
        os.environ["PTC_SHADE_SORT"] = sort
        try:
            pt = gpu.PathTracer(0).load_scene(d)
        finally:
            del os.environ["PTC_SHADE_SORT"]
        g = pt.render(w, h, spp, seed=seed, max_bounces=mb)
        assert _bits_equal(g, c), f"sort={sort}: {int((g != c).any(-1).sum())} pixels differ"
        imgs.append((g, pt.stats()))
    for k in COUNTERS:
        assert imgs[0][1][k] == imgs[1][1][k], k
