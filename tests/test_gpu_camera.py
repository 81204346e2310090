"""Camera models on a real MI355X (include/ptc_camera.h: ptc_set_camera_ex; csrc/pt_camera.h, csrc/pt_camera.hip).

Nearly everything here is equality of bits.  The rays k_raygen_proj writes are the host evaluation's and the numpy restatement's (tests/camera_reference.py);
tile shares, adaptive frames and every launch policy give the plain frame; an orthographic image of a quad whose edges lie on pixel boundaries is the quad's
mask whatever the camera's distance; a panorama of an environment is that environment, and an environment again; the guides lie on the projection's own
rays.  The denoiser under the two new footprints and the reprojection under a rolled perspective camera are held to float64 evaluations with the tolerance
the existing denoise and temporal tests use (16 x the float32-float64 gap of the same evaluation).

The shapes are small on purpose: 33 x 17 x 3 samples is no multiple of 256, crosses block and wave boundaries, and 33 is no multiple of the 32-pixel tile."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_reference as ref  # noqa: E402
import lens_reference as lref  # noqa: E402
import pass_policies as pp  # noqa: E402
import temporal_reference as tref  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
W, H, FIRST, NS, SEED = 33, 17, 3, 3, 0x1234567890ABCDEF
PANORAMA_SEED = ref.PANORAMA_SEED      # tests/test_camera_host.py::test_panorama_precondition clears it
E_STATE = -2
EMISSION = ((3.1, 0.2, 0.7), (0.3, 2.7, 0.4), (0.5, 0.6, 4.3))


@pytest.fixture(scope="module")
def gpu(pbr):
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pbr


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def rot(axis, angle):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def matrix(rotation=np.eye(3), position=(0.0, 0.0, 0.0), scale=1.0):
    m = np.eye(4)
    m[:3, :3] = np.asarray(rotation) * scale
    m[:3, 3] = position
    return m


# no axis of the basis is a world axis, the camera is rolled about its own axis, and the columns carry a uniform scale
MAT = matrix(rot((1, 2, 3), 0.7) @ rot((0, 0, 1), 0.5), (3.1, -1.7, 2.3), 2.5)
CAMERAS = {
    "orthographic": dict(projection="orthographic", xmag=2.4, ymag=1.3),
    "equirect": dict(projection="equirect"),
    "perspective": dict(projection="perspective", yfov=0.9, aspect=W / H),
}
PROJ = {"orthographic": ref.ORTHOGRAPHIC, "equirect": ref.EQUIRECT, "perspective": ref.PERSPECTIVE}


def _quads(pbr, mat=MAT):
    """Three emissive quads of distinct colours facing the camera of `mat` at view depths 2, 3.5 and 6, overlapping in the image, and nothing else."""
    S = pbr.scene
    pos, f, s, u, _, _ = (np.asarray(v, F64) for v in ref.basis(mat))
    mats = [S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, e) for e in EMISSION]
    meshes = []
    for m, (z, cx, cy, half) in enumerate(((2.0, -0.45, 0.1, 0.4), (3.5, 0.2, -0.15, 0.9), (6.0, 1.6, 0.5, 2.2))):
        c = pos + z * f + cx * s + cy * u
        v, i = pbr.scenes._quad(c - half * s + half * u, c + half * s + half * u, c + half * s - half * u, c - half * s - half * u)      # s x (-u) = X x Y = -f: the front faces the camera
        meshes.append(S.MeshDesc(v, i, m))
    cam = S.CameraDesc((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.9, W / H, matrix=mat, **{k: v for k, v in CAMERAS["orthographic"].items()})
    return S.SceneDesc(mats, meshes, [S.InstanceDesc(k) for k in range(3)], cam, "camera_quads")


_state = {}


def _tracer(gpu):
    if "pt" not in _state:
        d = _quads(gpu)
        _state["desc"], _state["pt"] = d, gpu.PathTracer(0).load_scene(d)
    return _state["desc"], _state["pt"]


def _host(pbr, mat, lens=None, **cam):
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    assert pbr.load_library().ptc_scene_begin(pt._h) == 0
    pt.set_camera_ex(mat, **cam)
    if lens:
        pt.set_camera_lens(*lens)
    return pt


# ---- 1. the rays ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lens", [("orthographic", None), ("equirect", None), ("orthographic", (0.15, 3.5, 6, 0.3)), ("perspective", None), ("perspective", (0.15, 3.5, 6, 0.3))])
def test_device_rays_equal_host_rays_bit_for_bit(gpu, name, lens):
    """The launcher a batch would choose — k_raygen_proj under ORTHOGRAPHIC / EQUIRECT (a lens is ignored there), k_raygen / k_raygen_lens on the extended
    camera's basis under PERSPECTIVE — into lane 0's queue, read back; the host evaluation of the same headers; the numpy restatement."""
    desc, pt = _tracer(gpu)
    cam = CAMERAS[name]
    pt.set_camera_ex(MAT, **cam)
    pt.set_camera_lens(*(lens or (0.0, 1.0, 0, 0.0)))
    host = _host(gpu, MAT, lens, **cam)
    scattered = np.random.default_rng(5).permutation(W * H)[:97]
    for pixels in (np.arange(W * H), scattered):
        o, d = pt.debug_camera_rays(W, H, SEED, FIRST, NS, pixels)
        ho, hd = host.debug_camera_rays(W, H, SEED, FIRST, NS, pixels)
        assert o.shape == (NS * len(pixels), 3)
        assert _bits_equal(o, ho) and _bits_equal(d, hd), (name, lens)
        if name == "perspective":
            ro, rd, _ = lref.camera_rays(ref.basis(MAT, cam["yfov"], cam["aspect"]), lens or (0.0, 1.0, 0, 0.0), W, H, SEED, FIRST, NS, pixels)
        else:
            ro, rd, _ = ref.camera_rays(ref.basis(MAT, projection=PROJ[name]), PROJ[name], cam.get("xmag", 1.0), cam.get("ymag", 1.0), W, H, SEED, FIRST, NS, pixels)
        assert _bits_equal(o, ro) and _bits_equal(d, rd), (name, lens)
    pt.set_camera_lens()


# ---- 2. the projection under the frame machinery --------------------------------------------------------------------------------------------------------
def _render(pt, w, h, spp, name="orthographic", mat=MAT, seed=SEED, max_bounces=0, **kw):
    pt.set_camera_ex(mat, **CAMERAS[name])
    return pt.render(w, h, spp, seed=seed, max_bounces=max_bounces, **kw)


def test_rendered_orthographic_image_is_the_reference_rays_image(gpu):
    """Emitters at max_bounces = 0: the image is the emission of what each reference ray hits first, summed per pixel in sample order and divided by spp."""
    desc, pt = _tracer(gpu)
    got = _render(pt, W, H, NS)
    cam = CAMERAS["orthographic"]
    o, d, _ = ref.camera_rays(ref.basis(MAT, projection=ref.ORTHOGRAPHIC), ref.ORTHOGRAPHIC, cam["xmag"], cam["ymag"], W, H, SEED, 0, NS, np.arange(W * H))
    _, prim, _ = pt.trace_closest(o, d)
    _, _, tri_mat = pt.flat_scene()
    Le = np.concatenate([np.asarray(EMISSION, F32), np.zeros((1, 3), F32)])
    which = np.where(prim >= 0, tri_mat[np.maximum(prim, 0)], 3).reshape(NS, H, W)
    assert {int(m) for m in np.unique(which)} == {0, 1, 2, 3}, "the image shows all three quads and the background"
    acc = np.zeros((H, W, 3), F32)
    for k in range(NS):
        acc = (acc + Le[which][k]).astype(F32)
    want = np.ones((H, W, 4), F32)
    want[..., :3] = acc / F32(NS)
    assert _bits_equal(got, want)


def test_tile_shares_sum_to_the_unsharded_orthographic_frame(gpu):
    desc, pt = _tracer(gpu)
    w, h, spp = 70, 40, 3
    full = _render(pt, w, h, spp)
    total = np.zeros_like(full)
    for r in range(2):
        pt.frame_begin(w, h, spp, SEED, 0, 0, r, 2)
        pt.frame_add_samples(spp)
        pt.frame_resolve()
        share = pt.read_radiance()
        assert (share[..., 3] > 0).any() and not (share[..., 3] > 0).all()
        total += share
    assert _bits_equal(total, full)
    assert (full[..., :3] > 0).any() and not _bits_equal(full, _render(pt, w, h, spp, "perspective"))


def test_adaptive_orthographic_frame_holds_the_uniform_frames_bits(gpu):
    """max_bounces = 0 and emitters only: a pixel is noisy exactly where a quad's edge crosses it (the camera is rolled: no edge follows a pixel row), so
    covered and empty pixels stop at the first decision and edge pixels go on."""
    desc, pt = _tracer(gpu)
    pt.set_camera_ex(MAT, **CAMERAS["orthographic"])
    img = pt.render_adaptive(W, H, 24, seed=SEED, max_bounces=0, threshold=0.05, radius=0, min_samples=8, step_samples=8)
    counts = pt.read_sample_counts()
    present = sorted(int(n) for n in np.unique(counts))
    assert len(present) >= 2 and present[0] == 8, present
    for n in (present[0], present[-1]):
        uniform = _render(pt, W, H, n)
        sel = counts == n
        assert sel.any() and _bits_equal(img[sel], uniform[sel]), n


def _cornell(pbr, name):
    """The Cornell box under a new projection: ORTHOGRAPHIC from outside its open side, turned so that three walls show; EQUIRECT from a point inside."""
    d = pbr.scenes.cornell_box()
    if name == "orthographic":
        d.camera.matrix, d.camera.projection, d.camera.xmag, d.camera.ymag = pbr.ptc.look_at_matrix((1.1, 0.7, 3.0), (0.0, 0.0, 0.0)), "orthographic", 1.25, 1.25
    else:
        d.camera.matrix, d.camera.projection = matrix(position=(0.1, -0.2, 0.15)), "equirect"
    return d


@pytest.mark.parametrize("name", ["orthographic", "equirect"])
def test_launch_policies_give_the_default_frame(gpu, name):
    """tests/pass_policies.py's sweep — lanes, path order, batch size, the capped segment layout, the shade sort, the small grid: the image's bits and the nine
    counters are those of a context under the default environment."""
    desc = _cornell(gpu, name)
    with pp.tracer(gpu, desc, **pp.CAPPED_ENV) as pt:
        segs = int(pp.policy_field(pt, "shade_segments"))
    shapes = {"ragged": pp.RAGGED, "capped": (pp.CAPPED_W, pp.capped_height(segs), pp.CAPPED_SPP)}
    assert all(w * h * s < 160000 for w, h, s in shapes.values())
    frame = lambda pt, w, h, spp: pp.frame_record(pt, pt.render(w, h, spp, seed=pp.SEED, max_bounces=pp.BOUNCES))
    base = {}
    for shape, (w, h, spp) in shapes.items():
        with pp.tracer(gpu, desc) as pt:
            assert pt.get_camera_ex()["projection"] == name
            base[shape] = frame(pt, w, h, spp)
    img = base["ragged"]["image"]
    assert np.isfinite(img).all() and (img[..., :3] > 0).any(-1).mean() > 0.2 and base["ragged"]["counters"]["shadow_rays"] > 0
    for policy, env, shape, check in pp.ENV_POLICIES:
        w, h, spp = shapes[shape]
        with pp.tracer(gpu, desc, **env) as pt:
            got = frame(pt, w, h, spp)
            layout = pp.layout_of(pt, w * h, spp)
            check(pt, layout)
            pp.assert_same_frame(got, base[shape], f"{name} under {policy} {env}, layout {layout}")


# ---- 3. orthographic physics ----------------------------------------------------------------------------------------------------------------------------
def _ortho_quad(pbr):
    """A 16 x 16 frame over [-8, 8]^2 (xmag = ymag = 8: a pixel is one world unit, and every sample's origin is exact in binary32).  One emissive quad in the
    plane z = -5 facing +z, its edges on the pixel boundaries x = -5, 3 and y = -1, 6: columns 3..10, and — the image is upright, row 0 at y = +8 — rows 2..8.
    Not symmetric about either axis: a mirrored or a flipped image is another mask."""
    S = pbr.scene
    v, i = pbr.scenes._quad((-5, -1, -5), (3, -1, -5), (3, 6, -5), (-5, 6, -5))
    cam = S.CameraDesc((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), math.pi / 2, 1.0, matrix=np.eye(4), projection="orthographic", xmag=8.0, ymag=8.0)
    return S.SceneDesc([S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0, EMISSION[0])], [S.MeshDesc(v, i, 0)], [S.InstanceDesc(0)], cam, "ortho_quad")


def test_orthographic_image_of_a_quad_is_its_mask_at_every_distance(gpu):
    pt = gpu.PathTracer(0).load_scene(_ortho_quad(gpu))
    n = 16
    want = np.zeros((n, n), bool)
    want[2:9, 3:11] = True
    # precondition, from the reference's origins: no sample lies within 1e-4 pixel of an edge line, so float32 intersection cannot put it on the other side
    o, _, _ = ref.camera_rays(ref.basis(np.eye(4), projection=ref.ORTHOGRAPHIC), ref.ORTHOGRAPHIC, 8.0, 8.0, n, n, SEED, 0, 2, np.arange(n * n))
    edge = np.minimum(np.abs(o[:, :1].astype(F64) - np.array([-5.0, 3.0])).min(1), np.abs(o[:, 1:2].astype(F64) - np.array([-1.0, 6.0])).min(1)).min()
    assert edge > 1e-4, edge
    images = []
    for back in (0.0, 1.0, 7.0):
        pt.set_camera_ex(matrix(position=(0.0, 0.0, back)), "orthographic", xmag=8.0, ymag=8.0)
        images.append(pt.render(n, n, 2, seed=SEED, max_bounces=0))
    img = images[0]
    lit = (img[..., :3] != 0).any(-1)
    assert int(lit.sum()) == 7 * 8 and np.array_equal(lit, want)
    assert _bits_equal(img[want][:, :3], np.broadcast_to(np.asarray(EMISSION[0], F32), (56, 3))) and (img[~want][:, :3] == 0).all()
    assert _bits_equal(images[1], img) and _bits_equal(images[2], img)
    for back in (0.0, 7.0):      # the same scene through a perspective camera: the quad shrinks with the distance
        pt.set_camera_ex(matrix(position=(0.0, 0.0, back)), "perspective", yfov=math.pi / 2, aspect=1.0)
        images.append(int((pt.render(n, n, 2, seed=SEED, max_bounces=0)[..., :3] != 0).any(-1).sum()))
    assert images[3] != 56 and images[4] != 56 and images[3] > images[4] > 0, images[3:]


# ---- 4. the panorama round trip ---------------------------------------------------------------------------------------------------------------------------
def panorama_scene(pbr, env):
    """An environment and one small black triangle (a commit needs geometry) at distance 1 around the direction of the centre of pixel (10, 5) of a 32 x 16
    panorama: 0.02 across, a tenth of the pixel's 0.196 rad."""
    S = pbr.scene
    o, d = ref.point(ref.basis(np.eye(4), projection=ref.EQUIRECT), ref.EQUIRECT, 1.0, 1.0, F32(10.5 / 32), F32(5.5 / 16), dt=F64)
    c = np.asarray(d, F64).reshape(3)
    a = np.cross(c, (0.0, 1.0, 0.0))
    a /= np.linalg.norm(a)
    b = np.cross(c, a)
    tri = [c + 0.01 * a, c - 0.01 * a + 0.01 * b, c - 0.01 * a - 0.01 * b]
    v, i = pbr.scenes._quad(tri[0], tri[1], tri[2], tri[2])
    cam = S.CameraDesc((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), math.pi / 2, 1.0, matrix=np.eye(4), projection="equirect")
    d = S.SceneDesc([S.Material((0.0, 0.0, 0.0, 1.0), 0.0, 1.0)], [S.MeshDesc(v, i[:3], 0)], [S.InstanceDesc(0)], cam, "panorama")
    d.env = np.ascontiguousarray(env, F32)
    return d, np.asarray(tri, F64)


def panorama_env():
    """8 x 4 distinct texels, every channel its own: (h, w, 3)."""
    k = np.arange(32, dtype=F32).reshape(4, 8)
    return np.stack([0.25 + k / 8, 5.0 - k / 16, 1.0 + (k * 7 % 32) / 4], -1).astype(F32)


def panorama_excluded(tri, w=32, h=16):
    """The pixels whose rectangle meets the bounding box of the triangle's directions."""
    u, v = ref.env_uv(tri / np.linalg.norm(tri, axis=1, keepdims=True))
    x0, x1, y0, y1 = int(math.floor(u.min() * w)), int(math.floor(u.max() * w)), int(math.floor(v.min() * h)), int(math.floor(v.max() * h))
    mask = np.zeros((h, w), bool)
    mask[y0:y1 + 1, x0:x1 + 1] = True
    return mask


def test_panorama_round_trip(gpu):
    env = panorama_env()
    desc, tri = panorama_scene(gpu, env)
    out = panorama_excluded(tri)
    assert 1 <= out.sum() <= 4
    first = gpu.PathTracer(0).load_scene(desc).render(32, 16, 2, seed=PANORAMA_SEED, max_bounces=0)
    want = np.repeat(np.repeat(env, 4, 0), 4, 1)      # pixel (x, y) sees texel (x // 4, y // 4); (t + t) / 2 is exact
    assert _bits_equal(first[~out][:, :3], want[~out])
    again, _ = panorama_scene(gpu, first[..., :3])      # the capture as the environment of a second context
    second = gpu.PathTracer(0).load_scene(again).render(32, 16, 2, seed=PANORAMA_SEED, max_bounces=0)
    assert _bits_equal(second[~out], first[~out])



# ---- 5. guides ------------------------------------------------------------------------------------------------------------------------------------------
def test_orthographic_guides_over_a_plane(gpu):
    """A plane perpendicular to the camera's axis, 4.25 in front of it: Z is that distance to 1 ulp, and pos_class.xyz is o + Z d of the restatement's
    pixel-centre rays — k_guides_pos_proj's bytes.  The camera is rolled about its axis and scaled, and the axis is a world axis, so that the plane z = -2 and
    the distance from z = 2.25 are exact in binary32: the yardstick is the intersection's rounding, not the scene's.  A new extended camera invalidates the guides."""
    S = gpu.scene
    mat = matrix(rot((0, 0, 1), 0.5), (0.3, -0.4, 2.25), 2.5)
    assert (ref.basis(mat)[1] == F32([0, 0, -1])).all()
    v, i = gpu.scenes._quad((-9, -9, -2), (9, -9, -2), (9, 9, -2), (-9, 9, -2))
    cam = S.CameraDesc((0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 0.9, 1.0, matrix=mat, **CAMERAS["orthographic"])
    pt = gpu.PathTracer(0).load_scene(S.SceneDesc([S.Material((0.6, 0.5, 0.4, 1.0), 0.0, 1.0)], [S.MeshDesc(v, i, 0)], [S.InstanceDesc(0)], cam, "ortho_plane"))
    pt.frame_begin(W, H, 1, seed=1, max_bounces=0)
    pt.frame_guides()
    ak, nz, pk = pt.read_guide(0), pt.read_guide(1), pt.debug_guide_positions()
    assert (ak[..., 3] == 1).all() and _bits_equal(pk[..., 3], ak[..., 3])
    Z = nz[..., 3]
    worst = np.abs(Z.astype(F64) - 4.25).max()
    print(f"orthographic guides: Z within {worst:.3e} of 4.25 (one ulp {np.spacing(F32(4.25)):.3e})")
    assert worst <= np.spacing(F32(4.25))
    go, gd = ref.guide_rays(ref.basis(mat, projection=ref.ORTHOGRAPHIC), ref.ORTHOGRAPHIC, 2.4, 1.3, W, H)
    assert _bits_equal(gd, np.broadcast_to(ref.basis(mat)[1], gd.shape))
    assert _bits_equal(pk[..., :3], ref.guide_positions(go, gd, Z))
    assert not _bits_equal(go, np.broadcast_to(go[0, 0], go.shape))      # the origins are the pixels' own
    pt.set_camera_ex(mat, **CAMERAS["orthographic"])      # a new camera: the guides of the old one are gone
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.read_guide(0)
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.debug_guide_positions()


def test_equirect_guides_inside_a_box(gpu):
    """From a point inside the Cornell box [-1, 1]^3 every class-1 pixel's position lies on a face: one coordinate is +-1.  The bound is 4 ulp of the coordinate
    scale, taken per pixel as the largest magnitude in P = o + Z d, which is max(Z, 1) (|o| < 1, |d| <= 1, |P| <= 1): the error of P is that of Z, of the
    product and of the sum, each a rounding at that magnitude.  pos_class is o + Z d of the restatement's rays bit for bit; a miss (the open side) keeps o."""
    pt = gpu.PathTracer(0).load_scene(_cornell(gpu, "equirect"))
    w, h = 64, 32
    pt.frame_begin(w, h, 1, seed=1, max_bounces=0)
    pt.frame_guides()
    ak, nz, pk = pt.read_guide(0), pt.read_guide(1), pt.debug_guide_positions()
    K, Z = ak[..., 3], nz[..., 3]
    assert (K == 1).sum() > 0.6 * w * h and (K == 0).any() and (K == 2).any()
    go, gd = ref.guide_rays(ref.basis(matrix(position=(0.1, -0.2, 0.15)), projection=ref.EQUIRECT), ref.EQUIRECT, 1.0, 1.0, w, h)
    assert _bits_equal(pk[..., :3], ref.guide_positions(go, gd, Z))
    assert _bits_equal(pk[K == 0][:, :3], go[K == 0])
    P = pk[..., :3].astype(F64)
    off = np.abs(np.abs(P) - 1.0).min(-1)[K == 1]
    bound = 4 * np.spacing(np.maximum(Z, F32(1.0)))[K == 1].astype(F64)
    print(f"equirect guides: worst distance from a face {off.max():.3e}, worst share of its bound {(off / bound).max():.2f}")
    assert (off <= bound).all()
    assert (np.abs(P[K == 2][:, 1] - 0.998) < 1e-6).all()      # the emitter's plane


# ---- 6. the denoiser under the projections' footprints ------------------------------------------------------------------------------------------------------
def _synthetic(ak, seed):
    """albedo x a smooth ramp + seeded noise, alpha 1 (tests/test_gpu_denoise.py's input)"""
    h, w = ak.shape[:2]
    rng = np.random.default_rng(seed)
    ramp = 0.2 + 0.8 * (np.arange(w)[None, :, None] / w) * (0.5 + 0.5 * np.arange(h)[:, None, None] / h)
    img = np.ones((h, w, 4), F32)
    img[..., :3] = np.maximum(ak[..., :3] * ramp + 0.15 * rng.standard_normal((h, w, 3)), 0.0)
    return img


@pytest.mark.parametrize("name", ["orthographic", "equirect"])
def test_denoiser_is_the_specified_filter_under_the_projections_footprint(gpu, name):
    """tests/test_gpu_denoise.py::test_filter_is_the_specified_one with the projection's own P and footprint — ORTHOGRAPHIC 2 ymag / h at every depth (no Z in the
    plane-distance weight), EQUIRECT pi / h at unit distance: the library's image lies within 16 x E32 of the float64 evaluation, E32 the float32-float64 gap
    of the same evaluation over the image maximum."""
    desc = gpu.scenes.by_name("sphere10k")      # curved surfaces: the plane-distance weight decides between neighbours there
    if name == "orthographic":
        desc.camera.matrix, desc.camera.projection, desc.camera.xmag, desc.camera.ymag = gpu.ptc.look_at_matrix(desc.camera.position, desc.camera.target), "orthographic", 2.2, 1.2
    else:
        desc.camera.matrix, desc.camera.projection = matrix(rot((0, 1, 0), 0.4), (0.3, 1.0, 2.5)), "equirect"
    pt = gpu.PathTracer(0).load_scene(desc)
    noisy = pt.render(W, H, 4, seed=3)
    pt.frame_begin(W, H, 4, seed=1, max_bounces=8)
    pt.frame_guides()
    ak, nz = pt.read_guide(0), pt.read_guide(1)
    assert (ak[..., 3] == 1).mean() > 0.3
    go, gd = ref.guide_rays(ref.basis(desc.camera.matrix, projection=PROJ[name]), PROJ[name], desc.camera.xmag, desc.camera.ymag, W, H)
    P = ref.guide_positions(go, gd, nz[..., 3])
    pix, flat = ref.footprint(PROJ[name], H, ymag=desc.camera.ymag)
    worst = 0.0
    for label, img in (("rendered 4 spp", noisy), ("synthetic", _synthetic(ak, 11))):
        pt.write_radiance(img)
        for iters in (1, 4):
            for demod in (1, 0):
                p = dict(iterations=iters, sigma_l=4.0, sigma_n=128.0, sigma_p=1.0, demodulate=demod)
                pt.denoise(**p)
                pt.select_output(gpu.ptc.OUTPUT_DENOISED)
                got = pt.read_radiance()
                pt.select_output(gpu.ptc.OUTPUT_RADIANCE)
                e64, e32 = (ref.atrous(img[..., :3], ak, nz, P, pix, flat, dt=dt, **p) for dt in (F64, F32))
                top = float(e64.max())
                E32 = float(np.abs(e32.astype(F64) - e64).max()) / top
                err = float(np.abs(got[..., :3].astype(F64) - e64).max()) / top
                print(f"{name} {label}, {iters} iterations, demodulate {demod}: E32 {E32:.3g}, library error {err:.3g}, ratio {err / E32:.2f}")
                worst = max(worst, err / E32)
                assert np.array_equal(got[..., 3], img[..., 3])
                assert err <= 16 * E32, (label, iters, demod, err, E32)
                if name == "orthographic":      # the perspective rule (Z in the weight) is another image, far outside the tolerance: the test tells the two apart
                    other = float(np.abs(ref.atrous(img[..., :3], ak, nz, P, pix, False, dt=F64, **p) - e64).max()) / top
                    print(f"   with Z in the plane-distance weight the image would differ by {other:.3g}")
                    assert other > 16 * E32
    print(f"{name}: worst library error / E32 = {worst:.2f} (bound 16)")


# ---- 7. an extended perspective camera, end to end ----------------------------------------------------------------------------------------------------------
def _project(X, bas, w, h, dt):
    """Steps 1-2 of the temporal specification (temporal_reference.reproject) through an explicit basis."""
    pos, f, s, up, sx, sy = (np.asarray(t, dt) for t in bas)
    d = X.astype(dt) - pos
    z = (d * f).sum(-1)
    zs = np.where(z > 0, z, dt(1))
    xp = (((d * s).sum(-1) / zs) / sx + dt(1)) * dt(0.5) * dt(w) - dt(0.5)
    yp = (((d * up).sum(-1) / zs) / sy + dt(1)) * dt(0.5) * dt(h) - dt(0.5)
    return xp, yp, z > 0


def test_extended_perspective_camera_end_to_end(gpu):
    """A camera rolled 30 degrees about its axis, which ptc_set_camera cannot express: guides, ptc_focus_distance_at_pixel and two ptc_temporal_accumulate with
    a camera move between them succeed.  The move is a further roll of 10 degrees, the scene is static: the motion buffer puts every class-1 pixel where the
    projection of its hit point through the PREVIOUS basis puts it, within 16 x the float32-float64 gap of that projection (in pixels) — the existing temporal
    test's tolerance."""
    w, h = 48, 32
    yfov, aspect = math.radians(40.0), w / h
    desc = gpu.scenes.cornell_box()
    look = gpu.ptc.look_at_matrix(desc.camera.position, desc.camera.target)
    mats = [look @ matrix(rot((0, 0, 1), math.radians(a))) for a in (30.0, 40.0)]
    desc.camera.matrix, desc.camera.fov_y, desc.camera.aspect = mats[0], yfov, aspect
    pt = gpu.PathTracer(0).load_scene(desc)
    assert pt.get_camera_ex()["projection"] == "perspective"
    shade = pt.shading_tables()[0]
    tri = np.ascontiguousarray(shade.reshape(shade.shape[0], -1, 4)[:, :3, :3]).astype(F64)
    guides = []
    for k, m in enumerate(mats):
        pt.set_camera_ex(m, "perspective", yfov=yfov, aspect=aspect)
        pt.frame_begin(w, h, 1, seed=1 + k, max_bounces=6)
        pt.frame_add_samples(1)
        pt.frame_guides()
        pt.frame_resolve()
        prim, uv = pt.read_guide_hit()
        guides.append((pt.read_guide(0), pt.read_guide(1), prim, uv))
        Z = guides[-1][1][h // 2, w // 2, 3]
        assert Z > 0 and _bits_equal(F32(pt.focus_distance_at_pixel(w // 2, h // 2)), lref.focus_distance(ref.basis(m, yfov, aspect), w, h, w // 2, h // 2, Z))
        pt.temporal_accumulate(max_history=32, sigma_z=1.0, demodulate=1)
    motion = pt.read_temporal(2)
    ak, nz, prim, uv = guides[1]
    surf = ak[..., 3] == 1
    assert surf.mean() > 0.5
    pr = np.where(surf, prim, 0)
    u, v = uv[..., 0].astype(F64)[..., None], uv[..., 1].astype(F64)[..., None]
    X = (((1.0 - u) - v) * tri[pr, 0] + u * tri[pr, 1]) + v * tri[pr, 2]
    prev = ref.basis(mats[0], yfov, aspect)
    (x64, y64, front), (x32, y32, _) = _project(X, prev, w, h, F64), _project(X.astype(F32), prev, w, h, F32)
    keep = surf & front
    assert keep.sum() == surf.sum()
    E32 = max(np.abs(x32.astype(F64) - x64)[keep].max(), np.abs(y32.astype(F64) - y64)[keep].max())
    err = max(np.abs(motion[..., 0].astype(F64) - x64)[keep].max(), np.abs(motion[..., 1].astype(F64) - y64)[keep].max())
    ys, xs = np.mgrid[0:h, 0:w]
    moved = np.hypot(x64 - xs, y64 - ys)[keep]
    print(f"rolled perspective camera: motion E32 {E32:.3g} px, library error {err:.3g} px, ratio {err / E32:.2f}; a pixel moved {moved.mean():.2f} px on average")
    assert err <= 16 * E32
    assert moved.mean() > 1.0 and (motion[..., 2][keep] > 0).mean() > 0.5      # a real move, and most of the history is found again


# ---- 8. the command-line renderer ---------------------------------------------------------------------------------------------------------------------------
def _read_pfm(path, w, h):
    head, body = open(path, "rb").read().split(b"-1.0\n", 1)
    assert head.startswith(b"PF\n%d %d" % (w, h))
    return np.ascontiguousarray(np.frombuffer(body, "<f4").reshape(h, w, 3)[::-1])        # PFM rows are bottom-up


def test_cpp_host_cli_renders_through_the_assets_camera(gpu, tmp_path):
    """ptc_render --gltf cam.glb --camera 1: the float image and the PNG's bytes are those of the Python render through Asset.apply_camera(1) with the frame's
    aspect; --ortho switches that camera's projection."""
    from PIL import Image

    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    w, h = 48, 40
    desc = gpu.scenes.cornell_box()
    q = (math.cos(0.25), 0.0, 0.0, math.sin(0.25))      # (w, x, y, z): a roll of 0.5 rad
    cams = [dict(type="orthographic", xmag=1.1, ymag=1.1, translation=(0.0, 0.0, 3.0)), dict(type="perspective", yfov=0.8, translation=(0.2, 0.1, 3.4), rotation=q)]
    path, out, png = str(tmp_path / "cam.glb"), str(tmp_path / "c.pfm"), str(tmp_path / "c.png")
    gpu.gltf.write_glb(desc, path, cameras=cams)
    common = [exe, "--gltf", path, "--width", str(w), "--height", str(h), "--spp", "4", "--seed", "5", "--bounces", "3", "--out", out, "--png", png]
    a = gpu.gltf.Asset(path)
    pt = gpu.PathTracer(0)
    a.load_into(pt)
    for extra, switch in ((["--camera", "1"], {}), (["--camera", "0"], {}), (["--camera", "1", "--ortho", "1.5,1.25"], dict(projection=1, xmag=1.5, ymag=1.25))):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        p = a.camera(int(extra[1]), w / h).update(**switch)
        pt._ck(pt._L.ptc_set_camera_ex(pt._h, C.byref(p)))
        img = pt.render(w, h, 4, seed=5, max_bounces=3)
        assert (img[..., :3] > 0).any(-1).mean() > 0.3
        assert _bits_equal(_read_pfm(out, w, h), np.ascontiguousarray(img[..., :3])), extra
        assert np.array_equal(np.asarray(Image.open(png)), pt.tonemap()), extra
    a.close()


# ---- 9. what the first review asked for ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["orthographic", "equirect"])
def test_sampled_denoiser_under_the_projections_footprint(gpu, name):
    """ptc_denoise_sampled under ORTHOGRAPHIC and EQUIRECT, as tests/test_gpu_sampled.py holds it under the look-at camera: the float64 evaluation from the
    library's own read-backs (radiance, counts, the sampled variance, guides) with the projection's P and footprint, to 16 x E32; other classes pass through."""
    import sampled_reference as sref

    desc = gpu.scenes.by_name("sphere10k")
    if name == "orthographic":
        desc.camera.matrix, desc.camera.projection, desc.camera.xmag, desc.camera.ymag = gpu.ptc.look_at_matrix(desc.camera.position, desc.camera.target), "orthographic", 2.2, 1.2
    else:
        desc.camera.matrix, desc.camera.projection = matrix(rot((0, 1, 0), 0.4), (0.3, 1.0, 2.5)), "equirect"
    pt = gpu.PathTracer(0).load_scene(desc)
    pt.set_sample_covariance(1)
    pt.frame_begin(W, H, 16, seed=3, max_bounces=4)
    pt.frame_set_adaptive(threshold=0.1, radius=1)
    pt.frame_add_samples(8)
    while pt.frame_adapt():
        pt.frame_add_samples(8)
    pt.frame_resolve()
    pt.frame_guides()
    rad, counts = pt.read_radiance(), pt.read_sample_counts()
    ak, nz = pt.read_guide(0), pt.read_guide(1)
    surf = ak[..., 3] == 1
    assert surf.mean() > 0.3 and (counts[surf] >= 4).all()
    go, gd = ref.guide_rays(ref.basis(desc.camera.matrix, projection=PROJ[name]), PROJ[name], desc.camera.xmag, desc.camera.ymag, W, H)
    P = ref.guide_positions(go, gd, nz[..., 3])
    pix, flat = ref.footprint(PROJ[name], H, ymag=desc.camera.ymag)
    for demod in (1, 0):
        p = dict(iterations=3, sigma_l=4.0, sigma_n=128.0, sigma_p=1.0, demodulate=demod)
        pt.denoise_sampled(**p)
        pt.select_output(gpu.ptc.OUTPUT_DENOISED)
        got = pt.read_radiance()
        pt.select_output(gpu.ptc.OUTPUT_RADIANCE)
        sv = pt.read_sampled_variance()
        D = sref.demodulated(rad, ak, demod)
        var_n = sv[..., 1].astype(F64) * sv[..., 0].astype(F64)
        e64, e32 = (ref.atrous(rad[..., :3], ak, nz, P, pix, flat, dt=dt, D=D, var_n=var_n, n=counts, **p) for dt in (F64, F32))
        top = float(e64.max())
        E32 = float(np.abs(e32.astype(F64) - e64).max()) / top
        err = float(np.abs(got[..., :3].astype(F64) - e64).max()) / top
        print(f"{name} sampled, demodulate {demod}: E32 {E32:.3g}, library error {err:.3g}, ratio {err / E32:.2f} (bound 16)")
        assert np.array_equal(got[..., 3], rad[..., 3]) and _bits_equal(got[~surf], rad[~surf])
        assert err <= 16 * E32, (name, demod, err, E32)


def test_a_raster_frame_refuses_a_change_to_another_projection(gpu):
    """ptc_frame_begin refuses a raster frame under ORTHOGRAPHIC / EQUIRECT; so does ptc_set_camera_ex while a raster frame is open, with nothing changed — the
    frame's later batches would run k_raygen on a basis that has no projection.  A perspective change, and any change during a path frame, are taken."""
    pt = gpu.PathTracer(0).load_scene(gpu.scenes.cornell_box())
    kind = gpu.ptc.INTEGRATOR_RASTER_COMPAT
    plain = pt.render(W, H, 1, seed=1, integrator=kind)
    pt.frame_begin(W, H, 1, seed=1, max_bounces=8, integrator=kind)
    for name in ("orthographic", "equirect"):
        with pytest.raises(gpu.PtcError, match="ptc error -2.*raster frame.*PTC_PROJ_" + name.upper()[:5]):
            pt.set_camera_ex(MAT, name)
        assert pt.get_camera_ex() is None
    pt.frame_add_samples(1)
    pt.frame_resolve()
    assert _bits_equal(pt.read_radiance(), plain)
    pt.frame_begin(W, H, 1, seed=1, max_bounces=8, integrator=kind)
    pt.set_camera_ex(MAT, "perspective", yfov=0.9, aspect=W / H)      # taken: the raster integrators serve it
    pt.frame_begin(W, H, 2, seed=1, max_bounces=2)
    pt.set_camera_ex(MAT, "equirect")      # a path frame: taken, for the batches queued afterwards
    pt.frame_add_samples(2)
    pt.frame_resolve()
    assert np.isfinite(pt.read_radiance()).all()
    with pytest.raises(gpu.PtcError, match="ptc error -2"):
        pt.frame_begin(W, H, 1, seed=1, max_bounces=8, integrator=kind)


def _write_env_pfm(path, env):
    """A PFM that ptc_render --env reads as the map `env` (h, w, 3; row 0 = +y): --env takes the file's top row for the map's LAST row, and a PFM stores its rows
    bottom-up, so the map's rows go out in their own order."""
    h, w = env.shape[:2]
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h) + np.ascontiguousarray(env, "<f4").tobytes())


def test_cpp_host_cli_panorama_round_trips_through_env(gpu, tmp_path):
    """ptc_render --panorama --pfm p.pfm, then --env p.pfm: the round trip of test_panorama_round_trip through the command-line renderer.  The 32 x 16 capture
    (PANORAMA_SEED, 2 spp, bounces 0) of the 8 x 4 environment is that environment and the library's capture bit for bit outside the triangle's pixels, by the
    look-at camera's position (--cam-pos) and by --cam-matrix alike; fed back through --env, the second capture equals the first on the same pixels."""
    exe = os.path.join(os.path.dirname(gpu.ptc.LIB_PATH), "ptc_render")
    env = panorama_env()
    desc, tri = panorama_scene(gpu, env)
    out = panorama_excluded(tri)
    glb, env0 = str(tmp_path / "tri.glb"), str(tmp_path / "env0.pfm")
    gpu.gltf.write_glb(desc, glb)
    _write_env_pfm(env0, env)
    common = [exe, "--gltf", glb, "--panorama", "--width", "32", "--height", "16", "--spp", "2", "--seed", str(PANORAMA_SEED), "--bounces", "0"]
    look = ["--cam-pos", "0", "0", "0", "--cam-target", "0", "0", "-1"]
    captures = {}
    for label, cam, env_file in (("first", look, env0), ("matrix", ["--cam-matrix", "1,0,0,0,0,1,0,0,0,0,1,0,0,0,0,1"], env0), ("second", look, str(tmp_path / "first.pfm"))):
        pfm = str(tmp_path / (label + ".pfm"))
        r = subprocess.run(common + cam + ["--env", env_file, "--pfm", pfm], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        captures[label] = _read_pfm(pfm, 32, 16)[::-1]      # written as --env reads it: rows reversed
    want = np.repeat(np.repeat(env, 4, 0), 4, 1)
    library = gpu.PathTracer(0).load_scene(desc).render(32, 16, 2, seed=PANORAMA_SEED, max_bounces=0)[..., :3]
    assert _bits_equal(captures["first"][~out], want[~out]) and _bits_equal(captures["first"], library)
    assert _bits_equal(captures["matrix"], captures["first"])
    assert _bits_equal(captures["second"][~out], captures["first"][~out])
