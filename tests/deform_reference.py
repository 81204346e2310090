"""numpy restatement of the deformation arithmetic (include/ptc.h, csrc/pt_deform.h), for tests/test_deform_host.py and
tests/test_gpu_deform.py, and the four-mesh scene both use.

`deform(...)` is the specification in float32, in the order written: numpy's float32 `+` and `*` round like IEEE binary32 without contraction, so the
library — the host evaluation and the kernel — must give the same BITS.  Nothing here calls the library."""
import dataclasses

import numpy as np

F32 = np.float32


def deform(base, dpos=None, dnormal=None, dtangent=None, morph_weights=None, joints=None, weights=None, joint_matrices=None):
    """base: MESH_VERTEX[n] (or (n, 12) float32).  dpos / dnormal / dtangent: (T, n, 3) float32 or None (zeros).  joints (n, 4) uint16, weights (n, 4),
    joint_matrices (n_joints, 12): J[c * 3 + r] of a column-major 4x4.  Returns (n, 12) float32: the posed vertices."""
    v = np.ascontiguousarray(base).view(F32).reshape(-1, 12).copy()
    p, n, t = v[:, 0:3].copy(), v[:, 3:6].copy(), v[:, 6:9].copy()
    if dpos is not None:
        dpos = np.asarray(dpos, F32)
        zero = np.zeros_like(dpos[0])
        for k in range(dpos.shape[0]):
            w = F32(morph_weights[k])
            p = p + w * dpos[k]
            n = n + w * (zero if dnormal is None else np.asarray(dnormal, F32)[k])
            t = t + w * (zero if dtangent is None else np.asarray(dtangent, F32)[k])
    if joints is not None:
        a, J, j = np.asarray(weights, F32), np.asarray(joint_matrices, F32).reshape(-1, 12), np.asarray(joints).astype(np.int64)
        S = ((a[:, 0:1] * J[j[:, 0]] + a[:, 1:2] * J[j[:, 1]]) + a[:, 2:3] * J[j[:, 2]]) + a[:, 3:4] * J[j[:, 3]]

        def through(x, translate):
            rows = []
            for r in range(3):
                y = (S[:, 0 + r] * x[:, 0] + S[:, 3 + r] * x[:, 1]) + S[:, 6 + r] * x[:, 2]
                rows.append(y + S[:, 9 + r] if translate else y)
            return np.stack(rows, 1)

        p, n, t = through(p, True), through(n, False), through(t, False)
    assert p.dtype == F32 and n.dtype == F32 and t.dtype == F32
    v[:, 0:3], v[:, 3:6], v[:, 6:9] = p, n, t
    return v


def mat34(m4):
    """(12,) float32 of a 4x4 given as m4[row][col]: rows 0..2, column by column."""
    m4 = np.asarray(m4, np.float64)
    return np.array([m4[r][c] for c in range(4) for r in range(3)], F32)


def trs(t=(0, 0, 0), axis=(0, 0, 1), angle=0.0, s=(1, 1, 1)):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    m = np.eye(4)
    m[:3, :3] = R @ np.diag(np.asarray(s, np.float64))
    m[:3, 3] = t
    return m


# ---- the scene of the tests --------------------------------------------------------------------------------------------------------
# four meshes whose vertex counts put every slice of the object-space vertex array at an odd offset:
#   0: 3 vertices, plain (an emissive triangle)      1: 257 vertices, T = 3, no skin, instanced twice
#   2: 64 vertices, skin only, one joint, EMISSIVE   3: 130 vertices, T = 1, 70 joints, the highest joint index in use
N_VERTS = (3, 257, 64, 130)


def _strip(n, rng, width=0.5, length=3.0):
    """a band of n vertices as a triangle strip in the xy plane, slightly wavy in z"""
    from pbr_amd.scene import MESH_VERTEX

    v = np.zeros(n, MESH_VERTEX)
    i = np.arange(n)
    x = (i // 2) * (length / (n // 2)) - length / 2
    v["position"] = np.stack([x, np.where(i % 2, width, -width), 0.05 * np.sin(3 * x)], 1).astype(F32)
    nrm = np.stack([-0.15 * np.cos(3 * x), np.zeros(n), np.ones(n)], 1)
    v["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    v["tangent"] = np.array([1, 0, 0, 1], F32)
    v["tangent"][1::3, 3] = -1
    v["texCoords"] = rng.random((n, 2), F32)
    idx = np.array([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(n - 2)], np.uint32).reshape(-1)
    return v, idx


def _grid(m, rng, size=1.0):
    from pbr_amd.scene import MESH_VERTEX

    v = np.zeros(m * m, MESH_VERTEX)
    gy, gx = np.mgrid[0:m, 0:m]
    v["position"] = np.stack([(gx.ravel() / (m - 1) - 0.5) * size, (gy.ravel() / (m - 1) - 0.5) * size, np.zeros(m * m)], 1).astype(F32)
    v["normal"] = np.array([0, 0, 1], F32)
    v["tangent"] = np.array([1, 0, 0, 1], F32)
    v["texCoords"] = rng.random((m * m, 2), F32)
    idx = []
    for y in range(m - 1):
        for x in range(m - 1):
            a = y * m + x
            idx += [a, a + 1, a + m, a + 1, a + m + 1, a + m]
    return v, np.array(idx, np.uint32)


@dataclasses.dataclass
class DeformScene:
    desc: object            # SceneDesc with the deformation fields set, the default pose
    poses: dict             # name -> {mesh: (morph_weights or None, joint_matrices or None)}


def scene(pbr, bvh_builder=None, w=64, h=48):
    from pbr_amd.scene import MESH_VERTEX, CameraDesc, InstanceDesc, Material, MeshDesc, SceneDesc

    rng = np.random.default_rng(5)
    mats = [Material((0.8, 0.7, 0.6, 1.0), 0.0, 1.0), Material((1.0, 1.0, 1.0, 1.0), 0.0, 1.0, emissive=(6.0, 5.0, 4.0)),
            Material((0.3, 0.5, 0.9, 1.0), 0.2, 0.6)]
    tri = np.zeros(3, MESH_VERTEX)
    tri["position"] = np.array([[-0.6, 2.4, 1.5], [0.6, 2.4, 1.5], [0.0, 2.4, 2.5]], F32)
    tri["normal"] = np.array([0, -1, 0], F32)
    tri["tangent"] = np.array([1, 0, 0, 1], F32)
    m0 = MeshDesc(tri, np.array([0, 1, 2], np.uint32), 1)

    v1, i1 = _strip(257, rng)
    d = lambda n, s: (s * rng.standard_normal((n, 3))).astype(F32)      # noqa: E731
    m1 = MeshDesc(v1, i1, 0, morph_dpos=np.stack([d(257, 0.1) for _ in range(3)]), morph_dnormal=np.stack([d(257, 0.2) for _ in range(3)]))

    v2, i2 = _grid(8, rng)
    w2 = np.zeros((64, 4), F32)
    w2[:, 0] = 1.0
    w2[::5] = np.array([0.5, 0.25, 0.125, 0.125], F32)                   # every entry names the one joint
    m2 = MeshDesc(v2, i2, 1, n_joints=1, joints=np.zeros((64, 4), np.uint16), weights=w2)

    v3, i3 = _strip(130, rng, width=0.4, length=2.6)
    j3 = rng.integers(0, 70, (130, 4)).astype(np.uint16)
    j3[129] = (69, 0, 69, 1)
    w3 = rng.random((130, 4), F32)
    w3 = (w3 / w3.sum(1, keepdims=True)).astype(F32)                      # used as given: the sum is 1 up to rounding
    m3 = MeshDesc(v3, i3, 2, morph_dpos=d(130, 0.08)[None], morph_dnormal=d(130, 0.1)[None], morph_dtangent=d(130, 0.1)[None],
                  n_joints=70, joints=j3, weights=w3)

    inst = [InstanceDesc(0), InstanceDesc(1, t=(0.0, 1.2, 0.0)), InstanceDesc(1, t=(0.3, -1.3, 0.4), q_wxyz=(0.9659258, 0.0, 0.0, 0.2588190), s=(0.9, 1.1, 1.0)),
            InstanceDesc(2, t=(-1.6, 0.0, 0.6), s=(1.0, 1.0, 1.0)), InstanceDesc(3, t=(0.4, 0.0, 0.5), s=(1.1, 1.0, 0.9))]
    cam = CameraDesc((0.0, 0.0, 5.5), (0.0, 0.0, 0.0), 0.9, w / h)
    desc = SceneDesc(mats, [m0, m1, m2, m3], inst, cam, name="deform", bvh_builder=bvh_builder)

    bend = np.stack([mat34(trs(t=(0.01 * k, 0.02 * np.sin(k), 0.03 * np.cos(k)), axis=(0.2, 1.0, 0.1), angle=0.01 * k, s=(1.0, 1.0 + 0.002 * k, 1.0))) for k in range(70)])
    gentle = np.stack([mat34(trs(t=(0.05 + 0.0005 * k, -0.1, 0.1), axis=(0.2, 1.0, 0.1), angle=0.25 + 0.0005 * k, s=(1.0, 1.1 + 0.0002 * k, 1.0))) for k in range(70)])
    poses = {
        "a": {1: (np.array([0.5, -0.25, 1.5], F32), None), 2: (None, mat34(trs(t=(0.1, 0.2, 0.0), axis=(0, 0, 1), angle=0.3, s=(1.2, 0.8, 1.0)))[None]),
              3: (np.array([0.75], F32), bend)},
        # another pose of mesh 3 alone (its morph weight stays)
        "shift": {3: (None, np.stack([mat34(trs(t=(0.25, 0.1, 0.0))) for _ in range(70)]))},
        # the temporal pair: a SMOOTH non-rigid pose (small morph weights, joint matrices that differ by little), then mesh 3 (a class-1 surface) shifted
        # parallel to the image plane: every joint matrix translated by the same vector.  Pose "a" is no input for the temporal reference: random deltas
        # and random joints per vertex make a surface as rough as the reference's plane-distance threshold (about a pixel's width), and 1.7 % of its
        # pixels have a tap within 1 % of that threshold; these poses leave 0.3 % (tests/test_deform_host.py holds that, without a GPU).
        "t": {1: (np.array([0.05, -0.025, 0.15], F32), None), 2: (None, mat34(trs(t=(0.1, 0.2, 0.0), axis=(0, 0, 1), angle=0.3, s=(1.2, 0.8, 1.0)))[None]),
              3: (np.array([0.075], F32), gentle)},
        "t_shifted": {3: (None, gentle + np.array([0] * 9 + [0.25, 0.1, 0.0], F32))},
        # the emissive grid squeezed onto a line: every one of its triangles has zero area, the set of emitters changes
        "collapse": {2: (None, mat34(trs(s=(0.0, 1.0, 1.0)))[None])},
        "nonfinite": {3: (None, np.concatenate([bend[:5], np.full((1, 12), np.nan, F32), bend[6:]]))},
    }
    return DeformScene(desc, poses)


def default_pose(me):
    w = None if me.morph_dpos is None else np.zeros(me.morph_dpos.shape[0], F32)
    J = None if me.joints is None else np.tile(mat34(np.eye(4)), (me.n_joints, 1))
    return w, J


def posed_vertices(desc, pose):
    """{mesh: (n, 12) float32}: the reference vertices of every mesh of `desc` under `pose` ({mesh: (weights or None, matrices or None)}; a missing half is the default)."""
    out = {}
    for m, me in enumerate(desc.meshes):
        w0, J0 = default_pose(me)
        w, J = pose.get(m, (None, None))
        out[m] = deform(me.vertices, me.morph_dpos, me.morph_dnormal, me.morph_dtangent, w0 if w is None else w, me.joints, me.weights, J0 if J is None else J)
    return out


def plain_desc(desc, verts):
    """The same scene as plain meshes that hold `verts` ({mesh: (n, 12) float32})."""
    from pbr_amd.scene import MESH_VERTEX, MeshDesc

    meshes = [MeshDesc(np.ascontiguousarray(verts[m], F32).view(MESH_VERTEX).reshape(-1), me.indices, me.material) for m, me in enumerate(desc.meshes)]
    return dataclasses.replace(desc, meshes=meshes)


def merged(*poses):
    out = {}
    for p in poses:
        for m, (w, J) in p.items():
            w0, J0 = out.get(m, (None, None))
            out[m] = (w0 if w is None else w, J0 if J is None else J)
    return out


def apply_pose(pt, pose):
    for m, (w, J) in pose.items():
        pt.update_mesh_pose(m, w, J)
    return pt
