"""Inputs for the sweep of the device BVH builders (csrc/pt_build.hip) over the sizes at which its kernels change path, and over triangle soups that leave
the builders nothing to decide by: for tests/test_build_sweep_host.py (the CPU anchor) and tests/test_gpu_build_sweep.py (the device).  Pure numpy, seeded.

The counts sit on either side of the constants of pt_build.hip: 64 lanes (k_sah_small's partition steps), kSortTile = 512 keys per wave and 4 tiles = 2048 keys per
block of the sort, kSahBig = 1024 (one wave or several workgroups cut a range), kSahChunk = 4096 (a second workgroup for one range), 256 tiles = 131,072 keys per
round of k_sort_scan_tiles, and 1024 x 256 = 262,144 triangles per trip of k_bld_prims' grid-stride loop.

`desc(pbr, kind, N)`: exactly N triangles in two meshes with one identity instance each; materials and camera are the Cornell box's.  The first N - max(1, N // 16)
triangles are diffuse, the rest emissive, so that the emitter table, its cdf and the shading records are part of every comparison.

Kinds.  Generic (no two triangles coincide exactly):
  uniform     centres uniform in [-0.8, 0.8]^3, a random small shape each; the edge shrinks with N (0.04 at 1k, 0.0025 at 262k) so that the scene stays sparse
  line        centres differ in x only (one shape, in a plane x = const, moved along x): two SAH axes are off, two Morton axes constant
  geom        centres at x = 0.9 * 0.5^min(k, 110) (no denormal), y = z = 0, edge about 1e-3: a deep lopsided tree, and many equal centres at the tail, where the
              vertices' float32 x absorbs the centre's; the triangles there are n distinct sizes of one shape about the common centre
Tie-heavy:
  same        one triangle N times: every centre, box and Morton key is the same
  outlier     `same` with triangle 0 moved to (50, 50, 50): a cut that leaves one triangle on one side
  lattice     64 distinct triangles tiled to N: runs of about N / 64 equal keys, which lie across the boundaries of the sort's tiles
  degdupzero  `uniform` with every third triangle's x coordinates -0.0 or +0.0, the first 300 triangles of zero area (third vertex = second) and the last 400 exact
              copies of the first 400"""
import numpy as np

GENERIC = ("uniform", "line", "geom")
TIE_HEAVY = ("same", "outlier", "lattice", "degdupzero")
KINDS = GENERIC + TIE_HEAVY
BUILDERS = ("lbvh", "sah")

CASES = ([("uniform", n) for n in (2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 131072, 131073, 262445)]
         + [(k, n) for k in ("line", "geom", "same", "outlier", "lattice") for n in (65, 1024, 4097)]
         + [("degdupzero", 2049)])
TRACED = 8193                                                 # up to this count a case is traced against the oracle as well
SMALL_CASES = [c for c in CASES if c[1] <= TRACED]
LARGE_CASES = [c for c in CASES if c[1] > TRACED]

# the walk of the stale-scratch tests: small trees on a context whose grow-only scratch and spare tree set were sized by large ones
WALK = [("uniform", 262445), ("uniform", 65), ("same", 4097), ("outlier", 1024), ("uniform", 131073), ("uniform", 2), ("uniform", 8193)]


def case_id(case):
    return "%s-%d" % case


def _edge(n):
    return min(0.3, 1.265 / np.sqrt(n))


def _card(e):
    """A triangle in the plane x = 0 whose box is centred on the origin: corners (3, 3)."""
    return np.array([[0.0, -e, -e], [0.0, e, -e], [0.0, 0.0, e]])


def _uniform(rng, n):
    ctr = rng.uniform(-0.8, 0.8, (n, 1, 3))
    return ctr + _edge(n) * rng.uniform(-1.0, 1.0, (n, 3, 3))


def soup(kind, n):
    """float32 (n, 3, 3): the corners of the n triangles of `kind`."""
    assert kind in KINDS and n >= 2
    rng = np.random.default_rng([KINDS.index(kind), n])
    if kind == "uniform":
        pos = _uniform(rng, n)
    elif kind == "line":
        x = rng.permutation(np.linspace(-0.8, 0.8, n))
        pos = np.tile(_card(0.05) + (0.0, 0.25, -0.125), (n, 1, 1))
        pos[:, :, 0] = x[:, None]
    elif kind == "geom":
        x = 0.9 * 0.5 ** np.minimum(np.arange(n), 110).astype(np.float64)
        shape = 1e-3 * np.array([[-1.0, -1.0, -1.0], [1.0, -1.0, 1.0], [0.0, 1.0, 0.0]])         # its box is centred on the origin in all three axes
        pos = shape[None] * rng.permutation(np.linspace(0.5, 2.0, n))[:, None, None]           # n distinct sizes about the same centre
        pos[:, :, 0] += x[:, None]                                                             # float32 absorbs x below about 2^-34: equal centres from there on
    elif kind in ("same", "outlier"):
        one = np.array([0.1, 0.2, -0.3]) + 0.04 * np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
        pos = np.tile(one, (n, 1, 1))
        if kind == "outlier":
            pos[0] += 50.0 - np.array([0.1, 0.2, -0.3])
    elif kind == "lattice":
        g = np.linspace(-0.6, 0.6, 4)
        ctr = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(64, 1, 3)
        base = ctr + 0.04 * rng.uniform(-1.0, 1.0, (64, 3, 3))
        pos = base[np.arange(n) % 64]
    else:
        assert n >= 800
        pos = _uniform(rng, n)
        third = np.arange(0, n, 3)
        pos[third, :, 0] = np.where(rng.random((len(third), 3)) < 0.5, -0.0, 0.0)
        pos[:300, 2] = pos[:300, 1]
        pos[-400:] = pos[:400]
    pos = pos.astype(np.float32)
    if kind in GENERIC:
        flat = np.ascontiguousarray(pos.reshape(n, 9)).view(np.dtype((np.void, 36)))
        assert len(np.unique(flat)) == n, "%s %d: two triangles coincide" % (kind, n)
    return pos


def desc(pbr, kind, n):
    """The SceneDesc of soup(kind, n)."""
    sc = pbr.scene
    base = pbr.scenes.cornell_box()
    pos = soup(kind, n)
    n_lit = max(1, n // 16)
    meshes = []
    for part, mat in ((pos[:n - n_lit], 0), (pos[n - n_lit:], 3)):       # material 0 is diffuse, 3 the emitter
        v = np.zeros(3 * len(part), sc.MESH_VERTEX)
        v["position"], v["normal"], v["tangent"] = part.reshape(-1, 3), (0, 0, 1), (1, 0, 0, 1)
        meshes.append(sc.MeshDesc(v, np.arange(3 * len(part), dtype=np.uint32), mat))
    assert max(base.materials[3].emissive) > 0 and max(base.materials[0].emissive) == 0
    ident = lambda m: sc.InstanceDesc(m, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    d = sc.SceneDesc(base.materials, meshes, [ident(0), ident(1)], base.camera, "%s%d" % (kind, n))
    assert d.n_triangles == n
    return d
