"""The scenes and the layout arithmetic of tests/test_gpu_pass_policies.py without a GPU, on description-only contexts.

1. passes_surface and passes_volume (pbr_amd/scenes.py) load; the alpha, glass and emission-texture tables of passes_surface are not empty; passes_volume has a
   medium and no conflict with it; the camera's rays cross every feature of both scenes (on the description: outlines, not occlusion — the GPU module holds the
   activity counters).
2. tests/pass_policies.py restates ptc_seg_layout and ptc_seg_slots: held to csrc/ptc_internal.h through tools/seg_layout_host.cpp, a stand-alone program over the
   header, on a sweep of (n, max_seg).
3. The two frame shapes give the layouts the GPU module relies on at 256 segments, and the capped height follows other segment counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lens_reference as lref  # noqa: E402
import pass_policies as pp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "physically-based-renderer_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
F64 = np.float64


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------------------
def _world_triangles(desc):
    """(n, 3, 3) float64 world positions and (n,) material ids; the scenes here use identity instances."""
    tris, mats = [], []
    for it in desc.instances:
        assert tuple(it.t) == (0.0, 0.0, 0.0) and tuple(it.s) == (1.0, 1.0, 1.0) and it.matrix is None
        m = desc.meshes[it.mesh]
        P = m.vertices["position"].astype(F64)[m.indices.reshape(-1, 3)]
        tris.append(P)
        mats += [m.material] * len(P)
    return np.concatenate(tris), np.array(mats)


def _rays_crossing(desc, w, h):
    """Per triangle, the pixel-centre pinhole rays of a w x h image whose line crosses it in front of the camera (Moeller-Trumbore in float64, no occlusion)."""
    pos, f, s, u, sx, sy = (np.asarray(v, F64) for v in lref.camera_basis(desc.camera))
    px, py = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    d = f[None] + ((2 * px.ravel() / w - 1) * sx)[:, None] * s[None] + ((2 * py.ravel() / h - 1) * sy)[:, None] * u[None]
    tris, mats = _world_triangles(desc)
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    pv = np.cross(d[:, None, :], e2[None])
    det = (pv * e1[None]).sum(-1)
    tv = pos[None, None] - tris[None, :, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        bu = (pv * tv).sum(-1) / det
        qv = np.cross(tv, e1[None])
        bv = (qv * d[:, None, :]).sum(-1) / det
        t = (qv * e2[None]).sum(-1) / det
    hit = (np.abs(det) > 1e-12) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0)
    return hit.sum(0), mats


def test_passes_surface_loads_with_every_table(pbr):
    m = pbr.ptc
    for top, n_tris in (("normal", 30), ("invisible", 30), ("none", 24)):
        desc = pbr.scenes.by_name("passes_surface", top=top)
        assert desc.n_triangles == n_tris and desc.n_triangles < 100
        pt = pbr.PathTracer(m.DEVICE_NONE).load_scene(desc)
        abits, amode, _, n_prims, _ = pt.alpha_tables()
        gbits, gmats, g_prims, _ = pt.glass_tables()
        recs, cdf, prim_map, total = pt.emissive_tex_table()
        assert n_prims == g_prims == n_tris == prim_map.size
        alpha_prims = [p for p in range(n_tris) if (abits[p >> 5] >> (p & 31)) & 1]
        glass_prims = [p for p in range(n_tris) if (gbits[p >> 5] >> (p & 31)) & 1]
        assert alpha_prims == [10, 11] + ([26, 27] if top != "none" else [])                     # the BLEND sheet, then the MASK sheet between the panes
        assert glass_prims == list(range(12, 24)) + ([24, 25, 28, 29] if top != "none" else [])      # the slab, then the two thin panes
        assert list(amode[[5, 7]]) == [m.ALPHA_BLEND, m.ALPHA_MASK]
        assert len(recs) == 2 and total > 0 and list(np.flatnonzero(prim_map >= 0)) == [8, 9]
        assert pt.stats()["n_emitters"] == 2
        L, h = pt._L, pt._h
        assert L.ptc_frame_begin(h, 8, 8, 1, 1, 2, m.INTEGRATOR_PATH, 0, 1) == -3                 # PTC_E_DEVICE: nothing in the description refuses the frame before that
        pt.close()
    # the variants keep what bit equality between them needs: the ids of everything else, and the largest extent (the ray epsilon's)
    a, b = (_world_triangles(pbr.scenes.passes_surface(top=t))[0] for t in ("invisible", "none"))
    assert np.array_equal(a[:24], b)
    assert (a.reshape(-1, 3).max(0) - a.reshape(-1, 3).min(0)).max() == (b.reshape(-1, 3).max(0) - b.reshape(-1, 3).min(0)).max() == 8.0
    assert a[24:, :, 1].min() > b[:, :, 1].max()                                                   # they lie above everything else


def test_passes_volume_loads_without_a_medium_conflict(pbr):
    m = pbr.ptc
    desc = pbr.scenes.by_name("passes_volume")
    assert desc.n_triangles == 8 and desc.medium is not None and desc.env is not None
    pt = pbr.PathTracer(m.DEVICE_NONE).load_scene(desc)
    assert pt.get_medium()["sigma_t"] > 0
    assert not pt.alpha_tables()[0].any() and not pt.glass_tables()[0].any() and pt.emissive_tex_table()[0].shape[0] == 0
    L, h = pt._L, pt._h
    assert L.ptc_frame_begin(h, 8, 8, 1, 1, 2, m.INTEGRATOR_PATH, 0, 1) == -3, L.ptc_last_error(h)  # PTC_E_DEVICE, not the PTC_E_STATE of a medium conflict
    assert b"medium" not in L.ptc_last_error(h)
    pt.close()


def test_camera_rays_cross_every_feature(pbr):
    w, h = pp.RAGGED[:2]
    count, mats = _rays_crossing(pbr.scenes.passes_surface(), w, h)
    per_material = {int(k): int(count[mats == k].sum()) for k in np.unique(mats)}
    print("passes_surface: pixel-centre rays crossing the triangles of each material:", per_material)
    assert sorted(per_material) == list(range(10)) and all(v >= 4 for v in per_material.values()), per_material
    desc = pbr.scenes.passes_volume()
    count, mats = _rays_crossing(desc, w, h)
    assert all(int(count[mats == k].sum()) >= 4 for k in range(3))
    # and the medium's box: rays that enter it (slab test)
    pos, f, s, u, sx, sy = (np.asarray(v, F64) for v in lref.camera_basis(desc.camera))
    lo, hi = np.asarray(desc.medium["box_lo"], F64), np.asarray(desc.medium["box_hi"], F64)
    with np.errstate(divide="ignore"):
        t0, t1 = (lo - pos) / f, (hi - pos) / f
    assert np.minimum(t0, t1).max() < np.maximum(t0, t1).min()                                      # the central ray


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_layout_restatement_equals_the_header(tmp_path):
    exe = tmp_path / "seg_layout_host"
    cmd = ["c++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC, os.path.join(ROOT, "tools", "seg_layout_host.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = []
    for max_seg in (1, 2, 4, 9, 256, 304, 16384):
        ns = {0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4255, 157784, max_seg * 512 - 1, max_seg * 512, max_seg * 512 + 1, max_seg * 576, max_seg * 640 + 1,
              max_seg * 1000 + 7, 0x7fffffff, 0xfffffff0 - 64 * max_seg - 64}
        cases += [(n, max_seg) for n in sorted(ns)]
    rng = np.random.default_rng(3)
    cases += [(int(n), int(m)) for n, m in zip(rng.integers(0, 1 << 24, 400), rng.integers(1, 16385, 400))]
    r = subprocess.run([str(exe)], input="".join(f"{n} {m}\n" for n, m in cases), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    for (n, m), row in zip(cases, rows):
        n_seg, seg_len = pp.seg_layout(n, m)
        assert row == (n, m, n_seg, seg_len, pp.seg_slots(n, m)), (row, n_seg, seg_len)
        assert seg_len % 64 == 0 and 1 <= n_seg <= m
        if n + 511 < 1 << 32:                                                                       # the header's own claim, where its 32-bit sums do not wrap
            assert n <= n_seg * seg_len <= pp.seg_slots(n, m), (n, m)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_frame_shapes_give_the_layouts_claimed():
    w, h, spp = pp.RAGGED
    assert w * h == 851 and 851 % 64 != 0 and w * h * spp == 4255
    assert pp.seg_layout(4255, 256) == (9, 512) and pp.seg_layout(4255, 16384) == (9, 512)
    assert (9 + 3) // 4 == 3 and 9 % 4 == 1                                                      # a walk grid of 3 blocks; the last has one live wave
    assert pp.seg_layout(851, 256) == (2, 448)                                                    # one sample per batch
    assert pp.seg_layout(2 * 851, 256) == (4, 448)                                                # two
    assert pp.capped_height(256) == 121 and pp.CAPPED_W * 121 * pp.CAPPED_SPP == 157784 < 160000
    assert pp.seg_layout(157784, 256) == (256, 640) and 640 % 512 != 0 and -(-157784 // 256) == 617
    assert pp.seg_layout(157784, 16384) == (309, 512)                                             # the same frame under the default 64 segments per CU: not capped
    for segs in (64, 128, 208, 256, 304, 320):                                                    # other CU counts: the derived height keeps the three conditions
        n = pp.CAPPED_W * pp.capped_height(segs) * pp.CAPPED_SPP
        assert pp.is_capped(n, segs), (segs, n, pp.seg_layout(n, segs))
        assert pp.is_capped(pp.capped_paths(segs), segs)
