"""Light probes without a GPU (include/ptc.h: ptc_probes_begin, ptc_probes_read_sh, ptc_render_probes, ptc_sh9_eval, ptc_sh9_irradiance and the three
ptc_debug_probe_* hooks): symbols, the host evaluation of csrc/pt_probes.h against its numpy restatement (tests/probes_reference.py) bit for bit, the
statistics the definition promises (uniform directions, an orthonormal basis), the closed forms of the irradiance, and the validation table.

The PTC_E_STATE refusals of a probe frame need a probe frame, and a probe frame needs a device: tests/test_gpu_probes.py holds them.  Here every call that
would render validates its arguments first (PTC_E_ARG) and then fails with PTC_E_DEVICE, as rendering does on a description-only context."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probes_reference as ref  # noqa: E402

NEW = ("ptc_probes_begin", "ptc_probes_read_sh", "ptc_render_probes", "ptc_sh9_eval", "ptc_sh9_irradiance", "ptc_debug_probe_rays", "ptc_debug_probe_project",
       "ptc_debug_probe_resolve")
E_ARG, E_STATE, E_DEVICE = -1, -2, -3
F32, F64 = np.float32, np.float64
SEEDS = (0, 1, 0xFFFFFFFF, 1 << 32, 0x1234567890ABCDEF)      # both halves of the seed reach the hash
FP = C.POINTER(C.c_float)


def _fp(a):
    return a.ctypes.data_as(FP)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ctx(pbr):
    return pbr.PathTracer(pbr.ptc.DEVICE_NONE)


def _positions(n, seed=3):
    return np.random.default_rng(seed).uniform(-2, 2, (n, 3)).astype(F32)


def test_symbols_and_abi(pbr):
    header = open(os.path.join(ROOT, "include", "ptc.h")).read()
    L = pbr.load_library()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in pbr.ptc.ABI_SYMBOLS and hasattr(L, sym) and getattr(L, sym).argtypes is not None, sym
    assert "#define PTC_ABI_VERSION 4" in header and L.ptc_abi_version() == 4            # additive: the ABI version stays
    for m in ("render_probes", "probes_begin", "read_probes_sh", "debug_probe_rays", "debug_probe_project"):
        assert callable(getattr(pbr.PathTracer, m)), m
    assert callable(pbr.ptc.sh9_eval) and callable(pbr.ptc.sh9_irradiance)


@pytest.mark.parametrize("n", [1, 63, 65])
def test_probe_rays_equal_reference_bit_for_bit(pbr, n):
    pt = _ctx(pbr)
    P = _positions(n)
    for seed in SEEDS:
        for base in (0, 1000):
            for first, ns in ((0, 1), (3, 5), (0xFFFFFFF0, 4)):
                o, d, key = pt.debug_probe_rays(P, seed, first, ns, index_base=base)
                ro, rd, rkey = ref.probe_rays(P, base, seed, first, ns)
                assert o.shape == (ns * n, 3) and o.dtype == F32 and key.dtype == np.uint32
                assert _same_bits(o, ro) and _same_bits(d, rd) and np.array_equal(key, rkey), (seed, base, first, ns)
    # the index base is a shift of the probe index: probe j of base b is probe 0 of base b + j
    _, d, key = pt.debug_probe_rays(P, 7, 2, 3, index_base=1000)
    for j in (0, n - 1):
        _, dj, kj = pt.debug_probe_rays(P[j:j + 1], 7, 2, 3, index_base=1000 + j)
        assert _same_bits(d[j::n], dj) and np.array_equal(key[j::n], kj)


def _lpath(rng, n_paths):
    """Random radiance with what a sum must survive: zeros, negatives, denormals, large values; alpha is never read."""
    L = rng.normal(0, 3, (n_paths, 4)).astype(F32)
    kind = ((np.arange(n_paths) + int(rng.integers(0, 4))) % 4)[:, None]      # every kind in any four paths in a row
    L = np.where(kind == 0, F32(0), L)
    L = np.where(kind == 1, (L * F32(1e-41)).astype(F32), L)      # denormals
    L = np.where(kind == 2, L * F32(1e6), L)
    L[:, 3] = np.nan
    return np.ascontiguousarray(L, F32)


@pytest.mark.parametrize("n", [1, 63, 65])
def test_projection_and_resolve_equal_reference_bit_for_bit(pbr, n):
    pt = _ctx(pbr)
    rng = np.random.default_rng(n)
    for seed, base, first, ns in ((0x1234567890ABCDEF, 0, 0, 7), (1, 1000, 5, 3)):
        L = _lpath(rng, n * ns)
        assert (np.abs(L[:, :3]) < 1.1754944e-38).any() and (L[:, :3] < 0).any() and (L[:, :3] == 0).any()
        acc = pt.debug_probe_project(n, seed, first, ns, L, index_base=base)
        want = ref.project(n, base, seed, first, ns, L)
        assert acc.shape == (n, 9, 3) and _same_bits(acc, want), (seed, base)
        # accumulation continues: a second batch on top of the first is the whole range in one go
        L2 = _lpath(rng, n * 2)
        acc2 = pt.debug_probe_project(n, seed, first + ns, 2, L2, acc=acc, index_base=base)
        assert _same_bits(acc2, ref.project(n, base, seed, first, ns + 2, np.concatenate([L, L2])))
        for N in (1, 3, ns + 2, 4096, 65535):
            assert _same_bits(pbr.ptc.probe_resolve(acc2, N), ref.resolve(acc2, N)), N


def test_directions_are_uniform_and_the_basis_is_orthonormal(pbr):
    """65,536 probe directions (256 probes x 256 samples) from ptc_debug_probe_rays, the basis from ptc_sh9_eval with unit coefficients.  mean(d) = 0,
    mean(d_c^2) = 1/3, 4 pi mean(b_i b_j) = delta_ij, each within 5 standard errors computed in float64 from the sample itself; | |d| - 1 | <= 2^-22."""
    n, ns = 256, 256
    _, d32, _ = _ctx(pbr).debug_probe_rays(np.zeros((n, 3), F32), 0x1234567890ABCDEF, 0, ns)
    d = d32.astype(F64)
    N = d.shape[0]
    assert N == 65536
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 2.0 ** -22
    for c in range(3):
        for v, want in ((d[:, c], 0.0), (d[:, c] ** 2, 1.0 / 3.0)):
            se = v.std(ddof=1) / math.sqrt(N)
            assert abs(v.mean() - want) <= 5 * se, (c, want, v.mean(), se)
    unit = np.zeros((9, 9, 3), F32)
    unit[np.arange(9), np.arange(9), 0] = 1                                # set k: coefficient k is 1 in the red channel, so sh9_eval returns b_k there
    b = np.stack([pbr.ptc.sh9_eval(unit[k], d32)[:, 0] for k in range(9)], -1).astype(F64)
    worst = 0.0
    for i in range(9):
        for j in range(i, 9):
            v = 4 * math.pi * b[:, i] * b[:, j]
            se = v.std(ddof=1) / math.sqrt(N)
            want = 1.0 if i == j else 0.0
            # b_0 b_0 is a constant: its standard error is 0 (up to the rounding of the mean) and the float32 constant 0.2820948 carries the whole
            # difference, 2 x 1e-7 relative at most; every other pair is held to 5 standard errors
            tol = 5 * se + (1e-6 if i == j == 0 else 0.0)
            worst = max(worst, abs(v.mean() - want) / tol)
            assert abs(v.mean() - want) <= tol, (i, j, v.mean(), se)
    print(f"largest |4 pi mean(b_i b_j) - delta_ij| in units of its tolerance: {worst:.2f}")
    # the float32 basis is the float64 basis with exact constants to float32 accuracy
    assert np.abs(b - ref.basis64(d)).max() <= 4e-7


def test_irradiance_closed_forms(pbr):
    """float32 constants against float64 closed forms: 1e-6 relative (to pi L where the expected value is 0)."""
    pi = math.pi
    Lr = np.array([1.0, 0.37, 12.5])
    normals = np.array([(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1), (0.6, 0.0, 0.8), (1 / math.sqrt(3),) * 3], F64)
    # constant radiance L: only coef_0 = 2 sqrt(pi) L; E = pi L for any normal
    sh = np.zeros((9, 3), F64)
    sh[0] = 2 * math.sqrt(pi) * Lr
    E = pbr.ptc.sh9_irradiance(sh.astype(F32), normals.astype(F32)).astype(F64)
    assert E.shape == (8, 3) and np.abs(E - pi * Lr).max() <= 1e-6 * pi * Lr.max() and (np.abs(E / (pi * Lr) - 1) <= 1e-6).all()
    # radiance L for y > 0, else 0: coef_0 = sqrt(pi) L, coef_1 = 0.4886025 pi L (= sqrt(3 pi) L / 2), the rest 0 in bands 0..1; band 2 vanishes
    sh = np.zeros((9, 3), F64)
    sh[0] = math.sqrt(pi) * Lr
    sh[1] = 0.5 * math.sqrt(3 * pi) * Lr
    assert abs(0.5 * math.sqrt(3 * pi) / (0.4886025 * pi) - 1) < 1e-7
    E = pbr.ptc.sh9_irradiance(sh.astype(F32), normals[:6].astype(F32)).astype(F64)
    want = np.array([1.0, 0.0, 0.5, 0.5, 0.5, 0.5])[:, None] * pi * Lr
    assert (np.abs(E - want) <= 1e-6 * pi * Lr).all(), (E, want)
    # and the wrapper is the restatement bit for bit, broadcasting included
    rng = np.random.default_rng(2)
    shr = rng.normal(0, 1, (5, 9, 3)).astype(F32)
    nr = rng.normal(0, 1, (5, 3))
    nr = (nr / np.linalg.norm(nr, axis=1)[:, None]).astype(F32)
    assert _same_bits(pbr.ptc.sh9_irradiance(shr, nr), ref.sh9_irradiance(shr, nr))
    assert _same_bits(pbr.ptc.sh9_irradiance(shr[0], nr), ref.sh9_irradiance(shr[0], nr))


def test_sh9_eval_against_the_basis(pbr):
    rng = np.random.default_rng(4)
    d = rng.normal(0, 1, (64, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F32)
    sh = rng.normal(0, 1, (64, 9, 3)).astype(F32)
    got = pbr.ptc.sh9_eval(sh, d)
    assert got.shape == (64, 3) and got.dtype == F32 and _same_bits(got, ref.sh9_eval(sh, d))
    exact = np.einsum("nkc,nk->nc", sh.astype(F64), ref.basis64(d))
    assert np.abs(got - exact).max() <= 3e-6
    for k in range(9):      # a single unit coefficient evaluates to that basis function
        one = np.zeros((9, 3), F32)
        one[k] = 1
        assert _same_bits(pbr.ptc.sh9_eval(one, d)[:, 0], ref.basis(d)[:, k]), k
    with pytest.raises(pbr.PtcError):
        pbr.ptc.sh9_eval(np.zeros((8, 3), F32), d)


def test_validation_and_device_errors(pbr):
    """Every PTC_E_ARG case; a valid call then fails with PTC_E_DEVICE on a description-only context; nothing of the context changes."""
    L = pbr.load_library()
    pt = _ctx(pbr).load_scene(pbr.scenes.cornell_box())
    before = (pt.get_camera_lens(), L.ptc_light_count(pt._h))
    P = _positions(4)
    out = np.zeros((4, 9, 3), F32)
    inf, nan = float("inf"), float("nan")
    begin = lambda pos, n, base, spp, mb: L.ptc_probes_begin(pt._h, pos, n, base, spp, 1, mb)
    assert begin(None, 4, 0, 8, 2) == E_ARG and b"probes_begin" in L.ptc_last_error(pt._h)
    assert begin(_fp(P), 0, 0, 8, 2) == E_ARG and begin(_fp(P), -1, 0, 8, 2) == E_ARG
    assert begin(_fp(P), 4, 0, 0, 2) == E_ARG and begin(_fp(P), 4, 0, 8, -1) == E_ARG
    assert begin(_fp(P), 4, 0xFFFFFFFD, 8, 2) == E_ARG                                    # probe indices beyond 32 bits
    for bad in (inf, -inf, nan):
        Q = P.copy()
        Q[3, 1] = bad
        assert begin(_fp(Q), 4, 0, 8, 2) == E_ARG, bad
        assert L.ptc_render_probes(pt._h, _fp(Q), 4, 8, 1, 2, _fp(out)) == E_ARG
    assert L.ptc_render_probes(pt._h, _fp(P), 4, 8, 1, 2, None) == E_ARG
    assert L.ptc_probes_begin(None, _fp(P), 4, 0, 8, 1, 2) == E_ARG and L.ptc_render_probes(None, _fp(P), 4, 8, 1, 2, _fp(out)) == E_ARG
    assert begin(_fp(P), 4, 0, 8, 2) == E_DEVICE                                          # validated, then: no device
    assert begin(_fp(P), 4, 0xFFFFFFFC, 8, 0) == E_DEVICE                                 # the last index is 2^32 - 1
    assert L.ptc_render_probes(pt._h, _fp(P), 4, 8, 1, 2, _fp(out)) == E_DEVICE
    assert L.ptc_probes_read_sh(pt._h, _fp(out)) == E_DEVICE and L.ptc_probes_read_sh(pt._h, None) == E_DEVICE and L.ptc_probes_read_sh(None, None) == E_ARG
    with pytest.raises(pbr.PtcError, match="ptc error -3"):
        pt.render_probes(P, 8)
    with pytest.raises(pbr.PtcError, match="ptc error -1"):
        pt.render_probes(P, 0)
    with pytest.raises(pbr.PtcError):
        pt.render_probes(np.zeros((4, 2), F32), 8)
    assert (pt.get_camera_lens(), L.ptc_light_count(pt._h)) == before
    # the pure functions and the hooks: NULL pointers and empty ranges
    v = np.zeros(27, F32)
    assert L.ptc_sh9_eval(None, _fp(v), _fp(v)) == E_ARG and L.ptc_sh9_eval(_fp(v), None, _fp(v)) == E_ARG and L.ptc_sh9_eval(_fp(v), _fp(v), None) == E_ARG
    assert L.ptc_sh9_irradiance(None, _fp(v), _fp(v)) == E_ARG and L.ptc_sh9_irradiance(_fp(v), _fp(v), None) == E_ARG
    assert L.ptc_debug_probe_resolve(None, 1, 1, _fp(v)) == E_ARG and L.ptc_debug_probe_resolve(_fp(v), 1, 0, _fp(v)) == E_ARG and L.ptc_debug_probe_resolve(_fp(v), 0, 1, _fp(v)) == E_ARG
    od, key = np.zeros((4, 6), F32), np.zeros(4, np.uint32)
    kp = key.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.ptc_debug_probe_rays(pt._h, None, 4, 0, 1, 0, 1, _fp(od), kp) == E_ARG and L.ptc_debug_probe_rays(pt._h, _fp(P), 4, 0, 1, 0, 0, _fp(od), kp) == E_ARG
    assert L.ptc_debug_probe_rays(pt._h, _fp(P), 0, 0, 1, 0, 1, _fp(od), kp) == E_ARG and L.ptc_debug_probe_rays(pt._h, _fp(P), 4, 0, 1, 0xFFFFFFFF, 2, _fp(od), kp) == E_ARG
    assert L.ptc_debug_probe_rays(pt._h, _fp(P), 4, 0, 1, 0, 1, None, kp) == E_ARG and L.ptc_debug_probe_rays(None, _fp(P), 4, 0, 1, 0, 1, _fp(od), kp) == E_ARG
    lp = np.zeros((4, 4), F32)
    assert L.ptc_debug_probe_project(pt._h, 4, 0, 1, 0, 1, None, _fp(out)) == E_ARG and L.ptc_debug_probe_project(pt._h, 4, 0, 1, 0, 1, _fp(lp), None) == E_ARG
    assert L.ptc_debug_probe_project(pt._h, 4, 0, 1, 0, 0, _fp(lp), _fp(out)) == E_ARG
    assert not out.any()                                                                  # no refused call wrote its output


def test_wrapper_shapes_and_dtypes(pbr):
    pt = _ctx(pbr)
    o, d, key = pt.debug_probe_rays([[0, 0, 0], [1, 2, 3]], 5, 0, 3)
    assert o.shape == d.shape == (6, 3) and o.dtype == d.dtype == F32 and key.shape == (6,) and key.dtype == np.uint32
    assert np.array_equal(o[:2], np.array([[0, 0, 0], [1, 2, 3]], F32)) and np.array_equal(o[:2], o[4:])
    acc = pt.debug_probe_project(2, 5, 0, 3, np.ones((6, 4), F32))
    assert acc.shape == (2, 9, 3) and acc.dtype == F32
    assert np.array_equal(acc[..., 0], acc[..., 1]) and np.array_equal(acc[..., 0], acc[..., 2])      # equal channels in, equal channels out
    c = pbr.ptc.probe_resolve(acc, 3)
    assert c.shape == (2, 9, 3) and c.dtype == F32
    E = pbr.ptc.sh9_irradiance(c, np.array([0, 1, 0], F32))
    assert E.shape == (2, 3) and E.dtype == F32
    assert pbr.ptc.sh9_eval(c[0], np.array([0, 0, 1], F32)).shape == (3,)
    with pytest.raises(pbr.PtcError):
        pt.debug_probe_project(2, 5, 0, 3, np.ones((5, 4), F32))


def test_cli_refuses_bad_probe_arguments_before_any_device_work(pbr):
    """ptc_render --probe-grid / --probes / --probes-out: exit code 1 and the reason, on a machine without a GPU too."""
    import subprocess

    exe = os.path.join(os.path.dirname(pbr.ptc.LIB_PATH), "ptc_render")
    for args, text in ((["--probe-grid", "2,2,2"], "--probes-out"), (["--probes-out", "x.pfm"], "either --probe-grid"),
                       (["--probe-grid", "2,0,2", "--probes-out", "x.pfm"], "three counts"), (["--probe-grid", "2,2,2", "--probes", "p.txt", "--probes-out", "x.pfm"], "either --probe-grid"),
                       (["--probe-grid", "2,2,2", "--probes-out", "x.pfm", "--raster"], "path integrator"), (["--probe-grid", "2,2,2", "--probes-out", "x.pfm", "--spp", "0"], "--spp"),
                       (["--probes", "/nonexistent/p.txt", "--probes-out", "x.pfm"], "cannot read")):
        r = subprocess.run([exe, "--scene", "cornell"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and text in r.stderr and "ptc_create" not in r.stderr, (args, r.stderr)
