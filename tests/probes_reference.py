"""numpy restatement of the light probes (csrc/pt_probes.h), for tests/test_probes_host.py and tests/test_gpu_probes.py.

Everything is float32 in the order the header writes it (numpy's + - * / sqrt on float32 arrays are correctly rounded; `_fma` of lens_reference.py is the
single rounding).  pcg, seed_hash, path_key, rng_f and sincos2pi are lens_reference.py's: the header calls csrc/pt_device.h's, as the lens does."""
import numpy as np

from lens_reference import F32, F64, U64, _fma, path_key, rng_f, seed_hash, sincos2pi  # noqa: F401

FOUR_PI = F32(12.566371)
# the nine constants of the basis, as the header spells them
C0, C1, C2, C6A, C6B, C8 = F32(0.2820948), F32(0.4886025), F32(1.0925484), F32(0.9461747), F32(-0.3153916), F32(0.5462742)
BAND_A = np.array([3.1415927] + [2.0943952] * 3 + [0.7853982] * 5, F32)      # A_l per coefficient: pi, 2 pi / 3, pi / 4


def probe_dirs(seed, idx, sample):
    """(d (.., 3), key) of pt_probe_dir for the probe indices idx (= base + j) and the samples `sample` (broadcast)."""
    key = path_key(seed_hash(seed), np.asarray(idx, U64), np.asarray(sample, U64))
    u1, u2 = rng_f(key, 0, 0), rng_f(key, 0, 1)
    z = _fma(F32(-2.0), u1, F32(1.0))
    r = np.sqrt(np.maximum(_fma(-z, z, F32(1.0)), F32(0.0)))
    sn, co = sincos2pi(u2)
    vx, vy, vz = r * co, r * sn, z
    inv = F32(1.0) / np.sqrt(_fma(vz, vz, _fma(vy, vy, vx * vx)))
    return np.stack([vx * inv, vy * inv, vz * inv], -1).astype(F32), key.astype(np.uint32)


def probe_rays(positions, base, seed, first_sample, n_samples):
    """ptc_debug_probe_rays: (origins, dirs, keys) of n_samples * n rays in path order p = sample_local * n + j."""
    P = np.asarray(positions, F32).reshape(-1, 3)
    n = P.shape[0]
    idx = np.tile(np.arange(n, dtype=U64) + U64(base), n_samples)
    smp = np.repeat(np.arange(n_samples, dtype=U64) + U64(first_sample), n)
    d, key = probe_dirs(seed, idx, smp)
    return np.tile(P, (n_samples, 1)), d, key


def basis(d):
    """(.., 9) float32: pt_sh9_basis for k = 0..8 at the directions d (.., 3)."""
    d = np.asarray(d, F32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.broadcast_to(C0, x.shape), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), _fma(C6A, z * z, C6B), C2 * (x * z), C8 * (x * x - y * y)], -1).astype(F32)


def project(n, base, seed, first_sample, n_samples, lpath, acc=None):
    """ptc_debug_probe_project / k_accumulate_sh: acc[j][k][c] = acc[j][k][c] + L_c * b_k, sample after sample; lpath (n_samples * n, >= 3) in path order."""
    L = np.asarray(lpath, F32).reshape(n_samples, n, -1)[..., :3]
    a = np.zeros((n, 9, 3), F32) if acc is None else np.array(acc, F32).reshape(n, 9, 3)
    idx = np.arange(n, dtype=U64) + U64(base)
    for s in range(n_samples):
        d, _ = probe_dirs(seed, idx, U64(first_sample + s))
        b = basis(d)                                          # (n, 9)
        a = a + (L[s][:, None, :] * b[:, :, None]).astype(F32)   # product, then sum: two roundings
    return a


def resolve(acc, n_samples):
    """coef = acc * (4 pi / (float)N): the scale is rounded once, then the product."""
    return (np.asarray(acc, F32) * (FOUR_PI / F32(n_samples))).astype(F32)


def sh9_eval(sh, d):
    """pt_sh9_eval: sum over k ascending of sh[k][c] * b_k(d), float32; sh (.., 9, 3), d (.., 3)."""
    sh, b = np.asarray(sh, F32), basis(d)
    o = np.zeros(np.broadcast_shapes(sh.shape[:-2], b.shape[:-1]) + (3,), F32)
    for k in range(9):
        o = o + sh[..., k, :] * b[..., k, None]
    return o


def sh9_irradiance(sh, n):
    """pt_sh9_irradiance: sum over k ascending of (A_k * sh[k][c]) * b_k(n), float32."""
    sh, b = np.asarray(sh, F32), basis(n)
    o = np.zeros(np.broadcast_shapes(sh.shape[:-2], b.shape[:-1]) + (3,), F32)
    for k in range(9):
        o = o + (BAND_A[k] * sh[..., k, :]) * b[..., k, None]
    return o


def basis64(d):
    """The real SH basis up to band 2 in float64 with exact constants (the yardstick of the closed-form tests)."""
    d = np.asarray(d, F64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    pi = np.pi
    c0, c1, c2, c6, c8 = 0.5 / np.sqrt(pi), np.sqrt(3 / (4 * pi)), 0.5 * np.sqrt(15 / pi), 0.25 * np.sqrt(5 / pi), 0.25 * np.sqrt(15 / pi)
    return np.stack([np.full(x.shape, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c6 * (3 * z * z - 1), c2 * x * z, c8 * (x * x - y * y)], -1)
