"""numpy restatement of the thin-lens camera (csrc/pt_lens.h), for tests/test_lens_host.py and tests/test_gpu_lens.py.

Everything is float32 in the order the header writes it (numpy's + - * / sqrt on float32 arrays are correctly rounded); `dt=F64` evaluates the same
expressions in float64 — the yardstick of the geometry tests is the gap between the two.

A fused multiply-add is the exact product and sum rounded ONCE.  The product of two float32 is exact in float64, the sum is not always: rounding it to
float64 and then to float32 can differ from the single rounding when the float64 sum lands on a float32 tie.  `_fma` therefore rounds the float64 sum to
odd (TwoSum gives its error exactly) before the final rounding, which is the single rounding for every input (53 >= 2 * 24 + 2 bits)."""
import numpy as np

from denoise_reference import camera_basis  # noqa: F401  (pos, f, s, u, sx, sy) in float32, as ptc_make_camera builds them

F32, F64 = np.float32, np.float64
U64 = np.uint64
_M = U64(0xFFFFFFFF)
HALF_PI = F32(1.57079632679489661923)


def _fma(a, b, c, dt=F32):
    if dt is F64:
        return np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)
    a, b, c = np.broadcast_arrays(np.asarray(a, F32).astype(F64), np.asarray(b, F32).astype(F64), np.asarray(c, F32).astype(F64))
    p = a * b
    s = np.ascontiguousarray(p + c)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    odd = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return odd.astype(F32)


def pcg(v):
    v = np.asarray(v, U64) & _M
    s = (v * U64(747796405) + U64(2891336453)) & _M
    w = (((s >> ((s >> U64(28)) + U64(4))) ^ s) * U64(277803737)) & _M
    return ((w >> U64(22)) ^ w) & _M


def seed_hash(seed):
    seed = int(seed)
    return pcg((U64(seed & 0xFFFFFFFF) + pcg(U64(seed >> 32))) & _M)


def path_key(sh, pixel, sample):
    return pcg((np.asarray(pixel, U64) + pcg((np.asarray(sample, U64) + sh) & _M)) & _M)


def rng_f(key, bounce, dim):
    x = pcg(pcg(U64(bounce * 8 + dim)) ^ np.asarray(key, U64))
    return (x >> U64(8)).astype(F32) * F32(1.0 / 16777216.0)


def sincos2pi(u, dt=F32):
    """(sin, cos) of 2 pi u by the polynomial of sincos2pi (csrc/pt_device.h)."""
    u = np.asarray(u, dt)
    x4 = u * dt(4.0)
    q = np.minimum(x4.astype(np.int32), 3)
    r = x4 - q.astype(dt)
    swap = r > dt(0.5)
    rr = np.where(swap, dt(1.0) - r, r)
    x = rr * dt(HALF_PI)
    x2 = x * x
    f = lambda a, b, c: _fma(a, b, c, dt)
    ps = f(x2, f(x2, f(x2, f(x2, dt(F32(2.7557319e-6)), dt(F32(-1.9841270e-4))), dt(F32(8.3333333e-3))), dt(F32(-1.6666667e-1))), dt(1.0))
    s = x * ps
    c = f(x2, f(x2, f(x2, f(x2, dt(F32(2.4801587e-5)), dt(F32(-1.3888889e-3))), dt(F32(4.1666667e-2))), dt(-0.5)), dt(1.0))
    s, c = np.where(swap, c, s), np.where(swap, s, c)
    S = np.select([q == 0, q == 1, q == 2], [s, c, -s], -c)
    C = np.select([q == 0, q == 1, q == 2], [c, -s, -c], s)
    return S.astype(dt), C.astype(dt)


def lens_point(R, blades, rotation, u1, u2, dt=F32):
    """(lx, ly) of pt_lens_point."""
    R, u1, u2 = dt(F32(R)), np.asarray(u1, F32).astype(dt), np.asarray(u2, F32).astype(dt)
    if blades == 0:
        r = np.sqrt(u1)
        sn, co = sincos2pi(u2, dt)
        rr = R * r
        return rr * co, rr * sn
    n = int(blades)
    x = u1 * dt(n)
    k = np.minimum(x.astype(np.int32), n - 1)
    a = x - k.astype(dt)
    su = np.sqrt(a)
    rot = dt(F32(rotation))
    t0 = rot + k.astype(dt) / dt(n)
    t0 = t0 - np.floor(t0)
    t1 = rot + (k + 1).astype(dt) / dt(n)
    t1 = t1 - np.floor(t1)
    s0, c0 = sincos2pi(t0, dt)
    s1, c1 = sincos2pi(t1, dt)
    b0, b1 = su * (dt(1.0) - u2), su * u2
    px, py = _fma(b1, c1, b0 * c0, dt), _fma(b1, s1, b0 * s0, dt)
    return R * px, R * py


def lens_ray(basis, lens, dvx, dvy, u1, u2, dt=F32):
    """(o, d) of the ray part of pt_lens_ray for view-space slopes (dvx, dvy) and the lens pair (u1, u2); lens = (R, F, blades, rotation).
    The basis is an input: its float32 values are used as they are in either precision."""
    pos, f, s, u, _, _ = basis
    R, F, blades, rotation = lens
    dvx, dvy = np.asarray(dvx, dt), np.asarray(dvy, dt)
    fm = lambda a, b, c: _fma(a, b, c, dt)
    if F32(R) > 0:
        lx, ly = lens_point(R, blades, rotation, u1, u2, dt)
        Fd = dt(F32(F))
        qx, qy = fm(Fd, dvx, -lx), fm(Fd, dvy, -ly)
        o = np.stack([fm(dt(s[c]), lx, fm(dt(u[c]), ly, dt(pos[c]))) for c in range(3)], -1)
        v = np.stack([fm(dt(s[c]), qx, fm(dt(u[c]), qy, dt(f[c]) * Fd)) for c in range(3)], -1)
    else:
        v = np.stack([fm(dt(s[c]), dvx, fm(dt(u[c]), dvy, dt(f[c]))) for c in range(3)], -1)
        o = np.broadcast_to(np.asarray(pos, dt), v.shape).copy()
    inv = dt(1.0) / np.sqrt(fm(v[..., 2], v[..., 2], fm(v[..., 1], v[..., 1], v[..., 0] * v[..., 0])))
    return o.astype(dt), (v * inv[..., None]).astype(dt)


def slopes(basis, w, h, px, py, jx, jy, dt=F32):
    """(dvx, dvy) of k_raygen for pixel (px, py) and the jitter (jx, jy)."""
    sx, sy = basis[4], basis[5]
    fx = (np.asarray(px, dt) + np.asarray(jx, dt)) / dt(w)
    fy = (np.asarray(py, dt) + np.asarray(jy, dt)) / dt(h)
    return (dt(2.0) * fx - dt(1.0)) * dt(sx), (dt(2.0) * fy - dt(1.0)) * dt(sy)


def camera_rays(basis, lens, w, h, seed, first_sample, n_samples, pixels, dt=F32):
    """ptc_debug_camera_rays: (origins, dirs, keys) of n_samples * n_pixels rays in path order p = sample_local * n_pixels + j."""
    pixels = np.asarray(pixels, U64).reshape(-1)
    pix = np.tile(pixels, n_samples)
    smp = np.repeat(np.arange(n_samples, dtype=U64) + U64(first_sample), pixels.size)
    key = path_key(seed_hash(seed), pix, smp)
    jx, jy = rng_f(key, 0, 0), rng_f(key, 0, 1)
    dvx, dvy = slopes(basis, w, h, (pix % U64(w)).astype(F32), (pix // U64(w)).astype(F32), jx, jy, dt)
    o, d = lens_ray(basis, lens, dvx, dvy, rng_f(key, 0, 2), rng_f(key, 0, 3), dt)
    return o, d, key.astype(np.uint32)


def focus_distance(basis, w, h, px, py, Z):
    """ptc_focus_distance_at_pixel from the depth guide Z of pixel (px, py)."""
    dvx, dvy = slopes(basis, w, h, F32(px), F32(py), F32(0.5), F32(0.5))
    return (np.asarray(Z, F32) / np.sqrt(_fma(dvy, dvy, _fma(dvx, dvx, F32(1.0))))).astype(F32)
