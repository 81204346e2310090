"""numpy restatement of the camera models (csrc/pt_camera.h, include/ptc_camera.h), for tests/test_camera_host.py and tests/test_gpu_camera.py.

Everything is float32 in the order the header writes it (numpy's + - * / sqrt on float32 arrays are correctly rounded; `_fma` of lens_reference.py is the
single rounding); `dt=F64` evaluates the same expressions in float64.  The RNG, the key and sincos2pi are lens_reference.py's, which restate pt_device.h."""
import math

import numpy as np

from lens_reference import F32, F64, U64, _fma, path_key, rng_f, seed_hash, sincos2pi  # noqa: F401

PERSPECTIVE, ORTHOGRAPHIC, EQUIRECT = 0, 1, 2
NAMES = {PERSPECTIVE: "perspective", ORTHOGRAPHIC: "orthographic", EQUIRECT: "equirect"}
PANORAMA_SEED = 7      # the seed of the panorama round trip (tests/test_gpu_camera.py); tests/test_camera_host.py holds its precondition


def _dot3(a, b, dt=F32):
    r = _fma(a[..., 2], b[..., 2], _fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0], dt), dt)
    return np.asarray(r).reshape(np.shape(a)[:-1])      # _fma makes a 0-d result 1-d


def _normalize3(a, dt=F32):
    inv = dt(1.0) / np.sqrt(_dot3(a, a, dt))
    return (a * np.asarray(inv)[..., None]).astype(dt)


def _cross3(a, b):
    return np.stack([_fma(a[1], b[2], -(a[2] * b[1])), _fma(a[2], b[0], -(a[0] * b[2])), _fma(a[0], b[1], -(a[1] * b[0]))]).astype(F32).reshape(3)


def matrix16(matrix):
    """The 16 column-major float32 entries of a 4x4 (mathematical) matrix."""
    return np.ascontiguousarray(np.asarray(matrix, F32).T).reshape(16)


def basis(matrix, yfov=math.pi / 2, aspect=1.0, projection=PERSPECTIVE):
    """(pos, f, s, u, sx, sy) in float32 as ptc_set_camera_ex fills DevCamera from a 4x4 camera-to-world matrix: X, Y, Z = the normalised columns,
    s = X, u = -Y, f = -Z; sy = (float)tan((double)yfov / 2), sx = aspect sy under PERSPECTIVE, 1 otherwise."""
    m = matrix16(matrix)
    X, Y, Z = (_normalize3(m[4 * k:4 * k + 3]) for k in range(3))
    if projection == PERSPECTIVE:
        sy = F32(math.tan(float(F32(yfov)) * 0.5))
        sx = F32(F32(aspect) * sy)
    else:
        sx = sy = F32(1.0)
    return m[12:15].copy(), (-Z).astype(F32), X, (-Y).astype(F32), sx, sy


def accepted(matrix):
    """The validation of ptc_set_camera_ex's matrix: finite, no zero column, pairwise |dot| of the normalised columns <= 1e-4, right-handed."""
    m = matrix16(matrix)
    if not np.isfinite(m).all():
        return False
    cols = [m[4 * k:4 * k + 3] for k in range(3)]
    if any(not (_dot3(c, c) > 0) for c in cols):
        return False
    X, Y, Z = (_normalize3(c) for c in cols)
    if not all(np.isfinite(v).all() for v in (X, Y, Z)):
        return False
    if max(abs(_dot3(X, Y)), abs(_dot3(X, Z)), abs(_dot3(Y, Z))) > F32(1e-4):
        return False
    return bool(_dot3(_cross3(X, Y), Z) > 0)


def point(bas, projection, xmag, ymag, fx, fy, dt=F32):
    """(o, d) of pt_proj_point for the image point (fx, fy) in [0, 1)^2: ORTHOGRAPHIC or EQUIRECT.  The basis is an input: its float32 values are used as
    they are in either precision."""
    pos, f, s, u, _, _ = bas
    fx, fy = np.asarray(fx, dt), np.asarray(fy, dt)
    fm = lambda a, b, c: _fma(a, b, c, dt)
    if projection == ORTHOGRAPHIC:
        ox = (dt(2.0) * fx - dt(1.0)) * dt(F32(xmag))
        oy = (dt(2.0) * fy - dt(1.0)) * dt(F32(ymag))
        o = np.stack([fm(dt(s[c]), ox, fm(dt(u[c]), oy, dt(pos[c]))) for c in range(3)], -1)
        d = np.broadcast_to(np.asarray(f, dt), o.shape).copy()
        return o.astype(dt), d
    assert projection == EQUIRECT
    t = fx + dt(0.5)
    t = t - np.floor(t)
    sp, cp = sincos2pi(t, dt)
    st, ct = sincos2pi(dt(0.5) * fy, dt)
    X, Y, Z = s, -u, -f
    a, b = st * cp, st * sp
    v = np.stack([fm(dt(X[c]), a, fm(dt(Y[c]), ct, dt(Z[c]) * b)) for c in range(3)], -1).astype(dt)
    d = _normalize3(v, dt)
    o = np.broadcast_to(np.asarray(pos, dt), d.shape).copy()
    return o, d


def image_point(w, h, px, py, jx, jy, dt=F32):
    """(fx, fy) of k_raygen for pixel (px, py) and the jitter (jx, jy)."""
    return (np.asarray(px, dt) + np.asarray(jx, dt)) / dt(w), (np.asarray(py, dt) + np.asarray(jy, dt)) / dt(h)


def camera_rays(bas, projection, xmag, ymag, w, h, seed, first_sample, n_samples, pixels, dt=F32):
    """ptc_debug_camera_rays under ORTHOGRAPHIC / EQUIRECT: (origins, dirs, keys) of n_samples * n_pixels rays in the order p = sample_local * n_pixels + j."""
    pixels = np.asarray(pixels, U64).reshape(-1)
    pix = np.tile(pixels, n_samples)
    smp = np.repeat(np.arange(n_samples, dtype=U64) + U64(first_sample), pixels.size)
    key = path_key(seed_hash(seed), pix, smp)
    fx, fy = image_point(w, h, (pix % U64(w)).astype(F32), (pix // U64(w)).astype(F32), rng_f(key, 0, 0), rng_f(key, 0, 1), dt)
    o, d = point(bas, projection, xmag, ymag, fx, fy, dt)
    return o, d, key.astype(np.uint32)


def guide_rays(bas, projection, xmag, ymag, w, h):
    """The pixel-centre rays of ptc_frame_guides, (h, w, 3) origins and directions: the jitter is (0.5, 0.5)."""
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = image_point(w, h, xs.astype(F32), ys.astype(F32), F32(0.5), F32(0.5))
    return point(bas, projection, xmag, ymag, fx, fy)


def guide_positions(o, d, Z):
    """pos_class.xyz of k_guides_pos_proj: o + Z d, a product and a sum per component."""
    return (o + (np.asarray(Z, F32)[..., None] * d).astype(F32)).astype(F32)


def env_uv(d):
    """Float64 restatement of the environment lookup's mapping of ptc_set_env_latlong_rgb32f: a unit direction -> (u, v) in [0, 1]^2, row 0 = +y,
    u = atan2(d.z, d.x) / 2 pi + 1/2, v = acos(d.y) / pi."""
    d = np.asarray(d, F64)
    u = np.arctan2(d[..., 2], d[..., 0]) / (2 * np.pi) + 0.5
    v = np.arccos(np.clip(d[..., 1], -1.0, 1.0)) / np.pi
    return u, v


def atrous(col, albedo_class, normal_depth, P, pix, flat, iterations, sigma_l, sigma_n, sigma_p, demodulate, dt=F64, D=None, var_n=None, n=None):
    """The denoiser's specification (denoise_reference.atrous, tap by tap) with the two things a projection decides handed in: P, the (h, w, 3) position of
    every pixel's first hit (origin + Z direction of its own guide ray), and the footprint — `pix` the world size of a pixel, at unit distance (flat False:
    the plane-distance weight divides by sigma_p Z pix) or at every depth (flat True: by sigma_p pix).  tests/test_camera_host.py holds it to
    denoise_reference.atrous on a perspective input.
    D, var_n, n: the form of ptc_denoise_sampled / ptc_denoise_accumulated (temporal_reference.denoise_accumulated): D (h, w, 3) is the demodulated input, and
    where n >= 4 the variance is var_n instead of the 7x7 estimate; pixels of the other classes show `col`."""
    from denoise_reference import B3, EPS_A, EPS_L, G3, LUM, _shift

    H, W = col.shape[:2]
    K = albedo_class[..., 3].astype(dt)
    surf = albedo_class[..., 3] == 1
    n_, Z = normal_depth[..., :3].astype(dt), normal_depth[..., 3].astype(dt)
    P = np.asarray(P).astype(dt)
    pix = dt(pix)
    lum, one = LUM.astype(dt), np.ones((H, W), dt)
    Ad = np.maximum(albedo_class[..., :3].astype(dt), dt(EPS_A)) if demodulate else np.ones((H, W, 3), dt)
    cur = col.astype(dt) / Ad if D is None else np.asarray(D)[..., :3].astype(dt)
    L = (cur * lum).sum(-1)
    m1, m2, cnt = (np.zeros((H, W), dt) for _ in range(3))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            g = _shift(one, dy, dx) * (_shift(K, dy, dx, -1.0) == K) * np.maximum((n_ * _shift(n_, dy, dx)).sum(-1), 0) ** dt(sigma_n)
            q = _shift(L, dy, dx)
            m1 += g * q
            m2 += g * q * q
            cnt += g
    cnt = np.where(surf, cnt, 1)
    spatial = np.maximum(m2 / cnt - (m1 / cnt) ** 2, 0)
    if D is not None:
        spatial = np.where(np.asarray(n) >= 4, np.asarray(var_n).astype(dt), spatial)
    var = np.where(surf, spatial, 0).astype(dt)
    for i in range(iterations):
        st = 1 << i
        gv, gw = np.zeros((H, W), dt), np.zeros((H, W), dt)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = dt(G3[dy + 1] * G3[dx + 1]) * _shift(one, dy, dx)
                gv += k * _shift(var, dy, dx)
                gw += k
        sd = np.sqrt(np.maximum(gv / gw, 0))
        L = (cur * lum).sum(-1)
        acc, vacc, wsum = np.zeros_like(cur), np.zeros((H, W), dt), np.zeros((H, W), dt)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * st, dx * st
                same = _shift(one, oy, ox) * (_shift(K, oy, ox, -1.0) == K)
                wn = np.maximum((n_ * _shift(n_, oy, ox)).sum(-1), 0) ** dt(sigma_n)
                dist = np.abs((n_ * (_shift(P, oy, ox) - P)).sum(-1))
                den = (dt(sigma_p) * pix if flat else dt(sigma_p) * Z * pix) * dt(st * math.hypot(dx, dy))
                den = np.broadcast_to(den, (H, W))
                wp = np.exp(-dist / np.where(den > 0, den, 1)) if (dx or dy) else one
                wl = np.exp(-np.abs(_shift(L, oy, ox) - L) / (dt(sigma_l) * sd + dt(EPS_L)))
                w = dt(B3[dy + 2] * B3[dx + 2]) * same * wn * wp * wl
                acc += w[..., None] * _shift(cur, oy, ox)
                vacc += w * w * _shift(var, oy, ox)
                wsum += w
        ws = np.where(surf, wsum, 1)
        cur = np.where(surf[..., None], acc / ws[..., None], cur)
        var = np.where(surf, vacc / (ws * ws), var)
    return cur * Ad if D is None else np.where(surf[..., None], cur * Ad, col.astype(dt))


def footprint(projection, h, yfov=None, ymag=None):
    """(pix, flat) of the denoiser's plane-distance weight (pt_proj_footprint)."""
    if projection == ORTHOGRAPHIC:
        return F32(F32(2.0) * F32(ymag)) / F32(h), True
    if projection == EQUIRECT:
        return F32(3.14159265358979323846) / F32(h), False
    return F32(F32(2.0) * F32(math.tan(float(F32(yfov)) * 0.5))) / F32(h), False
