"""numpy evaluation of the denoiser's specification (DESIGN.md "Denoiser") and a float32 mirror of the guide rays, for tests/test_gpu_denoise.py.

`atrous(...)` is the specification written out tap by tap, in float64 or float32 (`dt`): the library's result is held against the float64 evaluation,
with the float32-float64 gap of this same code as the yardstick.  `guide_dirs(...)` repeats the camera basis of ptc_make_camera and the pixel-centre
ray of k_raygen_guides operation by operation in float32 (a fused multiply-add = the exact product and sum in float64, rounded once)."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
B3 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
G3 = np.array([1 / 4, 1 / 2, 1 / 4])
LUM = np.array([0.2126, 0.7152, 0.0722])
EPS_A, EPS_L = 1e-3, 1e-6


def _fma(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def _dot(a, b):
    return _fma(a[..., 2], b[..., 2], _fma(a[..., 1], b[..., 1], (a[..., 0] * b[..., 0]).astype(F32)))


def _cross(a, b):
    return np.stack([_fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), _fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     _fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1).astype(F32)


def _normalize(a):
    inv = (F32(1.0) / np.sqrt(_dot(a, a))).astype(F32)
    return (a * inv[..., None]).astype(F32)


def camera_basis(cam):
    """(pos, f, s, u, sx, sy) in float32, as ptc_make_camera builds them."""
    pos, tgt = np.asarray(cam.position, F32), np.asarray(cam.target, F32)
    f = _normalize((tgt - pos).astype(F32))
    s = _normalize(_cross(f, np.array([0.0, -1.0, 0.0], F32)))
    u = _cross(s, f)
    sy = F32(math.tan(float(F32(cam.fov_y)) * 0.5))
    sx = F32(F32(cam.aspect) * sy)
    return pos, f, s, u, sx, sy


def guide_dirs(cam, w, h):
    """(h, w, 3) float32 unit directions of the pixel-centre rays and the camera position."""
    pos, f, s, u, sx, sy = camera_basis(cam)
    px, py = np.meshgrid(np.arange(w, dtype=F32), np.arange(h, dtype=F32))
    fx, fy = ((px + F32(0.5)) / F32(w)).astype(F32), ((py + F32(0.5)) / F32(h)).astype(F32)
    dvx, dvy = ((F32(2.0) * fx - F32(1.0)) * sx).astype(F32), ((F32(2.0) * fy - F32(1.0)) * sy).astype(F32)
    inner = np.stack([_fma(u[k], dvy, f[k]) for k in range(3)], -1)
    v = np.stack([_fma(s[k], dvx, inner[..., k]) for k in range(3)], -1)
    return _normalize(v), pos


def _shift(a, dy, dx, fill=0.0):
    """out[y, x] = a[y + dy, x + dx], `fill` outside the image."""
    out = np.full_like(a, fill)
    h, w = a.shape[:2]
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def atrous(col, albedo_class, normal_depth, dirs, cam_pos, fov_y, iterations, sigma_l, sigma_n, sigma_p, demodulate, dt=F64):
    """The specified filter.  col: (h, w, 3) radiance; albedo_class / normal_depth: the guides as ptc_read_guide_rgba32f returns them; dirs, cam_pos:
    guide_dirs().  Returns the (h, w, 3) result in `dt` (iterations = 0 is the library's business: a copy)."""
    H, W = col.shape[:2]
    K = albedo_class[..., 3].astype(dt)
    surf = albedo_class[..., 3] == 1
    n_, Z = normal_depth[..., :3].astype(dt), normal_depth[..., 3].astype(dt)
    P = cam_pos.astype(dt) + Z[..., None] * dirs.astype(dt)
    pix = dt(2.0 * math.tan(fov_y / 2) / H)
    lum, one = LUM.astype(dt), np.ones((H, W), dt)
    Ad = np.maximum(albedo_class[..., :3].astype(dt), dt(EPS_A)) if demodulate else np.ones((H, W, 3), dt)
    cur = col.astype(dt) / Ad
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
    var = np.where(surf, np.maximum(m2 / cnt - (m1 / cnt) ** 2, 0), 0).astype(dt)
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
                den = dt(sigma_p) * Z * pix * dt(st * math.hypot(dx, dy))
                wp = np.exp(-dist / np.where(den > 0, den, 1)) if (dx or dy) else one
                wl = np.exp(-np.abs(_shift(L, oy, ox) - L) / (dt(sigma_l) * sd + dt(EPS_L)))
                w = dt(B3[dy + 2] * B3[dx + 2]) * same * wn * wp * wl
                acc += w[..., None] * _shift(cur, oy, ox)
                vacc += w * w * _shift(var, oy, ox)
                wsum += w
        ws = np.where(surf, wsum, 1)
        cur = np.where(surf[..., None], acc / ws[..., None], cur)
        var = np.where(surf, vacc / (ws * ws), var)
    return cur * Ad
