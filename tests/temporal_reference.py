"""numpy evaluation of the temporal accumulation's specification, for tests/test_temporal_host.py and tests/test_gpu_temporal.py.

`accumulate(...)` is steps 1-6 written out tap by tap, in float64 or float32 (`dt`).  Every step is evaluated from the PREVIOUS STATE it is handed (`prev`):
the history and moments as the library itself left them, the guides the caller read one frame earlier, that frame's camera and primitive positions — so
reference and library never drift apart over a sequence.  P' is rebuilt as pos' + Z' dirs' in `dt`.  `temporal_variance(...)` is the variance rule of
ptc_denoise_accumulated.

The discrete decisions of the specification (which history taps are valid, whether W reaches W_min) flip under rounding when they are close; such pixels
are returned as the FRAGILE mask and left out of tolerance comparisons: a candidate tap with |dist / threshold - 1| < 0.01, or |W - W_min| < 1e-3."""
import math

import numpy as np

from denoise_reference import B3, EPS_A, EPS_L, G3, LUM, _shift, camera_basis, guide_dirs

F32, F64 = np.float32, np.float64
W_MIN = 0.01
FRAGILE_TAP, FRAGILE_W = 0.01, 1e-3


def triangle_positions(verts, idx):
    """(n_tris, 3, 3) float32: the three world positions of every primitive, as the shading records hold them."""
    return np.ascontiguousarray(verts[:, :3][idx.astype(np.int64)], F32)


def previous_state(history, moments, normal_depth, albedo_class, camera, tri_pos):
    """What a step needs of the frame before it: the library's TEMPORAL_HISTORY and TEMPORAL_MOMENTS read-backs, that frame's guides, camera and positions."""
    return dict(history=history, moments=moments, nz=normal_depth, K=albedo_class[..., 3], camera=camera, tri_pos=tri_pos)


def reproject(prim, uv, surf, prev, w, h, dt=F64):
    """Steps 1-2: X (h, w, 3), x_prev, y_prev and `front` (class 1 and z > 0) from the previous positions and camera."""
    tri = prev["tri_pos"].astype(dt)
    pr = np.where(surf, prim, 0)
    u, v = uv[..., 0].astype(dt)[..., None], uv[..., 1].astype(dt)[..., None]
    X = (((dt(1) - u) - v) * tri[pr, 0] + u * tri[pr, 1]) + v * tri[pr, 2]
    pos, f, s, up, sx, sy = (np.asarray(t, dt) for t in camera_basis(prev["camera"]))
    d = X - pos
    z = (d * f).sum(-1)
    front = surf & (z > 0)
    zs = np.where(front, z, dt(1))
    xp = (((d * s).sum(-1) / zs) / sx + dt(1)) * dt(0.5) * dt(w) - dt(0.5)
    yp = (((d * up).sum(-1) / zs) / sy + dt(1)) * dt(0.5) * dt(h) - dt(0.5)
    return X, np.where(front, xp, dt(0)), np.where(front, yp, dt(0)), front


def accumulate(col, albedo_class, normal_depth, prim, uv, prev, max_history=32, sigma_z=1.0, demodulate=1, dt=F64):
    """One ptc_temporal_accumulate.  col: (h, w, 3) radiance; albedo_class, normal_depth, prim, uv: this frame's guides; prev: previous_state(...) or None.
    Returns a dict: history (h, w, 4) = (D_new, n_new), moments = (m1, m2, Var_t, a), motion = (x_prev, y_prev, W, reprojected n), accumulated (h, w, 3),
    fragile (h, w) bool, valid (h, w) bool (class 1 with W >= W_min)."""
    H_, W_ = albedo_class.shape[:2]
    surf = albedo_class[..., 3] == 1
    zero = np.zeros((H_, W_), dt)
    Hc, hn, h1, h2, Wsum, xp, yp = np.zeros((H_, W_, 3), dt), zero.copy(), zero.copy(), zero.copy(), zero.copy(), zero.copy(), zero.copy()
    fragile = np.zeros((H_, W_), bool)
    if prev is not None:
        X, xp, yp, front = reproject(prim, uv, surf, prev, W_, H_, dt)
        inside = front & (xp > -1) & (xp < W_) & (yp > -1) & (yp < H_)
        fx, fy = np.floor(np.where(inside, xp, 0)), np.floor(np.where(inside, yp, 0))
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        tx, ty = (xp - fx).astype(dt), (yp - fy).astype(dt)
        pos, f, s, up, sx, sy = (np.asarray(t, dt) for t in camera_basis(prev["camera"]))
        dirs_p, _ = guide_dirs(prev["camera"], W_, H_)
        Zp = prev["nz"][..., 3].astype(dt)
        Pp = pos + Zp[..., None] * dirs_p.astype(dt)
        Np = prev["nz"][..., :3].astype(dt)
        Dp, np_, m1p, m2p = prev["history"][..., :3].astype(dt), prev["history"][..., 3].astype(dt), prev["moments"][..., 0].astype(dt), prev["moments"][..., 1].astype(dt)
        pixp = dt(2) * sy / dt(H_)
        sD, sn, s1, s2 = np.zeros((H_, W_, 3), dt), zero.copy(), zero.copy(), zero.copy()
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                ok = inside & (qx >= 0) & (qx < W_) & (qy >= 0) & (qy < H_)
                qx, qy = np.clip(qx, 0, W_ - 1), np.clip(qy, 0, H_ - 1)
                cand = ok & (prev["K"][qy, qx] == 1) & (np_[qy, qx] > 0)
                dist = np.abs((Np[qy, qx] * (X - Pp[qy, qx])).sum(-1))
                thr = dt(sigma_z) * Zp[qy, qx] * pixp
                valid = cand & (dist <= thr)
                fragile |= cand & (np.abs(dist / np.where(thr > 0, thr, 1) - 1) < FRAGILE_TAP)
                b = np.where(valid, (tx if i else dt(1) - tx) * (ty if j else dt(1) - ty), dt(0)).astype(dt)
                Wsum += b
                sD += b[..., None] * Dp[qy, qx]
                sn += b * np_[qy, qx]
                s1 += b * m1p[qy, qx]
                s2 += b * m2p[qy, qx]
        fragile |= inside & (np.abs(Wsum - W_MIN) < FRAGILE_W)
        good = Wsum >= dt(W_MIN)
        Ws = np.where(good, Wsum, dt(1))
        Hc, hn, h1, h2 = np.where(good[..., None], sD / Ws[..., None], 0), np.where(good, sn / Ws, 0), np.where(good, s1 / Ws, 0), np.where(good, s2 / Ws, 0)
    A = np.maximum(albedo_class[..., :3].astype(dt), dt(EPS_A)) if demodulate else np.ones((H_, W_, 3), dt)
    D = col.astype(dt) / A
    L = (D * LUM.astype(dt)).sum(-1)
    n_new = np.minimum(hn + dt(1), dt(max_history))
    a = dt(1) / n_new
    D_new = (dt(1) - a)[..., None] * Hc + a[..., None] * D
    m1 = (dt(1) - a) * h1 + a * L
    m2 = (dt(1) - a) * h2 + a * (L * L)
    var = np.maximum(m2 - m1 * m1, 0)
    s3 = surf[..., None]
    history = np.where(s3, np.concatenate([D_new, n_new[..., None]], -1), np.concatenate([col.astype(dt), zero[..., None]], -1)).astype(dt)
    moments = np.where(s3, np.stack([m1, m2, var, a], -1), 0).astype(dt)
    motion = np.where(s3, np.stack([xp, yp, Wsum, hn], -1), 0).astype(dt)
    accumulated = np.where(s3, D_new * A, col.astype(dt)).astype(dt)
    return dict(history=history, moments=moments, motion=motion, accumulated=accumulated, fragile=fragile & surf, valid=surf & (Wsum >= dt(W_MIN)))


def temporal_variance(history, moments, spatial_variance):
    """The variance ptc_denoise_accumulated hands the filter: a Var_t, the variance of the accumulated mean, where n_new >= 4; elsewhere the 7x7 spatial
    estimate over lum(D_new) (`spatial_variance`: the denoiser's, evaluated on D_new without demodulation)."""
    return np.where(history[..., 3] >= 4, moments[..., 3] * moments[..., 2], spatial_variance)


def denoise_accumulated(history, moments, radiance, albedo_class, normal_depth, dirs, cam_pos, fov_y, iterations, sigma_l, sigma_n, sigma_p, demodulate, dt=F64):
    """ptc_denoise_accumulated: the denoiser's filter (as denoise_reference.atrous writes it out) with D_new = history[..., :3] as its demodulated
    input and temporal_variance(...) as its variance.  history, moments: the library's read-backs after the frame's accumulate; radiance: (h, w, 3), what the
    pixels of other classes show.  Returns (h, w, 3) in `dt` (iterations >= 1)."""
    H, W = albedo_class.shape[:2]
    K = albedo_class[..., 3].astype(dt)
    surf = albedo_class[..., 3] == 1
    n_, Z = normal_depth[..., :3].astype(dt), normal_depth[..., 3].astype(dt)
    P = cam_pos.astype(dt) + Z[..., None] * dirs.astype(dt)
    pix = dt(2.0 * math.tan(fov_y / 2) / H)
    lum, one = LUM.astype(dt), np.ones((H, W), dt)
    Ad = np.maximum(albedo_class[..., :3].astype(dt), dt(EPS_A)) if demodulate else np.ones((H, W, 3), dt)
    cur = history[..., :3].astype(dt)
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
    var = np.where(surf, temporal_variance(history.astype(dt), moments.astype(dt), spatial), 0).astype(dt)
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
    return np.where(surf[..., None], cur * Ad, radiance.astype(dt))
