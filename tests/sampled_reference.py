"""The per-sample RGB covariance of include/ptc.h / DESIGN.md §8d in numpy, operation for operation: the six sums an adaptive frame keeps while
ptc_set_sample_covariance is on, and the variance ptc_denoise_sampled makes of them.

With dt = float32 every elementwise numpy operation on float32 arrays is one correctly rounded IEEE binary32 operation in the order written, which is the
library's arithmetic contract: the sums and the variance are compared bit for bit.  With dt = float64 the same functions are the yardstick the float32
mirror is reported against, and the quadratic form is checked against np.var of the demodulated luminance."""
import numpy as np

F32, F64 = np.float32, np.float64
LUM = (0.2126, 0.7152, 0.0722)
EPS_A = 1e-3
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # the order of the sums: rr, gg, bb, rg, rb, gb


def accumulate(L, count=None, dt=F32):
    """L (N, h, w, >= 3): sample k of every pixel; count (h, w): the samples a pixel receives, its first count[p] ones in sample order (None: all N).
    Returns (s (h, w, 3), q (h, w, 6)): the RGB sums and the six sums of products."""
    L = np.asarray(L)[..., :3].astype(dt)
    N, h, w = L.shape[:3]
    count = np.full((h, w), N, np.int64) if count is None else np.asarray(count).astype(np.int64)
    s, q = np.zeros((h, w, 3), dt), np.zeros((h, w, 6), dt)
    for k in range(int(count.max()) if count.size else 0):
        on = k < count
        x = L[k]
        for ch in range(3):
            s[..., ch][on] = (s[..., ch] + x[..., ch])[on]
        for i, (a, b) in enumerate(PAIRS):
            q[..., i][on] = (q[..., i] + x[..., a] * x[..., b])[on]
    return s, q


def weights(albedo, demodulate, dt=F32):
    """a_c = w_c / max(A_c, 1e-3), or w_c: (h, w, 3)."""
    A = np.asarray(albedo)[..., :3].astype(dt)
    wl = np.broadcast_to(np.array(LUM, dt), A.shape)
    return wl / np.maximum(A, dt(EPS_A)) if demodulate else wl.copy()


def variance_of_mean(mu, q, count, albedo, demodulate, dt=F32):
    """V (h, w) before the clamp, from the per-pixel means mu = s / (float)n (h, w, 3) and the sums q; 0 where count = 0."""
    mu, q = np.asarray(mu)[..., :3].astype(dt), np.asarray(q).astype(dt)
    n = np.asarray(count)
    got = n > 0
    fn = np.where(got, n, 1).astype(dt)
    c = [q[..., i] / fn - mu[..., a] * mu[..., b] for i, (a, b) in enumerate(PAIRS)]
    a = weights(albedo, demodulate, dt)
    ar, ag, ab = a[..., 0], a[..., 1], a[..., 2]
    V = (((ar * ar) * c[0] + (ag * ag) * c[1]) + (ab * ab) * c[2]) + dt(2) * ((((ar * ag) * c[3] + (ar * ab) * c[4])) + (ag * ab) * c[5])
    return np.where(got, V, dt(0)).astype(dt)


def variance(s, q, count, albedo, demodulate, dt=F32):
    """V (h, w) before the clamp, from the sums."""
    n = np.asarray(count)
    fn = np.where(n > 0, n, 1).astype(dt)
    return variance_of_mean(np.asarray(s)[..., :3].astype(dt) / fn[..., None], q, count, albedo, demodulate, dt)


def sampled_variance(V, count, dt=F32):
    """(h, w, 2): (Var_s, 1 / (float)n) = (max(V, 0), 1 / fn), (0, 0) where count = 0: what ptc_read_sampled_variance returns."""
    n = np.asarray(count)
    got = n > 0
    fn = np.where(got, n, 1).astype(dt)
    return np.stack([np.where(got, np.maximum(np.asarray(V).astype(dt), dt(0)), dt(0)), np.where(got, dt(1) / fn, dt(0))], -1).astype(dt)


def demodulated(radiance, albedo, demodulate, dt=F32):
    """D = radiance / max(A, 1e-3), or the radiance: (h, w, 3)."""
    C = np.asarray(radiance)[..., :3].astype(dt)
    return C / np.maximum(np.asarray(albedo)[..., :3].astype(dt), dt(EPS_A)) if demodulate else C


def luminance(rgb, dt=F64):
    rgb = np.asarray(rgb).astype(dt)
    return (rgb[..., 0] * dt(LUM[0]) + rgb[..., 1] * dt(LUM[1])) + rgb[..., 2] * dt(LUM[2])
