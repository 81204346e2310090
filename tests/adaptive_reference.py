"""The adaptive-sampling schedule of include/ptc.h / DESIGN.md ("Adaptive sampling") in numpy float32, operation for operation.

Input: the per-sample radiances L[k] (K, h, w, >= 3), sample k of every pixel.  `Schedule` takes the same calls as an adaptive frame (add / adapt) and keeps
what the frame keeps: the RGB sum, m1, m2 and count per pixel and the active set.  Every elementwise numpy operation on float32 arrays is one correctly
rounded IEEE binary32 operation, which is the library's arithmetic contract, so the count map is compared exactly."""
import numpy as np

TILE = 32          # kTile: the ownership tile; the keep rule's neighbourhood is clipped to it
F = np.float32


def luminance(rgb):
    rgb = np.asarray(rgb, F)
    return (F(0.2126) * rgb[..., 0] + F(0.7152) * rgb[..., 1]) + F(0.0722) * rgb[..., 2]


class Schedule:
    def __init__(self, L, threshold, radius, spp_total, owned=None):
        self.L = np.asarray(L, F)
        _, self.h, self.w = self.L.shape[:3]
        self.threshold, self.radius, self.spp_total = F(threshold), int(radius), int(spp_total)
        self.owned = np.ones((self.h, self.w), bool) if owned is None else np.asarray(owned, bool)
        self.active = self.owned.copy()
        self.sum = np.zeros((self.h, self.w, 3), F)
        self.m1 = np.zeros((self.h, self.w), F)
        self.m2 = np.zeros((self.h, self.w), F)
        self.count = np.zeros((self.h, self.w), np.uint32)
        self.done = 0          # samples every active pixel has received
        self.passes = 0
        self.history = []      # the active set's size after every decision step

    def add(self, n):
        """ptc_frame_add_samples(n): n more samples for every active pixel; nothing at all when no pixel is active."""
        if not self.active.any():
            return
        assert self.done + n <= self.spp_total
        a = self.active
        for k in range(self.done, self.done + n):
            rgb = self.L[k][..., :3]
            for ch in range(3):
                self.sum[..., ch][a] = (self.sum[..., ch] + rgb[..., ch])[a]
            l = luminance(rgb)
            self.m1[a] = (self.m1 + l)[a]
            self.m2[a] = (self.m2 + l * l)[a]
        self.count[a] += np.uint32(n)
        self.done += n

    def flags(self):
        n = F(self.done)
        with np.errstate(all="ignore"):
            mean = self.m1 / n
            var = np.fmax(self.m2 / n - mean * mean, F(0))
            e = np.sqrt(var / n) / (mean + F(0.01))
            return self.active & (e > self.threshold)

    def adapt(self):
        """ptc_frame_adapt: one decision step; returns the number of pixels still active."""
        if not self.active.any():
            return 0
        assert self.done > 0
        if self.done >= self.spp_total:
            self.active[:] = False
        else:
            flag = self.flags()
            ys, xs = np.mgrid[0:self.h, 0:self.w]
            keep = np.zeros_like(flag)
            r = self.radius
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    ny, nx = ys + dy, xs + dx
                    ok = (ny >= 0) & (ny < self.h) & (nx >= 0) & (nx < self.w) & (ny // TILE == ys // TILE) & (nx // TILE == xs // TILE)
                    keep |= ok & flag[np.clip(ny, 0, self.h - 1), np.clip(nx, 0, self.w - 1)]
            self.active &= keep
        self.passes += 1
        self.history.append(int(self.active.sum()))
        return self.history[-1]

    def run(self, min_samples, step_samples):
        """ptc_render_adaptive's loop."""
        self.add(min(min_samples, self.spp_total))
        while self.adapt():
            self.add(min(step_samples, self.spp_total - self.done))
        return self.count

    def image(self):
        """The resolve: sum / (float)count per pixel, alpha 1; zeros where nothing was accumulated."""
        out = np.zeros((self.h, self.w, 4), F)
        got = self.count > 0
        with np.errstate(all="ignore"):
            for ch in range(3):
                out[..., ch][got] = (self.sum[..., ch] / self.count.astype(F))[got]
        out[..., 3][got] = F(1)
        return out


def sample_order_mean(L, n):
    """float32 sum of L[0..n) in sample order, divided by (float)n: the uniform n-spp frame."""
    acc = np.zeros(np.asarray(L[0]).shape[:2] + (3,), F)
    for k in range(n):
        acc = acc + np.asarray(L[k], F)[..., :3]
    return acc / F(n)


def distinct_counts(count, owned=None):
    """{count: share of the owned pixels}"""
    c = count if owned is None else count[owned]
    vals, num = np.unique(c, return_counts=True)
    return {int(v): float(k) / c.size for v, k in zip(vals, num)}
