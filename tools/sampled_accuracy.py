"""What the samples' own variance buys the denoiser (GPU box; -> profiles/sampled_variance_accuracy.txt): relMSE = mean((x - ref)^2 / (ref^2 + 0.01)) of the noisy
frame, of ptc_denoise and of ptc_denoise_sampled against the library's 1024-spp render with another seed, 128 x 128, on cornell, sphere10k and
textured_objects: uniform frames with statistics at 8 and 32 spp and an adaptive frame (threshold 0.05, max 64), demodulation on and off.

  python tools/sampled_accuracy.py [--size W H] [--ref-spp N]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import pbr_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=(128, 128))
ap.add_argument("--ref-spp", type=int, default=1024)
args = ap.parse_args()
W, H = args.size
FILTER = dict(iterations=4, sigma_l=4.0, sigma_n=128.0, sigma_p=1.0)


def rel_mse(x, ref):
    x, ref = x[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))


def denoised(pt, call, **p):
    call(**p)
    pt.select_output(pbr_amd.ptc.OUTPUT_DENOISED)
    img = pt.read_radiance()
    pt.select_output(pbr_amd.ptc.OUTPUT_RADIANCE)
    return img


print(f"{W}x{H}, reference {args.ref_spp} spp seed 7, frames seed 1, max_bounces 8; {pbr_amd.load_library().ptc_build_info().decode()}")
for name in ("cornell", "sphere10k", "textured_objects"):
    d = pbr_amd.scenes.by_name(name)
    d.camera.aspect = W / H
    pt = pbr_amd.PathTracer(0).load_scene(d)
    ref = pt.render(W, H, args.ref_spp, seed=7)
    pt.set_sample_covariance(1)
    for label, spp, adaptive in (("uniform 8 spp", 8, False), ("uniform 32 spp", 32, False), ("adaptive threshold 0.05 max 64", 64, True)):
        if adaptive:
            pt.render_adaptive(W, H, spp, seed=1, threshold=0.05)
        else:
            pt.frame_begin(W, H, spp, seed=1)
            pt.frame_set_adaptive()
            pt.frame_add_samples(spp)
            pt.frame_resolve()
        noisy = pt.read_radiance()
        mean_n = float(pt.read_sample_counts().mean())
        pt.frame_guides()
        e_n = rel_mse(noisy, ref)
        for demod in (1, 0):
            e_p = rel_mse(denoised(pt, pt.denoise, demodulate=demod, **FILTER), ref)
            e_s = rel_mse(denoised(pt, pt.denoise_sampled, demodulate=demod, **FILTER), ref)
            print(f"{name}, {label} (mean count {mean_n:.1f}), demodulate {demod}: noisy {e_n:.4g}, ptc_denoise {e_p:.4g}, ptc_denoise_sampled {e_s:.4g}; "
                  f"sampled / noisy {e_s / e_n:.3f}, sampled / ptc_denoise {e_s / e_p:.3f}", flush=True)
    pt.close()
