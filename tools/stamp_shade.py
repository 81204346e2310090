"""Where a k_shade wave spends its cycles, per phase of a 64-slot batch.

The cycle stamps are instrumentation that the product's source does not carry: apply profiles/instr_stamp_shade.patch, build that
tree with EXTRA=-DPT_STAMP_SHADE into a library of its own and select it with PTC_LIB (the patch's head has the commands)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import pbr_amd
from pbr_amd import scenes
pt = pbr_amd.PathTracer(0).load_scene(scenes.atrium())
spp = int(sys.argv[1]) if len(sys.argv) > 1 else 16
pt.frame_begin(1920, 1080, spp, seed=3, max_bounces=8)
pt.frame_add_samples(spp); pt.sync()
st = pt.stats(); c = pt.raw_counters()
names = ["front end (next batch; with PTC_SHADE_SORT=1: class words, rings)", "ray + hit + record loads", "arithmetic", "compaction + stores (ballot, mbcnt prefix)"]
t = [c[7], c[8], c[9], c[10]]
tot = float(sum(t))
for nm, v in zip(names, t): print("%-32s %.3f" % (nm, v / tot))
print("seconds_shade", st["seconds_shade"], "segments", st["segments"], "memtime ticks per segment-lane", tot / st["segments"])
