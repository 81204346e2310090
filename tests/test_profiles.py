"""The measurement artefacts bench.py depends on are committed and well-formed (no GPU needed): the per-kernel model calibrated from the
rocprofv3 PMC profile, the VALU issue-rate microbenchmark, and the arithmetic that turns counted units into roofline fractions."""
import ast
import hashlib
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF = os.path.join(ROOT, "profiles")
CSRC = os.path.join("physically-based-renderer_amd", "csrc")
# the hashed kernel sources: the one list is csrc/Makefile's KERNEL_SRC
KERNEL_SRC = [os.path.join(CSRC, f) for f in re.search(r"^KERNEL_SRC = (.*)$", open(os.path.join(ROOT, CSRC, "Makefile")).read(), re.M).group(1).split()]


def _kernel_source_sha256():
    """csrc/Makefile's KERNEL_SHA: sha256 over its KERNEL_SRC list in that order — every file that holds device code (what ptc_build_info reports)."""
    h = hashlib.sha256()
    for f in KERNEL_SRC:
        h.update(open(os.path.join(ROOT, f), "rb").read())
    return h.hexdigest()


def test_kernel_models_were_measured_on_the_kernels_in_the_tree():
    """bench.py's roofline block multiplies live counts by per-unit figures from a rocprofv3 PMC profile.  The profile names the kernels it was
    taken on (sha256 of the kernel sources, checked against the profiled library by tools/make_kernel_model.py): editing a kernel without
    profiling again fails HERE, instead of silently reporting a fraction that belongs to other code."""
    sha = _kernel_source_sha256()
    import sys
    sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
    import pbr_amd
    L = pbr_amd.load_library()
    assert L.ptc_build_info().decode().endswith(sha), "libptc.so was built from other kernel sources than the tree's: make -C physically-based-renderer_amd/csrc"
    defaults = L.ptc_launch_policy(None).decode()
    for f in ("r04_kernel_model.json", "r04_textured_kernel_model.json"):
        m = json.load(open(os.path.join(PROF, f)))
        assert m["kernel_source_sha256"] == sha, f"{f} was measured on kernels {m['kernel_source_sha256'][:12]}, the tree holds {sha[:12]}: run tools/profile.sh + tools/make_kernel_model.py again"
        assert len(m["git_commit"]) >= 40
        # ... and under the launch policy the library still defaults to: block sizes, chunk, ring, thresholds, lanes, batch size, overlap mode, nodelets (ptc_launch_policy).
        # Changing TRACE_MIN_WAVES, the overlap default or the batch size without profiling again fails here; what follows from them on a device (blocks per CU,
        # stack entries in LDS) is in the model's full `launch_policy`, which bench.py compares with the running context's.
        assert m["launch_policy_defaults"] == defaults, f"{f}: the library's launch defaults moved since the profile:\n  profile {m['launch_policy_defaults']}\n  library {defaults}"
        assert m["launch_policy"].startswith(defaults.split(" | ")[0]) and "trace_blocks_per_cu=" in m["launch_policy"]


def test_kernel_model_and_ceilings_are_committed():
    model = json.load(open(os.path.join(PROF, "r04_kernel_model.json")))
    for k in ("k_trace_closest", "k_trace_any", "k_shade"):
        m = model[k]
        for key in ("valu_winstr_per_unit", "hbm_bytes_per_unit", "serialised_ms_per_launch", "serialised_units_per_launch", "dispatches", "unit"):
            assert key in m and m[key], (k, key)
        assert 0.3 < m["valu_lane_utilisation"] <= 1.0
        assert 0.1 < m["valu_issue_duty_per_cycle"] < 1.0
    # a node visit of the 8-wide tree costs ~6 wave-instructions per lane-visit (=~380 lane slots, everything amortised)
    assert 3.0 < model["k_trace_closest"]["valu_winstr_per_unit"] < 12.0
    valu = json.load(open(os.path.join(PROF, "r02_valu_issue.json")))
    ns = valu["ns_per_instr_per_simd_at_7_waves"]
    assert 0.8 < ns < 1.6                                   # one wave64 instruction per ~2 cycles and SIMD at >= 2 resident waves
    assert 1.6 < valu["ns_per_instr_one_wave"] / ns < 2.2   # a lone wave issues at half that rate
    assert 600 < 1024 / ns < 1229                            # G wave-instr/s: below the paper figure 1024 x 2.4 GHz / 2
    peak = 1024 * 2.4 / 2.0                                  # the guide's peak: what the headline fraction is against
    # exclusive fractions reproduce from the model alone: units x instr / time / peak
    for k, lo, hi in (("k_trace_closest", 0.4, 0.8), ("k_trace_any", 0.4, 0.8), ("k_shade", 0.1, 0.6)):
        m = model[k]
        frac = m["serialised_units_per_launch"] * m["valu_winstr_per_unit"] / (m["serialised_ms_per_launch"] * 1e-3) / 1e9 / peak
        assert lo < frac < hi, (k, frac)
    for f in ("r04_kernel_stats.csv", "r04_pmc_summary.json", "r02_gather_bench.json", "r04_bench.json", "r04_textured_kernel_stats.csv", "r04_textured_pmc_summary.json",
              "r03_valu_mix.json", "r04_fuzz_parity.txt", "r04_refit_curve.txt", "r04_rebuild_kernel_stats.csv"):
        assert os.path.getsize(os.path.join(PROF, f)) > 100, f


def test_bench_line_of_the_committed_run_has_the_contract_fields():
    d = json.load(open(os.path.join(PROF, "r04_bench.json")))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["unit"] == "Mpaths/s" and d["dtype"] == "f32" and d["scaling"] == "strong" and d["vs_baseline"] is None and d["data"] == "synthetic"
    r = d["roofline"]
    assert r["bound"] == "valu_issue" and 0 < r["frac"] <= 1 and 0 < r["frac_exclusive"] <= 1 and r["traffic"] > 0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and abs(r["peak"] - 1228.8) < 1e-6       # against the guide's peak, the measured ceiling beside it
    assert r["frac"] < r["frac_of_measured_ceiling"] < 1 and 0 < r["issue_duty_per_cycle"] < 1
    assert r["model_stale"] is False and r["model_stale_why"] == [] and r["model_kernel_sha256"] == r["library_kernel_sha256"] and len(r["model_commit"]) >= 40
    assert d["launch_policy"] == r["model_launch_policy"] and d["launch_policy"].startswith(d["launch_policy_defaults"].split(" | ")[0])
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1
    assert abs(d["value"] - d["config"]["paths"] / (d["ms_per_step"] * 1e-3 * d["steps"]) / 1e6) / d["value"] < 1e-6
    ast.parse(open(os.path.join(ROOT, "bench.py")).read())


STRIPPED_PATCHES = ("instr_diag", "instr_stamp", "instr_stamp_shade", "exp_leaf_extra", "exp_shade_variants", "exp_misc", "exp_oracle_fp16_slab")


def _foreign_conditionals(path):
    """Preprocessor conditionals of a file that are neither a tunable's default (`#ifndef NAME`, `#define NAME ...`, `#endif` and nothing else but
    comments between them) nor the file's include guard, as (line number, text)."""
    import re
    code = [(i + 1, ln.strip()) for i, ln in enumerate(open(os.path.join(ROOT, path), encoding="utf-8")) if ln.strip() and not ln.strip().startswith("//")]
    directive = re.compile(r"#\s*(ifndef|ifdef|if|elif|else|endif)\b\s*(\w*)")
    bad, k, seen_directive = [], 0, False
    while k < len(code):
        no, ln = code[k]
        m = directive.match(ln)
        if m:
            kind, name = m.groups()
            define = re.match(r"#\s*define\s+%s\b" % re.escape(name), code[k + 1][1]) if kind == "ifndef" and k + 2 < len(code) else None
            if define and re.match(r"#\s*endif\b", code[k + 2][1]):
                k += 3          # a tunable's default
                continue
            if define and not seen_directive and re.match(r"#\s*endif\b", code[-1][1]):
                code.pop()      # the include guard: first directive of the file, closed by its last line
                k += 2
                continue
            bad.append((no, ln))
        seen_directive = seen_directive or ln.startswith("#")
        k += 1
    return bad


def test_kernel_and_oracle_sources_hold_no_experiment_conditionals():
    """The hashed kernel sources and the oracle are what ships and what specifies: every conditional in them is a tunable's `#ifndef` default (the sweeps
    set those with EXTRA=-D..., the policy string reports them) or an include guard; no #ifdef / #if / #elif / #else.  Instrumentation and rejected variants are
    kept as profiles/instr_*.patch and profiles/exp_*.patch."""
    assert _foreign_conditionals(KERNEL_SRC[0]) == [] and "#ifndef TRACE_BLOCK" in open(os.path.join(ROOT, KERNEL_SRC[0]), encoding="utf-8").read()
    for f in KERNEL_SRC + [os.path.join("oracle", "ptc_oracle.c")]:
        assert _foreign_conditionals(f) == [], f


def test_stripped_instrumentation_and_experiments_apply_as_patches():
    """What left the sources stays usable: each patch applies to the tree as it stands (git apply needs no repository)."""
    import subprocess
    for name in STRIPPED_PATCHES:
        r = subprocess.run(["git", "apply", "--check", os.path.join("profiles", name + ".patch")], cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr)


def test_render_arithmetic_has_one_definition():
    """DESIGN.md's arithmetic contract: an expression is written once in the product (csrc/pt_device.h, host + device) and once in the oracle.  Four literals that
    only the RNG hash, sincos2pi, pt_log2 and rrt_odt hold each occur in exactly one file under csrc/; no header has a device part behind a macro any more; and the
    list of hashed sources this file uses is the Makefile's, with the shared device header on it."""
    src = {f: open(os.path.join(ROOT, CSRC, f), encoding="utf-8").read() for f in sorted(os.listdir(os.path.join(ROOT, CSRC)))}
    for literal in ("747796405", "2.7557319e-6", "0.3205989", "0.983729f"):
        assert [f for f, text in src.items() if literal in text] == ["pt_device.h"], literal
    assert not [f for f, text in src.items() if "PT_LIGHTS_DEVICE_PART" in text]
    make = re.search(r"^KERNEL_SRC = (.*)$", src["Makefile"], re.M).group(1).split()
    assert [os.path.basename(f) for f in KERNEL_SRC] == make and {"pt_kernels.hip", "pt_device.h", "pt_shading.h"} <= set(make)
    assert set(f for f in make if f.endswith(".h")) <= set(re.search(r"^HDR = (.*)$", src["Makefile"], re.M).group(1).split())


def test_scene_build_rules_have_one_definition():
    """The rules that turn a scene description into the bytes in HBM are written once (csrc/pt_scene_rules.h, host + device) and once in the oracle: the host
    builder and the device builders call them.  Six expressions that only a build rule holds and that stood in two or more files before — the Morton scale, the cost
    term's fixed point, the nudge of an upper plane, the z term of the slot score, the half area of a box, the order-preserving map — each occur in exactly one file
    under csrc/, that header;
    it is on the hashed list; and the device files no longer point at ptc_scene.cpp for their definitions."""
    src = {f: open(os.path.join(ROOT, CSRC, f), encoding="utf-8").read() for f in sorted(os.listdir(os.path.join(ROOT, CSRC)))}
    for expr in ("2097152.0f", "* PTC_SA_COST_ONE", "(float)q2 * sc", "(sl & 4) ? d[i][2]", "ex * ey + ey * ez + ez * ex", "? ~u : (u | 0x80000000u)"):
        assert [f for f, text in src.items() if expr in text] == ["pt_scene_rules.h"], expr
    assert "pt_scene_rules.h" in [os.path.basename(f) for f in KERNEL_SRC]
    for f in ("pt_refit.hip", "pt_build.hip", "ptc_scene.cpp", "ptc_api_scene.cpp"):
        assert '#include "pt_scene_rules.h"' in src[f], f
    for f in ("pt_refit.hip", "pt_build.hip"):
        assert "pt_scene_rules.h" in src[f].split("#include")[0] and "in the host's order" not in src[f] and "ptc_scene.cpp)." not in src[f].split("#include")[0], f
