"""Builds the product library orb_ygz_slam_amd/lib/libygzf.so for gfx950 with hipcc (in-tree, so that the .so travels
to the GPU box with the repo snapshot).  hipcc cross-compiles without a GPU."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRCS = ["csrc/extract_kernels.hip", "csrc/match_kernels.hip", "csrc/align_kernels.hip", "csrc/fast10_kernels.hip", "csrc/dso_kernels.hip", "csrc/stereo_kernels.hip", "csrc/direct_kernels.hip", "csrc/kfdb_kernels.hip", "csrc/kfstore_kernels.hip", "csrc/remap_kernels.hip", "csrc/pose_kernels.hip", "csrc/sim3_kernels.hip", "csrc/sim3_opt_kernels.hip", "csrc/pnp_kernels.hip", "csrc/tri_kernels.hip", "csrc/ygzf_plan.hip", "csrc/ygzf_remap_plan.hip", "csrc/ygzf_api.hip", "csrc/ygzf_api_match.hip", "csrc/ygzf_api_align.hip", "csrc/ygzf_api_detect.hip",
        "csrc/ygzf_api_stereo.hip", "csrc/ygzf_api_kfdb.hip", "csrc/ygzf_api_kfstore.hip", "csrc/ygzf_api_remap.hip", "csrc/ygzf_api_pose.hip", "csrc/ygzf_api_sim3.hip", "csrc/ygzf_api_sim3_opt.hip", "csrc/ygzf_api_pnp.hip", "csrc/ygzf_api_tri.hip", "csrc/ygzf_mgpu.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
         "-ffp-contract=off",                               # bit-exact float paths: no FMA contraction
         "-fhip-fp32-correctly-rounded-divide-sqrt",        # IEEE division in fastAtan2
         "-Wall", "-Wno-unused-function", "-Wno-unused-variable"]
# The SLP vectoriser pairs the aligner's fp32 accumulations into v_pk_* instructions and pays for every pair with register moves
# (488 instead of 420 vector instructions per feature in k_sia_run, which is issue-bound); the integer kernels of the other files keep it.
# k_pose_opt's sums must round as tests/pose_opt_cases.py restates them: no contraction (already the library's rule; stated for this file so that it
# survives a change of FLAGS).  k_sim3_ransac's fp32 operations must each round as tests/sim3_cases.py repeats them, bit for bit: the same.
# k_sim3_opt's numeric Jacobian is a dither of float roundings (csrc/sim3_opt_math.h): one contracted product would move entries by thousands.
# k_pnp_hyp / k_pnp_refine: EPnP's null-space basis is decided by rounding (csrc/pnp_math.h), so one contracted product is another pose.
# k_triangulate: the gates of csrc/tri_math.h are met with equality in tests/triangulate_cases.py, and the Jacobi SVD's stop rule reads single roundings.
FILE_FLAGS = {"csrc/align_kernels.hip": ["-fno-slp-vectorize"], "csrc/pose_kernels.hip": ["-ffp-contract=off"], "csrc/sim3_kernels.hip": ["-ffp-contract=off"],
              "csrc/sim3_opt_kernels.hip": ["-ffp-contract=off"], "csrc/pnp_kernels.hip": ["-ffp-contract=off"], "csrc/tri_kernels.hip": ["-ffp-contract=off"]}


def hipcc():
    for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if p and os.path.exists(p):
            return p
    raise RuntimeError("hipcc not found")


def lib_path():
    return os.path.join(HERE, "lib", "libygzf.so")


def needs_build():
    out = lib_path()
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    deps = [os.path.join(HERE, s) for s in SRCS if os.path.exists(os.path.join(HERE, s))]
    deps += [os.path.join(HERE, "csrc", f) for f in os.listdir(os.path.join(HERE, "csrc")) if f.endswith(".h")]
    deps.append(os.path.join(ROOT, "include", "ygzf.h"))
    return any(os.path.getmtime(d) > t for d in deps)


def check_handover_isa(verbose=False):
    """The matcher's fence-free hand-over between the workgroups of a pair (csrc/match_kernels.hip: st_dev / ld_dev) is correct because of what
    these builtins compile to on gfx950, so the build looks: the device assembly of that file must show k_handover_probe as exactly one
    `global_load_dword ... sc1` and one `global_store_dword ... sc1`, and k_match_last must carry the scoped accesses of its hand-over (22 stores of
    records / query parameters, at least as many loads) plus the fenced alternative.  Raises RuntimeError otherwise (build() then falls back to the fenced hand-over with a warning)."""
    import re
    src = "csrc/match_kernels.hip"
    cmd = [hipcc()] + [f for f in FLAGS if not f.startswith("-W")] + FILE_FLAGS.get(src, []) + ["-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", src, "-o", "-"]
    if verbose:
        print(" ".join(cmd))
    asm = subprocess.run(cmd, cwd=HERE, check=True, capture_output=True, text=True).stdout
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_ZN4ygzf\w+):[^\n]*\n(.*?)^\s*s_endpgm", asm, re.S | re.M)}

    def count(body, op):
        return len(re.findall(r"global_%s_dword\w* [^\n]*\bsc1\b" % op, body))
    probe = next((b for n, b in bodies.items() if "k_handover_probe" in n), None)
    match = next((b for n, b in bodies.items() if "k_match_last" in n), None)
    if probe is None or match is None:
        raise RuntimeError("check_handover_isa: k_handover_probe / k_match_last not found in the assembly of %s" % src)
    got = {"probe_loads_sc1": count(probe, "load"), "probe_stores_sc1": count(probe, "store"),
           "probe_plain": len(re.findall(r"global_(load|store)_dword\w* ", probe)) - count(probe, "load") - count(probe, "store"),
           "match_stores_sc1": count(match, "store"), "match_loads_sc1": count(match, "load"), "match_wbl2": match.count("buffer_wbl2"), "match_inv": match.count("buffer_inv")}
    ok = (got["probe_loads_sc1"] == 1 and got["probe_stores_sc1"] == 1 and got["probe_plain"] == 0 and got["match_stores_sc1"] >= 22 and
          got["match_loads_sc1"] >= 22 and got["match_wbl2"] >= 1 and got["match_inv"] >= 1)
    if not ok:
        raise RuntimeError("check_handover_isa: the compiler no longer lowers the matcher's device-scope accesses to sc1 loads / stores (%r)" % (got,))
    return got


def build(force=False, verbose=False, phase_clock=False):
    """phase_clock: the instrumented variant (-DYGZF_PHASE_CLOCK: s_memtime stamps in k_fast_tab / k_describe, tools/fast_phases.py) into
    lib_ab/libygzf_clk.so -- loaded with YGZF_LIBRARY; the product library carries none of it."""
    out = os.path.join(HERE, "lib_ab", "libygzf_clk.so") if phase_clock else lib_path()
    if not force and not phase_clock and not needs_build():
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    os.makedirs(os.path.join(HERE, "lib"), exist_ok=True)
    import fcntl
    with open(os.path.join(HERE, "lib", ".build.lock"), "w") as lock:   # several ranks of one node may get here at once
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not phase_clock and not needs_build():
            return out
        srcs = [s for s in SRCS if os.path.exists(os.path.join(HERE, s))]
        tmp = out + ".tmp.%d" % os.getpid()
        objdir = os.path.join(HERE, "lib", "obj.%d" % os.getpid())
        os.makedirs(objdir, exist_ok=True)
        try:
            from concurrent.futures import ThreadPoolExecutor
            extra = ["-DYGZF_PHASE_CLOCK"] if phase_clock else []

            def compile_one(src, more=()):
                obj = os.path.join(objdir, os.path.basename(src) + ".o")
                cmd = [hipcc()] + FLAGS + FILE_FLAGS.get(src, []) + extra + list(more) + ["-I" + os.path.join(ROOT, "include"), "-c", src, "-o", obj]
                if verbose:
                    print(" ".join(cmd))
                subprocess.check_call(cmd, cwd=HERE)
                return obj
            with ThreadPoolExecutor(max_workers=min(len(srcs) + 1, os.cpu_count() or 1)) as pool:
                isa = pool.submit(check_handover_isa, verbose)
                objs = list(pool.map(compile_one, srcs))
                try:
                    isa.result()
                except RuntimeError as e:
                    # The fence-free hand-over is an optimisation whose proof is the ISA; the fenced path is always correct.  A compiler that lowers
                    # the scoped accesses differently (or renames what the check greps for) costs the library a few microseconds per matcher
                    # launch, not its build: recompile that one file with full fences and say so.  tests/test_handover_isa.py keeps the strict check.
                    sys.stderr.write("[ygzf build] WARNING: %s\n[ygzf build] building csrc/match_kernels.hip with -DYGZF_FORCE_HANDOVER_FENCE\n" % e)
                    compile_one("csrc/match_kernels.hip", ["-DYGZF_FORCE_HANDOVER_FENCE"])
            cmd = [hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + objs + ["-o", tmp]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd, cwd=HERE)
            os.replace(tmp, out)                                         # a loaded library is never rewritten in place
        finally:
            shutil.rmtree(objdir, ignore_errors=True)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, phase_clock="--phase-clock" in sys.argv))
