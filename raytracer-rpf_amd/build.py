"""Builds raytracer-rpf_amd/lib/librpf_hip.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.
hipcc cross-compiles without a GPU.  -ffp-contract=off is REQUIRED: the kernels rely on the reference's
fp64 operation order for the discrete decisions (see csrc/rpf_kernels.hip)."""
import os
import shutil
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB = os.path.join(_HERE, "lib", "librpf_hip.so")
# the fused per-pixel kernels compile as one translation unit per sample layout, build and size-class part, in parallel (the single
# kernel TU of rounds 1-2 took 3.2 minutes).  Each unit is rpf_filter_impl.inc through rpf_impl_unit.inc: the listed builds read stage 1b
# from the member pool (RPF_FLAG_SAMPLED_LISTED), the scheduled ones form stage 3c from the entry's gains
# (RPF_FLAG_SCHEDULE_FUSED, section 15e); part 4, the *_member TUs, is the count pass under the membership test (RPF_FLAG_MEMBER_FUSED)
IMPL_TUS = ["rpf_impl_%s_%s%s%s.hip" % (lay, li, sc, part) for lay in ("d19", "d27") for li in ("", "listed_") for sc in ("", "sched_")
            for part in ("small", "mid", "large")] + ["rpf_impl_d19_member.hip", "rpf_impl_d27_member.hip"]
KERNEL_TUS = IMPL_TUS + ["rpf_kernels.hip"]
KERNEL_TUS += ["rpf_film.hip"]  # the film step (pbrt's reconstruction filter): rpf_filter_film / rpf_film_splat_device
KERNEL_TUS += ["rpf_generic.hip"]  # the layout-generic kernel pair (RPF_FLAG_GENERIC): n_random / n_feat at run time
KERNEL_TUS += ["rpf_generic_packed.hip"]  # ... its count pass and packed kernels for N <= 64 (RPF_FLAG_GENERIC_PACKED)
KERNEL_TUS += ["rpf_generic_wave.hip"]  # ... and its one-wave kernels for 64 < N <= 832 (RPF_FLAG_GENERIC_WAVE)
KERNEL_TUS += ["rpf_generic_wide.hip"]  # the wide layout-generic kernel: 65535 < box*box*S <= 262144 (RPF_FLAG_WIDE_NBHD)
KERNEL_TUS += ["rpf_spike.hip"]  # the spike pass after the last filter pass: clamp, row sums, energy add (RPF_FLAG_SPIKE_CLAMP)
KERNEL_TUS += ["rpf_generic_wide_count.hip"]  # ... and the count pass that deals a wide pass by size class (RPF_FLAG_WIDE_CLASSES)
KERNEL_TUS += ["rpf_generic_sampled_count.hip"]  # the count pass of a sampled pass: the draws of a pixel's key (RPF_FLAG_SAMPLED_NBHD)
KERNEL_TUS += ["rpf_generic_sampled_mask.hip"]  # ... and the count pass that leaves the draws as acceptance masks for the compiled kernels (RPF_FLAG_SAMPLED_FUSED)
KERNEL_TUS += ["rpf_generic_quad.hip"]  # the four-wave layout-generic kernels for 832 < N <= 3136 (RPF_FLAG_GENERIC_QUAD)
KERNEL_TUS += ["rpf_report.hip"]  # the per-pass activity report: per-pixel chains, per-row chains and counts (RPF_FLAG_PASS_REPORT)
# the C ABI (host code only; rpf_api.h is what they share): context, validation and pass loops | pass router | film step | multi-GPU | spike pass | pass report
# (the names start with rpf_api: the spill scan below skips them by that)
API_TUS = ["rpf_api.hip", "rpf_api_routes.hip", "rpf_api_film.hip", "rpf_api_multi.hip", "rpf_api_spike.hip", "rpf_api_report.hip"]
SOURCES = [os.path.join(_HERE, "csrc", f) for f in KERNEL_TUS + API_TUS]
HEADERS = [os.path.join(_HERE, "csrc", "rpf_internal.h"), os.path.join(_HERE, "csrc", "rpf_api.h"), os.path.join(_HERE, "csrc", "rpf_xlane.h"),
           os.path.join(_HERE, "csrc", "rpf_impl_unit.inc"), os.path.join(_HERE, "csrc", "rpf_filter_impl.inc"), os.path.join(_HERE, "csrc", "rpf_packed_impl.inc"),
           os.path.join(_HERE, "csrc", "rpf_device_common.h"), os.path.join(_HERE, "csrc", "rpf_reflog.h"),
           os.path.join(_HERE, "csrc", "rpf_generic_common.h"),  # what the rpf_generic*.hip share
           os.path.join(_HERE, "csrc", "rpf_generic_sampled_draws.h"),  # ... the draws of a sampled pass, which its two count TUs share
           os.path.join(_HERE, "csrc", "rpf_generic_sampled_bitmap.inc"),  # ... the steps the bitmap count kernels of routes 11 and 12 share
           os.path.join(_HERE, "csrc", "rpf_generic_stream_stages.inc"),  # ... and the stage bodies of rpf_generic.hip and rpf_generic_wide.hip
           os.path.join(_ROOT, "include", "rpf_hip.h")]


def hipcc_path():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


OBJ_DIR = os.path.join(_ROOT, "build", "obj")


def _stale(target, deps):
    return (not os.path.exists(target)) or any(os.path.getmtime(f) > os.path.getmtime(target) for f in deps)


SCAN_OK = os.path.join(OBJ_DIR, "spill_scan.ok")  # written by build() after scripts/check_spills.py passed


def is_stale():
    return _stale(LIB, SOURCES + HEADERS) or not os.path.exists(SCAN_OK)


def build(force=False, verbose=False, defs=(), tag=None):
    """one object per translation unit, compiled in parallel, then the link.
    defs / tag: an experiment variant -- extra -D flags, objects under build/obj_<tag>, library lib/librpf_hip_<tag>.so
    (measured side by side with the shipped library through hip.py's RPF_HIP_LIB; never what tests or bench.py load by default)"""
    if tag:
        return _build_variant(list(defs), tag, verbose)
    if not force and not is_stale():
        return LIB
    return _build(LIB, OBJ_DIR, [], True, force, verbose)


def _build_variant(defs, tag, verbose):
    return _build(os.path.join(_HERE, "lib", "librpf_hip_%s.so" % tag), os.path.join(_ROOT, "build", "obj_" + tag), defs, False, False, verbose)


def _build(LIB, OBJ_DIR, defs, shipped, force, verbose):
    SCAN_OK = os.path.join(OBJ_DIR, "spill_scan.ok")
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    os.makedirs(OBJ_DIR, exist_ok=True)
    flags = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17",
             "-I" + os.path.join(_ROOT, "include"), "-I" + os.path.join(_HERE, "csrc")] + list(defs)
    objs, cmds = [], []
    for src in SOURCES:
        obj = os.path.join(OBJ_DIR, os.path.basename(src) + ".o")
        objs.append(obj)
        if force or _stale(obj, [src] + HEADERS):
            # -save-temps=obj keeps the device assembly next to the object: scripts/check_spills.py reads it below
            cmds.append([hipcc_path()] + flags + ["-save-temps=obj", "-c", src, "-o", obj])
    # at most MAX_JOBS compilers at a time, 16 at the most (one hipcc per translation unit all at once oversubscribes a machine
    # that gives the build a share of its cores).  The largest units (the rpf_impl_* parts) start first
    jobs = max(1, min(16, int(os.environ.get("MAX_JOBS", 16))))
    cmds.sort(key=lambda c: not os.path.basename(c[-3]).startswith("rpf_impl_"))
    running, failed = [], None
    while (cmds and failed is None) or running:
        while cmds and failed is None and len(running) < jobs:
            cmd = cmds.pop(0)
            if verbose:
                print(" ".join(cmd))
            running.append((cmd, subprocess.Popen(cmd)))
        cmd, pr = running.pop(0)
        try:
            rc = pr.wait(timeout=0.2 if (cmds and failed is None) else None)
        except subprocess.TimeoutExpired:
            running.append((cmd, pr))
            continue
        if rc != 0 and failed is None:
            failed = subprocess.CalledProcessError(rc, cmd)
    if failed is not None:
        raise failed
    import glob
    asm = sorted(f for f in glob.glob(os.path.join(OBJ_DIR, "*gfx950*.s")) if "rpf_api" not in os.path.basename(f))
    if asm:
        # the scan's verdict is kept next to the objects (is_stale() wants it) and, when every kernel TU was compiled in this
        # invocation, the per-kernel resource usage of the build goes to profiles/ (tracked: the figures of what ships)
        full = shipped and len(asm) == len(KERNEL_TUS)
        report = os.path.join(_ROOT, "profiles", "r03_resource_usage.txt") if full else os.path.join(OBJ_DIR, "resource_usage_partial.txt")
        chk = subprocess.run([sys.executable, os.path.join(_ROOT, "scripts", "check_spills.py"), "--report", report] + asm,
                             stdout=subprocess.PIPE, text=True)
        if chk.returncode != 0:
            if os.path.exists(SCAN_OK):
                os.remove(SCAN_OK)
            for a in asm:  # the objects of a refused build must not be linked by a later invocation
                o = os.path.join(OBJ_DIR, os.path.basename(a).split("-hip-amdgcn")[0] + ".hip.o")
                if os.path.exists(o):
                    os.remove(o)
            raise RuntimeError("spill code in front of an EXEC restore, or a DPP read hazard, in a kernel TU (see scripts/check_spills.py):\n" + chk.stdout)
        with open(SCAN_OK, "w") as f:
            f.write("check_spills.py: no spill code in front of an EXEC restore, no DPP read hazard\n" + chk.stdout)
        if verbose:
            print(chk.stdout)
    for f in glob.glob(os.path.join(OBJ_DIR, "*")):  # the -save-temps intermediates (~100 MB) have served their purpose
        if f not in objs and f != SCAN_OK and not (f.endswith(".txt") and "resolution" not in f):
            os.remove(f)
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB


HOST_LIB = os.path.join(_HERE, "lib", "librpf_host.so")
HOST_SOURCES = [os.path.join(_HERE, "host", "rpf_host.cpp")]
HOST_HEADERS = [os.path.join(_HERE, "host", "rpf_host.h"), os.path.join(_ROOT, "include", "rpf_hip.h")]


def build_host(force=False, verbose=False):
    """host-side C++ mirror of the reference interface (g++, no HIP), linked against librpf_hip.so"""
    build(force=False)
    stale = (not os.path.exists(HOST_LIB)) or any(
        os.path.getmtime(f) > os.path.getmtime(HOST_LIB) for f in HOST_SOURCES + HOST_HEADERS + [LIB])
    if not force and not stale:
        return HOST_LIB
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-I" + os.path.join(_ROOT, "include"),
           "-I" + os.path.join(_HERE, "host"), "-o", HOST_LIB] + HOST_SOURCES + [
           "-L" + os.path.dirname(LIB), "-lrpf_hip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return HOST_LIB


if __name__ == "__main__":
    force = "--force" in sys.argv
    if "--variant" in sys.argv:  # python build.py --variant <tag> -DNAME=VALUE ...
        print(build(verbose=True, defs=[a for a in sys.argv[1:] if a.startswith("-D")], tag=sys.argv[sys.argv.index("--variant") + 1]))
        sys.exit(0)
    print(build(force=force, verbose=True))
    print(build_host(force=force, verbose=True))
