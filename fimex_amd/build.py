"""Builds libfimex_amd.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.

Usage: python -m fimex_amd.build [--force] [--jobs N]
The library travels to the GPU box with the source tree; nothing is JIT-compiled there.
"""
import argparse
import concurrent.futures
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
HOST = os.path.join(HERE, "host")
OBJ = os.path.join(HERE, "_build")
LIB = os.path.join(HERE, "libfimex_amd.so")
TUNING_LIB = os.path.join(HERE, "libfimex_amd_tuning.so")  # the same sources with -DFIMEX_AMD_TUNING: reads FIMEX_AMD_<NAME> switches
HOSTLIB = os.path.join(HERE, "libfimex_amd_host.so")
HOSTCLI = os.path.join(HERE, "host_cli")  # executable of the C++ host mirror (listed in .gitignore by name)
STENCIL_LIB = os.path.join(HERE, "libstencil_math_host.so")  # csrc/stencil_math.hpp compiled for the CPU (tests/test_stencil_math_host.py)
STENCIL_SHIM = os.path.join(ROOT, "tests", "stencil_math_host.hip")
PROJECTION_LIB = os.path.join(HERE, "libprojection_host.so")  # csrc/proj_math.hpp and the string parser compiled for the CPU (tests/test_projection_host.py)
PROJECTION_SHIM = os.path.join(ROOT, "tests", "projection_host.hip")
FORWARD_MATH_LIB = os.path.join(HERE, "libforward_math_host.so")  # csrc/forward_math.hpp compiled for the CPU (tests/test_forward_math_host.py)
FORWARD_MATH_SHIM = os.path.join(ROOT, "tests", "forward_math_host.hip")
MERGE_MATH_LIB = os.path.join(HERE, "libmerge_math_host.so")  # csrc/merge_math.hpp compiled for the CPU with g++ (tests/test_merge_math_host.py)
MERGE_MATH_SHIM = os.path.join(ROOT, "tests", "merge_math_host.cc")

MERGE_VECTOR_MATH_LIB = os.path.join(HERE, "libmerge_vector_math_host.so")  # csrc/merge_vector_math.hpp compiled for the CPU with g++ (tests/test_merge_vector_math_host.py)
MERGE_VECTOR_MATH_SHIM = os.path.join(ROOT, "tests", "merge_vector_math_host.cc")
MERGE_VECTOR_TYPED_MATH_LIB = os.path.join(HERE, "libmerge_vector_typed_math_host.so")  # csrc/merge_vector_typed_math.hpp compiled for the CPU with g++ (tests/test_merge_vector_typed_math_host.py)
MERGE_VECTOR_TYPED_MATH_SHIM = os.path.join(ROOT, "tests", "merge_vector_typed_math_host.cc")
BLEND_MATH_LIB = os.path.join(HERE, "libblend_math_host.so")  # csrc/blend_math.hpp compiled for the CPU with g++ (tests/test_blend_math_host.py)
BLEND_MATH_SHIM = os.path.join(ROOT, "tests", "blend_math_host.cc")
VERTICAL_SEARCH_LIB = os.path.join(HERE, "libvertical_search_host.so")  # csrc/vertical_search.hpp compiled for the CPU (tests/test_vertical_search_host.py)
VERTICAL_SEARCH_SHIM = os.path.join(ROOT, "tests", "vertical_search_host.hip")

DEVICE_SOURCES = ["capi.hip", "capi_regrid.hip", "capi_regrid_multi.hip", "capi_vector.hip", "capi_fill.hip", "capi_vertical.hip", "capi_vertical_plan.hip", "capi_merge.hip", "capi_merge_typed.hip", "capi_merge_vector.hip", "capi_merge_vector_typed.hip", "capi_derived.hip", "capi_time_quality.hip", "capi_extract.hip", "backward_plan.hip", "gather.hip", "staged.hip", "staged2_plan.hip", "staged2.hip", "staged2_typed.hip", "staged2_vector.hip", "staged2_vector_typed.hip", "staged2_list.hip", "staged2_list_typed.hip", "forward_plan.hip", "forward.hip", "forward_median.hip", "forward_tiled.hip", "vector.hip", "convert.hip", "fill_sum.hip", "fill_prologue.hip", "fill.hip", "creepfill.hip", "fill_rects.hip", "projection_parse.hip", "projection.hip", "coordsearch.hip", "hostpipe.hip", "batch.hip", "vertical.hip", "vertical_levels.hip", "vertical_velocity.hip", "merge.hip", "merge_typed.hip", "merge_vector.hip", "merge_vector_typed.hip", "scaled_convert.hip", "pressure_convert.hip",
                  "time_accumulate.hip", "time_interpolate.hip", "quality.hip", "extract.hip", "vertical_plan.hip"]

# -ffp-contract=off: the kernels reproduce the reference's IEEE arithmetic operation by operation
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
               "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP kernels cannot be built")
    return exe


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _headers():
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    hdrs += [os.path.join(ROOT, "include", h) for h in ("fimex_amd.h", "fimex_amd_derived_host.h", "fimex_amd_time_quality_host.h", "fimex_amd_extract_host.h", "fimex_amd_vertical_plan_host.h", "fimex_amd_vector_regrid_host.h", "fimex_amd_vector_regrid_typed_host.h", "fimex_amd_merge_typed_host.h", "fimex_amd_merge_vector_host.h", "fimex_amd_merge_vector_typed_host.h", "fimex_amd_regrid_multi_host.h")]
    return hdrs


def _compile(src, force, tuning=False):
    obj = os.path.join(OBJ, os.path.basename(src) + (".tuning.o" if tuning else ".o"))
    if force or _newer(obj, [src] + _headers()):
        cmd = [_hipcc()] + HIPCC_FLAGS + (["-DFIMEX_AMD_TUNING"] if tuning else []) + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, r.stdout, r.stderr))
        if r.stderr.strip():
            sys.stderr.write(r.stderr)
    return obj


def build_device(force=False, jobs=4, tuning=False):
    """libfimex_amd.so, or with tuning=True libfimex_amd_tuning.so (experiment switches read from the environment)."""
    os.makedirs(OBJ, exist_ok=True)
    srcs = [os.path.join(CSRC, s) for s in DEVICE_SOURCES]
    lib = TUNING_LIB if tuning else LIB
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
        objs = list(ex.map(lambda s: _compile(s, force, tuning), srcs))
    if force or _newer(lib, objs):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs + [
            "-Wl,-rpath,/opt/rocm/lib", "-Wl,--no-undefined"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s\n%s" % (r.stdout, r.stderr))
    return lib


def build_host(force=False):
    """C++ host mirror of the reference classes, linked against the C ABI only."""
    if not os.path.isdir(HOST):
        return None
    srcs = sorted(os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".cc") and f not in ("host_cli.cc", "Projection.cc"))
    if not srcs:
        return None
    deps = srcs + [os.path.join(HOST, f) for f in os.listdir(HOST) if f.endswith(".h")] + [
        os.path.join(ROOT, "include", "fimex_amd.h")]
    if force or _newer(HOSTLIB, deps + [LIB]):
        cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-o", HOSTLIB] + srcs + [
            "-L" + HERE, "-lfimex_amd", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("host library build failed:\n%s\n%s" % (r.stdout, r.stderr))
    cli_src = os.path.join(HOST, "host_cli.cc")
    if os.path.exists(cli_src) and (force or _newer(HOSTCLI, [cli_src, HOSTLIB] + deps)):
        cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-o", HOSTCLI, cli_src,
               "-L" + HERE, "-lfimex_amd_host", "-lfimex_amd", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("host_cli build failed:\n%s\n%s" % (r.stdout, r.stderr))
    return HOSTLIB


def _build_shim(what, compiler, sources, deps, out, force):
    """One host-only shared library of a shim under tests/ and the header it compiles: compiler "hipcc" (--cuda-host-only, for
    headers that need HIP's) or "g++" (no HIP header at all).  deps: what a newer file of rebuilds it, besides the sources."""
    if force or _newer(out, sources + deps):
        front = [_hipcc(), "--cuda-host-only", "-Wno-unused-function"] if compiler == "hipcc" else ["g++"]
        back = ["-Wl,-rpath,/opt/rocm/lib"] if compiler == "hipcc" else []
        cmd = front + ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I" + CSRC] + sources + ["-o", out] + back
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("%s shim build failed:\n%s\n%s" % (what, r.stdout, r.stderr))
        if r.stderr.strip():
            sys.stderr.write(r.stderr)
    return out


def _csrc(*names):
    return [os.path.join(CSRC, n) for n in names]


def build_stencil_host(force=False):
    """The backward stencil rules the kernels compile (csrc/stencil_math.hpp), for the host only: the tests run it on the CPU, without a GPU."""
    return _build_shim("stencil", "hipcc", [STENCIL_SHIM], _headers(), STENCIL_LIB, force)


def build_projection_host(force=False):
    """The projections' point math (csrc/proj_math.hpp) and the PROJ.4 string parser, for the host only: the tests run them on the CPU."""
    return _build_shim("projection", "hipcc", [PROJECTION_SHIM] + _csrc("projection_parse.hip"), _headers(), PROJECTION_LIB, force)


def build_forward_math_host(force=False):
    """The forward aggregation rules the kernels compile (csrc/forward_math.hpp), for the host only: the tests run them on the CPU."""
    return _build_shim("forward math", "hipcc", [FORWARD_MATH_SHIM], _headers(), FORWARD_MATH_LIB, force)


def build_merge_math_host(force=False):
    """The merge's per-cell arithmetic the kernels compile (csrc/merge_math.hpp), with g++ and no HIP header: the tests run it on the CPU."""
    return _build_shim("merge math", "g++", [MERGE_MATH_SHIM], _csrc("merge_math.hpp"), MERGE_MATH_LIB, force)


def build_merge_vector_math_host(force=False):
    """The merge's per-cell arithmetic on a vector pair (csrc/merge_vector_math.hpp), with g++ and no HIP header: the tests run it on the CPU."""
    return _build_shim("merge vector math", "g++", [MERGE_VECTOR_MATH_SHIM], _csrc("merge_vector_math.hpp", "merge_math.hpp"), MERGE_VECTOR_MATH_LIB, force)


def build_merge_vector_typed_math_host(force=False):
    """The merge's per-cell arithmetic on a vector pair in its stored types (csrc/merge_vector_typed_math.hpp), with g++ and no HIP header: the tests run it on the CPU."""
    return _build_shim("merge vector typed math", "g++", [MERGE_VECTOR_TYPED_MATH_SHIM],
                       _csrc("merge_vector_typed_math.hpp", "merge_vector_math.hpp", "merge_math.hpp"), MERGE_VECTOR_TYPED_MATH_LIB, force)


def build_blend_math_host(force=False):
    """The 1-D blends the kernels and the host entries compile (csrc/blend_math.hpp), with g++ and no HIP header: the tests run them on the CPU."""
    return _build_shim("blend math", "g++", [BLEND_MATH_SHIM], _csrc("blend_math.hpp") + [os.path.join(ROOT, "include", "fimex_amd.h")],
                       BLEND_MATH_LIB, force)


def build_vertical_search_host(force=False):
    """The level search of the vertical kernels (csrc/vertical_search.hpp), for the host only: the tests run it on the CPU."""
    return _build_shim("vertical search", "hipcc", [VERTICAL_SEARCH_SHIM], _headers(), VERTICAL_SEARCH_LIB, force)


def clean():
    """Removes every built artefact, so that the next build starts from the sources alone."""
    shutil.rmtree(OBJ, ignore_errors=True)
    for f in (LIB, TUNING_LIB, HOSTLIB, HOSTCLI, STENCIL_LIB, PROJECTION_LIB, FORWARD_MATH_LIB, MERGE_MATH_LIB, MERGE_VECTOR_MATH_LIB, MERGE_VECTOR_TYPED_MATH_LIB, BLEND_MATH_LIB, VERTICAL_SEARCH_LIB,
              os.path.join(HERE, "host_cli.so")):
        if os.path.exists(f):
            os.remove(f)


def build_all(force=False, jobs=4):
    if force:
        clean()
    lib = build_device(force=force, jobs=jobs)
    build_device(force=force, jobs=jobs, tuning=True)
    host = build_host(force=force)
    build_stencil_host(force=force)
    build_projection_host(force=force)
    build_forward_math_host(force=force)
    build_merge_math_host(force=force)
    build_merge_vector_math_host(force=force)
    build_merge_vector_typed_math_host(force=force)
    build_blend_math_host(force=force)
    build_vertical_search_host(force=force)
    return lib, host


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    print(build_all(force=a.force, jobs=a.jobs))
