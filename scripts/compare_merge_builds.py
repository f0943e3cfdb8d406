#!/usr/bin/env python3
"""Compares the grid merging of two builds of the library: the same bits, and the same time.

  compare_merge_builds.py --parent DIR [--rounds 4] [--out profiles/merge_shell_parent_vs_new.json]

DIR holds libfimex_amd.so and libfimex_amd_tuning.so built from the commit to compare with; the other side is this tree's.  The driver
(compare_builds.py) alternates the sides, one fresh process per side and round, and stops at the first that does not end normally.

Bits: the worker runs tests/test_gpu_merge.py, test_gpu_merge_typed.py, test_gpu_merge_vector.py, test_gpu_merge_vector_typed.py and
test_gpu_merge_slices.py under pytest in its own process, on the side's library, with the modules' `_identical` wrapped: every array
a test compares with its expectation -- the results of the fused entries, of the chains, of border_smooth, overlay and their typed
forms, in place and out of place, device and host -- is hashed (sha256 of its bytes) before it is compared.  One case per test
function: the sha256 over the labels and hashes of all its arrays, and their number.  A failing test ends the worker.

Time: scripts/bench_merge.py, bench_merge_typed.py, bench_merge_vector.py and bench_merge_vector_typed.py with their default
workloads, each run once per worker.  Per script the fused form counts, and border_smooth_typed / overlay_typed where bench_merge_typed.py
times them: the median of the script's timed calls, without the calls above 0.4 s where the script lists every call (the known
hipMallocAsync stalls; bench_merge.py reports its median only).  That is one figure per round; the driver takes the median over the
rounds and the parent's (max - min) over its rounds as the margin.  The scripts compare fused with chain themselves.
"""
import argparse, contextlib, functools, hashlib, io, json, os, statistics, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import compare_builds  # beside this script

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
compare_builds.add_arguments(ap, os.path.join(ROOT, "profiles", "merge_shell_parent_vs_new.json"))
ap.set_defaults(rounds=4)
args = ap.parse_args()

TEST_MODULES = ["test_gpu_merge", "test_gpu_merge_typed", "test_gpu_merge_vector", "test_gpu_merge_vector_typed", "test_gpu_merge_slices"]
STALL_MS = 400.0
# script -> [(case, path of the timed form in the script's result, path of its list of every call or None)]
BENCHES = {
    "bench_merge": [("fused", ("ms_median",), None)],
    "bench_merge_typed": [("typed_fused", ("ms_median", "typed_fused"), ("ms_every_call", "typed_fused")),
                          ("border_smooth_typed", ("elementwise_short_float", "ms_median", "border_smooth_typed"), None),
                          ("overlay_typed", ("elementwise_short_float", "ms_median", "overlay_typed"), None)],
    "bench_merge_vector": [("fused", ("ms_median", "fused"), ("ms_every_call", "fused"))],
    "bench_merge_vector_typed": [("fused", ("ms_median", "fused"), ("ms_every_call", "fused"))],
}


def worker():
    import importlib
    import numpy as np
    import pytest
    from fimex_amd import capi as fa
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    if args.lib:
        fa.LIB_PATH = os.path.join(args.lib, "libfimex_amd.so")
        fa.TUNING_LIB_PATH = os.path.join(args.lib, "libfimex_amd_tuning.so")
    seen = {}  # test function -> [hash of (label, array)]

    def hashing(identical):
        def wrapped(got, want, label):
            test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("[")[0]
            seen.setdefault(test, []).append(hashlib.sha256(label.encode() + np.ascontiguousarray(got).tobytes()).hexdigest())
            return identical(got, want, label)
        return wrapped

    # test_gpu_merge_vector takes _identical from test_gpu_merge, test_gpu_merge_vector_typed from test_gpu_merge_typed: wrap before they import it
    for name in TEST_MODULES:
        m = importlib.import_module(name)
        if name in ("test_gpu_merge", "test_gpu_merge_typed"):
            m._identical = hashing(m._identical)
    with contextlib.redirect_stdout(io.StringIO()) as log:
        rc = pytest.main(["-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"] + [os.path.join(ROOT, "tests", name + ".py") for name in TEST_MODULES])
    if rc != 0:
        sys.exit("the merge tests do not pass on this side:\n" + log.getvalue()[-3000:])
    for test, hashes in sorted(seen.items()):
        print(json.dumps({"case": "bits %s (%d arrays)" % (test, len(hashes)), "sha256": hashlib.sha256("".join(hashes).encode()).hexdigest()}), flush=True)

    for script, forms in BENCHES.items():
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "result.json")
            sys.argv = [script + ".py", "--out", out]
            with contextlib.redirect_stdout(io.StringIO()):
                importlib.import_module(script).main()
            with open(out) as f:
                r = json.load(f)["results"][0]
        for case, median_path, calls_path in forms:
            pick = lambda path: functools.reduce(lambda d, k: d[k], path, r)
            ms, left_out = pick(median_path), 0
            if calls_path:
                calls = pick(calls_path)
                kept = [c for c in calls if c <= STALL_MS]
                ms, left_out = statistics.median(kept), len(calls) - len(kept)
            print(json.dumps({"case": "time %s %s" % (script, case), "sha256": "not hashed: the script compares fused with chain itself",
                              "seconds": [ms / 1e3], "calls_above_0.4_s_left_out": left_out}), flush=True)


WHAT = ("Grid merging, the four forms (float, stored types, float vector pairs, packed vector pairs).  Bits: every array that the five "
        "test_gpu_merge*.py modules compare with an expectation, hashed per test function.  Time: the fused forms of scripts/bench_merge*.py "
        "and the typed elementwise kernels, the scripts' own medians (HIP events around one call), one figure per round.")

worker() if args.worker else compare_builds.drive(__file__, args, WHAT, worker_timeout=900)
