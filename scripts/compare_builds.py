"""Driver of the scripts that compare two builds of the library on the GPU (compare_staged2_builds.py, compare_projection_builds.py, compare_forward_builds.py, compare_gather_builds.py).

The comparing script is its own worker: `script --worker [--lib DIR]` loads this tree's library, or the one in DIR, runs every case
once and prints one JSON line per case: {"case": name, "sha256": of the output bytes} and, for a timed case, "seconds": the timed
launches.  drive() alternates the two sides, one fresh process per side and round under a time limit of its own, and stops at the
first process that does not end normally.  Per timed case and round the minimum of the launches counts, then the median over the
rounds.  Margin: new median - parent median <= the parent's own (max - min) over its rounds.  The sha256 of a case must be one value,
the same on both sides, in every round.
"""
import json, os, statistics, subprocess, sys


def add_arguments(ap, default_out):
    ap.add_argument("--parent", help="directory with the other build's libfimex_amd.so")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=default_out)
    ap.add_argument("--parent-commit", default="parent")
    ap.add_argument("--worker", action="store_true", help="one side, one round: prints a JSON line per case")
    ap.add_argument("--lib", default=None, help="worker: directory of the library to load instead of this tree's")


def drive(script, args, what, worker_timeout=300):
    """script: the comparing script's own path; args: what add_arguments parsed; what: the first sentences of the result's "what"."""
    sides = {"parent": ["--lib", os.path.abspath(args.parent)], "new": []}
    runs = {s: {} for s in sides}  # side -> case -> list of rounds
    for rnd in range(args.rounds):
        for side, extra in sides.items():
            try:
                r = subprocess.run([sys.executable, os.path.abspath(script), "--worker"] + extra, capture_output=True, text=True, timeout=worker_timeout)
            except subprocess.TimeoutExpired:
                sys.exit("round %d, %s: no end after %d s" % (rnd, side, worker_timeout))
            if r.returncode != 0:
                sys.exit("round %d, %s: exit %d\n%s" % (rnd, side, r.returncode, r.stderr[-2000:]))
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    c = json.loads(line)
                    runs[side].setdefault(c["case"], []).append(c)
            print("round", rnd, side, "done", flush=True)
    cases, ok = {}, True
    for case in runs["new"]:
        e = {}
        timed = "seconds" in runs["new"][case][0]
        for side in sides:
            e[side] = {}
            if timed:
                mins = [min(c["seconds"]) for c in runs[side][case]]
                e[side] = {"rounds_seconds_min": mins, "rounds_seconds_all": [c["seconds"] for c in runs[side][case]], "median": statistics.median(mins),
                           "spread": max(mins) - min(mins)}
            e[side]["sha256"] = sorted({c["sha256"] for c in runs[side][case]})
        if timed:
            e["new_minus_parent"] = e["new"]["median"] - e["parent"]["median"]
            e["within_margin"] = e["new_minus_parent"] <= e["parent"]["spread"]
            ok = ok and e["within_margin"]
        e["same_bits"] = len(e["parent"]["sha256"]) == 1 and e["parent"]["sha256"] == e["new"]["sha256"]
        ok = ok and e["same_bits"]
        cases[case] = e
        if timed:
            print(case, "parent %.4f ms  new %.4f ms  margin %.4f ms  same bits %s" % (e["parent"]["median"] * 1e3, e["new"]["median"] * 1e3,
                                                                                      e["parent"]["spread"] * 1e3, e["same_bits"]), flush=True)
        elif not e["same_bits"]:
            print(case, "bits differ", flush=True)
    what += ("  Commit %s against this tree, alternating in one GPU call: one fresh process per side and round runs every case; per timed case "
             "and round the minimum of its launches, then the median over rounds.  Margin: new median - parent median <= parent's (max - min) "
             "over its rounds.  sha256: of the output's bytes; one value on both sides means the same bits in every round." % args.parent_commit)
    with open(args.out, "w") as f:
        json.dump({"what": what, "device": "MI355X", "rounds": args.rounds, "all_within_margin_and_same_bits": ok, "cases": cases}, f, indent=1)
        f.write("\n")
    print("all within margin and same bits:", ok, flush=True)
