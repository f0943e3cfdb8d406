#!/usr/bin/env python3
"""Prints every pair of projection strings the CPU tests of the projections use, good and refused, one "source<TAB>target" per line:
the input of tests/projection_host_main.hip (the parser and the point math under sanitizers, see there)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import projection_cases as pc
from test_projection_host import REFUSALS

pairs = [(pc.GEO, dst) for dst in pc.ALL] + [(pc.GEO_W, dst) for dst in pc.ELLIPSOIDAL] + list(pc.DATUM_PAIRS)
pairs += [(pc.GEO_W if proj == pc.UTM33 else pc.GEO, proj + " " + extra) for proj in (pc.STERE, pc.UTM33) for extra in pc.UNIT_EXTRAS]
pairs += [(pc.GEO_W + " +pm=lisbon", pc.UTM33), (pc.GEO_W, "+proj=latlong +ellps=bessel")]
pairs += [(pc.GEO_W, bad) for bad, _ in REFUSALS] + [(bad, pc.GEO_W) for bad, _ in REFUSALS]
for src, dst in pairs:
    print(src + "\t" + dst)
