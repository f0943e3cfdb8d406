#!/usr/bin/env python3
"""Records tests/golden/derived_answers.npz, the pin of tests/derived_ref.py (tests/test_derived_ref.py).

Run from anywhere on a machine where build() found a reference tree:  python scripts/record_derived_answers.py
mifi_specific_to_relative_humidity is answered by the reference's own C code (oracle/_ref/libmifi_ref.so: its unmodified sources,
recipe in oracle/Makefile); the restatement has no say in that record.  ScaleValue, the theta2T loop, the packing to short and the
accumulation are C++ behind boost with no object code at hand: their records are the restatement's answers on the day of recording,
a pin against drift (numpy, the C library), not against the reference.  Inputs are generated from seeds by tests/derived_ref.py and
stored as passed, so that numpy's generators need not stay stable; float results are stored as bit patterns.  Keys:
  scaled.in.<IN>.v<variant>          values of the stored type IN (fimex_amd_datatype number)
  scaled.par.<IN>.<OUT>.v<variant>   oldFill, oldScale, oldOffset, newFill, newScale, newOffset
  scaled.out.<IN>.<OUT>.v<variant>   the converted values, as bytes
  humidity.{q,t,p}                   -> humidity.rh (float32 bits, the reference's object code), humidity.packed
  pack.rh                            -> pack.packed: values outside short, NaN
  theta.{theta,p,add_offset}         -> theta.T (float32 bits)
  accumulate.<type>.in               [nt][n] -> accumulate.<type>.acc, .deacc (float64 bits), whole batch from position 0
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import derived_ref as dr  # noqa: E402


def main():
    ref = dr.reference_lib()
    if ref is None:
        sys.exit("oracle/_ref/libmifi_ref.so is absent: build() found no reference tree")
    out = {}
    for variant in dr.RECORDED_SCALED_VARIANTS:
        for i in dr.TYPES:
            for o in dr.TYPES:
                par = dr.scaled_parameters(i, o, variant)
                x = dr.scaled_values(dr.DTYPES[i], dr.RECORDED_SCALED_N, 100 * variant + i, par[0])
                out["scaled.in.%d.v%d" % (i, variant)] = x
                out["scaled.par.%d.%d.v%d" % (i, o, variant)] = np.array(par, np.float64)
                out["scaled.out.%d.%d.v%d" % (i, o, variant)] = dr.as_bytes(dr.convert_scaled(x, par[0], par[1], par[2], o, par[3], par[4], par[5]))
    q, t, p = dr.recorded_humidity_inputs()
    rh = ref.specific_to_relative(q, t, p)
    out.update({"humidity.q": q, "humidity.t": t, "humidity.p": p, "humidity.rh": rh.view(np.uint32),
                "humidity.packed": dr.pack_relative_humidity(rh)})
    out.update({"pack.rh": dr.PACK_CASES, "pack.packed": dr.pack_relative_humidity(dr.PACK_CASES)})
    theta, p, off = dr.recorded_theta_inputs()
    out.update({"theta.theta": theta, "theta.p": p, "theta.add_offset": np.float32(off),
                "theta.T": dr.theta_to_temperature(theta, p, off).view(np.uint32)})
    for code in dr.RECORDED_ACCUMULATE_TYPES:
        x = dr.accumulate_input(300 + code, dr.DTYPES[code], 5, 37)
        out.update({"accumulate.%d.in" % code: x, "accumulate.%d.acc" % code: dr.accumulate(x).view(np.uint64),
                    "accumulate.%d.deacc" % code: dr.deaccumulate(x).view(np.uint64)})
    path = os.path.join(ROOT, "tests", "golden", dr.FIXTURE)
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
