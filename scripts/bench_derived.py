#!/usr/bin/env python3
"""The entries of SURVEY 8f n9 on 65 levels of 2000 x 2000, device-resident and HIP-event timed, in one call:
  scaled conversion short -> float and float -> short, each next to the existing fimex_amd_data2interpolation_device /
  fimex_amd_interpolation2data_device on the same types and count (the nearest code of the parent: the same bytes, less arithmetic);
  theta2T and specific2relative, with hybrid levels (ps) and with a pressure field;
  accumulate over 8 steps of one such field in float.
Every case is timed against a device-to-device copy that moves its algorithmic bytes (half read, half written).  Within a case the
candidates alternate, call by call, so that a drift of the machine hits all of them alike; the figures are medians over --launches
rounds after 3 warm-up rounds.  Repeat the command to see the spread between runs.  Writes profiles/derived.json (or --out) and prints
one JSON line per case.

usage: python scripts/bench_derived.py [--launches 20] [--out FILE]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NX = NY = 2000
NZ = 65
STEPS = 8
CDM_SHORT, CDM_FLOAT = 2, 4


def alternating(torch, fns, reps, warm=3):
    """{name: (median ms, min ms)} of the callables, one call of each per round."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in ts.items()}


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--launches", type=int, default=20)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "derived.json"))
    args = ap_.parse_args()
    import torch
    from fimex_amd import capi as fa
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    plane, vol = NX * NY, NX * NY * NZ
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    results = []

    def case(name, alg, formula, fns, result, extra=None):
        src = torch.zeros(alg // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        fns = dict(fns)
        fns["copy"] = lambda: dst.copy_(src)
        t = alternating(torch, fns, args.launches)
        del src, dst
        first = next(iter(fns))
        r = {"case": name, "levels": NZ, "nx": NX, "ny": NY, "launches": args.launches, "algorithmic_bytes": alg,
             "algorithmic_bytes_formula": formula, "ms_median": t[first][0], "ms_min": t[first][1], "TBps": alg / t[first][0] / 1e9,
             "copy_payload_bytes": alg // 2, "copy_ms_median": t["copy"][0], "copy_ms_min": t["copy"][1], "copy_TBps": alg / t["copy"][0] / 1e9,
             "kernel_over_copy": t[first][0] / t["copy"][0], "device": torch.cuda.get_device_name(0)}
        for k in fns:
            if k not in (first, "copy"):
                r.update({"counterpart": k, "counterpart_ms_median": t[k][0], "counterpart_ms_min": t[k][1],
                          "kernel_over_counterpart": t[first][0] / t[k][0]})
        r.update(extra or {})
        r.update(result())
        print(json.dumps(r), flush=True)
        results.append(r)

    # ---- scaled conversion: packed temperature (0.01 K steps, offset 273.15 K) to float and back
    eta = ((torch.arange(NZ, dtype=torch.float32, device="cuda") + 0.5) / NZ)[:, None, None]
    T = (210.0 + 80.0 * eta + 2.0 * torch.randn((NZ, NY, NX), device="cuda", generator=gen)).contiguous()
    packed = torch.empty((NZ, NY, NX), dtype=torch.int16, device="cuda")
    fa.convert_scaled_device(T.data_ptr(), CDM_FLOAT, vol, float("nan"), 1.0, 0.0, CDM_SHORT, -32767.0, 0.01, 273.15, packed.data_ptr(), stream=st)
    packed.view(-1)[::1009] = -32767
    f_new, f_old = torch.empty_like(T), torch.empty_like(T)
    case("scaled conversion short -> float", 6 * vol, "nz*ny*nx*(2 [in] + 4 [out])",
         {"convert_scaled": lambda: fa.convert_scaled_device(packed.data_ptr(), CDM_SHORT, vol, -32767.0, 0.01, 273.15, CDM_FLOAT, float("nan"),
                                                             1.0, 0.0, f_new.data_ptr(), stream=st),
          "fimex_amd_data2interpolation_device (no scale, no offset)":
              lambda: fa.data2interpolation_device(packed.data_ptr(), CDM_SHORT, vol, -32767.0, f_old.data_ptr(), stream=st)},
         lambda: {"nan_share_of_output": float(torch.isnan(f_new).float().mean()), "output_min": float(torch.nan_to_num(f_new, 1e9).min()),
                  "output_max": float(torch.nan_to_num(f_new, -1e9).max())})
    s_new, s_old = torch.empty_like(packed), torch.empty_like(packed)
    case("scaled conversion float -> short", 6 * vol, "nz*ny*nx*(4 [in] + 2 [out])",
         {"convert_scaled": lambda: fa.convert_scaled_device(f_new.data_ptr(), CDM_FLOAT, vol, float("nan"), 1.0, 0.0, CDM_SHORT, -32767.0, 0.01,
                                                             273.15, s_new.data_ptr(), stream=st),
          "fimex_amd_interpolation2data_device (no scale, no offset)":
              lambda: fa.interpolation2data_device(f_new.data_ptr(), vol, CDM_SHORT, -32767.0, s_old.data_ptr(), stream=st)},
         lambda: {"round_trip_identical_share": float((s_new == packed).float().mean())})
    del packed, f_old, s_new, s_old, f_new

    # ---- theta2T and specific2relative
    jj = torch.arange(NY, dtype=torch.float32, device="cuda")[:, None]
    ii = torch.arange(NX, dtype=torch.float32, device="cuda")[None, :]
    ps = (600.0 + 440.0 * (0.5 + 0.5 * torch.sin(0.011 * ii) * torch.cos(0.007 * jj))).reshape(1, NY, NX).contiguous()  # hPa
    e = (np.arange(NZ) + 0.5) / NZ
    b = e ** 2
    hybrid = fa.VerticalLevels.hybrid_sigma_ap(1000.0 * (e - b) + 0.1, b, ps.data_ptr())
    pfield = torch.empty((1, NZ, NY, NX), dtype=torch.float32, device="cuda")
    fa.vertical_levels_device(hybrid, NX, NY, 1, pfield.data_ptr(), stream=st)
    field = fa.VerticalLevels.from_field(pfield.data_ptr(), NZ)
    q = (0.015 * eta ** 3 * torch.rand((NZ, NY, NX), device="cuda", generator=gen)).contiguous()
    theta = (T * (1000.0 / pfield[0]) ** 0.2857).contiguous()
    out = torch.empty_like(T)
    rh = torch.empty((NZ, NY, NX), dtype=torch.int16, device="cuda")
    for label, lv, pbytes, pform in (("hybrid levels", hybrid, 4 * plane, "1 [ps]"), ("pressure field", field, 4 * vol, "nz [p]")):
        case("theta2T, " + label, 8 * vol + pbytes, "4*ny*nx*(nz [theta] + nz [T] + %s)" % pform,
             {"theta_to_temperature": lambda lv=lv: fa.theta_to_temperature_device(lv, NX, NY, 1, theta.data_ptr(), 0.0, out.data_ptr(), stream=st)},
             lambda: {"finite_share_of_output": float(torch.isfinite(out).float().mean()), "output_min": float(out.min()),
                      "output_max": float(out.max())})
        case("specific2relative, " + label, 10 * vol + pbytes, "ny*nx*(4*nz [q] + 4*nz [T] + 2*nz [rh] + 4*%s)" % pform,
             {"specific_to_relative_humidity": lambda lv=lv: fa.specific_to_relative_humidity_device(lv, NX, NY, 1, q.data_ptr(), T.data_ptr(),
                                                                                                    rh.data_ptr(), stream=st)},
             lambda: {"output_min": int(rh.min()), "output_max": int(rh.max()), "mean_relative_humidity": float(rh.float().mean()) / 25000.0})
    del theta, out, rh, q, pfield, T

    # ---- accumulate
    x = torch.rand((STEPS, vol), device="cuda", generator=gen)
    acc = torch.empty((STEPS, vol), dtype=torch.float64, device="cuda")
    case("accumulate, %d steps of float" % STEPS, 12 * vol * STEPS, "steps*nz*ny*nx*(4 [in] + 8 [out])",
         {"accumulate": lambda: fa.accumulate_device(x.data_ptr(), CDM_FLOAT, vol, STEPS, 0, None, acc.data_ptr(), stream=st)},
         lambda: {"output_max": float(acc.max())}, {"steps": STEPS})

    doc = {"script": "scripts/bench_derived.py",
           "timing": "HIP events around one call; the candidates of a case alternate call by call; median of the rounds after 3 warm-up rounds",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
