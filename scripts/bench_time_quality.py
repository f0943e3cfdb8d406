#!/usr/bin/env python3
"""The entries of SURVEY 8f n10 on 2000 x 2000 cells, device-resident and HIP-event timed, in one call:
  time interpolation  25 hourly steps onto 145 ten-minute steps, as float and as packed short: fimex_amd_time_interpolate_device next
                      to the chain it replaces, one fimex_amd_get_values_1d_f_device(LINEAR_WEAK_EXTRAPOL) call per output step (for
                      the shorts behind one fimex_amd_data2interpolation_device over the series), and next to a device copy that moves
                      (nOld * sizeof(T) + nNew * 4) * n bytes.  The two results are compared bit for bit once.
  quality mask        65 levels of packed shorts against one 2-D status of unsigned bytes, "max:<limit>" with 1 %, 30 % and 100 % of
                      the cells masked, next to a device copy that moves the status bytes plus the data bytes the kernel touches
                      (32 per 16-byte group with some cells masked, 16 per group with all of them masked).
Within a case the candidates alternate, call by call, so that a drift of the machine hits all of them alike; the figures are medians
over --launches rounds after 3 warm-up rounds, and the spread is (max - min) / median of those rounds.  Writes profiles/time_quality.json
(or --out) and prints one JSON line per case.

usage: python scripts/bench_time_quality.py [--launches 10] [--out FILE]"""
import argparse, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NX = NY = 2000
N_OLD, N_NEW = 25, 145
NZ = 65
CDM_SHORT, CDM_FLOAT, CDM_UCHAR = 2, 4, 7


def alternating(torch, fns, reps, warm=3):
    """{name: (median ms, min ms, max ms)} of the callables, one call of each per round."""
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
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--launches", type=int, default=10)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_quality.json"))
    args = ap_.parse_args()
    import torch
    from fimex_amd import capi as fa
    fa.load(); fa.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    n = NX * NY
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    results = []
    device = torch.cuda.get_device_name(0)

    def stats(t, k, prefix):
        return {prefix + "ms_median": t[k][0], prefix + "ms_min": t[k][1], prefix + "ms_max": t[k][2], prefix + "spread": (t[k][2] - t[k][1]) / t[k][0]}

    # ---- time interpolation
    old = np.arange(N_OLD) * 3600.0
    new = np.arange(N_NEW) * 600.0
    t1, t2 = fa.time_mapping(old, new)
    series_f = (280.0 + 10.0 * torch.randn((N_OLD, n), device="cuda", generator=gen)).contiguous()
    series_s = torch.empty((N_OLD, n), dtype=torch.int16, device="cuda")
    fa.convert_scaled_device(series_f.data_ptr(), CDM_FLOAT, N_OLD * n, float("nan"), 1.0, 0.0, CDM_SHORT, -32767.0, 0.01, 273.15, series_s.data_ptr(),
                             stream=st)
    out_fused = torch.empty((N_NEW, n), dtype=torch.float32, device="cuda")
    out_chain = torch.empty((N_NEW, n), dtype=torch.float32, device="cuda")
    as_float = torch.empty((N_OLD, n), dtype=torch.float32, device="cuda")

    def chain(src):
        for i in range(N_NEW):
            a, b = int(t1[i]), int(t2[i])
            fa.get_values_1d_device(fa.BLEND_LINEAR_WEAK_EXTRAPOL, src[a].data_ptr(), src[b].data_ptr(), out_chain[i].data_ptr(), n, old[a], old[b],
                                    new[i], stream=st)

    def chain_short():
        fa.data2interpolation_device(series_s.data_ptr(), CDM_SHORT, N_OLD * n, float("nan"), as_float.data_ptr(), stream=st)
        chain(as_float)

    for label, series, code, elem, chain_fn, chain_slices in (
            ("float", series_f, CDM_FLOAT, 4, lambda: chain(series_f), "3 * nNew float slices, less one input per copy step"),
            ("packed short", series_s, CDM_SHORT, 2, chain_short, "nOld short + nOld float slices for the conversion, then 3 * nNew float slices")):
        alg = (N_OLD * elem + N_NEW * 4) * n
        src = torch.zeros(alg // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        fns = {"fused": lambda series=series, code=code: fa.time_interpolate_device(series.data_ptr(), code, n, old, new, out_fused.data_ptr(), stream=st),
               "chain": chain_fn, "copy": lambda: dst.copy_(src)}
        t = alternating(torch, fns, args.launches)
        del src, dst
        fns["fused"](); fns["chain"](); torch.cuda.synchronize()
        identical = bool(torch.equal(out_fused.view(torch.int32), out_chain.view(torch.int32)))
        spread = max((t[k][2] - t[k][1]) / t[k][0] for k in ("fused", "chain"))
        r = {"case": "time interpolation, " + label, "nx": NX, "ny": NY, "nOld": N_OLD, "nNew": N_NEW, "launches": args.launches,
             "algorithmic_bytes": alg, "algorithmic_bytes_formula": "(nOld*%d [in] + nNew*4 [out])*ny*nx" % elem, "chain_moves": chain_slices,
             "fused_TBps": alg / t["fused"][0] / 1e9, "copy_payload_bytes": alg // 2, "copy_TBps": alg / t["copy"][0] / 1e9,
             "fused_over_copy": t["fused"][0] / t["copy"][0], "fused_over_chain": t["fused"][0] / t["chain"][0],
             "spread_of_the_two": spread, "fused_not_slower_than_chain_beyond_spread": bool(t["fused"][0] <= t["chain"][0] * (1.0 + spread)),
             "fused_equals_chain_bit_for_bit": identical, "device": device}
        for k in fns:
            r.update(stats(t, k, k + "_"))
        print(json.dumps(r), flush=True)
        results.append(r)
    del series_f, series_s, out_fused, out_chain, as_float

    # ---- quality mask
    status = torch.randint(0, 100, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    data = torch.randint(-20000, 20000, (NZ, n), dtype=torch.int16, device="cuda", generator=gen)
    for share, limit in ((0.01, 98.0), (0.30, 69.0), (1.00, -1.0)):
        m = (status.float() > limit).view(-1, 8)  # the eight shorts of a lane's 16 bytes
        all_ = int(m.all(dim=1).sum()); some = int(m.any(dim=1).sum()) - all_
        touched = NZ * (32 * some + 16 * all_)
        alg = n + touched
        src = torch.zeros(alg // 2, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
        fns = {"mask": lambda limit=limit: fa.quality_mask_device(data.data_ptr(), CDM_SHORT, NZ * n, status.data_ptr(), CDM_UCHAR, n, fa.QUALITY_MAX,
                                                                  -32767.0, limit=limit, stream=st),
               "copy": lambda: dst.copy_(src)}
        t = alternating(torch, fns, args.launches)
        del src, dst
        r = {"case": "quality mask, %g %% masked" % (100 * share), "nx": NX, "ny": NY, "levels": NZ, "launches": args.launches,
             "masked_share_of_status": float(m.float().mean()), "groups_all_masked": all_, "groups_some_masked": some, "groups": n // 8,
             "touched_bytes": alg, "touched_bytes_formula": "ny*nx [status] + levels*(32*groups_some_masked + 16*groups_all_masked)",
             "data_bytes": 2 * NZ * n, "mask_TBps_of_touched": alg / t["mask"][0] / 1e9, "copy_payload_bytes": alg // 2,
             "copy_TBps": alg / t["copy"][0] / 1e9, "mask_over_copy": t["mask"][0] / t["copy"][0],
             "masked_share_of_data": float((data == -32767).float().mean()), "device": device}
        for k in fns:
            r.update(stats(t, k, k + "_"))
        print(json.dumps(r), flush=True)
        results.append(r)

    doc = {"script": "scripts/bench_time_quality.py",
           "timing": "HIP events around one call (the chain: around its 145 calls); the candidates of a case alternate call by call; median of the "
                     "rounds after 3 warm-up rounds; spread = (max - min) / median of the rounds",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
