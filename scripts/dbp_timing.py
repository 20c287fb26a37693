"""Timing of digital backpropagation (plx_dbp_apply_dev) on the config-1 receive batch: 1024 frames x 2048 samples per
polarisation, 80 km spans, CNLSE step.  Reports ms per call at 1, 2, 4 and 8 steps per span over 1 and 10 spans, for the
resident route, the forced streamed route (PLX_DBP_STREAMED) and, as the yardstick, plx_cde_apply_dev on the same batch;
and the FP64 rate each DBP route achieves under a counted-flop model, as a fraction of the 78.6 TFLOP/s peak bench.py
uses.  Flop model per frame and step: two polarisations x (forward + inverse FFT at 5 N log2 N each + the spectral
multiply, 6 N) + the Kerr step, 20 N (powers, phase, rotation; sin/cos not counted).  Run time is bounded: each case is
timed with 2 warm-up and 5 timed calls.
usage: python scripts/dbp_timing.py [--out FILE]"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64 = 78.6e12


def main():
    import torch
    from polmux_amd import _abi
    from polmux_amd.dbp import DbpPlan, dbp_betat, dbp_desc
    from polmux_amd.rx import cde_transfer
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    F, N, L, fs = 1024, 2048, 8e4, 56e9
    alpha, gam = math.log(10) * 1e-4 * 0.2, 1.368e-6
    bt = dbp_betat(N, fs, 1550e-9, 17e-6, 0.0)
    rng = np.random.default_rng(1)
    u = (rng.standard_normal((F, 2, N)) + 1j * rng.standard_normal((F, 2, N))) * math.sqrt(2.0)
    x = torch.from_numpy(u).cuda()
    out = torch.empty_like(x)
    sc = torch.full((F,), 1.0, dtype=torch.float64, device=x.device)
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn, reps=5, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / reps

    lib = _abi.get()
    H = np.ascontiguousarray(cde_transfer(256, fs, 1550e-9, 10 * L, 17e-6, 0.0)).view(np.float64)
    cde = C.c_void_p()
    lib.call("plx_cde_create", C.byref(cde), 256, 128, H.ctypes.data)
    ms_cde = timed(lambda: lib.call("plx_cde_apply_dev", cde, x.data_ptr(), out.data_ptr(), N, 2 * F, stream))
    lib.call("plx_cde_destroy", cde)
    rows = []
    flop_step = F * (2 * (2 * 5 * N * math.log2(N) + 6 * N) + 20 * N)
    for nspans in (1, 10):
        for steps in (1, 2, 4, 8):
            r = dict(nspans=nspans, steps_per_span=steps)
            for route, streamed in (("resident", False), ("streamed", True)):
                plan = DbpPlan(dbp_desc(N, F, nspans, steps, 0, L, alpha, gam, 1.0, bt), streamed=streamed)
                ms = timed(lambda: plan.apply(x, out, sc, stream))
                plan.close()
                r[route + "_ms"] = round(ms, 4)
                r[route + "_fp64_frac"] = round(flop_step * nspans * steps / (ms * 1e-3) / PEAK_FP64, 4)
            r["streamed_over_resident"] = round(r["streamed_ms"] / r["resident_ms"], 2)
            r["resident_over_cde"] = round(r["resident_ms"] / ms_cde, 2)
            rows.append(r)
            print(json.dumps(r), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), frames=F, nfft=N, span_m=L, cde_ms=round(ms_cde, 4),
               peak_fp64=PEAK_FP64, rows=rows)
    print(json.dumps(dict(cde_ms=res["cde_ms"])))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
