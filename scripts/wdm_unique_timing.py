"""Cost of a WDM frame as ONE field (HotPathConfig(wdm_field='unique')) on the shape of BASELINE
config[2]: 16 PDM-QPSK channels x 2^16 samples, 32 frames per batch, one 80-km span with PMD.  Reports
  * k_wdm_mux and k_wdm_select alone: ms per call and bytes/s (mux reads 32 nch + writes 32 B per sample, select reads 32 +
    writes 32 nch), as a fraction of 8 TB/s, beside k_stokes_sum's measured rate;
  * the channel-filter pass of the 'pick' receiver (plx_filter_apply_dev over the 2 F nch rows);
  * the fibre: ms per span and steps of the one field ('gps-' on one column; mux and select included) beside 'gps-' and
    'gpsx' on sixteen separate columns at the same dphimax.
HIP events, profiler off.  Bounded: 1 warm-up and --reps timed runs of each.  Run it under a time limit.
usage: python scripts/wdm_unique_timing.py [--out FILE] [--frames F] [--reps R]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12                  # B/s, the HBM figure the project's reports are relative to
STOKES_SUM = 4.7e12          # B/s, k_stokes_sum as measured


def timed(torch, fn, reps):
    fn()                                                  # warm-up
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    import torch
    from polmux_amd import pipeline
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    F = args.frames
    base = dict(nsymb=1024, nt=64, nch=16, manakov="yes", pavg_mw=1.0, length=8e4, dphimax=5e-3, dzmax=2e4, nplates=100)
    n, nch = 65536, 16
    res = dict(device=torch.cuda.get_device_name(0), nfft=n, nch=nch, frames=F, peak_bytes_per_s=PEAK,
               stokes_sum_bytes_per_s=STOKES_SUM)

    # --- the one field ---
    hp = pipeline.HotPath(pipeline.HotPathConfig(flag="gps-", wdm_field="unique", **base), max_frames=F)
    st = hp.stream()
    ux0, uy0 = hp.make_batch(F)
    ux, uy = ux0.clone(), uy0.clone()
    sh, dl = hp.wdm_shift, hp.wdm_delay
    res["shift_bins"], res["delay_samples"] = [int(v) for v in sh], [int(v) for v in dl]
    kernels = {}
    ms = timed(torch, lambda: hp.lib.call("plx_wdm_mux_dev", ux0.data_ptr(), uy0.data_ptr(), hp.wx.data_ptr(), hp.wy.data_ptr(),
                                          n, nch, F, sh.ctypes.data, st), 10)
    b = (32 * nch + 32) * n * F
    kernels["k_wdm_mux"] = dict(ms=round(ms, 4), bytes=b, bytes_per_s=round(b / ms * 1e3, -9), of_peak=round(b / ms * 1e3 / PEAK, 3))
    ms = timed(torch, lambda: hp.lib.call("plx_wdm_select_dev", hp.wx.data_ptr(), hp.wy.data_ptr(), ux.data_ptr(), uy.data_ptr(),
                                          n, nch, F, sh.ctypes.data, dl.ctypes.data, st), 10)
    kernels["k_wdm_select"] = dict(ms=round(ms, 4), bytes=b, bytes_per_s=round(b / ms * 1e3, -9), of_peak=round(b / ms * 1e3 / PEAK, 3))

    def chfilt():
        for src in (ux, uy):
            hp.lib.call("plx_filter_apply_dev", hp.chfilt, src.data_ptr(), F * nch, st)
    ms = timed(torch, chfilt, 5)
    b = 2 * 32 * nch * n * F                               # every row read and written once, at the least
    kernels["channel filter (plx_filter, 2 F nch rows)"] = dict(ms=round(ms, 4), bytes_at_least=b,
                                                                bytes_per_s_at_least=round(b / ms * 1e3, -9))
    res["kernels"] = kernels
    print(json.dumps(kernels), flush=True)

    rows = []

    def fibre_row(name, hp, ux0, uy0):
        ux, uy = ux0.clone(), uy0.clone()
        info = (C.c_int32 * 8)()
        hp.lib.call("plx_ssfm_info", hp.ssfm, info)
        hp.fibre(ux, uy)                                  # warm-up
        torch.cuda.synchronize()
        ms_tot, steps = 0.0, 0
        for _ in range(args.reps):
            ux.copy_(ux0)
            uy.copy_(uy0)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            hp.fibre(ux, uy)
            t1.record()
            torch.cuda.synchronize()
            ms_tot += t0.elapsed_time(t1)
            nc = hp.last_ncycle(F)
            steps += int(nc.max())
        r = dict(plan=name, fused=int(info[0]), columns=hp.nfc, frames=F, steps_per_span=steps // args.reps,
                 steps_min_max=[int(nc.min()), int(nc.max())], ms_per_span=round(ms_tot / args.reps, 3),
                 ms_per_step=round(ms_tot / steps, 4))
        rows.append(r)
        print(json.dumps(r), flush=True)

    fibre_row("unique gps- (mux + one column + select)", hp, ux0, uy0)
    hp.close()
    del ux, uy, ux0, uy0, hp
    torch.cuda.empty_cache()
    for name, kw in (("sepfields gps-", dict(flag="gps-")), ("sepfields gpsx xpm", dict(flag="gpsx", xpm_dualpol="manakov"))):
        hp = pipeline.HotPath(pipeline.HotPathConfig(**base, **kw), max_frames=F)
        ux0, uy0 = hp.make_batch(F)
        fibre_row(name, hp, ux0, uy0)
        hp.close()
        del ux0, uy0, hp
        torch.cuda.empty_cache()
    res["rows"] = rows
    res["unique_over_sepfields"] = round(rows[0]["ms_per_span"] / rows[1]["ms_per_span"], 3)
    res["unique_over_xpm"] = round(rows[0]["ms_per_span"] / rows[2]["ms_per_span"], 3)
    print(json.dumps({k: res[k] for k in ("unique_over_sepfields", "unique_over_xpm")}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
