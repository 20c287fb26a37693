"""Cost of the per-channel receiver of 'sepfields' WDM frames (HotPathConfig(wdm_receiver='channel')) on
the shape of BASELINE config[2]: 16 PDM-QPSK channels x 2^16 samples, 32 frames per batch.  Reports
  * the one plx_pick_wdm_dev launch (both polarisations, all channel-frames, a delay per channel) against the two
    plx_pick_dev calls it replaces: ms per call and bytes/s (16 B read and 16 B written per 2-sps sample);
  * plx_cde_apply_dev on the 2 F nch rows with 16 tables (plx_cde_create_wdm) against one table (plx_cde_create);
  * beside them one fibre() call of the plan (one 80-km span with PMD, 'gps-' on sixteen columns) and one receive().
HIP events, profiler off.  Bounded: 1 warm-up and --reps timed runs of each.  Run it under a time limit.
usage: python scripts/wdm_rx_timing.py [--out FILE] [--frames F] [--reps R]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8e12                  # B/s, the HBM figure the project's reports are relative to


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
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    F = args.frames
    base = dict(nsymb=1024, nt=64, nch=16, flag="gps-", manakov="yes", pavg_mw=1.0, length=8e4, dphimax=5e-3, dzmax=2e4,
                nplates=100, nspans=10)
    hp = pipeline.HotPath(pipeline.HotPathConfig(wdm_receiver="channel", **base), max_frames=F)
    cfg, lib, st = hp.cfg, hp.lib, hp.stream()
    n, nch, CF, Lrx, half = cfg.nfft, hp.nch, F * hp.nch, hp.Lrx, cfg.nt // 2
    res = dict(device=torch.cuda.get_device_name(0), nfft=n, nch=nch, frames=F, peak_bytes_per_s=PEAK,
               delay_symbols=[round(float(v), 2) for v in hp.rx_delay_symbols], delay_samples=[int(v) for v in hp.rx_delay])
    ux, uy = hp.make_batch(F)
    vx, vy, rx = ux.view(CF, n), uy.view(CF, n), hp.rx[:CF]
    kernels = {}
    b = 2 * 32 * Lrx * CF                                 # both polarisations: 16 B in, 16 B out per 2-sps sample

    def row(ms):
        return dict(ms=round(ms, 4), bytes=b, bytes_per_s=round(b / ms * 1e3, -9), of_peak=round(b / ms * 1e3 / PEAK, 4))

    def two():
        for pol, src in enumerate((vx, vy)):
            lib.call("plx_pick_dev", src.data_ptr(), rx.data_ptr() + pol * Lrx * 16, n, Lrx, 0, half, hp.rx_scale, CF, 2 * Lrx, st)
    kernels["two plx_pick_dev calls (sample 0)"] = row(timed(torch, two, args.reps))
    kernels["one plx_pick_wdm_dev launch (per-channel delay)"] = row(timed(torch, lambda: lib.call(
        "plx_pick_wdm_dev", vx.data_ptr(), vy.data_ptr(), rx.data_ptr(), n, Lrx, half, hp.rx_scale, nch, F,
        hp.rx_delay.ctypes.data, st), args.reps))
    zero = np.zeros(nch, np.int64)
    kernels["one plx_pick_wdm_dev launch (all delays 0)"] = row(timed(torch, lambda: lib.call(
        "plx_pick_wdm_dev", vx.data_ptr(), vy.data_ptr(), rx.data_ptr(), n, Lrx, half, hp.rx_scale, nch, F, zero.ctypes.data, st),
        args.reps))
    print(json.dumps(kernels), flush=True)

    # --- the equaliser: 16 tables against one ---
    N = min(cfg.fft_length, Lrx)
    one = C.c_void_p()
    H0 = np.ascontiguousarray(hp.cde_H[nch // 2]).view(np.float64)
    lib.call("plx_cde_create", C.byref(one), N, cfg.cde_L, H0.ctypes.data)
    cde = {}
    bc = 2 * 16 * Lrx * 2 * CF                            # every row read and written once, at the least
    for name, plan in (("one table (plx_cde_create)", one), ("%d tables (plx_cde_create_wdm)" % nch, hp.cde)):
        ms = timed(torch, lambda: lib.call("plx_cde_apply_dev", plan, rx.data_ptr(), hp.eq.data_ptr(), Lrx, 2 * CF, st), args.reps)
        cde[name] = dict(ms=round(ms, 4), rows=2 * CF, bytes_at_least=bc, bytes_per_s_at_least=round(bc / ms * 1e3, -9))
    lib.call("plx_cde_destroy", one)
    res["kernels"], res["cde_apply"] = kernels, cde
    print(json.dumps(cde), flush=True)

    # --- beside them: one span of the fibre and the whole receiver ---
    wx, wy = ux.clone(), uy.clone()
    sav = cfg.nspans
    cfg.nspans = 1                                        # (one span is the yardstick: the receive side is per batch, not per span)
    res["fibre_ms_per_span"] = round(timed(torch, lambda: (wx.copy_(ux), wy.copy_(uy), hp.fibre(wx, wy)), 2), 3)
    cfg.nspans = sav
    res["receive_ms"] = round(timed(torch, lambda: hp.receive(wx, wy), 2), 3)
    print(json.dumps({k: res[k] for k in ("fibre_ms_per_span", "receive_ms")}), flush=True)
    hp.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
