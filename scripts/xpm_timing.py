"""Cost of the Manakov cross-phase modulation between 'sepfields' channels (PLX_SSFM_XPM_MANAKOV) on
the shape of BASELINE config[2]: 16 PDM-QPSK channels x 2^16 samples, 32 frames per batch, one 80-km span with PMD.  Three
fibre plans propagate the same batch: 'gps-' on the fused sweep (two sweeps per step), 'gps-' with PLX_SSFM_SHARE_DEVICE
(three sweeps per step: the step the XPM plan is built on) and 'gpsx' with the new flag (three sweeps + k_stokes_sum, the
Kerr load reading the 32-byte record).  Reports ms per span, steps, ms per step and the per-class kernel times of
plx_ssfm_kernel_times (0 = k_col_fwd / k_colx16, 1 = row pass, 2 = k_col_inv, 3 = control + k_stokes_sum + read-backs), and
the XPM step relative to the three-sweep step beside the 1.34 x estimate by bytes.  Bounded: 1 warm-up and 3 timed spans
per plan.
usage: python scripts/xpm_timing.py [--out FILE] [--frames F]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_EST = (192 + 32 + 32 / 16 + 32) / 192          # three sweeps + sum pass (read, write / nfc) + record read, over three sweeps


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
    plans = [("gps- fused", dict(flag="gps-")),
             ("gps- three sweeps", dict(flag="gps-", share_device=True)),
             ("gpsx xpm", dict(flag="gpsx", xpm_dualpol="manakov"))]
    rows = []
    for name, kw in plans:
        hp = pipeline.HotPath(pipeline.HotPathConfig(**base, **kw), max_frames=F)
        info = (C.c_int32 * 8)()
        hp.lib.call("plx_ssfm_info", hp.ssfm, info)
        ux0, uy0 = hp.make_batch(F)
        ux, uy = ux0.clone(), uy0.clone()
        hp.fibre(ux, uy)                                  # warm-up
        torch.cuda.synchronize()
        hp.lib.call("plx_ssfm_profile", hp.ssfm, 1)
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
            nc = np.zeros(F, np.int32)
            hp.lib.call("plx_ssfm_results", hp.ssfm, F, None, C.c_void_p(nc.ctypes.data))
            steps += int(nc.max())
        kms, kl = (C.c_double * 4)(), (C.c_int64 * 4)()
        hp.lib.call("plx_ssfm_kernel_times", hp.ssfm, kms, kl)
        r = dict(plan=name, fused=int(info[0]), frames=F, steps_per_span=steps // args.reps,
                 ms_per_span=round(ms_tot / args.reps, 3), ms_per_step=round(ms_tot / steps, 4),
                 class_ms_per_step=[round(kms[k] / steps, 4) for k in range(4)], class_launches=[int(kl[k]) for k in range(4)])
        rows.append(r)
        print(json.dumps(r), flush=True)
        hp.close()
        del ux, uy, ux0, uy0, hp
        torch.cuda.empty_cache()
    three, xpm = rows[1], rows[2]
    res = dict(device=torch.cuda.get_device_name(0), nfft=65536, nch=16, frames=F, rows=rows,
               xpm_over_three_sweeps=round(xpm["ms_per_step"] / three["ms_per_step"], 3), bytes_estimate=round(BYTES_EST, 3),
               xpm_over_fused=round(xpm["ms_per_step"] / rows[0]["ms_per_step"], 3))
    print(json.dumps({k: res[k] for k in ("xpm_over_three_sweeps", "bytes_estimate", "xpm_over_fused")}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
