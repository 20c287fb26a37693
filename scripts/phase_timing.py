"""Timing of laser phase noise (plx_phase_noise_dev) on the config-1 batch: 1024 frames of 65536 samples.  Reports ms per
call of the transmitter rotation (both polarisations, two passes), the LO at the 2-sps pick instants and the LO phase
written for the cohmix route (set these against bench.py's ms_per_step of the same batch).  Each case is timed with 2
warm-up and 5 timed calls between device events.  Run under rocprofv3 --kernel-trace --stats for the
per-kernel times of k_phase_tile_sums and k_phase_apply.
usage: python scripts/phase_timing.py [--frames F] [--out FILE]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, warm=2, reps=5):
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    import torch
    from polmux_amd import _abi, pipeline
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    F = args.frames
    cfg = pipeline.HotPathConfig(tx_linewidth=1e-4, lo_linewidth=1e-4)
    hp = pipeline.HotPath(cfg, max_frames=F)
    n, half = cfg.nfft, cfg.nt // 2
    ux, uy = hp.make_batch(F)
    keys = list(range(F))
    res = dict(frames=F, nfft=n)
    res["tx_rotation_ms"] = _time(lambda: hp._phase(ux.data_ptr(), uy.data_ptr(), 1, n, 1.0, F, keys, _abi.PLX_PHASE_TX,
                                                    cfg.tx_linewidth, None))
    rx = hp.rx[:F]
    res["lo_pick_ms"] = _time(lambda: hp._phase(rx.data_ptr(), rx.data_ptr() + hp.Lrx * 16, half, 2 * hp.Lrx, -1.0, F, keys,
                                                _abi.PLX_PHASE_LO, cfg.lo_linewidth, None))
    phi = torch.empty((F, n), dtype=torch.float64, device=hp.dev)
    res["lo_phase_out_ms"] = _time(lambda: hp._phase(None, None, 1, n, 1.0, F, keys, _abi.PLX_PHASE_LO, cfg.lo_linewidth,
                                                     None, phi.data_ptr()))
    del phi
    sweep_bytes = 2 * 2 * 16 * n * F                      # read + write of both polarisations
    res["tx_rotation_GBps"] = sweep_bytes / (res["tx_rotation_ms"] * 1e-3) / 1e9
    hp.close()
    line = json.dumps({k: (round(v, 4) if isinstance(v, float) and math.isfinite(v) else v) for k, v in res.items()})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
