"""Cost of the device Tx filter (plx_tx_bandlimit_dev), HIP events around the calls after a warm-up,
profiler off.  Two batches of 1024 symbols x 64 samples:
  - production: 512 frames, one channel (512 pairs of 65 536 samples)
  - comb: --comb-frames frames of five channels as ONE field (wdm_field='unique'; 100 frames = 500 pairs)
For each it reports
  - ms of plx_tx_bandlimit_dev on the batch's pairs (two filter passes and the two new kernels)
  - ms of the two filter passes alone (plx_filter_apply_dev on the X rows and on the Y rows, the same plan), and from the
    difference the ms of k_txf_tile_power + k_txf_scale.  One C call is four launches and events cannot be put between them:
    the split is an estimate, and said so
  - bytes/s of the two new kernels from 96 B per sample pair (32 B read by the first, 64 B read and written by the second),
    and that as a fraction of 8 TB/s
  - beside them, ms of plx_tx_qpsk_dev on the same batch and of one fibre() call
Bounded: 1 warm-up and --reps timed runs of each.
usage: python scripts/tx_filter_timing.py [--out profiles/tx_filter_timing.json] [--frames 512] [--comb-frames 100] [--reps 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
BYTES_PER_SAMPLE_PAIR = 96


def timed(torch, fn, reps):
    """ms per call of fn() by HIP events: one warm-up, then reps calls between one pair of events"""
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def measure(torch, pipeline, name, F, reps, **kw):
    cfg = pipeline.HotPathConfig(nsymb=1024, nt=64, tx_data="random", tx_filter=dict(ftype="ideal", bw=1.6), **kw)
    hp = pipeline.HotPath(cfg, max_frames=F)
    try:
        lib, st, nch, n = hp.lib, hp.stream(), hp.nch, cfg.nfft
        npairs = F * nch
        ux, uy = hp.make_batch(F)                      # (its tensors are this batch's: the calls below write into them again)
        px, py = ux.data_ptr(), uy.data_ptr()
        tx = timed(torch, lambda: lib.call("plx_tx_qpsk_dev", px, py, cfg.nsymb, cfg.nt, nch, F, hp.tx_drive.ctypes.data,
                                           float(cfg.pavg_mw), pipeline.MASTER_SEED, None, hp.pat_frames.data_ptr(), hp.dpat_frames.data_ptr(),
                                           hp.tx_power.data_ptr(), st), reps)
        bl = timed(torch, lambda: lib.call("plx_tx_bandlimit_dev", hp.txfilt, px, py, npairs, float(cfg.pavg_mw),
                                           hp.tx_gain.data_ptr(), hp._txfilt_work.data_ptr(), st), reps)
        fl = timed(torch, lambda: (lib.call("plx_filter_apply_dev", hp.txfilt, px, npairs, st),
                                   lib.call("plx_filter_apply_dev", hp.txfilt, py, npairs, st)), reps)
        bl2 = timed(torch, lambda: lib.call("plx_tx_bandlimit_dev", hp.txfilt, px, py, npairs, float(cfg.pavg_mw),
                                            hp.tx_gain.data_ptr(), hp._txfilt_work.data_ptr(), st), reps)
        kern = 0.5 * (bl + bl2) - fl
        nbytes = npairs * n * BYTES_PER_SAMPLE_PAIR
        res = dict(batch=name, frames=F, nch=nch, pairs=npairs, nfft=n, reps=reps,
                   bandlimit_ms=round(bl, 4), bandlimit_again_ms=round(bl2, 4), filter_passes_ms=round(fl, 4),
                   new_kernels_ms_est=round(kern, 4), new_kernels_bytes=nbytes,
                   new_kernels_tb_per_s_est=round(nbytes / (kern * 1e-3) / 1e12, 3) if kern > 0 else None,
                   new_kernels_fraction_of_8tbs_est=round(nbytes / (kern * 1e-3) / HBM_BYTES_PER_S, 3) if kern > 0 else None,
                   tx_qpsk_ms=round(tx, 4))
        print(json.dumps(res), flush=True)
        ux, uy = hp.make_batch(F)
        ux0, uy0 = ux.clone(), uy.clone()

        def step():
            ux.copy_(ux0)
            uy.copy_(uy0)
            hp.fibre(ux, uy)
        freps = max(1, min(reps, 3))
        with_copy = timed(torch, step, freps)
        copy = timed(torch, lambda: (ux.copy_(ux0), uy.copy_(uy0)), freps)
        res["fibre_ms"] = round(with_copy - copy, 3)
        res["bandlimit_over_fibre"] = round(bl / res["fibre_ms"], 4)
        res["bandlimit_over_tx_qpsk"] = round(bl / tx, 3)
        print(json.dumps(res), flush=True)
        return res
    finally:
        hp.close()
        torch.cuda.empty_cache()


def main():
    import torch
    from polmux_amd import pipeline
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx_filter_timing.json"))
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--comb-frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the MI355X: nothing is measured without it"
    out = dict(device=torch.cuda.get_device_name(0))
    out["production"] = measure(torch, pipeline, "production", args.frames, args.reps)
    out["comb"] = measure(torch, pipeline, "comb", args.comb_frames, args.reps, nch=5, wdm_field="unique")
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
