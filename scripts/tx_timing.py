"""Cost of the device transmitter (plx_tx_qpsk_dev) on a C1 batch: 1024 frames x 65 536 samples
(1024 symbols x 64 samples), HIP events around the calls, profiler off.  Reports
  - ms of plx_tx_qpsk_dev, and its split into k_tx_bits / k_tx_wave.  One C call is two launches and events cannot be put
    between them, so the split comes from a second call with the same symbols at nt = 2: the same k_tx_bits work and 1/32
    of k_tx_wave's stores, T(64) = B + W, T(2) = B + W / 32 (W taken as proportional to its bytes; an estimate, and said so)
  - bytes/s of k_tx_wave (32 B per dual-polarisation sample) as a fraction of 8 TB/s
  - ms of make_batch for the same batch with tx_data='random' (the call plus the gain) and with the de Bruijn waveforms:
    variants = 1 (one waveform repeated) and variants = 4 (the gather by frame index)
  - ms of the fibre step on that batch
Bounded: 1 warm-up and --reps timed runs of each.
usage: python scripts/tx_timing.py [--out profiles/tx_timing.json] [--frames 1024] [--reps 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


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


def main():
    import torch
    from polmux_amd import _abi, pipeline, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tx_timing.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    F, nsymb, nt = args.frames, 1024, 64
    lib, dev = _abi.get(), torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream

    # --- the C call alone, at nt = 64 and at nt = 2 ---
    def tx_call(nt_):
        n = nsymb * nt_
        ux = torch.empty((F, n), dtype=torch.complex128, device=dev)
        uy = torch.empty_like(ux)
        pat = torch.empty((F, 4, nsymb), dtype=torch.uint8, device=dev)
        pdq = torch.empty_like(pat)
        power = torch.empty(F, dtype=torch.float64, device=dev)
        drive = synth.qpsk_drive_tables(nt_)
        return lambda: lib.call("plx_tx_qpsk_dev", ux.data_ptr(), uy.data_ptr(), nsymb, nt_, 1, F, drive.ctypes.data, 2.0,
                                20260101, None, pat.data_ptr(), pdq.data_ptr(), power.data_ptr(), st), (ux, uy, pat, pdq, power)
    call64, keep64 = tx_call(nt)
    t64 = timed(torch, call64, args.reps)
    call2, keep2 = tx_call(2)
    t2 = timed(torch, call2, args.reps)
    del keep2
    wave = (t64 - t2) * nt / (nt - 2.0)
    bits = t64 - wave
    nbytes = F * nsymb * nt * 32
    res = dict(device=torch.cuda.get_device_name(0), frames=F, nsymb=nsymb, nt=nt, reps=args.reps,
               tx_call_ms=round(t64, 4), tx_call_nt2_ms=round(t2, 4), k_tx_wave_ms_est=round(wave, 4), k_tx_bits_ms_est=round(bits, 4),
               k_tx_wave_bytes=nbytes, k_tx_wave_tb_per_s=round(nbytes / (wave * 1e-3) / 1e12, 3),
               k_tx_wave_fraction_of_8tbs=round(nbytes / (wave * 1e-3) / HBM_BYTES_PER_S, 3))
    del keep64
    torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)

    # --- make_batch of the three transmitters, and the fibre step ---
    for name, kw in (("random", dict(tx_data="random")), ("debruijn_repeat", dict(variants=1)), ("debruijn_gather", dict(variants=4))):
        hp = pipeline.HotPath(pipeline.HotPathConfig(nsymb=nsymb, nt=nt, **kw), max_frames=F)
        res["make_batch_%s_ms" % name] = round(timed(torch, lambda: hp.make_batch(F), args.reps), 4)
        if name == "random":
            ux, uy = hp.make_batch(F)
            ux0, uy0 = ux.clone(), uy.clone()

            def step():
                ux.copy_(ux0)
                uy.copy_(uy0)
                hp.fibre(ux, uy)
            with_copy = timed(torch, step, args.reps)
            copy = timed(torch, lambda: (ux.copy_(ux0), uy.copy_(uy0)), args.reps)
            res["fibre_step_ms"] = round(with_copy - copy, 3)
            res["ncycle_max"] = int(np.max(hp.last_ncycle(F)))
            del ux, uy, ux0, uy0
        hp.close()
        del hp
        torch.cuda.empty_cache()
        print(json.dumps({k: v for k, v in res.items() if k.startswith(("make_batch", "fibre"))}), flush=True)
    res["tx_call_over_fibre_step"] = round(res["tx_call_ms"] / res["fibre_step_ms"], 4)
    res["tx_call_over_gather"] = round(res["tx_call_ms"] / res["make_batch_debruijn_gather_ms"], 3)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
