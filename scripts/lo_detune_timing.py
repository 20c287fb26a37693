"""Timing of the LO frequency offset (plx_lo_detune_dev, HotPathConfig(lo_detuning, lo_detuning_spread)) at the shapes of
BASELINE config[1] (1024 frames of 2^16 samples) and config[2] (32 frames of 16 channels x 2^16).  Reports, per shape, ms per
call of the apply launch on the 2-sps samples (the pick route), of the d_phi launch (write and accumulate: the cohmix route)
with its algorithmic bytes as a fraction of 8 TB/s, and of one receive() of the batch with and without the option (pick front
end, transmitter fields: no fibre in the timed region).  HIP events, no profiler, one warm-up call, 5 timed calls.
usage: python scripts/lo_detune_timing.py [--shape 1|2|both] [--no-receive] [--out FILE]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BPS = 8e12


def _time(fn, warm=1, reps=5):
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


def kernels(lib, nfft, nch, F, nt):
    """the two launches on buffers of their own, offsets drawn on the device (K = 3) under the frame index"""
    import torch
    from polmux_amd import pipeline
    CF, half, Lrx = F * nch, nt // 2, 2 * nfft // nt
    st = torch.cuda.current_stream().cuda_stream
    rx = torch.ones((CF, 2, Lrx), dtype=torch.complex128, device="cuda")
    phi = torch.zeros((CF, nfft), dtype=torch.float64, device="cuda")
    bins = torch.zeros(CF, dtype=torch.int32, device="cuda")

    def call(pu, pv, stride, pitch, sign, pphi, acc):
        lib.call("plx_lo_detune_dev", pu, pv, stride, pitch, sign, nfft, nch, F, 2, 3, pipeline.MASTER_SEED, None, None, pphi,
                 acc, bins.data_ptr(), st)

    res = {}
    res["apply_ms"] = _time(lambda: call(rx.data_ptr(), rx.data_ptr() + Lrx * 16, half, 2 * Lrx, -1.0, None, 0))
    res["phi_write_ms"] = _time(lambda: call(None, None, 1, nfft, 1.0, phi.data_ptr(), 0))
    res["phi_accumulate_ms"] = _time(lambda: call(None, None, 1, nfft, 1.0, phi.data_ptr(), 1))
    nbytes = 8 * CF * nfft
    res["phi_bytes"] = nbytes
    res["phi_write_of_peak"] = nbytes / (res["phi_write_ms"] * 1e-3) / PEAK_BPS
    res["phi_accumulate_of_peak"] = 2 * nbytes / (res["phi_accumulate_ms"] * 1e-3) / PEAK_BPS
    res["apply_bytes"] = 2 * 2 * 16 * CF * Lrx                            # read + write of both polarisations
    return res


def receives(nch, F, kw):
    """one receive() of the batch's transmitter fields, without and with the option (fresh plans, same data)"""
    import torch
    from polmux_amd import pipeline
    res = {}
    for name, opt in (("receive_ms", {}), ("receive_detuned_ms", dict(lo_detuning=2.5 * 28e9 / 1024, lo_detuning_spread=3.5 * 28e9 / 1024))):
        hp = pipeline.HotPath(pipeline.HotPathConfig(nch=nch, **dict(kw, **opt)), max_frames=F)
        ux, uy = hp.make_batch(F)
        keys = list(range(F))
        res[name] = _time(lambda: hp.receive(ux, uy, noise_keys=keys))
        hp.close()
        del ux, uy
        torch.cuda.empty_cache()
    return res


def main():
    from polmux_amd import _abi
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["1", "2", "both"])
    ap.add_argument("--no-receive", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _abi.get()
    shapes = {"1": dict(nch=1, F=1024, kw={}), "2": dict(nch=16, F=32, kw=dict(variants=16))}
    out = {}
    for name in (["1", "2"] if args.shape == "both" else [args.shape]):
        s = shapes[name]
        res = dict(nfft=65536, nch=s["nch"], frames=s["F"])
        res.update(kernels(lib, 65536, s["nch"], s["F"], 64))
        if not args.no_receive:
            res.update(receives(s["nch"], s["F"], s["kw"]))
        out["config%s" % name] = {k: (float("%.4g" % v) if isinstance(v, float) and math.isfinite(v) else v) for k, v in res.items()}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
