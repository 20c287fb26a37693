"""numpy restatements for the tests of the one-field WDM route: the multiplexer as create_field('unique')
forms it, the channel selection, the comb of a test case on GSTATE, and the ctypes plumbing of the two calls."""
import ctypes as C
import math

import numpy as np


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def il(z):
    """complex array -> contiguous float64 copy (interleaved re, im), what the library calls a complex128 buffer"""
    return np.ascontiguousarray(z, dtype=np.complex128).view(np.float64).copy()


def cnormal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def edge_shifts(N, nch):
    """carrier offsets of both signs that include +-(N/2 - 1), the largest the calls accept"""
    if nch == 1:
        return np.array([-(N // 2 - 1)], dtype=np.int64)
    s = np.round(np.linspace(-(N // 2 - 1), N // 2 - 1, nch)).astype(np.int64)
    if nch > 3:
        s[1] += 7          # (not a regular comb: odd and even offsets, nothing that divides N)
        s[-2] -= 12
    return s


def mux_fft(s, shift):
    """gstate.create_field('unique'): spectra rolled by -shift[c] and summed (create_field.m:186-199); s [..., nch, N]"""
    z = 0
    for c in range(s.shape[-2]):
        z = z + np.roll(np.fft.fft(s[..., c, :]), -int(shift[c]), axis=-1)
    return np.fft.ifft(z)


def select_np(u, shift, delay=None):
    """r[..., c, n] = u[..., m] exp(+i 2 pi shift[c] m / N), m = (n + delay[c]) mod N; u [..., N]"""
    N = u.shape[-1]
    m = np.arange(N)
    out = []
    for c in range(len(shift)):
        k = (int(shift[c]) * m) % N
        r = u * np.exp(2j * np.pi * k / N)
        out.append(np.roll(r, -int(delay[c]) if delay is not None else 0, axis=-1))
    return np.stack(out, axis=-2)


def call_mux(lib, sx, sy, shift, stream=None):
    """plx_wdm_mux_dev on host arrays (the emulator): sx, sy [F, nch, N] complex (sy may be None) -> (ux, uy) [F, N]"""
    F, nch, N = sx.shape
    gx, gy = il(sx), (il(sy) if sy is not None else None)
    ox, oy = np.full(2 * F * N, np.nan), (np.full(2 * F * N, np.nan) if sy is not None else None)
    sh = np.ascontiguousarray(shift, dtype=np.int64)
    lib.call("plx_wdm_mux_dev", vp(gx), vp(gy) if gy is not None else None, vp(ox), vp(oy) if oy is not None else None,
             N, nch, F, vp(sh), stream)
    c = lambda a: a.view(np.complex128).reshape(F, N)
    return c(ox), (c(oy) if oy is not None else None)


def call_select(lib, ux, uy, shift, delay=None, stream=None):
    """plx_wdm_select_dev on host arrays: ux, uy [F, N] complex (uy may be None) -> (rx, ry) [F, nch, N]"""
    F, N = ux.shape
    nch = len(shift)
    gx, gy = il(ux), (il(uy) if uy is not None else None)
    ox, oy = np.full(2 * F * nch * N, np.nan), (np.full(2 * F * nch * N, np.nan) if uy is not None else None)
    sh = np.ascontiguousarray(shift, dtype=np.int64)
    dl = np.ascontiguousarray(delay, dtype=np.int64) if delay is not None else None
    lib.call("plx_wdm_select_dev", vp(gx), vp(gy) if gy is not None else None, vp(ox), vp(oy) if oy is not None else None,
             N, nch, F, vp(sh), vp(dl) if dl is not None else None, stream)
    c = lambda a: a.view(np.complex128).reshape(F, nch, N)
    return c(ox), (c(oy) if oy is not None else None)


def comb(nsymb=256, nt=16, nch=3, chspacing=0.4, lam=1550.0, symbolrate=28.0, length=8e4, disp=17.0, slope=0.0, nspans=1):
    """The comb of the linear known answer, on GSTATE as HotPath sets it while the tables are formed (restored on return):
    returns dict(x, t, shift, dfn, spacing, ds, delay, ...) with t = fiber_tables of the ONE column ('g---'), spacing in symbol rates, ds / delay = pipeline.wdm_walkoff."""
    from polmux_amd import pipeline, synth
    from polmux_amd.fiber import fiber_tables
    from polmux_amd.gstate import GSTATE, unique_field_shifts
    names = ("NSYMB", "NT", "NCH", "SYMBOLRATE", "FN", "LAMBDA")
    saved = {k: getattr(GSTATE, k) for k in names}            # the global state is the caller's: put back below
    try:
        GSTATE.NSYMB, GSTATE.NT, GSTATE.NCH, GSTATE.SYMBOLRATE = nsymb, nt, nch, symbolrate
        GSTATE.FN = fn = synth.fn_grid(nsymb, nt)
        GSTATE.LAMBDA = lam + chspacing * (np.arange(nch) - (nch - 1) / 2)
        x = {"length": length, "alphadB": 0.2, "aeff": 80.0, "n2": 2.7e-20, "lambda": lam, "disp": disp, "slope": slope}
        t = fiber_tables(x, [1, 0, 0, 0], 1, 0.0)
        shift = unique_field_shifts()
    finally:
        for k, v in saved.items():
            setattr(GSTATE, k, v)
    dfn = fn[1] - fn[0]
    ds, delay = pipeline.wdm_walkoff(shift, float(t["beta2"][0]), float(t["b30"]), nspans * length, symbolrate, dfn, nt)
    spacing = abs(int(shift[1]) - int(shift[0])) * dfn if nch > 1 else None
    return dict(x=x, t=t, shift=shift, dfn=dfn, spacing=spacing, ds=ds, delay=delay, fn=np.asarray(fn, dtype=float),
                omega=2 * math.pi * symbolrate * np.asarray(fn, dtype=float), nt=nt, symbolrate=symbolrate,
                length=nspans * length)


def undo_channel(r, cb, c, remainder=True):
    """what is left of channel c after select, taken out in numpy: the channel's own dispersion exp(+i (beta2_c w^2 / 2 +
    b30 w^3 / 6) L), beta2_c = beta2 + b30 Om_c, and (remainder) the sub-sample rest of the walk-off,
    exp(+i w (delay_symbols - delay / NT) / SYMBOLRATE)"""
    w, L, t = cb["omega"], cb["length"], cb["t"]
    om_c = -2 * math.pi * cb["symbolrate"] * cb["dfn"] * float(cb["shift"][c])
    b2c = float(t["beta2"][0]) + float(t["b30"]) * om_c
    ph = (0.5 * b2c * w ** 2 + float(t["b30"]) * w ** 3 / 6) * L
    if remainder:
        ph = ph + w * (cb["ds"][c] - cb["delay"][c] / cb["nt"]) / cb["symbolrate"]
    return np.fft.ifft(np.fft.fft(r) * np.exp(1j * ph))


def xcorr_lag(a, b):
    """lag (in samples, signed) at which the circular cross-correlation of a against b peaks: a[n] ~ b[n - lag]"""
    cc = np.abs(np.fft.ifft(np.fft.fft(a) * np.conj(np.fft.fft(b))))
    k = int(np.argmax(cc))
    return k if k <= a.size // 2 else k - a.size


def rel_l2_upto_phase(got, ref):
    """relative L2 distance of got from ref after the best constant phase"""
    ph = np.vdot(ref, got)
    ph = ph / abs(ph)
    return np.linalg.norm(got / ph - ref) / np.linalg.norm(ref)
