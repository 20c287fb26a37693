"""Digital backpropagation (DBP): the receiver equaliser that runs the fibre's split-step model backwards.

  DBP(inX, inY, samplingRateIn, lambdaRef, spanLength, nSpans, alphadB, D, S, gamma, stepsPerSpan, xi, manakov, scale)

An alternative to CDE_OFDE that also undoes the Kerr distortion: each step is the exact inverse of one forward step of
matrix_ssfm (fiber.m:459-555) -- loss undone, linear step with exp(+i betat dz), inverse nonlinear step with xi*gamma.
The operator is plx_dbp_* of include/polmux_hip.h; numpy in -> numpy out through the gateway, torch CUDA tensors in ->
torch out through a plan on the device.  No CPU implementation exists here.
"""
import ctypes as C
import math

import numpy as np

from . import _abi
from .rx import _is_torch, _split, _stream

CLIGHT = 299792458.0


def dbp_betat(nfft, samplingRateIn, lambdaRef, D, S):
    """beta(omega) [rad/m] on the nfft-point grid of sampling rate samplingRateIn [Hz], in FFT order: the conversions of
    fiber.m:308-309 (beta2 = -lambda^2 D / 2 pi c, beta3 = (lambda / 2 pi c)^2 (2 lambda D + lambda^2 S)) with D in
    s/m^2, S in s/m^3 and lambdaRef in m.  With gamma = 0 DBP multiplies the spectrum by exp(+i betat L nSpans), whose
    dispersion term is CDE_OFDE's transfer function (cde_transfer)."""
    b2 = -lambdaRef ** 2 / (2 * math.pi * CLIGHT) * D
    b3 = (lambdaRef / (2 * math.pi * CLIGHT)) ** 2 * (2 * lambdaRef * D + lambdaRef ** 2 * S)
    w = 2 * math.pi * np.fft.fftfreq(int(nfft), 1.0 / samplingRateIn)
    return 0.5 * b2 * w ** 2 + b3 * w ** 3 / 6


def dbp_desc(nfft, max_frames, nspans, steps, manakov, span_length, alphalin, gam, xi, betat):
    """A plx_dbp_desc (its tables kept alive on the struct).  steps: steps per span (uniform) or the explicit list of
    step lengths of one span in forward order."""
    d = _abi.DbpDesc()
    if np.ndim(steps) == 0:
        nsteps, dz = int(steps), None
    else:
        dz = np.ascontiguousarray(steps, dtype=np.float64)
        nsteps = dz.size
    bt = np.ascontiguousarray(betat, dtype=np.float64).reshape(-1)
    d.nfft, d.max_frames, d.nspans, d.nsteps = int(nfft), int(max_frames), int(nspans), nsteps
    d.manakov, d.span_length, d.alphalin, d.gam, d.xi = int(bool(manakov)), float(span_length), float(alphalin), float(gam), float(xi)
    d._keep = (bt, dz)
    d.betat = bt.ctypes.data
    d.dz = dz.ctypes.data if dz is not None else None
    return d


class DbpPlan:
    """A plx_dbp plan on the device: apply(rx, out, scale) on [frames, 2, nfft] complex128 tensors (HotPath.rx's layout)."""

    def __init__(self, desc, streamed=False):
        self.lib = _abi.get()
        self.desc = desc
        self.h = C.c_void_p()
        self.lib.call("plx_dbp_create", C.byref(self.h), C.byref(desc), _abi.PLX_DBP_STREAMED if streamed else 0)

    def apply(self, rx, out=None, scale=None, stream=None):
        """rx, out: [F, 2, nfft] complex128 device tensors (out may be rx); scale: [F] float64 device tensor or None."""
        out = rx if out is None else out
        F = rx.shape[0]
        self.lib.call("plx_dbp_apply_dev", self.h, rx.data_ptr(), out.data_ptr(), F,
                      scale.data_ptr() if scale is not None else None, stream if stream is not None else _stream())
        return out

    def close(self):
        if self.h:
            self.lib.call("plx_dbp_destroy", self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def DBP(inX, inY, samplingRateIn, lambdaRef, spanLength, nSpans, alphadB, D, S, gamma, stepsPerSpan, xi=1.0, manakov=True,
        scale=1.0):
    """[outX, outY] = DBP(...): backpropagate the received dual-polarisation field through nSpans spans of spanLength [m]
    (alphadB [dB/km], D [s/m^2], S [s/m^3], lambdaRef [m], gamma [1/(mW m)] as fiber_tables), stepsPerSpan uniform steps
    per span or an explicit list of one span's step lengths in forward order.  The input is the field after the
    receiver's amplifier, in units of scale * sqrt(mW); the output is in the same units.  xi scales the backpropagated
    nonlinearity; manakov selects the 8/9 Manakov step (else the CNLSE step)."""
    if _is_torch(inX):
        if tuple(inX.shape) != tuple(inY.shape):
            raise ValueError("DBP: inX and inY must have the same shape")
        n = inX.numel()
    else:
        inX, inY = np.asarray(inX), np.asarray(inY)
        if inX.shape != inY.shape:
            raise ValueError("DBP: inX and inY must have the same shape")
        n = inX.size
    if n < 256 or n & (n - 1):
        raise ValueError("DBP: the signal length must be a power of two >= 256")
    if int(nSpans) != nSpans or nSpans < 1:
        raise ValueError("DBP: nSpans must be a positive integer")
    if not spanLength > 0:
        raise ValueError("DBP: spanLength must be > 0")
    if np.ndim(stepsPerSpan) == 0:
        if int(stepsPerSpan) != stepsPerSpan or stepsPerSpan < 1:
            raise ValueError("DBP: stepsPerSpan must be a positive integer or a list of step lengths")
    elif len(stepsPerSpan) < 1 or abs(sum(stepsPerSpan) - spanLength) > 1e-9 * spanLength:
        raise ValueError("DBP: the explicit steps must sum to spanLength")
    if not (np.isfinite(scale) and scale != 0):
        raise ValueError("DBP: scale must be finite and nonzero")
    alphalin = math.log(10) * 1e-4 * alphadB                     # fiber.m:302
    betat = dbp_betat(n, samplingRateIn, lambdaRef, D, S)
    lib = _abi.get()
    if _is_torch(inX):
        import torch
        x = inX.reshape(-1).to(torch.complex128)
        y = inY.reshape(-1).to(torch.complex128)
        u = torch.stack([x, y]).unsqueeze(0).contiguous()         # [1, 2, n]
        plan = DbpPlan(dbp_desc(n, 1, nSpans, stepsPerSpan, manakov, spanLength, alphalin, gamma, xi, betat))
        try:
            sc = torch.full((1,), float(scale), dtype=torch.float64, device=u.device)
            plan.apply(u, u, sc)
            torch.cuda.current_stream().synchronize()
        finally:
            plan.close()
        return u[0, 0].reshape(inX.shape), u[0, 1].reshape(inY.shape)
    d = dbp_desc(n, 1, nSpans, stepsPerSpan, manakov, spanLength, alphalin, gamma, xi, betat)
    xr, xi_ = _split(inX.reshape(-1))
    yr, yi = _split(inY.reshape(-1))
    outs = [np.zeros(n) for _ in range(4)]
    lib.call("plx_dbp", xr.ctypes.data, xi_.ctypes.data, yr.ctypes.data, yi.ctypes.data, n, C.byref(d), float(scale),
             *[o.ctypes.data for o in outs])
    return (outs[0] + 1j * outs[1]).reshape(inX.shape), (outs[2] + 1j * outs[3]).reshape(inY.shape)
