"""CPU reference of the Manakov cross-phase modulation between dual-polarisation 'sepfields' channels (DESIGN.md section
8c) -- a test helper, not a test.  The reference stops at fiber.m:854, so this restates the DEFINITION, not MATLAB code:

    du_k/dz = -i g_k [ s P_k I + x sum_{j != k} (P_j I + u_j u_j^H) ] u_k,   g_k = gam[k]*8/9

xpm_nl_step applies exp(-i g_k leff H_k) through numpy's eigen-decomposition of the 2 x 2 Hermitian H_k per sample --
deliberately NOT the closed form the kernel uses -- and matrix_ssfm_xpm is the loop of fiber.m:512-551 around it, composed
from the oracle's own exported pieces (plxo.nextstep, plxo.checkstep, plxo.matrix_step) and the attenuation."""
import ctypes as C
import math

import numpy as np


def xpm_nl_step(gam89, leff, ux, uy, spm, xpm):
    """One nonlinear step.  ux, uy: [n, nfc] complex; gam89: [nfc] (or scalar) effective gamma, 8/9 included; every channel
    is updated from the fields at the START of the step.  Returns (ux, uy)."""
    ux = np.asarray(ux, dtype=np.complex128)
    uy = np.asarray(uy, dtype=np.complex128)
    if ux.ndim == 1:
        ux, uy = ux[:, None], uy[:, None]
    n, nfc = ux.shape
    g = np.broadcast_to(np.atleast_1d(np.asarray(gam89, dtype=float)), (nfc,))
    u = np.stack([ux, uy], -1)                                     # [n, nfc, 2]
    A = np.einsum("nka,nkb->nab", u, u.conj())                     # sum_j u_j u_j^H
    P = (np.abs(u) ** 2).sum(-1)                                   # [n, nfc]
    Pt = P.sum(1)
    I2 = np.eye(2)
    out = np.empty_like(u)
    for k in range(nfc):
        uk = u[:, k, :]
        B = A - uk[:, :, None] * uk[:, None, :].conj()             # the other channels
        H = spm * P[:, k, None, None] * I2 + xpm * ((Pt - P[:, k])[:, None, None] * I2 + B)
        H = 0.5 * (H + H.conj().transpose(0, 2, 1))
        w, V = np.linalg.eigh(H)
        ph = np.exp(-1j * g[k] * leff * w)                         # [n, 2]
        out[:, k, :] = np.einsum("nab,nb,ncb,nc->na", V, ph, V.conj(), uk)
    return out[:, :, 0].copy(), out[:, :, 1].copy()


def leff_of(alphalin, dz):
    """fiber.m:827-831"""
    return dz if alphalin == 0 else (1 - math.exp(-alphalin * dz)) / alphalin


def matrix_ssfm_xpm(plxo, ux, uy, betat, db1, dzmaxt, dphimaxt, gam, alphalin, Lf, nplates, fls, db0, theta, epsilon,
                    return_dz=False, replay_dz=None):
    """fiber.m:512-551 with xpm_nl_step as the nonlinear step (Manakov only: gam*8/9, :500).  Same results and hooks as
    plxo.matrix_ssfm: (rc, firstdz, ncycle, ux, uy[, dz list]); replay_dz[k] replaces nextstep's k-th result."""
    ux = np.array(ux, dtype=np.complex128, order="F").reshape(len(ux), -1, order="F")
    uy = np.array(uy, dtype=np.complex128, order="F").reshape(len(uy), -1, order="F")
    nfc = ux.shape[1]
    g = np.broadcast_to(np.atleast_1d(np.asarray(gam, dtype=float)), (nfc,)) * 8 / 9
    lcorr = Lf / nplates
    halfalpha = 0.5 * alphalin
    log = []
    nstep = [0]

    def nextstep():
        dz = plxo.nextstep(dzmaxt, dphimaxt, g, alphalin, ux, uy)
        k = nstep[0]
        nstep[0] += 1
        if replay_dz is not None and k < len(replay_dz):
            dz = float(replay_dz[k])
        log.append(dz)
        return dz

    def step(zc, dz, dz_miss, ntot):
        nonlocal ux, uy
        ux, uy = xpm_nl_step(g, leff_of(alphalin, dz), ux, uy, fls[2], fls[3])
        dzb, dz_miss, nmem, ntrunk = plxo.checkstep(zc, dz, lcorr, dz_miss, ntot)
        ux, uy = plxo.matrix_step(betat, db1, dzb, ux, uy, db0, theta, epsilon, lcorr, ntot, nmem)
        att = math.exp(-halfalpha * dz)
        ux, uy = ux * att, uy * att
        return dz_miss, ntot + ntrunk - nmem

    dz = nextstep()
    firstdz, zprop, ncycle, dz_miss, ntot = dz, dz, 1, 0.0, 0
    while zprop < Lf:
        dz_miss, ntot = step(zprop, dz, dz_miss, ntot)
        dz = nextstep()
        zprop = zprop + dz
        ncycle += 1
    step(Lf, Lf - zprop + dz, dz_miss, ntot)
    if return_dz:
        return 0, firstdz, ncycle, ux, uy, np.array(log)
    return 0, firstdz, ncycle, ux, uy


# ------------------------------------------------------------------ plumbing shared by the emulator and the GPU tests ---
def desc(n, nfc, fls, L, alpha, gam, dzmax, dphimax, betat, db1, nplates=1, manakov=1, frames=1):
    """A dual-polarisation plx_ssfm_desc (the arrays it points to are kept alive on the object)."""
    from polmux_amd._abi import SsfmDesc
    d = SsfmDesc()
    d.nfft, d.nfc, d.dual_pol, d.max_frames = n, nfc, 1, frames
    for i in range(4):
        d.fls[i] = fls[i]
    d.dzmaxt, d.dphimaxt, d.alphalin, d.length, d.nplates, d.manakov = dzmax, dphimax, alpha, L, nplates, manakov
    d._keep = (np.ascontiguousarray(gam, dtype=float), np.asfortranarray(betat, dtype=float), np.asfortranarray(db1, dtype=float))
    d.gam, d.betat, d.db1 = d._keep[0].ctypes.data, d._keep[1].ctypes.data, d._keep[2].ctypes.data
    return d


def tables(nsymb, nt, gvd, pmd, nplates, nfc, walkoff=6.8e-9, dgd=0.1):
    """betat, db1 [n, nfc] of a 28-Gbaud link with D = 17 ps/nm/km and a per-channel walk-off (fiber.m:355-358)."""
    from polmux_amd import synth
    omega = 2 * np.pi * 28 * synth.fn_grid(nsymb, nt)
    betat = np.stack([0.5 * omega ** 2 * -2.17e-8 * gvd + walkoff * (k - (nfc - 1) / 2) * omega for k in range(nfc)], 1)
    db1 = np.stack([np.sqrt(3 * np.pi / 8) * dgd / np.sqrt(nplates) / 28 * omega * pmd for _ in range(nfc)], 1)
    return betat, db1


def wdm_frame(nsymb, nt, nfc, pavg, seed=0):
    """nfc PDM-QPSK channels with their own de Bruijn seeds and unequal powers -> (ux, uy), each [n, nfc] Fortran order."""
    from polmux_amd import synth
    cols = [synth.pdm_qpsk_field(nsymb, nt, pavg * (1 + 0.15 * k), 2 + 2 * k + seed, 3 + 2 * k + seed)[:2] for k in range(nfc)]
    return np.asfortranarray(np.stack([c[0] for c in cols], 1)), np.asfortranarray(np.stack([c[1] for c in cols], 1))


def random_plates(nplates, seed):
    r = np.random.default_rng(seed)
    return (r.random(nplates) * 2 * np.pi - np.pi, r.random(nplates) * np.pi - np.pi / 2, 0.5 * np.arcsin(r.random(nplates) * 2 - 1))


def run_host(lib, d, flags, frames, brf=None):
    """Propagate `frames` (a list of (ux, uy), each [n, nfc]) as one batch through a plan of `lib` whose device memory is host
    memory (the emulator build).  brf: one (db0, theta, epsilon) per frame.  -> (firstdz[F], ncycle[F], [(ux, uy)], info[8])"""
    F, (n, nfc) = len(frames), frames[0][0].shape
    plan = C.c_void_p()
    lib.call("plx_ssfm_create_ex", C.byref(plan), C.byref(d), flags)
    try:
        if brf is not None:
            a, b, c = (np.ascontiguousarray(np.concatenate([p[i] for p in brf]), dtype=float) for i in range(3))
            lib.call("plx_ssfm_set_birefringence", plan, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(c.ctypes.data), F)
        gx = np.ascontiguousarray(np.stack([f[0].T for f in frames]), dtype=np.complex128)      # [F, nfc, n]
        gy = np.ascontiguousarray(np.stack([f[1].T for f in frames]), dtype=np.complex128)
        lib.call("plx_ssfm_propagate_dev", plan, C.c_void_p(gx.ctypes.data), C.c_void_p(gy.ctypes.data), F, None)
        first, ncyc = np.zeros(F), np.zeros(F, np.int32)
        lib.call("plx_ssfm_results", plan, F, C.c_void_p(first.ctypes.data), C.c_void_p(ncyc.ctypes.data))
        info = (C.c_int32 * 8)()
        lib.call("plx_ssfm_info", plan, info)
    finally:
        lib.call("plx_ssfm_destroy", plan)
    return first, ncyc, [(gx[f].T, gy[f].T) for f in range(F)], list(info)


def model_vs_one_field(propagate_sep, propagate_one, nsymb=256, nt=64, pavg=4.0, length=8e4):
    """The definition against one field that carries all the channels (SPM, XPM and four-wave mixing by construction).
    Three 28-Gbaud PDM-QPSK channels 464 / 256 = 1.8125 symbol rates apart (INTEGER bin offsets: a non-periodic carrier
    would put a discontinuity at the wrap), band-limited to one channel spacing, 80 km, D = 17, dphimax = 5e-3, dzmax = 2e4.
    propagate_sep(ux, uy [n, 3], betat [n, 3], xpm) and propagate_one(ux, uy [n], betat [n]) return (ux, uy).
    -> (errors with XPM, errors without): relative L2 per channel inside a rectangular filter of one channel spacing."""
    from polmux_amd import synth
    n, R, b2, mk = nsymb * nt, 28.0, -2.17e-8, np.array([-464, 0, 464])
    w = 2 * np.pi * R * synth.fn_grid(nsymb, nt)
    Om = 2 * np.pi * R * mk / nsymb
    mask = np.abs(np.fft.fftfreq(n) * n) < (mk[1] - mk[0]) / 2

    def filt(u):
        return np.fft.ifft(np.fft.fft(u, axis=0) * (mask if u.ndim == 1 else mask[:, None]), axis=0)

    ch = [synth.pdm_qpsk_field(nsymb, nt, pavg, 2 + 2 * k, 3 + 2 * k)[:2] for k in range(3)]
    ax, ay = filt(np.stack([c[0] for c in ch], 1)), filt(np.stack([c[1] for c in ch], 1))
    carrier = np.exp(2j * np.pi * np.outer(np.arange(n), mk) / n)                       # exp(i Omega_k t)
    bt_one = 0.5 * b2 * w ** 2
    bt_sep = bt_one[:, None] + b2 * w[:, None] * Om[None, :]
    ox, oy = propagate_one((ax * carrier).sum(1), (ay * carrier).sum(1), bt_one)
    back = np.exp(0.5j * b2 * Om ** 2 * length)                                          # removes exp(-i b2 Omega_k^2 L / 2)
    rx, ry = filt(ox[:, None] * carrier.conj()) * back, filt(oy[:, None] * carrier.conj()) * back
    errs = []
    for xpm in (1, 0):
        sx, sy = propagate_sep(ax, ay, bt_sep, xpm)
        sx, sy = filt(np.asarray(sx)), filt(np.asarray(sy))
        num = (np.abs(sx - rx) ** 2 + np.abs(sy - ry) ** 2).sum(0)
        errs.append(np.sqrt(num / (np.abs(rx) ** 2 + np.abs(ry) ** 2).sum(0)))
    return errs[0], errs[1]
