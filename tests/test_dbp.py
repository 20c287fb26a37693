"""CPU tests (-m "not gpu") of digital backpropagation (plx_dbp_*, polmux_amd.dbp): the C ABI surface, argument checks,
and both routes of the kernel source under the host emulator against the numpy restatement of the operator below (which
the GPU tests, tests/test_gpu_dbp.py, use as well)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from polmux_amd import _abi
from polmux_amd.dbp import dbp_betat, dbp_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------- numpy restatement ---
def np_dbp(u, betat, nspans, dz, manakov, L, alphalin, gam, xi, scale):
    """u: [F, 2, N] complex (X, Y of each frame), scale: [F].  u *= scale; each span, last first: undo its amplifier
    (exp(-alphalin L / 2)), then the inverse of each forward step of matrix_ssfm (fiber.m:459-555) in reverse order:
    loss undone, exp(+i betat dz) in the spectrum, inverse Kerr step; finally u /= scale."""
    sc = np.asarray(scale, dtype=float).reshape(-1, 1, 1)
    u = np.array(u, dtype=np.complex128) * sc
    for _ in range(nspans):
        u = u * np.exp(-0.5 * alphalin * L)
        for h in list(dz)[::-1]:
            u = u * np.exp(0.5 * alphalin * h)
            u = np.fft.ifft(np.fft.fft(u, axis=-1) * np.exp(1j * betat * h), axis=-1)
            leff = h if alphalin == 0 else -np.expm1(-alphalin * h) / alphalin
            c = xi * gam * leff * (8.0 / 9.0 if manakov else 1.0)
            ux, uy = u[:, 0], u[:, 1]
            p = np.abs(ux) ** 2 + np.abs(uy) ** 2
            if not manakov:           # undo the rotation by phi = c s3 / 3 of fiber.m:838-845
                phi = c * 2 * (ux.real * uy.imag - ux.imag * uy.real) / 3
                cs, sn = np.cos(phi), np.sin(phi)
                ux, uy = cs * ux - sn * uy, sn * ux + cs * uy
            e = np.exp(1j * c * p)
            u = np.stack([ux * e, uy * e], 1)
    return u / sc


def rand_frames(n, nf, pmw, seed):
    """nf random dual-polarisation frames, mean power pmw mW per polarisation, band-limited to half the grid"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((nf, 2, n)) + 1j * rng.standard_normal((nf, 2, n))
    z = np.fft.ifft(np.fft.fft(z, axis=-1) * (np.abs(np.fft.fftfreq(n)) < 0.25), axis=-1)
    return z * np.sqrt(pmw / np.mean(np.abs(z) ** 2))


# link of the tests: 2-sps samples of 28 GBd, 80 km spans of SMF
FS, LAM, D17, L80, ALPHA, GAM = 56e9, 1550e-9, 17e-6, 8e4, math.log(10) * 1e-4 * 0.2, 1.368e-6


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------------- ABI ---
def test_dbp_abi_header_table_and_library_agree():
    """Every plx_dbp symbol of include/polmux_hip.h is in _abi.SIGNATURES and exported by the hipcc-built library."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "polmux_hip.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(plx_dbp[a-z0-9_]*)\s*\(", src)))
    assert syms == ["plx_dbp", "plx_dbp_apply_dev", "plx_dbp_create", "plx_dbp_destroy"]
    if not os.path.exists(_abi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_abi.LIB_PATH)
    for s in syms:
        assert s in _abi.SIGNATURES and hasattr(lib, s)
    assert "#define PLX_DBP_STREAMED 1u" in src and _abi.PLX_DBP_STREAMED == 1


def _good(n=1024, **kw):
    a = dict(nfft=n, max_frames=2, nspans=2, steps=2, manakov=1, span_length=L80, alphalin=ALPHA, gam=GAM, xi=1.0,
             betat=dbp_betat(n, FS, LAM, D17, 0.0))
    a.update(kw)
    return a


@pytest.mark.parametrize("bad, msg", [
    (dict(nfft=1000, betat=np.zeros(1000)), "power of two"),
    (dict(nfft=128, betat=np.zeros(128)), "power of two"),
    (dict(max_frames=0), "max_frames"),
    (dict(nspans=0), "nspans"),
    (dict(steps=0), "nsteps"),
    (dict(span_length=-1.0), "span_length"),
    (dict(alphalin=-1e-5), "alphalin"),
    (dict(steps=[3e4, 4e4]), "sum to span_length"),
    (dict(steps=[9e4, -1e4]), "dz must be > 0"),
])
def test_dbp_create_argument_errors(bad, msg):
    """plx_dbp_create refuses bad descriptors with PLX_ERR_ARG and a message, before touching the device (hipcc build)."""
    b = _abi.Binding()
    d = dbp_desc(**_good(**bad))
    plan = C.c_void_p()
    with pytest.raises(_abi.PolmuxError, match=msg) as ei:
        b.call("plx_dbp_create", C.byref(plan), C.byref(d), 0)
    assert ei.value.code == _abi.PLX_ERR_ARG
    with pytest.raises(_abi.PolmuxError, match="null argument"):
        b.call("plx_dbp_create", None, C.byref(d), 0)
    with pytest.raises(_abi.PolmuxError, match="unknown flag"):
        b.call("plx_dbp_create", C.byref(plan), C.byref(dbp_desc(**_good())), 6)
    with pytest.raises(_abi.PolmuxError, match="null argument"):
        b.call("plx_dbp_apply_dev", None, None, None, 1, None, None)


def test_DBP_input_validation():
    from polmux_amd import DBP
    x = np.zeros(1024, complex)
    args = (FS, LAM, L80, 2, 0.2, D17, 0.0, GAM)
    with pytest.raises(ValueError, match="same shape"):
        DBP(x, x[:512], *args, 2)
    with pytest.raises(ValueError, match="power of two"):
        DBP(x[:1000], x[:1000], *args, 2)
    with pytest.raises(ValueError, match="nSpans"):
        DBP(x, x, FS, LAM, L80, 0, 0.2, D17, 0.0, GAM, 2)
    with pytest.raises(ValueError, match="spanLength"):
        DBP(x, x, FS, LAM, 0.0, 2, 0.2, D17, 0.0, GAM, 2)
    with pytest.raises(ValueError, match="stepsPerSpan"):
        DBP(x, x, *args, 0)
    with pytest.raises(ValueError, match="sum to spanLength"):
        DBP(x, x, *args, [1e4, 2e4])
    with pytest.raises(ValueError, match="scale"):
        DBP(x, x, *args, 2, scale=0.0)


def test_hotpath_dbp_config_is_checked():
    """equaliser='dbp' with the cohmix front end, or an unknown equaliser, is refused before anything is built."""
    from polmux_amd import pipeline
    with pytest.raises(ValueError, match="pick"):
        pipeline.HotPath(pipeline.HotPathConfig(nsymb=64, nt=16, equaliser="dbp", frontend="cohmix"), 1)
    with pytest.raises(ValueError, match="equaliser"):
        pipeline.HotPath(pipeline.HotPathConfig(nsymb=64, nt=16, equaliser="dsp"), 1)


def test_dbp_betat_is_fiber_tables_beta_and_cde_dispersion():
    """dbp_betat is fiber()'s betat (fiber_tables, fiber.m:308-356) on the 2-sps grid, and its dispersion (even) part
    times the link length is the phase of CDE_OFDE's transfer function (cde_transfer): same sign convention."""
    from polmux_amd import synth
    from polmux_amd.fiber import fiber_tables, parse_flag
    from polmux_amd.gstate import GSTATE
    from polmux_amd.rx import cde_transfer
    nsymb = 512
    GSTATE.NSYMB, GSTATE.NT, GSTATE.NCH, GSTATE.SYMBOLRATE = nsymb, 2, 1, 28.0
    GSTATE.FN, GSTATE.LAMBDA = synth.fn_grid(nsymb, 2), np.array([1550.0])
    x = {"length": L80, "alphadB": 0.2, "aeff": 80.0, "n2": 2.7e-20, "lambda": 1550.0, "disp": 17.0, "slope": 0.07,
         "dphimax": 5e-3, "dzmax": 2e4}
    fls, _, _ = parse_flag("g-s-", 1, x)
    t = fiber_tables(x, fls, 1, 0.0)
    bt = dbp_betat(2 * nsymb, FS, LAM, D17, 0.07e3)
    assert rel(bt, t["betat"][:, 0]) < 1e-13
    assert t["gam"][0] == pytest.approx(GAM, rel=1e-3)
    n = 2 * nsymb
    H = np.fft.ifftshift(cde_transfer(n, FS, LAM, 10 * L80, D17, 0.0))          # FFT order
    even = 0.5 * (bt + np.roll(bt[::-1], 1)) * 10 * L80
    keep = np.arange(n) != n // 2                                                 # (the Nyquist bin has no mirror)
    np.testing.assert_allclose(np.exp(1j * even[keep]), H[keep], atol=1e-9)


# ------------------------------------------------------------------ emulator ---
@pytest.fixture(scope="module")
def emu():
    from tests import _emu
    return _emu.binding()


def _emu_apply(emu, u, desc, scale, flags):
    plan = C.c_void_p()
    emu.call("plx_dbp_create", C.byref(plan), C.byref(desc), flags)
    try:
        a = np.ascontiguousarray(u, dtype=np.complex128).view(np.float64).copy()
        sc = np.ascontiguousarray(scale, dtype=float)
        emu.call("plx_dbp_apply_dev", plan, _vp(a), _vp(a), u.shape[0], _vp(sc), None)
    finally:
        emu.call("plx_dbp_destroy", plan)
    return a.view(np.complex128).reshape(u.shape)


@pytest.mark.parametrize("n", [256, 1024])
@pytest.mark.parametrize("manakov", [1, 0])
@pytest.mark.parametrize("flags", [0, 1])
def test_emu_dbp_routes_match_numpy(emu, n, manakov, flags):
    """Both routes of plx_dbp.hip (flags 0: resident, 1: PLX_DBP_STREAMED) under the emulator: 2 frames with their own
    scale, 2 spans, 2 steps per span (explicit, unequal, for the streamed route: two tables), both nonlinear forms, an
    out-of-place and an in-place call; <= 1e-12 of the numpy operator."""
    scale = np.array([0.5, 2.0])
    u = rand_frames(n, 2, 8.0, 7) / scale.reshape(-1, 1, 1)
    bt = dbp_betat(n, FS, LAM, D17, 60.0)
    steps = [3e4, 5e4] if flags else 2
    d = dbp_desc(n, 2, 2, steps, manakov, L80, ALPHA, GAM, 1.0, bt)
    ref = np_dbp(u, bt, 2, [3e4, 5e4] if flags else [4e4, 4e4], manakov, L80, ALPHA, GAM, 1.0, scale)
    assert rel(ref, u) > 1e-2                                       # the operator does something
    got = _emu_apply(emu, u, d, scale, flags)
    assert rel(got, ref) <= 1e-12
    # out of place through the gateway (one frame, scalar scale)
    xr, xi, yr, yi = u[1, 0].real.copy(), u[1, 0].imag.copy(), u[1, 1].real.copy(), u[1, 1].imag.copy()
    outs = [np.zeros(n) for _ in range(4)]
    emu.call("plx_dbp", _vp(xr), _vp(xi), _vp(yr), _vp(yi), n, C.byref(d), float(scale[1]), *[_vp(o) for o in outs])
    g = np.stack([outs[0] + 1j * outs[1], outs[2] + 1j * outs[3]])
    assert rel(g, ref[1]) <= 1e-12
