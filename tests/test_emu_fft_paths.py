"""The two host-driven users of the SSFM plan's FFT engine under the emulator, at every row-pass geometry a scalar plan can
take: the adaptive step (plx_scalar_ssfm_adaptive, fiber.m:639-679, 938-1009, and the dphiadapt first step :588-611)
against the oracle, and the spectral filter (plx_filter_apply_dev: the receiver's DCF, the streamed DBP, the front end)
against numpy's ifft(fft(x) * H).  Neither goes through the propagator's step loop, so the step-loop tests of
test_emu_kernels.py do not cover them.  Every case first checks that its tuning really reaches the row pass it is named
after (plx_ssfm_info), so that a later change of the dispatch cannot move it onto another kernel unnoticed."""
import ctypes as C

import numpy as np
import pytest

from polmux_amd._abi import SsfmDesc
from tests.test_emu_kernels import _desc, _il, _qpsk_field, _tables, _vp


@pytest.fixture(scope="module")
def emu():
    from tests import _emu
    return _emu.binding()


# (id, nfft, tuning, (p1, p2, info[6], info[7])) -- info[6]: row-pass workgroup size, info[7]: 2 = k_rowsm / k_rowreg,
# 1 = k_row4k on a scalar plan, 0 = k_row (plx_ssfm_info)
GEOMETRIES = [
    ("k_row_n2_16", 1 << 10, {}, (6, 4, 128, 0)),
    ("k_rowsm", 1 << 13, {}, (8, 5, 64, 2)),
    ("k_rowreg9_whole", 1 << 12, {"PLX_SSFM_P1": 3, "PLX_SSFM_ROWG_SPLIT": 0}, (3, 9, 256, 2)),
    ("k_rowreg9_split", 1 << 12, {"PLX_SSFM_P1": 3, "PLX_SSFM_ROWG_SPLIT": 1}, (3, 9, 256, 2)),
    ("k_rowreg10_whole", 1 << 12, {"PLX_SSFM_P1": 2, "PLX_SSFM_ROWG_SPLIT": 0}, (2, 10, 256, 2)),
    ("k_rowreg10_split", 1 << 12, {"PLX_SSFM_P1": 2, "PLX_SSFM_ROWG_SPLIT": 1}, (2, 10, 256, 2)),
    ("k_rowreg11_whole", 1 << 13, {"PLX_SSFM_P1": 2, "PLX_SSFM_ROWG_SPLIT": 0}, (2, 11, 256, 2)),
    ("k_rowreg11_split", 1 << 13, {"PLX_SSFM_P1": 2, "PLX_SSFM_ROWG_SPLIT": 1}, (2, 11, 256, 2)),
    ("k_row4k_whole", 1 << 14, {"PLX_SSFM_P1": 2, "PLX_SSFM_ROW4K_SPLIT": 0}, (2, 12, 256, 1)),
    ("k_row4k_split", 1 << 14, {"PLX_SSFM_P1": 2, "PLX_SSFM_ROW4K_SPLIT": 1}, (2, 12, 256, 1)),
]
IDS = [g[0] for g in GEOMETRIES]


def _set(tune, fields):
    tune.setenv("PLX_SSFM_COL_THREADS", "128")              # (narrow, wide column workgroups: a quarter of the emulated ones)
    tune.setenv("PLX_SSFM_LOGW", "6")
    for k, v in fields.items():
        tune.setenv(k, str(v))


def _geometry(emu, d):
    """(p1, p2, info[6], info[7]) of a plan made from descriptor d under the current tuning"""
    plan = C.c_void_p()
    emu.call("plx_ssfm_create", C.byref(plan), C.byref(d))
    info = (C.c_int32 * 8)()
    try:
        emu.call("plx_ssfm_info", plan, info)
    finally:
        emu.call("plx_ssfm_destroy", plan)
    return (info[1], info[2], info[6], info[7])


def _filter_desc(n, frames):
    """the descriptor plx_filter_create builds for its plan (plx_front.hip)"""
    d = SsfmDesc()
    d.nfft, d.nfc, d.dual_pol, d.max_frames = n, 1, 0, frames
    d.dzmaxt, d.dphimaxt, d.length, d.nplates = 1.0, 1.0, 1.0, 1
    d._keep = (np.zeros(1), np.zeros(n))
    d.gam, d.betat = d._keep[0].ctypes.data, d._keep[1].ctypes.data
    return d


def _adaptive_case(n, nfc, tolflag):
    """a scalar frame of nfc 'sepfields' channels (XPM on with two) through 500 m of fibre at ltol = 1e-6: 5 to 13 accepted
    steps and 3 to 5 rejected ones (short: the emulator runs three transforms per trial)"""
    nt, L = (16 if n.bit_length() % 2 else 32), 5e2        # (a De Bruijn pattern of 4^k symbols)
    fls = [1, 0, 1, 1 if nfc > 1 else 0]
    betat, db1 = _tables(n, nt, fls, 1, nfc)
    u = np.asfortranarray(np.stack([_qpsk_field(n, nt, 12.0 + 2 * k, (2 + k, 5 + k))[0] for k in range(nfc)], 1))
    gam = [1.2e-6, 1.3e-6][:nfc]
    dph = np.inf if tolflag == 2 else 2e-2
    return u, betat, db1, fls, gam, dph, L


def _run_adaptive(emu, oracle, tune, geom, nfc, tolflag):
    _, n, fields, want = geom
    u, betat, db1, fls, gam, dph, L = _adaptive_case(n, nfc, tolflag)
    alpha, ltol, safety = 4.6e-5, 1e-6, 0.9
    d = _desc(n, nfc, 0, fls, L, alpha, gam, L, dph, betat, db1)
    ur, ui = np.asfortranarray(u.real.copy()), np.asfortranarray(u.imag.copy())
    fd, nc, nr = C.c_double(), C.c_int32(), C.c_int32()
    # the gateway tier caches its plans by a hash of the descriptor, not of the tuning: drop them on both sides of the call
    emu.call("plx_release_all")
    _set(tune, fields)
    try:
        assert _geometry(emu, d) == want
        emu.call("plx_scalar_ssfm_adaptive", _vp(ur), _vp(ui), C.byref(d), tolflag, ltol, safety, C.byref(fd), C.byref(nc),
                 C.byref(nr))
    finally:
        emu.call("plx_release_all")
    if tolflag == 2:
        ofd, onc, onrej, ou = oracle.scalar_a_ssfm(u, betat, L, dph, gam, alpha, L, ltol, safety, fls)
        assert nr.value == onrej
    else:
        ofd, onc, ou = oracle.scalar_ssfm(u, betat, L, dph, gam, alpha, L, fls, tolflag=1, trg_err=ltol, trg_safety=safety)
    assert onc > 3
    assert nc.value == onc
    assert fd.value == pytest.approx(ofd, rel=1e-9)
    assert np.abs((ur + 1j * ui) - ou).max() < 1e-9 * np.abs(ou).max()


@pytest.mark.parametrize("tolflag", [2, 1])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=IDS)
def test_emu_adaptive_step_every_row_pass(emu, oracle, tune, geom, tolflag):
    """plx_scalar_ssfm_adaptive, tolflag 2 (scalar_a_ssfm) and 1 (dphiadapt), on one field: ncycle and nrej equal the oracle's,
    firstdz to 1e-9 relative, the field to 1e-9 of its maximum.  Its linear step takes the plan's row pass, whichever that is."""
    _run_adaptive(emu, oracle, tune, geom, 1, tolflag)


@pytest.mark.parametrize("tolflag", [2, 1])
@pytest.mark.parametrize("geom", [g for g in GEOMETRIES if g[0] == "k_row4k_split"], ids=lambda g: g[0])
def test_emu_adaptive_step_two_channels_long_rows(emu, oracle, tune, geom, tolflag):
    """the same with two 'sepfields' channels and XPM: the row pass covers both channels of the frame"""
    _run_adaptive(emu, oracle, tune, geom, 2, tolflag)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=IDS)
def test_emu_filter_every_row_pass(emu, tune, geom):
    """plx_filter_apply_dev: 3 signals on a plan for 4 -- a random signal, a delta (gives ifft(H)) and one tone of bin k (gives
    H[k] times the tone) -- with a random complex H (not of unit modulus) against numpy's ifft(fft(x) * H) to 2e-14 of max|y|;
    the 4th row of the same buffer is not touched."""
    _, n, fields, want = geom
    rng = np.random.default_rng(n + len(fields) + sum(fields.values()))
    H = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    k = int(rng.choice(np.flatnonzero(np.abs(H[1:]) >= 1.0))) + 1   # (a tone bin where |H| is not small: the transforms' rounding
                                                                    #  scales with the whole of H, the bar with |H[k]|)
    x = np.empty((4, n), np.complex128)
    x[0] = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x[1] = 0
    x[1, 0] = 1
    x[2] = np.exp(2j * np.pi * ((k * np.arange(n)) % n) / n)     # (phase reduced exactly: the tone to an ulp)
    x[3] = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ref = np.fft.ifft(np.fft.fft(x[:3], axis=-1) * H, axis=-1)
    hr, hi = np.ascontiguousarray(H.real), np.ascontiguousarray(H.imag)
    g = _il(x)
    guard = g.view(np.complex128).reshape(4, n)[3].copy()
    plan = C.c_void_p()
    _set(tune, fields)
    assert _geometry(emu, _filter_desc(n, 4)) == want
    emu.call("plx_filter_create", C.byref(plan), n, 4, _vp(hr), _vp(hi))
    try:
        emu.call("plx_filter_apply_dev", plan, _vp(g), 3, None)
    finally:
        emu.call("plx_filter_destroy", plan)
    y = g.view(np.complex128).reshape(4, n)
    for r in range(3):
        assert np.abs(y[r] - ref[r]).max() <= 2e-14 * np.abs(ref[r]).max(), r
    hh = np.fft.ifft(H)
    assert np.abs(y[1] - hh).max() <= 2e-14 * np.abs(hh).max()
    assert np.abs(y[2] - H[k] * x[2]).max() <= 2e-14 * abs(H[k])
    assert np.array_equal(y[3].view(np.float64), guard.view(np.float64))
