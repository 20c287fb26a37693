"""Manakov cross-phase modulation between dual-polarisation 'sepfields' channels (PLX_SSFM_XPM_MANAKOV, DESIGN.md section
8c): the CPU reference of tests/xpm_ref.py pinned to the oracle, its known answers, the kernels under the host emulator
against it, the flag's semantics, and the operator itself against one field that carries all the channels."""
import ctypes as C

import numpy as np
import pytest

from polmux_amd._abi import PLX_SSFM_XPM_MANAKOV, PolmuxError
from tests import xpm_ref

ALPHA, GAM, LSPAN = 4.6e-5, 1.3e-6, 8e4


@pytest.fixture(scope="module")
def emu():
    from tests import _emu
    return _emu.binding()


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_xpm_ref_pinned_to_oracle(oracle):
    """With xpm = 0 the helper's loop is the oracle's matrix_ssfm (two channels, 'gps-', six plates, Manakov).
    Observed: ncycle 32 = 32, firstdz equal to the last bit, field 2.8e-15 / 2.8e-15 of max |u| (X / Y)."""
    nsymb, nt, nfc, nplates, L = 64, 8, 2, 6, 2e4
    fls = [1, 1, 1, 0]
    betat, db1 = xpm_ref.tables(nsymb, nt, 1, 1, nplates, nfc)
    ux, uy = xpm_ref.wdm_frame(nsymb, nt, nfc, 12.0)
    brf = xpm_ref.random_plates(nplates, 3)
    gam = [1.2e-6, 1.3e-6]
    rc, ofd, onc, ox, oy = oracle.matrix_ssfm(ux, uy, betat, db1, 1e4, 2e-2, gam, ALPHA, L, nplates, 1, fls, *brf)
    rc2, fd, nc, hx, hy = xpm_ref.matrix_ssfm_xpm(oracle, ux, uy, betat, db1, 1e4, 2e-2, gam, ALPHA, L, nplates, fls, *brf)
    print("helper vs oracle: ncycle %d / %d, firstdz rel %.3g, field %.3g / %.3g" %
          (nc, onc, abs(fd - ofd) / ofd, _relmax(hx, ox), _relmax(hy, oy)))
    assert rc == 0 and rc2 == 0 and nc == onc and nc > 3
    assert fd == pytest.approx(ofd, rel=1e-13)
    assert np.abs(hx - ox).max() < 1e-11 * np.abs(ox).max()
    assert np.abs(hy - oy).max() < 1e-11 * np.abs(oy).max()


def test_xpm_nl_step_known_answers(oracle):
    r = np.random.default_rng(11)
    n, nfc = 64, 3
    ux = r.standard_normal((n, nfc)) + 1j * r.standard_normal((n, nfc))
    uy = r.standard_normal((n, nfc)) + 1j * r.standard_normal((n, nfc))
    g89 = np.array([1.1, 1.2, 1.3]) * 1e-1 * 8 / 9
    dz = 1.7
    leff = xpm_ref.leff_of(0.3, dz)
    # scalar limit: every y = 0 -> nl_step's weights (fiber.m:795, :797) with gam 8/9
    for spm in (0, 1):
        gx, gy = xpm_ref.xpm_nl_step(g89, leff, ux, np.zeros_like(uy), spm, 1)
        ref = oracle.nl_step(0.3, g89, dz, ux, spm, 1)
        assert np.abs(gx - ref).max() < 1e-13 * np.abs(ref).max() and np.abs(gy).max() == 0
    # a neighbour wholly in the orthogonal polarisation contributes P_j, not 2 P_j
    x0 = ux[:, :1]
    yn = uy[:, :1]
    gx, gy = xpm_ref.xpm_nl_step(g89[:2], leff, np.hstack([x0, 0 * x0]), np.hstack([0 * yn, yn]), 1, 1)
    want = x0[:, 0] * np.exp(-1j * g89[0] * leff * (np.abs(x0[:, 0]) ** 2 + np.abs(yn[:, 0]) ** 2))
    assert np.abs(gx[:, 0] - want).max() < 1e-13 * np.abs(want).max() and np.abs(gy[:, 0]).max() < 1e-13
    # ... and one in the same polarisation 2 P_j
    gx, _ = xpm_ref.xpm_nl_step(g89[:2], leff, np.hstack([x0, yn]), np.zeros((n, 2)), 1, 1)
    want = x0[:, 0] * np.exp(-1j * g89[0] * leff * (np.abs(x0[:, 0]) ** 2 + 2 * np.abs(yn[:, 0]) ** 2))
    assert np.abs(gx[:, 0] - want).max() < 1e-13 * np.abs(want).max()
    # unitary per sample: every P_k is kept
    gx, gy = xpm_ref.xpm_nl_step(g89, leff, ux, uy, 1, 1)
    P0, P1 = np.abs(ux) ** 2 + np.abs(uy) ** 2, np.abs(gx) ** 2 + np.abs(gy) ** 2
    assert np.abs(P1 - P0).max() < 1e-14 * P0.max()
    # samples where the neighbours vanish (b = 0): self-phase modulation alone, and nothing at all without it
    vx, vy = ux.copy(), uy.copy()
    vx[:5, 1:] = 0
    vy[:5, 1:] = 0
    gx, gy = xpm_ref.xpm_nl_step(g89, leff, vx, vy, 1, 1)
    ph = np.exp(-1j * g89[0] * leff * P0[:5, 0])
    assert np.abs(gx[:5, 0] - vx[:5, 0] * ph).max() < 1e-14 and np.abs(gy[:5, 0] - vy[:5, 0] * ph).max() < 1e-14
    assert np.all(gx[:5, 1:] == 0) and np.all(np.isfinite(gx)) and np.all(np.isfinite(gy))
    gx, gy = xpm_ref.xpm_nl_step(g89, leff, vx, vy, 0, 1)
    assert np.abs(gx[:5, 0] - vx[:5, 0]).max() < 1e-15 and np.abs(gy[:5, 0] - vy[:5, 0]).max() < 1e-15


@pytest.mark.parametrize("nfc", [3, 6, 8])
@pytest.mark.parametrize("spm", [1, 0])
def test_emu_xpm_single_nonlinear_step(emu, spm, nfc):
    """One nonlinear step of the kernels (betat = 0, dphimax = inf, dzmax = L: the span is one step) against the
    eigen-decomposition: exp(-alphalin L / 2) xpm_nl_step(...) to 1e-12 of max |u| (non-recursive stages).
    Some samples carry one channel only (b = 0).  Three channels run the tail of k_stokes_sum's channel loop only, six its
    unrolled body of four and then the tail, eight the body twice.  Observed (phases up to 1.55 / 1.85 / 2.73 rad at 3 / 6 / 8 channels): at most 1.2e-15 / 1.7e-15 / 1.8e-15."""
    nsymb, nt = 64, 8
    n = nsymb * nt
    gam = np.array([1.1e-6, 1.3e-6, 1.45e-6, 1.2e-6, 1.35e-6, 1.25e-6, 1.15e-6, 1.4e-6])[:nfc]
    ux, uy = xpm_ref.wdm_frame(nsymb, nt, nfc, 8.0 if nfc == 3 else 4.0)
    ux[:7, 1:] = 0
    uy[:7, 1:] = 0
    z = np.zeros((n, nfc))
    d = xpm_ref.desc(n, nfc, [0, 0, spm, 1], LSPAN, ALPHA, gam, LSPAN, np.inf, z, z)
    first, ncyc, out, info = xpm_ref.run_host(emu, d, PLX_SSFM_XPM_MANAKOV, [(ux, uy)])
    assert ncyc[0] == 1 and first[0] == LSPAN and info[0] == 0
    leff = xpm_ref.leff_of(ALPHA, LSPAN)
    rx, ry = xpm_ref.xpm_nl_step(gam * 8 / 9, leff, ux, uy, spm, 1)
    att = np.exp(-0.5 * ALPHA * LSPAN)
    scale = max(np.abs(rx).max(), np.abs(ry).max()) * att
    ex, ey = np.abs(out[0][0] - att * rx).max() / scale, np.abs(out[0][1] - att * ry).max() / scale
    print("single step spm=%d: %.3g %.3g (phase up to %.2f rad)" % (spm, ex, ey, (gam.max() * 8 / 9 * leff * 2 * (np.abs(ux) ** 2 + np.abs(uy) ** 2).sum(1)).max()))
    assert ex < 1e-12 and ey < 1e-12
    assert np.abs(out[0][0] - att * ux).max() > 1e-2 * scale           # the step did something


@pytest.mark.parametrize("nfc,nplates", [(2, 1), (3, 1), (2, 6), (3, 6), (5, 6)])
def test_emu_xpm_propagation(emu, oracle, nfc, nplates):
    """'gpsx' over 20 km, 512 samples, without PMD (one zero plate) and with six random plates: two frames at different
    powers in one batch against matrix_ssfm_xpm.  Observed: ncycle 16 / 33 (two channels), 20 / 41 (three), 23 / 48 (five), firstdz equal to the last bit,
    field <= 1.7e-14 of max |u|."""
    nsymb, nt, L = 64, 8, 2e4
    n = nsymb * nt
    fls = [1, 1, 1, 1]
    pmd = 1 if nplates > 1 else 0
    betat, db1 = xpm_ref.tables(nsymb, nt, 1, pmd, nplates, nfc)
    gam = np.array([1.2e-6, 1.3e-6, 1.4e-6, 1.25e-6, 1.35e-6])[:nfc]
    frames = [xpm_ref.wdm_frame(nsymb, nt, nfc, p, seed=s) for p, s in ((6.0, 0), (12.0, 6))]
    brf = [xpm_ref.random_plates(nplates, 3 + f) if pmd else (np.zeros(1), np.zeros(1), np.zeros(1)) for f in range(2)]
    d = xpm_ref.desc(n, nfc, fls, L, ALPHA, gam, 1e4, 2e-2, betat, db1, nplates=nplates, frames=2)
    first, ncyc, out, info = xpm_ref.run_host(emu, d, PLX_SSFM_XPM_MANAKOV, frames, brf=brf)
    assert info[0] == 0                                                   # three sweeps per step
    for f in range(2):
        rc, rfd, rnc, rx, ry = xpm_ref.matrix_ssfm_xpm(oracle, *frames[f], betat, db1, 1e4, 2e-2, gam, ALPHA, L, nplates, fls, *brf[f])
        print("frame %d: ncycle %d / %d, firstdz rel %.3g, field %.3g %.3g" %
              (f, ncyc[f], rnc, abs(first[f] - rfd) / rfd, _relmax(out[f][0], rx), _relmax(out[f][1], ry)))
        assert ncyc[f] == rnc and first[f] == pytest.approx(rfd, rel=1e-13)
        assert np.abs(out[f][0] - rx).max() < 1e-11 * np.abs(rx).max()
        assert np.abs(out[f][1] - ry).max() < 1e-11 * np.abs(ry).max()
    assert ncyc[0] != ncyc[1]
    # the step rule is untouched: firstdz of the same plan without XPM, bit for bit
    d0 = xpm_ref.desc(n, nfc, [1, 1, 1, 0], L, ALPHA, gam, 1e4, 2e-2, betat, db1, nplates=nplates, frames=2)
    first0, _, out0, _ = xpm_ref.run_host(emu, d0, 0, frames, brf=brf)
    assert np.array_equal(first0, first)
    assert np.abs(out0[0][0] - out[0][0]).max() > 1e-3 * np.abs(out[0][0]).max()      # ... and XPM is not a small term


def test_emu_xpm_flag_semantics(emu):
    nsymb, nt = 64, 4
    n = nsymb * nt
    betat, db1 = xpm_ref.tables(nsymb, nt, 1, 0, 1, 2)
    plan = C.c_void_p()

    def create(d, flags):
        emu.call("plx_ssfm_create_ex", C.byref(plan), C.byref(d), flags)
        emu.call("plx_ssfm_destroy", plan)

    d = xpm_ref.desc(n, 2, [1, 1, 1, 1], 1e3, 0.0, [1e-6, 1e-6], 1e3, 5e-3, betat, db1)
    with pytest.raises(PolmuxError, match="CNLSE with separate fields is not yet implemented"):      # fiber.m:854
        create(d, 0)
    d.manakov = 0
    with pytest.raises(PolmuxError, match="CNLSE with separate fields is not yet implemented"):
        create(d, PLX_SSFM_XPM_MANAKOV)
    d.manakov = 1
    with pytest.raises(PolmuxError, match="unknown flag"):
        create(d, 4)
    with pytest.raises(PolmuxError, match="unknown flag"):
        create(d, PLX_SSFM_XPM_MANAKOV | 4)
    create(d, PLX_SSFM_XPM_MANAKOV)
    # one channel: the flag changes nothing, bit for bit (the 'x' of a one-field flag is dropped, fiber.m:224)
    ux, uy = xpm_ref.wdm_frame(nsymb, nt, 1, 10.0)
    d1 = xpm_ref.desc(n, 1, [1, 0, 1, 1], 2e4, ALPHA, [GAM], 1e4, 2e-2, betat[:, :1], db1[:, :1])
    a = xpm_ref.run_host(emu, d1, 0, [(ux, uy)])
    b = xpm_ref.run_host(emu, d1, PLX_SSFM_XPM_MANAKOV, [(ux, uy)])
    assert a[1][0] == b[1][0] and a[0][0] == b[0][0] and a[3] == b[3]
    assert np.array_equal(a[2][0][0], b[2][0][0]) and np.array_equal(a[2][0][1], b[2][0][1])
    # several channels without the 'x': the flag changes nothing either
    fr = xpm_ref.wdm_frame(nsymb, nt, 2, 10.0)
    d2 = xpm_ref.desc(n, 2, [1, 0, 1, 0], 2e4, ALPHA, [GAM, GAM], 1e4, 2e-2, betat, db1)
    a = xpm_ref.run_host(emu, d2, 0, [fr])
    b = xpm_ref.run_host(emu, d2, PLX_SSFM_XPM_MANAKOV, [fr])
    assert a[3] == b[3] and np.array_equal(a[2][0][0], b[2][0][0]) and np.array_equal(a[2][0][1], b[2][0][1])


def test_xpm_model_against_one_field(oracle):
    """Oracle only (no kernels): separate fields with the operator of DESIGN 8c against plxo.matrix_ssfm on ONE field.
    Condition: the error with XPM is at most a tenth of the error without, on every channel.
    Observed (relative L2 per channel; 328 steps for the one field, 63 / 64 for the separate fields):
    with XPM 0.0049 / 0.0066 / 0.0049, without 0.324 / 0.325 / 0.323: a factor of 66 / 50 / 65."""
    z1 = np.zeros(1)

    def one(ux, uy, bt):
        rc, _, nc, ox, oy = oracle.matrix_ssfm(ux, uy, bt, 0 * bt, 2e4, 5e-3, [GAM], ALPHA, LSPAN, 1, 1, [1, 0, 1, 0], z1, z1, z1)
        assert rc == 0
        print("one field: %d steps" % nc)
        return ox[:, 0], oy[:, 0]

    def sep(ux, uy, bt, xpm):
        rc, _, nc, sx, sy = xpm_ref.matrix_ssfm_xpm(oracle, ux, uy, bt, 0 * bt, 2e4, 5e-3, [GAM] * 3, ALPHA, LSPAN, 1, [1, 0, 1, xpm], z1, z1, z1)
        print("separate fields, xpm=%d: %d steps" % (xpm, nc))
        return sx, sy

    with_xpm, without = xpm_ref.model_vs_one_field(sep, one)
    print("with XPM %s  without %s  factor %s" % (with_xpm, without, without / with_xpm))
    assert np.all(with_xpm <= 0.1 * without)
