"""Manakov cross-phase modulation between dual-polarisation 'sepfields' channels (PLX_SSFM_XPM_MANAKOV, DESIGN.md section
8c) on the MI355X: k_stokes_sum + k_col_fwd_xpm at production sizes against the CPU reference of tests/xpm_ref.py, batching,
the public interface (fiber(), HotPath) and the operator against the device's own single-field plan."""
import ctypes as C

import numpy as np
import pytest

from tests import xpm_ref

pytestmark = pytest.mark.gpu

FIELD_RTOL = 1e-9
ALPHA, GAM, LSPAN = 4.6e-5, 1.3e-6, 8e4
REF_MSG = "CNLSE with separate fields is not yet implemented"


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from polmux_amd import _abi
    b = _abi.get()
    assert b.path.endswith("polmux_amd/lib/libpolmux_hip.so")
    return b


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def run_gpu(lib, d, flags, frames, brf=None, log_steps=0):
    """The frames (a list of (ux, uy), each [n, nfc]) as one batch through a plan on the device.
    -> (firstdz[F], ncycle[F], [(ux, uy)], info[8]) and, with log_steps, every frame's own step sequence"""
    import torch
    F = len(frames)
    plan = C.c_void_p()
    lib.call("plx_ssfm_create_ex", C.byref(plan), C.byref(d), flags)
    try:
        if brf is not None:
            a, b, c = (np.ascontiguousarray(np.concatenate([p[i] for p in brf]), dtype=float) for i in range(3))
            lib.call("plx_ssfm_set_birefringence", plan, _vp(a), _vp(b), _vp(c), F)
        if log_steps:
            lib.call("plx_ssfm_log_steps", plan, log_steps)
        gx = torch.from_numpy(np.ascontiguousarray(np.stack([f[0].T for f in frames]))).cuda()      # [F, nfc, n]
        gy = torch.from_numpy(np.ascontiguousarray(np.stack([f[1].T for f in frames]))).cuda()
        lib.call("plx_ssfm_propagate_dev", plan, gx.data_ptr(), gy.data_ptr(), F, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        first, ncyc = np.zeros(F), np.zeros(F, np.int32)
        lib.call("plx_ssfm_results", plan, F, _vp(first), _vp(ncyc))
        info = (C.c_int32 * 8)()
        lib.call("plx_ssfm_info", plan, info)
        hx, hy = gx.cpu().numpy(), gy.cpu().numpy()
        dzs = []
        for f in range(F if log_steps else 0):
            dz = np.zeros(min(int(ncyc[f]), log_steps))
            lib.call("plx_ssfm_step_sequence", plan, f, _vp(dz), dz.size)
            dzs.append(dz)
    finally:
        lib.call("plx_ssfm_destroy", plan)
    res = (first, ncyc, [(hx[f].T, hy[f].T) for f in range(F)], list(info))
    return res + (dzs,) if log_steps else res


# nsymb, nt, channels, plates, span, launch powers [mW]: 2^12 (k_row), 2^16 with PMD (k_row256r<PMD>), 2^18 (k_rowreg)
SIZES = {"2^12": (256, 16, 3, 1, 2e4, (4.0, 6.0, 9.0)),
         "2^12-6ch": (256, 16, 6, 1, 1e4, (3.0, 4.5, 6.0)),          # k_stokes_sum: the unrolled body of four channels, then the tail
         "2^16-pmd": (1024, 64, 3, 6, 1.5e4, (3.0, 5.0, 7.0)),
         "2^18": (4096, 64, 2, 1, 1e4, (3.0, 4.5, 6.0))}


def _case(name):
    nsymb, nt, nfc, nplates, L, powers = SIZES[name]
    pmd = 1 if nplates > 1 else 0
    betat, db1 = xpm_ref.tables(nsymb, nt, 1, pmd, nplates, nfc)
    gam = np.array([1.2e-6, 1.3e-6, 1.4e-6, 1.25e-6, 1.35e-6, 1.15e-6])[:nfc]
    frames = [xpm_ref.wdm_frame(nsymb, nt, nfc, p, seed=4 * f) for f, p in enumerate(powers)]
    brf = [xpm_ref.random_plates(nplates, 3 + f) if pmd else (np.zeros(1), np.zeros(1), np.zeros(1)) for f in range(len(powers))]
    d = xpm_ref.desc(nsymb * nt, nfc, [1, 1, 1, 1], L, ALPHA, gam, 1e4, 2e-2, betat, db1, nplates=nplates, frames=len(powers))
    return d, frames, brf, (betat, db1, gam, L, nplates)


@pytest.mark.parametrize("name", list(SIZES))
def test_gpu_xpm_propagation_vs_reference(lib, oracle, name):
    """'gpsx' at production sizes, three frames per batch at different launch powers, against matrix_ssfm_xpm: ncycle
    equal, firstdz to 1e-12, field to 1e-9 of max |u|.  Where the free-running step counts differ (a tie of the step rule:
    zprop within rounding of the fibre end), the reference is run again under the device's own step sequence of that frame,
    as test_gpu_configs.py does.  Observed: DESIGN.md 8c (no frame needed the replay)."""
    from polmux_amd._abi import PLX_SSFM_XPM_MANAKOV
    d, frames, brf, (betat, db1, gam, L, nplates) = _case(name)
    first, ncyc, out, info, dzs = run_gpu(lib, d, PLX_SSFM_XPM_MANAKOV, frames, brf, log_steps=4096)
    assert info[0] == 0                                    # the three-sweep step
    for f in range(len(frames)):
        rc, rfd, rnc, rx, ry = xpm_ref.matrix_ssfm_xpm(oracle, *frames[f], betat, db1, 1e4, 2e-2, gam, ALPHA, L, nplates, [1, 1, 1, 1], *brf[f])
        if rnc != ncyc[f]:
            print("%s frame %d: free-running ncycle %d / %d, reference repeated under the device's step sequence" % (name, f, ncyc[f], rnc))
            assert first[f] == pytest.approx(rfd, rel=1e-12)
            rc, rfd, rnc, rx, ry = xpm_ref.matrix_ssfm_xpm(oracle, *frames[f], betat, db1, 1e4, 2e-2, gam, ALPHA, L, nplates, [1, 1, 1, 1],
                                                           *brf[f], replay_dz=dzs[f])
        ex = np.abs(out[f][0] - rx).max() / np.abs(rx).max()
        ey = np.abs(out[f][1] - ry).max() / np.abs(ry).max()
        print("%s frame %d: p1/p2 %d/%d, ncycle %d / %d, firstdz rel %.3g, field %.3g %.3g" %
              (name, f, info[1], info[2], ncyc[f], rnc, abs(first[f] - rfd) / rfd, ex, ey))
        assert ncyc[f] == rnc and first[f] == pytest.approx(rfd, rel=1e-12)
        assert ex < FIELD_RTOL and ey < FIELD_RTOL
    assert len(set(ncyc.tolist())) > 1                     # the frames did take different step sequences


def test_gpu_xpm_frame_alone_equals_frame_in_batch(lib):
    """A frame propagated alone is bit-identical to the same frame in a batch of three."""
    from polmux_amd._abi import PLX_SSFM_XPM_MANAKOV
    d, frames, brf, _ = _case("2^16-pmd")
    _, ncyc, out, _ = run_gpu(lib, d, PLX_SSFM_XPM_MANAKOV, frames, brf)
    for f in (0, 2):
        _, nc1, o1, _ = run_gpu(lib, d, PLX_SSFM_XPM_MANAKOV, [frames[f]], [brf[f]])
        assert nc1[0] == ncyc[f]
        assert np.array_equal(o1[0][0], out[f][0]) and np.array_equal(o1[0][1], out[f][1])


@pytest.mark.parametrize("plates", [1, 6])
def test_gpu_xpm_fiber_wrapper(lib, oracle, plates):
    """fiber(x, 'gpsx') with x.xpm_dualpol = 'manakov' on a three-channel 'sepfields' field (dgd = 0 with one zero plate:
    the PMD-free case; six given plates) against matrix_ssfm_xpm on fiber()'s own tables; without the option the
    reference's error; the option is part of the plan cache key."""
    import sys
    import polmux_amd as px
    from polmux_amd import synth
    from polmux_amd._abi import PolmuxError
    from polmux_amd.gstate import GSTATE, to_host_field
    fibermod = sys.modules["polmux_amd.fiber"]
    nsymb, nt, nch = 256, 16, 3
    x = dict(length=2e4, alphadB=0.2, aeff=80.0, n2=2.7e-20, disp=17.0, slope=0.0, dphimax=2e-2, dzmax=1e4, manakov="yes")
    x["lambda"] = 1550.0
    db0, th, ep = xpm_ref.random_plates(plates, 5) if plates > 1 else (np.zeros(1), np.zeros(1), np.zeros(1))
    x.update(dgd=0.1 if plates > 1 else 0.0, db0=db0, theta=th, epsilon=ep)

    def stage():
        px.reset_all(nsymb, nt, nch)
        GSTATE.SYMBOLRATE = 28.0
        px.lasersource(np.full(nch, 6.0), 1550.0, 0.4)
        cols = [synth.pdm_qpsk_field(nsymb, nt, 6.0, 2 + 2 * k, 3 + 2 * k) for k in range(nch)]
        px.create_field("sepfields", np.stack([c[0] for c in cols], 1), np.stack([c[1] for c in cols], 1), dict(power="average"))
        return to_host_field(GSTATE.FIELDX), to_host_field(GSTATE.FIELDY)
    fibermod.release_plans()
    try:
        ux, uy = stage()
        with pytest.raises(PolmuxError, match=REF_MSG):
            px.fiber(x, "gpsx")
        with pytest.raises(ValueError, match="xpm_dualpol"):
            px.fiber(dict(x, xpm_dualpol="cnlse"), "gpsx")
        ux, uy = stage()
        brf = px.fiber(dict(x, xpm_dualpol="manakov"), "gpsx")
        gx, gy = to_host_field(GSTATE.FIELDX), to_host_field(GSTATE.FIELDY)
        fls = [1, 1, 1, 1]
        gam = fibermod.fiber_tables(x, fls, nch, 0.0)["gam"]
        rc, rfd, rnc, rx, ry = xpm_ref.matrix_ssfm_xpm(oracle, ux, uy, brf["betat"], brf["db1"], 1e4, 2e-2, gam, brf_alpha(x), 2e4,
                                                       plates, fls, db0, th, ep)
        ex, ey = np.abs(gx - rx).max() / np.abs(rx).max(), np.abs(gy - ry).max() / np.abs(ry).max()
        print("fiber() plates=%d: ncycle %d / %d, field %.3g %.3g" % (plates, brf["ncycle"], rnc, ex, ey))
        assert brf["ncycle"] == rnc and brf["firstdz"] == pytest.approx(rfd, rel=1e-12)
        assert ex < FIELD_RTOL and ey < FIELD_RTOL
        # 'gps-' on the same field: another plan (the option is in the cache key), a different field, the same first step
        stage()
        b0 = px.fiber(dict(x, xpm_dualpol="manakov"), "gps-")
        assert len(fibermod._plans) == 2 and b0["firstdz"] == brf["firstdz"]
        assert np.abs(to_host_field(GSTATE.FIELDX) - gx).max() > 1e-3 * np.abs(gx).max()
        stage()
        with pytest.raises(PolmuxError, match=REF_MSG):      # ... and the plan with the option is not handed to a call without it
            px.fiber(x, "gpsx")
    finally:
        fibermod.release_plans()


def brf_alpha(x):
    import math
    return (math.log(10) * 1e-4) * x["alphadB"]              # fiber.m:302


def test_gpu_xpm_hotpath(lib, oracle):
    """HotPath(HotPathConfig(nch=3, flag='gpsx', manakov='yes', xpm_dualpol='manakov')): the batched fibre against
    matrix_ssfm_xpm, a run through receive(), and the configurations that must raise."""
    import torch
    from polmux_amd import pipeline
    from polmux_amd._abi import PolmuxError
    kw = dict(nsymb=256, nt=16, nch=3, flag="gpsx", manakov="yes", pavg_mw=4.0, length=2e4, dphimax=2e-2, dzmax=1e4, nplates=6,
              cma_mu=1 / 300, freqavg=20, variants=3)
    with pytest.raises(PolmuxError, match=REF_MSG):
        pipeline.HotPath(pipeline.HotPathConfig(**kw), max_frames=2)
    with pytest.raises(ValueError, match="dbp"):
        pipeline.HotPath(pipeline.HotPathConfig(xpm_dualpol="manakov", equaliser="dbp", **kw), max_frames=2)
    with pytest.raises(ValueError, match="xpm_dualpol"):
        pipeline.HotPath(pipeline.HotPathConfig(xpm_dualpol="yes", **kw), max_frames=2)
    cfg = pipeline.HotPathConfig(xpm_dualpol="manakov", **kw)
    hp = pipeline.HotPath(cfg, max_frames=2)
    try:
        db0, th, ep = hp.set_random_pmd(range(2))
        ux, uy = hp.make_batch(2, launch_scale=[1.0, 1.6])
        hx, hy = ux.cpu().numpy(), uy.cpu().numpy()              # [F, nch, n]
        hp.fibre(ux, uy)
        torch.cuda.synchronize()
        first, ncyc = np.zeros(2), np.zeros(2, np.int32)
        lib.call("plx_ssfm_results", hp.ssfm, 2, _vp(first), _vp(ncyc))
        gam, betat, db1 = hp._keep
        for f in range(2):
            rc, rfd, rnc, rx, ry = xpm_ref.matrix_ssfm_xpm(oracle, hx[f].T, hy[f].T, betat, db1, 1e4, 2e-2, gam, hp.alphalin, 2e4,
                                                           6, hp.fls, db0[f], th[f], ep[f])
            gx, gy = ux[f].cpu().numpy().T, uy[f].cpu().numpy().T
            ex, ey = np.abs(gx - rx).max() / np.abs(rx).max(), np.abs(gy - ry).max() / np.abs(ry).max()
            print("HotPath frame %d: ncycle %d / %d, field %.3g %.3g" % (f, ncyc[f], rnc, ex, ey))
            assert ncyc[f] == rnc and first[f] == pytest.approx(rfd, rel=1e-12)
            assert ex < FIELD_RTOL and ey < FIELD_RTOL
        assert hp.fls == [1, 1, 1, 1] and ncyc[0] != ncyc[1]
        err = hp.receive(ux, uy)
        torch.cuda.synchronize()
        assert tuple(err.shape) == (2 * 3, 2)                     # an error count per channel-frame and polarisation
        sym = hp.sym[:6].cpu().numpy()
        assert np.all(np.isfinite(sym.real)) and np.all(np.isfinite(sym.imag)) and np.all(err.cpu().numpy() >= 0)
    finally:
        hp.close()


def test_gpu_xpm_model_against_the_devices_single_field_plan(lib):
    """The condition of test_xpm_model_against_one_field on the device: separate fields with XPM (this feature's kernels)
    against the device's own single-field plan, Manakov.  The error with XPM is at most a tenth of the error without, on
    every channel."""
    from polmux_amd._abi import PLX_SSFM_XPM_MANAKOV

    def one(ux, uy, bt):
        d = xpm_ref.desc(len(ux), 1, [1, 0, 1, 0], LSPAN, ALPHA, [GAM], 2e4, 5e-3, bt[:, None], 0 * bt[:, None])
        _, nc, out, _ = run_gpu(lib, d, 0, [(ux[:, None], uy[:, None])])
        print("one field: %d steps" % nc[0])
        return out[0][0][:, 0], out[0][1][:, 0]

    def sep(ux, uy, bt, xpm):
        d = xpm_ref.desc(len(ux), 3, [1, 0, 1, xpm], LSPAN, ALPHA, [GAM] * 3, 2e4, 5e-3, bt, 0 * bt)
        _, nc, out, info = run_gpu(lib, d, PLX_SSFM_XPM_MANAKOV, [(ux, uy)])
        assert not xpm or info[0] == 0
        print("separate fields, xpm=%d: %d steps" % (xpm, nc[0]))
        return out[0]

    with_xpm, without = xpm_ref.model_vs_one_field(sep, one, length=LSPAN)
    print("with XPM %s  without %s  factor %s" % (with_xpm, without, without / with_xpm))
    assert np.all(with_xpm <= 0.1 * without)
