"""The two host-driven users of the SSFM plan's FFT engine on the MI355X, at the default geometry of every frame size up to
2^20 samples: the spectral filter (plx_filter_apply_dev, and through it the streamed route of DBP) against numpy, and the
adaptive step of fiber() (x.ltol, x.dphiadapt) against the oracle.  Neither goes through the propagator's step loop; the
emulated forms of the same checks, at forced geometries, are tests/test_emu_fft_paths.py."""
import ctypes as C

import numpy as np
import pytest

from polmux_amd.dbp import DbpPlan, dbp_betat, dbp_desc
from tests.test_dbp import ALPHA, D17, FS, GAM, L80, LAM, np_dbp, rand_frames, rel

pytestmark = pytest.mark.gpu

FIELD_RTOL = 1e-9      # as tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from polmux_amd import _abi
    b = _abi.get()
    assert b.path.endswith("polmux_amd/lib/libpolmux_hip.so")
    return b


# the row pass of the filter's plan at its default geometry: (p1, p2, info[6], info[7]) of plx_ssfm_info -- k_row with
# sixteen-point rows up to 2^12, k_rowsm at 2^13 ... 2^15, the generic k_row at 2^16 (k_row256r takes no multiplier table),
# k_rowreg with the table at 2^17 ... 2^19, k_row4k at 2^20
FILTER_GEOMETRY = {8: (4, 4, 128, 0), 9: (5, 4, 128, 0), 10: (6, 4, 128, 0), 11: (7, 4, 128, 0), 12: (8, 4, 128, 0),
                   13: (8, 5, 64, 2), 14: (8, 6, 64, 2), 15: (8, 7, 64, 2), 16: (8, 8, 64, 0), 17: (8, 9, 256, 2),
                   18: (8, 10, 256, 2), 19: (8, 11, 256, 2), 20: (8, 12, 256, 1)}


def _filter_geometry(lib, n, frames):
    """(p1, p2, info[6], info[7]) of a plan made from the descriptor plx_filter_create builds (plx_front.hip)"""
    from polmux_amd._abi import SsfmDesc
    d = SsfmDesc()
    d.nfft, d.nfc, d.dual_pol, d.max_frames = n, 1, 0, frames
    d.dzmaxt, d.dphimaxt, d.length, d.nplates = 1.0, 1.0, 1.0, 1
    keep = (np.zeros(1), np.zeros(n))
    d.gam, d.betat = keep[0].ctypes.data, keep[1].ctypes.data
    plan = C.c_void_p()
    lib.call("plx_ssfm_create", C.byref(plan), C.byref(d))
    info = (C.c_int32 * 8)()
    try:
        lib.call("plx_ssfm_info", plan, info)
    finally:
        lib.call("plx_ssfm_destroy", plan)
    return (info[1], info[2], info[6], info[7])


@pytest.mark.parametrize("p", list(range(8, 21)))
def test_gpu_filter_every_nfft(lib, p):
    """plx_filter_apply_dev on device rows: 3 signals on a plan for 4 -- a random signal, a delta (gives ifft(H)) and a tone of
    bin k (gives H[k] times the tone) -- with a random complex H against numpy's ifft(fft(x) * H) to 2e-14 of max|y|; the
    4th row of the buffer comes back bit-identical."""
    import torch
    n = 1 << p
    assert _filter_geometry(lib, n, 4) == FILTER_GEOMETRY[p]
    rng = np.random.default_rng(p)
    H = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    k = int(rng.choice(np.flatnonzero(np.abs(H[1:]) >= 1.0))) + 1   # (a tone bin where |H| is not small: the transforms' rounding
                                                                    #  scales with the whole of H, the bar with |H[k]|)
    x = np.empty((4, n), np.complex128)
    x[0] = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x[1] = 0
    x[1, 0] = 1
    x[2] = np.exp(2j * np.pi * ((k * np.arange(n)) % n) / n)
    x[3] = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ref = np.fft.ifft(np.fft.fft(x[:3], axis=-1) * H, axis=-1)
    hr, hi = np.ascontiguousarray(H.real), np.ascontiguousarray(H.imag)
    d = torch.from_numpy(x).cuda()
    plan = C.c_void_p()
    lib.call("plx_filter_create", C.byref(plan), n, 4, hr.ctypes.data, hi.ctypes.data)
    try:
        lib.call("plx_filter_apply_dev", plan, d.data_ptr(), 3, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        lib.call("plx_filter_destroy", plan)
    y = d.cpu().numpy()
    errs = [np.abs(y[r] - ref[r]).max() / np.abs(ref[r]).max() for r in range(3)]
    print("filter nfft 2^%d: max-abs error / max|y| = %.2e (random) %.2e (delta) %.2e (tone)" % (p, *errs))
    assert max(errs) <= 2e-14
    hh = np.fft.ifft(H)
    assert np.abs(y[1] - hh).max() <= 2e-14 * np.abs(hh).max()
    assert np.abs(y[2] - H[k] * x[2]).max() <= 2e-14 * abs(H[k])
    assert np.array_equal(y[3].view(np.float64), x[3].view(np.float64))


@pytest.mark.parametrize("p, manakov", [(16, 1), (17, 1), (17, 0), (18, 1), (19, 1), (20, 1)])
def test_gpu_dbp_streamed_large_nfft(p, manakov):
    """The streamed route of DBP (the filter above, one launch per step over both polarisations of every frame, and the
    element-wise Kerr kernel) at 2^16 ... 2^20 samples: 2 frames with their own scale, 2 spans of 2 steps, Manakov at every
    size and the CNLSE at one, against the numpy operator of tests/test_dbp.py to 1e-10 (the bar of the smaller sizes)."""
    import torch
    n = 1 << p
    scale = np.array([0.5, 2.0])
    u = rand_frames(n, 2, 6.0, p + manakov) / scale.reshape(-1, 1, 1)
    bt = dbp_betat(n, FS, LAM, D17, 60.0)
    d = dbp_desc(n, 2, 2, 2, manakov, L80, ALPHA, GAM, 1.0, bt)
    ref = np_dbp(u, bt, 2, [L80 / 2] * 2, manakov, L80, ALPHA, GAM, 1.0, scale)
    assert rel(ref, u) > 1e-2
    plan = DbpPlan(d, streamed=True)
    try:
        x = torch.from_numpy(np.ascontiguousarray(u)).cuda()
        out = torch.empty_like(x)
        plan.apply(x, out, torch.as_tensor(scale).cuda())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
    finally:
        plan.close()
    e = rel(got, ref)
    print("dbp streamed nfft 2^%d %s: max-abs error / max|ref| = %.2e" % (p, "manakov" if manakov else "cnlse", e))
    assert e <= 1e-10


@pytest.mark.parametrize("tolflag", [2, 1])
@pytest.mark.parametrize("p", [16, 18, 20])
def test_gpu_adaptive_step_large_frames(lib, oracle, p, tolflag):
    """fiber(x, 'g-s-') with x.ltol (scalar_a_ssfm, fiber.m:639-679) and with x.dphiadapt (the adaptive first step, :588-611)
    on 2^16, 2^18 and 2^20 samples -- the last one on the 4096-point rows of k_row4k -- against the oracle: ncycle (and nrej)
    equal, firstdz to 1e-9 relative, the field to FIELD_RTOL."""
    import polmux_amd as px
    from polmux_amd import synth
    from polmux_amd.fiber import fiber_tables, parse_flag
    from polmux_amd.gstate import GSTATE, to_host_field
    nt = 16
    nsymb = (1 << p) // nt
    L = 1e4
    px.reset_all(nsymb, nt, 1)
    GSTATE.SYMBOLRATE = 28.0
    px.lasersource(1.5, 1550.0)
    sx, _, _, _ = synth.pdm_qpsk_field(nsymb, nt, 3.0)
    px.create_field("sepfields", sx, None, dict(power="average"))
    u0 = to_host_field(GSTATE.FIELDX)
    x = dict(length=L, alphadB=0.2, aeff=80.0, n2=2.7e-20, disp=17.0, slope=0.0, ltol=1e-6)
    x["lambda"] = 1550.0
    if tolflag == 1:
        x.update(dphiadapt=True, dphimax=2e-2, dzmax=5e3)     # (below the length: fiber.m:139-141 would clamp a longer one)
    px.fiber(x, "g-s-")
    got = to_host_field(GSTATE.FIELDX)
    last = dict(px.fiber.last)
    xx = dict(x)
    xx.setdefault("dphimax", np.inf)
    xx.setdefault("dzmax", x["length"])
    fls, dph, dzm = parse_flag("g-s-", 1, xx)
    t = fiber_tables(xx, fls, 1, 0.0)
    if tolflag == 2:
        ofd, onc, onrej, ou = oracle.scalar_a_ssfm(u0, t["betat"], dzm, dph, t["gam"], t["alphalin"], L, 1e-6, 0.9, fls)
        assert last["nrej"] == onrej
    else:
        ofd, onc, ou = oracle.scalar_ssfm(u0, t["betat"], dzm, dph, t["gam"], t["alphalin"], L, fls, tolflag=1, trg_err=1e-6,
                                          trg_safety=0.9)
    e = np.abs(got - ou).max() / np.abs(ou).max()
    print("adaptive tolflag %d nfft 2^%d: ncycle %d (oracle %d), field error %.2e" % (tolflag, p, last["ncycle"], onc, e))
    assert last["ncycle"] == onc and onc > 3
    assert last["firstdz"] == pytest.approx(ofd, rel=1e-9)
    assert e <= FIELD_RTOL
