"""GPU tests of digital backpropagation (plx_dbp_*, polmux_amd.dbp, HotPathConfig(equaliser='dbp')) on the MI355X: both
routes against the numpy operator of tests/test_dbp.py, the exact inverse of the device propagator, the gamma = 0 limit,
and the receiver through HotPath."""
import ctypes as C
import math

import numpy as np
import pytest

from polmux_amd import _abi, synth
from polmux_amd.dbp import DbpPlan, dbp_betat, dbp_desc
from tests.test_dbp import ALPHA, D17, FS, GAM, L80, LAM, np_dbp, rand_frames, rel

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).cuda()


def _run(u, desc, scale, streamed):
    import torch
    plan = DbpPlan(desc, streamed=streamed)
    try:
        x = _dev(u)
        out = torch.empty_like(x)
        sc = torch.as_tensor(np.asarray(scale, dtype=float)).cuda()
        plan.apply(x, out, sc)
        torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        plan.close()


@pytest.mark.parametrize("n", [256, 2048, 4096, 32768])
@pytest.mark.parametrize("manakov", [1, 0])
@pytest.mark.parametrize("explicit", [False, True])
def test_gpu_dbp_parity_both_routes(n, manakov, explicit):
    """3 frames with their own scale, 2 spans, 3 steps per span (uniform, or an explicit unequal list): the resident
    route (n <= 4096) and the forced streamed route each match the numpy operator to 1e-10, and each other to 1e-12."""
    scale = np.array([0.5, 1.0, 3.0])
    u = rand_frames(n, 3, 6.0, n + manakov) / scale.reshape(-1, 1, 1)
    bt = dbp_betat(n, FS, LAM, D17, 60.0)
    dz = [2e4, 3.5e4, 2.5e4] if explicit else [L80 / 3] * 3
    d = dbp_desc(n, 4, 2, dz if explicit else 3, manakov, L80, ALPHA, GAM, 1.0, bt)
    ref = np_dbp(u, bt, 2, dz, manakov, L80, ALPHA, GAM, 1.0, scale)
    assert rel(ref, u) > 1e-2
    st = _run(u, d, scale, True)
    assert rel(st, ref) <= 1e-10
    if n <= 4096:
        rs = _run(u, d, scale, False)
        assert rel(rs, ref) <= 1e-10
        assert rel(rs, st) <= 1e-12


@pytest.mark.parametrize("nsymb, streamed", [(16, False), (256, True)])
@pytest.mark.parametrize("manakov", [1, 0])
def test_gpu_dbp_inverts_the_propagator(nsymb, streamed, manakov):
    """A noiseless full-rate frame (nt = 64: nfft 1024 on the resident route, 2^14 on the streamed one) through 2 spans
    of the device propagator with a fixed step list (plx_ssfm_set_step_sequence, flag 'g-s-') and an amplifier after
    each span; DBP with the same step list, xi = 1 and fiber_tables' betat and gam recovers the launched field to 1e-9."""
    import torch
    from polmux_amd.fiber import fiber_tables, parse_flag
    from polmux_amd.gstate import GSTATE
    nt = 64
    n = nsymb * nt
    GSTATE.NSYMB, GSTATE.NT, GSTATE.NCH, GSTATE.SYMBOLRATE = nsymb, nt, 1, 28.0
    GSTATE.FN, GSTATE.LAMBDA = synth.fn_grid(nsymb, nt), np.array([1550.0])
    x = {"length": L80, "alphadB": 0.2, "aeff": 80.0, "n2": 2.7e-20, "lambda": 1550.0, "disp": 17.0, "slope": 0.0,
         "dphimax": 5e-3, "dzmax": 2e4}
    fls, dphimaxt, dzmaxt = parse_flag("g-s-", 1, x)
    t = fiber_tables(x, fls, 1, 0.0)
    ux0, uy0, _, _ = synth.pdm_qpsk_field(nsymb, nt, 6.0)
    lib = _abi.get()
    sd = _abi.SsfmDesc()
    sd.nfft, sd.nfc, sd.dual_pol, sd.max_frames = n, 1, 1, 1
    for i in range(4):
        sd.fls[i] = fls[i]
    sd.dzmaxt, sd.dphimaxt, sd.alphalin, sd.length, sd.nplates, sd.manakov = dzmaxt, dphimaxt, t["alphalin"], L80, 1, manakov
    keep = (np.ascontiguousarray(t["gam"]), np.asfortranarray(t["betat"]), np.asfortranarray(t["db1"]))
    sd.gam, sd.betat, sd.db1 = (a.ctypes.data for a in keep)
    plan = C.c_void_p()
    lib.call("plx_ssfm_create", C.byref(plan), C.byref(sd))
    try:
        steps = np.array([1.5e4, 2.5e4, 2e4, 2e4])
        lib.call("plx_ssfm_set_step_sequence", plan, steps.ctypes.data, len(steps))
        lib.call("plx_ssfm_log_steps", plan, 16)
        ux, uy = _dev(ux0[None]), _dev(uy0[None])
        st = torch.cuda.current_stream().cuda_stream
        logs = []
        for _ in range(2):
            lib.call("plx_ssfm_propagate_dev", plan, ux.data_ptr(), uy.data_ptr(), 1, st)
            torch.cuda.synchronize()
            nc = np.zeros(1, np.int32)
            lib.call("plx_ssfm_results", plan, 1, None, nc.ctypes.data)
            log = np.zeros(16)
            lib.call("plx_ssfm_step_sequence", plan, 0, log.ctypes.data, 16)
            logs.append(log[:nc[0]].copy())
            g = math.exp(0.5 * t["alphalin"] * L80)
            ux.mul_(g)
            uy.mul_(g)
    finally:
        lib.call("plx_ssfm_destroy", plan)
    np.testing.assert_array_equal(logs[0], logs[1])
    rx = torch.stack([ux[0], uy[0]]).unsqueeze(0).contiguous().cpu().numpy()
    tx = np.stack([ux0, uy0])[None]
    assert rel(rx, tx) > 1e-1                                     # dispersion and Kerr phase really are there
    d = dbp_desc(n, 1, 2, logs[0], manakov, L80, t["alphalin"], t["gam"][0], 1.0, t["betat"][:, 0])
    got = _run(rx, d, [1.0], streamed)
    assert rel(got, tx) <= 1e-9


def test_gpu_dbp_without_kerr_is_the_circular_cd_filter():
    """gamma = 0: both routes equal ifft(fft(u) exp(+i betat L nspans)), the circular form of CDE_OFDE's filter, to 1e-12
    (loss and amplifiers cancel); and DBP() on numpy arrays and on device tensors agrees with it."""
    from polmux_amd import DBP
    n = 2048
    u = rand_frames(n, 2, 4.0, 3)
    bt = dbp_betat(n, FS, LAM, D17, 0.0)
    ref = np.fft.ifft(np.fft.fft(u, axis=-1) * np.exp(1j * bt * 3 * L80), axis=-1)
    d = dbp_desc(n, 2, 3, 4, 1, L80, ALPHA, 0.0, 1.0, bt)
    for streamed in (False, True):
        assert rel(_run(u, d, [1.0, 1.0], streamed), ref) <= 1e-12
    ox, oy = DBP(u[0, 0], u[0, 1], FS, LAM, L80, 3, 0.2, D17, 0.0, 0.0, 4)
    assert rel(np.stack([ox, oy]), ref[0]) <= 1e-12
    tx, ty = DBP(_dev(u[1, 0]), _dev(u[1, 1]), FS, LAM, L80, 3, 0.2, D17, 0.0, 0.0, 4)
    assert rel(np.stack([tx.cpu().numpy(), ty.cpu().numpy()]), ref[1]) <= 1e-12


def _ladder(equaliser):
    import torch
    from polmux_amd import pipeline
    # CDE with a 2048-point block (overlap 1024 samples): the 800 km of dispersion fit in the overlap, so that CDE is
    # limited by the Kerr effect and not by its block length
    cfg = pipeline.HotPathConfig(nsymb=1024, nt=16, pavg_mw=1.0, nspans=10, cma_mu=1 / 1000, freqavg=64, fft_length=2048,
                                 cde_L=1024, equaliser=equaliser, dbp_steps=4)
    hp = pipeline.HotPath(cfg, max_frames=3)
    try:
        ux, uy = hp.make_batch(3, launch_scale=[1.0, 10 ** 0.4, 10 ** 0.8])
        hp.fibre(ux, uy)
        hp.receive(ux, uy)
        evm = hp.evm(3).cpu().numpy()
        err = hp.errors_resolved(3).cpu().numpy()
        torch.cuda.synchronize()
        return evm, err
    finally:
        hp.close()


def test_gpu_dbp_helps_at_high_launch_power():
    """10 x 80 km, noiseless fibre, pick front end, launch ladder 0 / +4 / +8 dBm (nsymb 1024, nt 16).  At +8 dBm the
    EVM after DBP (4 steps per span) is below 0.75 x the EVM after CDE, and DBP makes no more bit errors than CDE.
    Calibrated on the CPU with the numpy DBP of tests/test_dbp.py, the CPU oracle's propagation (matrix_ssfm, same step
    rule), its CDE_OFDE and its DspPdmCohQpsk chain on the same frames: EVM with CDE / DBP = 0.028 / 0.018 at 0 dBm,
    0.049 / 0.027 at +4 dBm, 0.165 / 0.079 at +8 dBm (ratio 2.08 at +8 dBm; the test asks for 1.33)."""
    e_cde, b_cde = _ladder("cde")
    e_dbp, b_dbp = _ladder("dbp")
    assert e_dbp[2] < 0.75 * e_cde[2]
    assert e_dbp[0] <= e_cde[0]
    assert (b_dbp <= b_cde).all()


def test_gpu_dbp_streamed_route_through_hotpath():
    """config[4]'s receive length (nsymb 16384, nt 4: 32768 samples per polarisation) takes the streamed route inside
    HotPath: 2 frames, 3 spans; the equalised samples are the numpy DBP of the received ones, and the frames decode."""
    import torch
    from polmux_amd import pipeline
    cfg = pipeline.HotPathConfig(nsymb=16384, nt=4, pavg_mw=2.0, nspans=3, equaliser="dbp", dbp_steps=2)
    hp = pipeline.HotPath(cfg, max_frames=2)
    try:
        ux, uy = hp.make_batch(2)
        hp.fibre(ux, uy)
        hp.receive(ux, uy)
        torch.cuda.synchronize()
        rx, eq = hp.rx[:2].cpu().numpy(), hp.eq[:2].cpu().numpy()
        bt = dbp_betat(hp.Lrx, 2 * cfg.symbolrate * 1e9, cfg.lam * 1e-9, cfg.disp * 1e-6, 0.0)
        gam = 2 * math.pi * cfg.n2 / (cfg.lam * cfg.aeff) * 1e18
        ref = np_dbp(rx, bt, 3, [cfg.length / 2] * 2, False, cfg.length, hp.alphalin, gam, 1.0, [hp.dbp_scale] * 2)
        assert rel(eq, ref) <= 1e-10
        assert int(hp.errors_resolved(2).sum()) == 0
    finally:
        hp.close()
