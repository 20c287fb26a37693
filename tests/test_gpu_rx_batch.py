"""The receiver kernels (polmux_amd/csrc/plx_rx.hip) at the batch widths the headline and Monte-Carlo runs use (-m gpu):
64 frames and more, where the CMA driver packs 16 frames into a four-wave workgroup (kCmaPackMin), against the CPU oracle
frame by frame.  Every frame has its own input, so a frame that reads or writes a neighbour's data fails; output buffers
reach one frame beyond the call and are filled with NaN first, so an unwritten frame or a write past the last one fails.
Bars as test_gpu_parity.py: driver loops 1e-9 with pass counts equal, CDE 1e-11, decisions bit-exact (1e-10 rad screen)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from polmux_amd import _abi
    b = _abi.get()
    assert b.path.endswith("polmux_amd/lib/libpolmux_hip.so")
    return b


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _st():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _nan(shape):
    return np.full(shape, np.nan + 1j * np.nan)


def _screened_equal(got_bits, ref_sym, want_bits, tol=1e-10):
    """decisions bit-exact, except symbols whose phase sits within tol rad of a decision boundary"""
    ph = np.angle(ref_sym)
    near = (np.abs(np.abs(ph) - np.pi / 2) < tol) | (np.abs(ph) < tol) | (np.abs(np.abs(ph) - np.pi) < tol)    # [nsymb x 2]
    mask = np.repeat(~near, 2, axis=1)
    np.testing.assert_array_equal(got_bits[mask], want_bits[mask])
    assert near.mean() < 1e-3
    return int(near.sum())


def _qpsk(L, seed, noise, A):
    """QPSK of both polarisations through the 2x2 matrix A, plus noise: [L x 2]"""
    r = np.random.default_rng(seed)
    a = np.exp(1j * (np.pi / 4 + np.pi / 2 * r.integers(0, 4, (L, 2))))
    return a @ A + noise * (r.standard_normal((L, 2)) + 1j * r.standard_normal((L, 2)))


def _jones(th, psi):
    return np.array([[np.cos(th), np.sin(th) * np.exp(1j * psi)], [-np.sin(th) * np.exp(-1j * psi), np.cos(th)]])


_NOISE = (0.0, 0.004, 0.015, 0.03, 0.06, 0.1, 0.002)


def _frame_inputs(F, L, seed):
    """per frame: its own symbols, noise level, mixing and initial centre-tap matrix M"""
    xs = [_qpsk(L, seed + f, _NOISE[f % len(_NOISE)], _jones(0.05 + 0.37 * (f % 5), 0.3 * (f % 3))) for f in range(F)]
    Ms = [_jones(0.02 * (f % 11), 0.5 - 0.1 * (f % 7)) for f in range(F)]
    return xs, Ms


# ============================================================ CMA driver ===
# 63 frames: one-wave workgroups of 4 frames; 64, 65 and 200: four-wave workgroups of 16 frames, the last one with idle
# 16-lane groups (65: one frame in it; 200: eight)
@pytest.mark.parametrize("F,taps,L", [(63, 7, 1000), (63, 3, 1024), (64, 3, 1024), (65, 7, 1024), (200, 3, 1000),
                                      (200, 7, 1024)])
def test_cma_driver_batch_vs_oracle(lib, oracle, F, taps, L):
    mu = 1 / 600                                   # pass budget 50 ceil(1/(L mu)) = 50
    xs, Ms = _frame_inputs(F, L, 1000 * F + taps)
    R = np.array([1.0, 1.2])
    dx = _dev(np.stack([x.T for x in xs]))
    dM = _dev(np.stack([m.reshape(4) for m in Ms]))
    dy, dh = _dev(_nan((F + 1, 2, L))), _dev(_nan((F + 1, 2, 2, taps)))
    dp = _dev(np.full(F + 1, -7, np.int32))
    lib.call("plx_poldemux_dev", 1, dx.data_ptr(), dy.data_ptr(), L, F, taps, mu, _vp(R), dM.data_ptr(), dh.data_ptr(),
             dp.data_ptr(), _st())
    y, h, passes = _host(dy), _host(dh), _host(dp)
    assert np.isnan(y[F]).all() and np.isnan(h[F]).all() and passes[F] == -7
    for f in range(F):
        oy, h1, h2, n = oracle.cmapolardemux(xs[f], Ms[f], taps, mu, R)
        assert passes[f] == n, f
        np.testing.assert_allclose(y[f].T, oy, rtol=0, atol=1e-9, err_msg="frame %d" % f)
        np.testing.assert_allclose(h[f, 0].T, h1, rtol=0, atol=1e-9, err_msg="frame %d" % f)
        np.testing.assert_allclose(h[f, 1].T, h2, rtol=0, atol=1e-9, err_msg="frame %d" % f)
    wg = 16 if F >= 64 else 4                       # frames per workgroup (launch_demux)
    for g in range(0, F - 1, wg):                   # the frames of every workgroup stop after different numbers of passes
        assert len(set(passes[g: min(g + wg, F)].tolist())) > 1, g


# =========================================================== EASI driver ===
@pytest.mark.parametrize("method", [2, 3], ids=["easi", "easi_m"])
def test_easi_driver_65_frames_vs_oracle(lib, oracle, method):
    F, L, mu = 65, 256, 1 / 600                    # two 64-lane workgroups, one frame in the second
    xs, Ms = _frame_inputs(F, L, 7000 + method)
    dx = _dev(np.stack([x.T for x in xs]))
    dM = _dev(np.stack([m.reshape(4) for m in Ms]))
    dy, dh = _dev(_nan((F + 1, 2, L))), _dev(_nan((F + 1, 2, 2, 1)))
    dp = _dev(np.full(F + 1, -7, np.int32))
    lib.call("plx_poldemux_dev", method, dx.data_ptr(), dy.data_ptr(), L, F, 1, mu, None, dM.data_ptr(), dh.data_ptr(),
             dp.data_ptr(), _st())
    y, h, passes = _host(dy), _host(dh), _host(dp)
    assert np.isnan(y[F]).all() and np.isnan(h[F]).all() and passes[F] == -7
    ref = oracle.easipolardemux if method == 2 else oracle.easipolardemux_m
    for f in range(F):
        oy, h1, h2, n = ref(xs[f], Ms[f], mu)
        assert passes[f] == n, f
        np.testing.assert_allclose(y[f].T, oy, rtol=0, atol=1e-9, err_msg="frame %d" % f)
        np.testing.assert_allclose(h[f, 0].T, h1, rtol=0, atol=1e-9, err_msg="frame %d" % f)
        np.testing.assert_allclose(h[f, 1].T, h2, rtol=0, atol=1e-9, err_msg="frame %d" % f)
    if method == 2:                                  # (the .m twin runs its whole budget on these frames)
        assert len(set(passes.tolist())) > 2


# ============================================================== DSP plan ===
@pytest.mark.parametrize("kind", ["cma", "cma_txpolars1", "combo"])
def test_dsp_plan_65_frames_vs_oracle(lib, oracle, kind):
    """plx_dsp_run_dev on 65 frames of a plan made for 80.  With txpolars 1, k_rotpolar writes each frame's initial M from
    its own Kikuchi ratio r = mean(x1./x2); the frames cover both branches of rotpolar (|r| < 0.5 and |r| >= 0.5)."""
    from polmux_amd._abi import DspParams
    F, Fmax, L, power = 65, 80, 256, 2.0
    Lin = 2 * L
    r = np.random.default_rng(31)
    ins, ratios = [], []
    for f in range(F):
        beta = 1.2 * (f % 13) / 12                  # x1 = a1 + beta e^{i gamma} a2: r ~ beta e^{i gamma}
        A = np.array([[1.0, 0.25 * np.exp(0.4j * f)], [beta * np.exp(1j * (0.3 + 0.2 * f)), 1.0]])
        s = _qpsk(L, 500 + f, _NOISE[f % len(_NOISE)], A)
        s = s * np.exp(1j * (2 * np.pi * (1 + f % 3) / L * np.arange(L) + 0.1 * f))[:, None]
        x = r.standard_normal((Lin, 2)) + 1j * r.standard_normal((Lin, 2))
        x[::2] = s * 4 * np.sqrt(power)
        ins.append(x)
        ratios.append(abs(np.mean(s[:, 0] / s[:, 1])))
    ratios = np.array(ratios)
    if kind == "cma_txpolars1":
        assert (ratios < 0.5).sum() >= 5 and (ratios >= 0.5).sum() >= 5
    polmethod = {"cma": 1, "cma_txpolars1": 1, "combo": 3}[kind]
    txpol = 1 if kind == "cma_txpolars1" else 2
    p = DspParams()
    for k, v in dict(workatbaudrate=0, applynlr=0, nlralpha=0.0, power_mw=power, applypol=1, polmethod=polmethod,
                     cma_mu=1 / 600, cma_taps=7, cma_txpolars=txpol, cma_phizero=0.0, easi_mu=1 / 600, easi_txpolars=2,
                     easi_phizero=0.0, modorder=2, freqavg=20, phasavg=3, poworder=2).items():
        setattr(p, k, v)
    p.cma_R[0], p.cma_R[1] = 1.0, 1.0
    plan = C.c_void_p()
    lib.call("plx_dsp_create", C.byref(plan), Lin, 2, Fmax, C.byref(p))
    try:
        din, dout = _dev(np.stack([x.T for x in ins])), _dev(_nan((F + 1, 2, L)))
        lib.call("plx_dsp_run_dev", plan, din.data_ptr(), dout.data_ptr(), F, _st())
        out = _host(dout)
    finally:
        lib.call("plx_dsp_destroy", plan)
    assert np.isnan(out[F]).all()
    op = oracle.dsp_params(power_mw=power, applypol=True, polmethod="combo" if kind == "combo" else "cma", cma_mu=1 / 600,
                           cma_taps=7, cma_txpolars=txpol, easi_mu=1 / 600, modorder=2, freqavg=20, phasavg=3, poworder=2)
    for f in range(F):
        ref = oracle.dsp_pdm_coh_qpsk(ins[f], op)
        np.testing.assert_allclose(out[f].T, ref, rtol=0, atol=1e-9, err_msg="frame %d" % f)


# ========================================================= whole receiver ===
def _rx_oracle(oracle, cfg, hp, ox, oy):
    """2-sps pick -> CDE_OFDE -> DspPdmCohQpsk on the oracle (the 'pick' branch of test_gpu_configs._rx_oracle);
    returns (symbols [nsymb x 2], decided bits)"""
    half = cfg.nt // 2
    rx = np.stack([ox[::half], oy[::half]], 1) * hp.rx_scale
    ex, ey, _ = oracle.cde_ofde(rx[:, 0], rx[:, 1], 2 * cfg.symbolrate * 1e9, cfg.lam * 1e-9, cfg.length * cfg.nspans,
                                cfg.disp * 1e-6, 0.0, cfg.fft_length, cfg.cde_L)
    op = oracle.dsp_params(power_mw=hp.power_mw, applypol=True, polmethod="cma", cma_mu=cfg.cma_mu, cma_taps=cfg.cma_taps,
                           freqavg=cfg.freqavg, phasavg=cfg.phasavg, poworder=cfg.poworder)
    ref = oracle.dsp_pdm_coh_qpsk(np.stack([ex, ey], 1), op)
    return ref, oracle.samp2pat_coherent(np.angle(ref))


def test_hot_path_receive_65_frames_three_variants_vs_oracle(lib, oracle):
    """HotPath.receive on 65 frames carrying three Tx waveforms (variants=3: per-frame patterns, pat_frame_stride > 0), each
    frame with its own polarisation mixing, carrier offset and noise.  No fibre: the CDE undoes 1 km of dispersion the field
    never had, a mild distortion the 7-tap CMA absorbs.  Every frame's symbols, error count against its own variant's bits,
    and EVM."""
    from polmux_amd import pipeline
    F = 65
    cfg = pipeline.HotPathConfig(nsymb=256, nt=16, length=1e3, cma_mu=1 / 600, freqavg=20, variants=3)
    hp = pipeline.HotPath(cfg, max_frames=F + 1)
    try:
        n = cfg.nfft
        loss = np.exp(-0.5 * hp.alphalin * cfg.length)             # what the span would have taken (rx_scale restores it)
        r = np.random.default_rng(65)
        t = np.arange(n)
        fx, fy = [], []
        for f in range(F):
            vx, vy, _ = hp.var_host[f % 3]
            J = _jones(0.05 * (f % 7), 0.4 * (f % 5))      # (mild: most frames decide in the right quadrant)
            u = np.stack([vx, vy], 1) @ J * np.exp(1j * (2 * np.pi * (f % 4 - 1.5) / n * t + 0.1 * (f % 5 - 2)))[:, None]
            sig = 0.01 * (1 + f % 5) * np.sqrt(hp.power_mw / 2)
            u = loss * (u + sig * (r.standard_normal((n, 2)) + 1j * r.standard_normal((n, 2))))
            fx.append(u[:, 0])
            fy.append(u[:, 1])
        ux, uy = _dev(np.stack(fx)), _dev(np.stack(fy))
        err = _host(hp.receive(ux, uy)).copy()
        sym = _host(hp.sym[:F]).copy()
        evm = _host(hp.evm(F)).copy()
        assert hp.CF == F + 1 and hp.nvar == 3
    finally:
        hp.close()

    def counts(want, bits):
        return [int((want[:, :2] != bits[:, :2]).sum()), int((want[:, 2:] != bits[:, 2:]).sum())]
    refs, seen = [], 0
    for f in range(F):
        ref, want = _rx_oracle(oracle, cfg, hp, fx[f], fy[f])
        refs.append(ref)
        np.testing.assert_allclose(sym[f].T, ref, rtol=0, atol=1e-9, err_msg="frame %d" % f)
        got_bits = oracle.samp2pat_coherent(np.angle(sym[f].T))
        near = _screened_equal(got_bits, ref, want)
        e = counts(want, hp.var_host[f % 3][2])
        if near == 0:
            assert err[f].tolist() == e, f
        else:                                        # a screened symbol may move a count by its two bits at most
            assert np.abs(err[f] - e).sum() <= 2 * near, f
        if f % 3 and counts(want, hp.var_host[0][2]) != e:
            seen += 1
    assert seen >= 10        # frames whose counts against variant 0's bits differ: a lost pattern offset shows there
    # EVM of every frame: mean |s - s_hat|^2 over the oracle's symbols (both columns), s_hat the decided QPSK point
    ref = np.stack([rr.T for rr in refs])
    hat = (np.where(ref.real >= 0, 1, -1) + 1j * np.where(ref.imag > 0, 1, -1)) / np.sqrt(2)
    np.testing.assert_allclose(evm, (np.abs(ref - hat) ** 2).mean(axis=(1, 2)), rtol=0, atol=5e-9)
    hs = (np.where(sym.real >= 0, 1, -1) + 1j * np.where(sym.imag > 0, 1, -1)) / np.sqrt(2)
    np.testing.assert_allclose(evm, (np.abs(sym - hs) ** 2).mean(axis=(1, 2)), rtol=1e-13)


# =================================================================== CDE ===
# 2048 and 4096 points: H read from global memory (h_in_lds = 0), one block per workgroup, more than 64 KB of LDS;
# 2048/1024 is the CDE of test_gpu_dbp.py's DBP-versus-CDE margin (10 x 80 km at 56 GS/s)
@pytest.mark.parametrize("N,L,nx", [(2048, 1024, 2048), (2048, 2048, 2048), (4096, 4096, 4096), (4096, 2048, 8193)])
def test_cde_130_signals_vs_oracle(lib, oracle, N, L, nx):
    nsig = 130
    r = np.random.default_rng(N + nx)
    x = r.standard_normal((nsig, nx)) + 1j * r.standard_normal((nsig, nx))
    H = oracle.cde_transfer(N, 56e9, 1.55e-6, 8e5, 17e-6, 0.08e3)
    Hi = np.ascontiguousarray(H).view(np.float64)
    plan = C.c_void_p()
    lib.call("plx_cde_create", C.byref(plan), N, L, _vp(Hi))
    try:
        dx, dy = _dev(x), _dev(_nan((nsig + 1, nx)))
        lib.call("plx_cde_apply_dev", plan, dx.data_ptr(), dy.data_ptr(), nx, nsig, _st())
        y = _host(dy)
    finally:
        lib.call("plx_cde_destroy", plan)
    assert np.isnan(y[nsig]).all()
    for k in range(nsig):
        ref, rc = oracle.overlap_both_trans(x[k], H, L)
        assert rc == 0
        np.testing.assert_allclose(y[k], ref, rtol=0, atol=1e-11, err_msg="signal %d" % k)
