"""A WDM frame as ONE field in the batched path (HotPathConfig(wdm_field='unique')) on the MI355X: the
two kernels at production sizes, the fibre against the oracle and against create_field('unique') + fiber(), the receive side
against numpy, and end-to-end error counts, linear and nonlinear."""
import ctypes as C

import numpy as np
import pytest

from tests import wdm_ref

pytestmark = pytest.mark.gpu

FIELD_RTOL = 1e-9
SPACING = 456 / 256        # |s_1 - s_0| dFN of the comb below, in symbol rates (0.4 nm at 28 Gbaud, NSYMB 256)
COMB = dict(nsymb=256, nt=16, nch=3, chspacing=0.4, cma_mu=1 / 300, freqavg=20, cma_taps=7, fft_length=256, cde_L=128,
            variants=3, wdm_field="unique", mux_filter=dict(ftype="ideal", bw=0.9 * SPACING), oftype="ideal", obw=0.9 * SPACING)


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


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _mux_dev(lib, sx, sy, shift):
    """plx_wdm_mux_dev on device tensors [F, nch, N] -> device tensors [F, N]"""
    import torch
    F, nch, N = sx.shape
    ux = torch.full((F, N), float("nan"), dtype=torch.complex128, device=sx.device)
    uy = torch.full_like(ux, float("nan"))
    sh = np.ascontiguousarray(shift, dtype=np.int64)
    lib.call("plx_wdm_mux_dev", sx.data_ptr(), sy.data_ptr(), ux.data_ptr(), uy.data_ptr(), N, nch, F, _vp(sh), _stream())
    return ux, uy


@pytest.mark.parametrize("N,nch,F", [(1 << 16, 16, 4), (1 << 20, 2, 1)])
def test_gpu_mux_against_create_field(lib, N, nch, F):
    """mux through the shipped library against ifft(sum_c roll(fft(s_c), -s_c)) in numpy, complex normal samples, shifts of
    both signs that include +-(N/2 - 1): 1e-12 of max |u|; select of that field back (delay 0) against numpy's select."""
    import torch
    r = np.random.default_rng(21)
    shift = wdm_ref.edge_shifts(N, nch)
    sx, sy = wdm_ref.cnormal(r, (F, nch, N)), wdm_ref.cnormal(r, (F, nch, N))
    gx, gy = torch.from_numpy(sx).cuda(), torch.from_numpy(sy).cuda()
    ux, uy = _mux_dev(lib, gx, gy, shift)
    torch.cuda.synchronize()
    hx, hy = ux.cpu().numpy(), uy.cpu().numpy()
    ex, ey = wdm_ref.mux_fft(sx, shift), wdm_ref.mux_fft(sy, shift)
    dx, dy = _relmax(hx, ex), _relmax(hy, ey)
    print("gpu mux (%d, %d) x %d frames: %.3g %.3g of max |u|" % (N, nch, F, dx, dy))
    assert dx <= 1e-12 and dy <= 1e-12
    delay = np.array([(-1) ** c * (37 * c + 1) for c in range(nch)], dtype=np.int64)
    rx, ry = torch.full_like(gx, float("nan")), torch.full_like(gy, float("nan"))
    sh = np.ascontiguousarray(shift, dtype=np.int64)
    lib.call("plx_wdm_select_dev", ux.data_ptr(), uy.data_ptr(), rx.data_ptr(), ry.data_ptr(), N, nch, F, _vp(sh), _vp(delay),
             _stream())
    torch.cuda.synchronize()
    sx_, sy_ = wdm_ref.select_np(hx, shift, delay), wdm_ref.select_np(hy, shift, delay)
    dx, dy = _relmax(rx.cpu().numpy(), sx_), _relmax(ry.cpu().numpy(), sy_)
    print("gpu select (%d, %d) x %d frames: %.3g %.3g of max |r|" % (N, nch, F, dx, dy))
    assert dx <= 1e-12 and dy <= 1e-12


def _fibre_plan(**over):
    from polmux_amd import pipeline
    kw = dict(nsymb=256, nt=16, nch=3, wdm_field="unique", flag="g-s-", manakov="yes", pavg_mw=4.0, length=2e4, dphimax=2e-2,
              dzmax=1e4, cma_mu=1 / 300, freqavg=20, variants=3)
    kw.update(over)
    cfg = pipeline.HotPathConfig(**kw)
    return cfg, pipeline.HotPath(cfg, max_frames=2)


def test_gpu_unique_fibre_against_oracle_and_fiber(lib, oracle):
    """HotPath(nch=3, wdm_field='unique', flag='g-s-', manakov='yes'), two frames at different launch scales.  The test
    multiplexes make_batch's output itself with plx_wdm_mux_dev (the bits fibre() forms) and runs the oracle's matrix_ssfm
    with one column on THOSE bits: against hp.wx, hp.wy after fibre(): ncycle equal, firstdz to 1e-12, field <= 1e-9.  ux, uy
    after fibre() equal numpy's select of hp.wx, hp.wy to 1e-12.  Then gstate.create_field('unique') + fiber() on the same
    waveforms: ncycle equal, field <= 1e-9 (under the device's logged step sequence if a step boundary moves).
    fiber() follows fiber.m:296 and drops x.manakov when its flag has no 'p', so the Manakov equation of this plan is asked
    of it as 'gps-' with dgd = 0 and one zero plate (the PMD-free case, as tests/test_gpu_xpm.py does)."""
    import torch
    import polmux_amd as px
    from polmux_amd.gstate import GSTATE, to_host_field
    import sys
    fibermod = sys.modules["polmux_amd.fiber"]
    cfg, hp = _fibre_plan()
    try:
        assert hp.nfc == 1 and hp.fls == [1, 0, 1, 0] and list(hp.wdm_shift) == [-456, 0, 456]
        ux, uy = hp.make_batch(2, launch_scale=[1.0, 1.6])
        assert tuple(ux.shape) == (2, 3, 4096)
        tx, ty = ux.cpu().numpy(), uy.cpu().numpy()
        mx, my = _mux_dev(lib, ux, uy, hp.wdm_shift)
        torch.cuda.synchronize()
        mx, my = mx.cpu().numpy(), my.cpu().numpy()
        assert _relmax(mx, wdm_ref.mux_fft(tx, hp.wdm_shift)) <= 1e-12
        hp.fibre(ux, uy)
        torch.cuda.synchronize()
        first, ncyc = np.zeros(2), np.zeros(2, np.int32)
        lib.call("plx_ssfm_results", hp.ssfm, 2, _vp(first), _vp(ncyc))
        gam, betat, db1 = hp._keep
        assert betat.shape == (4096, 1) and gam.shape == (1,)
        wx, wy = hp.wx[:2].cpu().numpy(), hp.wy[:2].cpu().numpy()
        z1 = np.zeros(1)
        for f in range(2):
            rc, rfd, rnc, rx, ry = oracle.matrix_ssfm(mx[f], my[f], betat, db1, 1e4, 2e-2, gam, hp.alphalin, 2e4, 1, 1, hp.fls,
                                                      z1, z1, z1)
            ex, ey = _relmax(wx[f], rx[:, 0]), _relmax(wy[f], ry[:, 0])
            print("unique fibre frame %d: ncycle %d / %d, firstdz rel %.3g, field %.3g %.3g" %
                  (f, ncyc[f], rnc, abs(first[f] - rfd) / rfd, ex, ey))
            assert rc == 0 and ncyc[f] == rnc and first[f] == pytest.approx(rfd, rel=1e-12)
            assert ex <= FIELD_RTOL and ey <= FIELD_RTOL
        assert ncyc[0] != ncyc[1] and ncyc.min() > 3
        # the channels cut back out, walk-off taken out
        sx, sy = wdm_ref.select_np(wx, hp.wdm_shift, hp.wdm_delay), wdm_ref.select_np(wy, hp.wdm_shift, hp.wdm_delay)
        dx, dy = _relmax(ux.cpu().numpy(), sx), _relmax(uy.cpu().numpy(), sy)
        print("select after fibre(): %.3g %.3g (delays %s samples)" % (dx, dy, list(hp.wdm_delay)))
        assert dx <= 1e-12 and dy <= 1e-12
        assert hp.wdm_delay[0] < 0 < hp.wdm_delay[2] and hp.wdm_delay[1] == 0
        # the function surface: create_field('unique') + fiber() on the same waveforms
        x = dict(length=cfg.length, alphadB=cfg.alphadB, aeff=cfg.aeff, n2=cfg.n2, disp=cfg.disp, slope=cfg.slope,
                 dphimax=cfg.dphimax, dzmax=cfg.dzmax, manakov="yes", dgd=0.0, db0=z1, theta=z1, epsilon=z1, _log_dz=True)
        x["lambda"] = cfg.lam
        fibermod.release_plans()
        try:
            for f in range(2):
                hp.bind_gstate()
                px.create_field("unique", tx[f].T, ty[f].T)
                assert tuple(GSTATE.FIELDX.shape) == (1, 4096)
                assert _relmax(to_host_field(GSTATE.FIELDX)[:, 0], mx[f]) <= 1e-12          # (its input differs by ~1e-15)
                brf = px.fiber(x, "gps-")
                if brf["ncycle"] != ncyc[f]:
                    print("frame %d: fiber() free-running ncycle %d / %d, repeated under the plan's step sequence" %
                          (f, brf["ncycle"], ncyc[f]))
                    lib.call("plx_ssfm_log_steps", hp.ssfm, 1 << 14)
                    u2x, u2y = hp.make_batch(2, launch_scale=[1.0, 1.6])
                    hp.fibre(u2x, u2y)
                    torch.cuda.synchronize()
                    dz = np.zeros(int(ncyc[f]))
                    lib.call("plx_ssfm_step_sequence", hp.ssfm, f, _vp(dz), dz.size)
                    lib.call("plx_ssfm_log_steps", hp.ssfm, 0)
                    hp.bind_gstate()
                    px.create_field("unique", tx[f].T, ty[f].T)
                    brf = px.fiber(dict(x, _replay_dz=dz), "gps-")
                ex = _relmax(to_host_field(GSTATE.FIELDX)[:, 0], wx[f])
                ey = _relmax(to_host_field(GSTATE.FIELDY)[:, 0], wy[f])
                print("create_field('unique') + fiber() frame %d: ncycle %d / %d, field %.3g %.3g" % (f, brf["ncycle"], ncyc[f], ex, ey))
                assert brf["ncycle"] == ncyc[f]
                assert ex <= FIELD_RTOL and ey <= FIELD_RTOL
        finally:
            fibermod.release_plans()
    finally:
        hp.close()


def test_gpu_unique_receive_pick_against_numpy(lib):
    """hp.rx after receive() ('pick') against numpy's select -> optical filter -> pick -> rx_scale (and the launch ladder's
    gain) of the device's own hp.wx, hp.wy: 1e-12 of max."""
    import torch
    cfg, hp = _fibre_plan(oftype="ideal", obw=0.9 * SPACING)
    try:
        ux, uy = hp.make_batch(2, launch_scale=[1.0, 1.6])
        hp.fibre(ux, uy)
        torch.cuda.synchronize()
        wx, wy = hp.wx[:2].cpu().numpy(), hp.wy[:2].cpu().numpy()
        err = hp.receive(ux, uy)
        torch.cuda.synchronize()
        assert tuple(err.shape) == (6, 2)
        rx = hp.rx[:6].cpu().numpy()
        from polmux_amd import synth
        from polmux_amd.rxfront import myfilter
        h = myfilter(cfg.oftype, synth.fn_grid(cfg.nsymb, cfg.nt), 0.5 * cfg.obw, cfg.oord)     # the test's own table
        assert h.sum() == 2 * round(0.45 * 456) + 1                   # 'ideal', +-0.45 spacing: 205 bins each side and DC
        gain = np.repeat(1 / np.sqrt([1.0, 1.6]), 3)
        half = cfg.nt // 2
        for pol, w in enumerate((wx, wy)):
            s = wdm_ref.select_np(w, hp.wdm_shift, hp.wdm_delay).reshape(6, -1)
            s = np.fft.ifft(np.fft.fft(s, axis=-1) * h, axis=-1)
            want = hp.rx_scale * s[:, ::half] * gain[:, None]
            d = _relmax(rx[:, pol], want)
            print("receive (pick) polarisation %d: %.3g of max" % (pol, d))
            assert want.shape == rx[:, pol].shape and d <= 1e-12
    finally:
        hp.close()


def _end_to_end(nch, frames, launch_scale=None, **over):
    """error counts per channel-frame of a batch through fibre() + receive(), and the plan's ncycle"""
    import torch
    from polmux_amd import pipeline
    kw = dict(COMB, nch=nch)
    kw.update(over)
    hp = pipeline.HotPath(pipeline.HotPathConfig(**kw), max_frames=frames)
    try:
        ux, uy = hp.make_batch(frames, launch_scale=launch_scale)
        hp.fibre(ux, uy)
        nc = hp.last_ncycle(frames)
        hp.receive(ux, uy)
        e = hp.errors(frames * nch).cpu().numpy()
        torch.cuda.synchronize()
        return e, nc, hp.sym[:frames * nch].cpu().numpy().copy(), list(getattr(hp, "wdm_delay", []))
    finally:
        hp.close()


def test_gpu_unique_one_channel_is_the_one_channel_path(lib):
    """nch = 1 with wdm_field='unique' against the default plan: the field after fibre(), hp.rx, hp.sym and the error
    counts are bit-identical (shift 0 and delay 0 are copies, and one channel has no neighbours to filter away)."""
    import torch
    from polmux_amd import pipeline
    kw = dict(nsymb=256, nt=16, flag="g-s-", manakov="yes", pavg_mw=4.0, length=4e4, dphimax=2e-2, dzmax=1e4, cma_mu=1 / 300,
              freqavg=20, variants=2)
    got = []
    for field in ("sepfields", "unique"):
        hp = pipeline.HotPath(pipeline.HotPathConfig(wdm_field=field, **kw), max_frames=2)
        try:
            ux, uy = hp.make_batch(2, launch_scale=[1.0, 1.5])
            hp.fibre(ux, uy)
            fx, fy = ux.cpu().numpy().copy(), uy.cpu().numpy().copy()
            nc = hp.last_ncycle(2).copy()
            err = hp.receive(ux, uy).cpu().numpy().copy()
            torch.cuda.synchronize()
            got.append((fx, fy, nc, hp.rx[:2].cpu().numpy().copy(), hp.sym[:2].cpu().numpy().copy(), err))
            if field == "unique":
                assert list(hp.wdm_shift) == [0] and list(hp.wdm_delay) == [0] and hp.chfilt is None
                assert np.array_equal(hp.wx[:2].cpu().numpy(), fx)
        finally:
            hp.close()
    assert got[0][2].min() > 3
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)


LINEAR = dict(flag="g---", nspans=2, length=8e4, disp=17.0, pavg_mw=2.0)


@pytest.mark.parametrize("route", ["pick", "pick-dqpsk", "cohmix"])
def test_gpu_unique_end_to_end_linear(lib, route):
    """Three channels 0.4 nm apart over 2 x 80 km of D = 17, linear ('g---'), multiplexer and optical filters 'ideal' of
    0.9 spacing: no errors on any channel-frame.  The yardstick is the ONE-channel path fed the same band-limited waveform
    through the same fibre, which must be clean too.  The walk-off the select takes out is -/+30.4 symbols."""
    over = dict(LINEAR)
    if route == "pick-dqpsk":
        over["decoding"] = "dqpsk"
    if route == "cohmix":
        over["frontend"] = "cohmix"
    y, _, _, _ = _end_to_end(1, 2, **over)
    e, _, _, delay = _end_to_end(3, 2, **over)
    print("linear, %s: yardstick %s, comb %s of 1024 bits per channel-frame (delays %s samples)" % (route, y.tolist(), e.tolist(), delay))
    assert delay == [-487, 0, 487]
    assert y.tolist() == [0, 0]
    assert e.shape == (6,) and e.tolist() == [0] * 6


def test_gpu_unique_end_to_end_nonlinear(lib):
    """The same comb and filters over one nonlinear span ('g-s-', Manakov), 0.5 mW and 4 mW per channel as the two frames of
    one batch: no errors on any channel-frame, the frames take different numbers of steps, and a frame alone equals
    itself inside the batch (error counts and hp.sym bit for bit)."""
    over = dict(flag="g-s-", manakov="yes", dphimax=5e-3, dzmax=2e4, nspans=1, length=8e4, disp=17.0, pavg_mw=0.5)
    e, nc, sym, _ = _end_to_end(3, 2, launch_scale=[1.0, 8.0], **over)
    print("nonlinear: errors %s, ncycle %s" % (e.tolist(), nc.tolist()))
    assert e.tolist() == [0] * 6
    assert nc[0] != nc[1] and nc[1] > nc[0] > 3
    e1, nc1, sym1, _ = _end_to_end(3, 1, launch_scale=[8.0], **over)
    assert nc1[0] == nc[1] and e1.tolist() == e[3:].tolist()
    assert np.array_equal(sym1, sym[3:])


def test_gpu_unique_campaign_is_keyed_by_realisation(lib):
    """McCampaign over 8 realisations of the nonlinear comb with the receiver's amplifier and its ASE: counts of shape
    [8 * 3] (a count per channel-frame), and the same counts and EVM samples, realisation for realisation, whatever the
    order and the batching of the indices."""
    from polmux_amd import pipeline
    kw = dict(COMB, flag="g-s-", manakov="yes", dphimax=5e-3, dzmax=2e4, nspans=1, length=8e4, disp=17.0, pavg_mw=0.5,
              rx_amp=True, span_nf_db=24.0)
    camp = pipeline.McCampaign(pipeline.HotPathConfig(**kw), frames_per_call=4)
    try:
        a, va = camp.collect(camp.launch(list(range(8))), with_samples=True)
        order = [4, 5, 6, 7, 0, 1, 2, 3]
        b, vb = camp.collect(camp.launch(order), with_samples=True)
        c, vc = camp.collect(camp.launch([7, 2, 5]), with_samples=True)
    finally:
        camp.close()
    print("campaign counts %s" % a.tolist())
    _campaign_checks(a, va, b, vb, c, vc, order)


def test_gpu_unique_campaign_receiver_noise_is_keyed_by_realisation(lib):
    """The same with noise_sigma > 0 (receiver noise on the 2-sps samples, keyed by realisation): every channel-frame draws its
    own stream under its realisation's key, whatever the order and the batching; a campaign without the noise differs."""
    from polmux_amd import pipeline
    kw = dict(COMB, flag="g-s-", manakov="yes", dphimax=5e-3, dzmax=2e4, nspans=1, length=8e4, disp=17.0, pavg_mw=0.5)
    order = [4, 5, 6, 7, 0, 1, 2, 3]
    camp = pipeline.McCampaign(pipeline.HotPathConfig(**kw), frames_per_call=4, noise_sigma=0.35)
    try:
        a, va = camp.collect(camp.launch(list(range(8))), with_samples=True)
        b, vb = camp.collect(camp.launch(order), with_samples=True)
        c, vc = camp.collect(camp.launch([7, 2, 5]), with_samples=True)
        with pytest.raises(ValueError, match="one key per frame"):
            ux, uy = camp.hp.make_batch(2)
            camp.hp.receive(ux, uy, 0.35, 1, None, [0, 1, 2, 3, 4, 5])
    finally:
        camp.close()
    quiet = pipeline.McCampaign(pipeline.HotPathConfig(**kw), frames_per_call=4)
    try:
        q, vq = quiet.collect(quiet.launch(list(range(8))), with_samples=True)
    finally:
        quiet.close()
    print("campaign with receiver noise: counts %s, EVM %.3g ... against %.3g without" % (a.tolist(), va.mean(), vq.mean()))
    _campaign_checks(a, va, b, vb, c, vc, order)
    assert va.mean() > vq.mean()                              # independent noise adds to the mean-square error


def _campaign_checks(a, va, b, vb, c, vc, order):
    assert a.shape == (24,) and b.shape == (24,) and va.shape == (24,)
    a, b, va, vb = a.reshape(8, 3), b.reshape(8, 3), va.reshape(8, 3), vb.reshape(8, 3)
    for i, r in enumerate(order):
        assert np.array_equal(b[i], a[r]) and np.array_equal(vb[i], va[r])
    for i, r in enumerate([7, 2, 5]):
        assert np.array_equal(c.reshape(3, 3)[i], a[r]) and np.array_equal(vc.reshape(3, 3)[i], va[r])
    assert len(set(va.reshape(-1).tolist())) == 24            # every realisation and channel has its own noise
