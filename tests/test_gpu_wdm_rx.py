"""The per-channel receiver of 'sepfields' WDM frames (HotPathConfig(wdm_receiver='channel')) on the
MI355X: the two kernels through the shipped library, hp.rx and hp.eq against numpy and the oracle, end-to-end error counts
with and without the option, the dispersion part on a wide comb, and what must not change."""
import math

import numpy as np
import pytest

from tests import wdm_rx_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from polmux_amd import _abi
    b = _abi.get()
    assert b.path.endswith("polmux_amd/lib/libpolmux_hip.so")
    return wdm_rx_ref.Dev(b)


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------ the kernels ---
@pytest.mark.parametrize("nfft,nch,F,strides", [(256, 1, 3, (1, 2, 32)), (256, 3, 3, (1, 2, 32)), (256, 64, 2, (1, 2, 32)),
                                                (4096, 5, 2, (1, 2, 32)), (1 << 16, 16, 4, (1, 32))])
def test_gpu_pick_wdm_against_numpy(be, nfft, nch, F, strides):
    """tests/test_emu_wdm_rx.py's pick cases through the shipped library, and once at batch width (2^16 samples, 16 channels,
    4 frames): bit-exact against numpy's gather, all-zero delays equal to the two plx_pick_dev calls, delay d a roll by -d."""
    wdm_rx_ref.check_pick(be, nfft, nch, F, strides)


def test_gpu_pick_wdm_argument_errors(be):
    wdm_rx_ref.check_pick_errors(be)


@pytest.mark.parametrize("N,L,nx,nch,nrows", [(4, 2, 13, 3, 12), (256, 128, 643, 3, 12), (2048, 1024, 5123, 3, 12),
                                              (256, 128, 2048, 16, 128)])
def test_gpu_cde_per_channel_tables(be, N, L, nx, nch, nrows):
    """tests/test_emu_wdm_rx.py's CDE cases through the shipped library, and once at batch width (16 tables, the 128 rows of
    4 frames of 16 channels, 2 x 1024 samples): every row equals the same row through a one-table plan, bit for bit."""
    wdm_rx_ref.check_cde_tables(be, N, L, nx, nch, 2, nrows)


def test_gpu_cde_create_wdm_argument_errors(be):
    wdm_rx_ref.check_cde_errors(be)


# ------------------------------------------------------ the receiver of a plan ---
BASE = dict(nsymb=256, nt=16, cma_mu=1 / 300, freqavg=20, variants=3, wdm_field="sepfields")
# the end-to-end shape: 2 x 40 km, not the 2 x 80 km of test_gpu_unique_end_to_end_linear -- see test_gpu_channel_end_to_end_linear
LINEAR = dict(BASE, nch=3, chspacing=0.4, flag="g---", nspans=2, length=4e4)


def _plan(frames, **kw):
    from polmux_amd import pipeline
    return pipeline.HotPath(pipeline.HotPathConfig(**kw), max_frames=frames)


@pytest.fixture(scope="module")
def received(be):
    """one run of a three-channel plan with the option, a slope and a launch ladder: the field after fibre(), hp.rx, hp.eq and
    the plan's tables, read back once for the tests below"""
    import torch
    kw = dict(LINEAR, slope=0.06, wdm_receiver="channel")
    hp = _plan(2, **kw)
    try:
        ux, uy = hp.make_batch(2, launch_scale=[1.0, 1.6])
        hp.fibre(ux, uy)
        torch.cuda.synchronize()
        fx, fy = ux.cpu().numpy().reshape(6, -1).copy(), uy.cpu().numpy().reshape(6, -1).copy()
        err = hp.receive(ux, uy)
        torch.cuda.synchronize()
        assert tuple(err.shape) == (6, 2)
        return dict(kw=kw, fx=fx, fy=fy, rx=hp.rx[:6].cpu().numpy().copy(), eq=hp.eq[:6].cpu().numpy().copy(),
                    rx_scale=hp.rx_scale, rx_delay=hp.rx_delay.copy(), rx_delay_symbols=hp.rx_delay_symbols.copy(),
                    cde_H=hp.cde_H.copy(), fft_length=hp.cfg.fft_length, cde_L=hp.cfg.cde_L)
    finally:
        hp.close()


def test_gpu_channel_receive_pick_against_numpy(received):
    """hp.rx after receive() against rx_scale u[cf][(i half + rx_delay[c]) mod nfft] gain of the field read back after
    fibre(), under a launch ladder: 1e-12 of max.  The plan's delays are sepfields_walkoff of the comb's own tables."""
    from polmux_amd import pipeline
    g = received
    kw = g["kw"]
    cb = wdm_rx_ref.sep_comb(nch=3, chspacing=kw["chspacing"], length=kw["length"], slope=kw["slope"])
    ds, delay = pipeline.sepfields_walkoff(cb["t"]["b1"], kw["nspans"] * kw["length"], 28.0, kw["nt"])
    assert np.array_equal(g["rx_delay"], delay) and np.array_equal(g["rx_delay_symbols"], ds)
    assert delay[0] < 0 < delay[2] and delay[1] == 0 and abs(delay[0]) >= kw["nt"]
    gain = np.repeat(1 / np.sqrt([1.0, 1.6]), 3)
    half, n = kw["nt"] // 2, kw["nsymb"] * kw["nt"]
    idx = (np.arange(2 * kw["nsymb"])[None, :] * half + delay[np.arange(6) % 3][:, None]) % n
    for pol, u in enumerate((g["fx"], g["fy"])):
        want = g["rx_scale"] * np.take_along_axis(u, idx, 1) * gain[:, None]
        d = _relmax(g["rx"][:, pol], want)
        print("receive (per-channel pick) polarisation %d: %.3g of max, delays %s" % (pol, d, delay.tolist()))
        assert want.shape == g["rx"][:, pol].shape and d <= 1e-12


def test_gpu_channel_eq_against_oracle_cde_ofde(received, oracle):
    """hp.eq against the oracle's CDE_OFDE of hp.rx, called per channel with (LAMBDA[c], Dch[c], slope): the bar of
    test_cde_vs_oracle for the same operator (1e-11 absolute; the samples are of order 4)."""
    g = received
    kw = g["kw"]
    cb = wdm_rx_ref.sep_comb(nch=3, chspacing=kw["chspacing"], length=kw["length"], slope=kw["slope"])
    assert len(set(cb["t"]["Dch"].tolist())) == 3
    worst = 0.0
    for cf in range(6):
        c = cf % 3
        ex, ey, rc = oracle.cde_ofde(g["rx"][cf, 0], g["rx"][cf, 1], 2 * 28.0 * 1e9, cb["lam"][c] * 1e-9,
                                     kw["length"] * kw["nspans"], cb["t"]["Dch"][c] * 1e-6, kw["slope"] * 1e-6,
                                     g["fft_length"], g["cde_L"])
        worst = max(worst, np.abs(g["eq"][cf, 0] - ex).max(), np.abs(g["eq"][cf, 1] - ey).max())
        np.testing.assert_allclose(g["eq"][cf, 0], ex, rtol=0, atol=1e-11)
        np.testing.assert_allclose(g["eq"][cf, 1], ey, rtol=0, atol=1e-11)
    print("hp.eq against the oracle's CDE_OFDE per channel: %.3g absolute" % worst)


def _counts(frames, **kw):
    """error counts per channel-frame of one batch through fibre() + receive(), and the plan's rx_delay (None without the option)"""
    import torch
    hp = _plan(frames, **kw)
    try:
        ux, uy = hp.make_batch(frames)
        hp.fibre(ux, uy)
        hp.receive(ux, uy)
        e = hp.errors(frames * hp.nch).cpu().numpy()
        torch.cuda.synchronize()
        return e, getattr(hp, "rx_delay", None)
    finally:
        hp.close()


@pytest.mark.parametrize("decoding", ["rotation", "dqpsk"])
def test_gpu_channel_end_to_end_linear(be, decoding):
    """Three channels 0.4 nm apart over 2 x 40 km of D = 17, linear ('g---'), two frames: with wdm_receiver='channel' no
    errors on any of the 6 channel-frames, and the one-channel plan, the yardstick, is clean too; with wdm_receiver=None on
    the same plan each outer channel counts more than a quarter of its 1024 bits (the parent's behaviour; asserted so that
    the first statement cannot hold for a vacuous reason).  The walk-off taken out is -/+15.2 symbols.
    The shape: test_gpu_unique_end_to_end_linear's, with spans of 40 km instead of 80 km.  The same chain on the host
    (numpy's exp(-i betat L), the pick, the oracle's overlap-save, dsp_pdm_coh_qpsk and samp2pat_coherent) is NOT clean at
    2 x 80 km with these unfiltered NRZ waveforms: the one-channel yardstick counts 16 of 1024 (the first 8 symbols of the
    frame, where CDE_OFDE's zero extension meets a periodic frame) and the comb 2 / 0 / 0.  At 2 x 40 km it counts 0 for the
    yardstick and 0 / 0 / 0 for the comb with the smallest decision margin 0.23 of the mean symbol modulus (0.71 is ideal),
    and 479 / 0 / 487 without the per-channel delay."""
    kw = dict(LINEAR, decoding=decoding)
    y, _ = _counts(2, **dict(kw, nch=1))
    e, delay = _counts(2, **dict(kw, wdm_receiver="channel"))
    p, none = _counts(2, **kw)
    print("linear, %s: yardstick %s, per-channel receiver %s, receiver at sample 0 %s of 1024 bits per channel-frame (delays %s "
          "samples)" % (decoding, y.tolist(), e.tolist(), p.tolist(), delay.tolist()))
    assert none is None and list(delay) == [-244, 0, 244]
    assert abs(delay[0]) >= kw["nt"] and abs(delay[2]) >= kw["nt"]             # at least one symbol
    assert y.tolist() == [0, 0]
    assert e.shape == (6,) and e.tolist() == [0] * 6
    p = p.reshape(2, 3)
    assert (p[:, 0] > 256).all() and (p[:, 2] > 256).all()


WIDE = dict(nsymb=256, nt=32, nch=3, chspacing=12.0, slope=0.09, flag="g---", nspans=2, length=8e4, variants=1,
            tx_filter=dict(ftype="ideal", bw=1.6), cma_mu=1 / 300, freqavg=20, wdm_receiver="channel")


def test_gpu_channel_dispersion_on_a_wide_comb(be):
    """Each channel's own dispersion.  Three channels 12 nm apart, slope 0.09 ps/nm^2/km (Dch = 15.92 / 17 / 18.08), linear,
    2 x 80 km, nt = 32, every channel band-limited inside the receiver's Nyquist band (tx_filter 'ideal', 1.6 symbol rates:
    the unfiltered NRZ waveform aliases at 2 sps and no table removes that).  The figure is the relative rms error between
    hp.eq / (4 sqrt 2) (after the walk-off pick) and the transmitted 2-sps samples, over the samples 64 ... 448 of 512 (the
    first and last half-overlap of CDE_OFDE carry its zero extension, whichever table is used).
    First, on the numpy model alone (exp(-i betat L), pick, H_c): the outer channels' figure with the shared table is at
    least 10 times their figure with their own table (measured on the host: 0.637 against 0.0222 and 0.629 against 0.0176;
    what is left is the sub-sample rest of the walk-off).  Then the device: hp.eq against the model 1e-9 of max, and its
    figure against the model's 1e-9, per channel.  The walk-off here is -877 / +950 symbols of a 256-symbol frame: the delays are
    taken modulo nfft."""
    import torch
    from polmux_amd import pipeline
    from polmux_amd.rx import cde_transfer
    kw = WIDE
    n, half, Ltot = kw["nsymb"] * kw["nt"], kw["nt"] // 2, kw["nspans"] * kw["length"]
    cb = wdm_rx_ref.sep_comb(nsymb=kw["nsymb"], nt=kw["nt"], nch=3, chspacing=kw["chspacing"], length=kw["length"], slope=kw["slope"])
    ds, delay = pipeline.sepfields_walkoff(cb["t"]["b1"], Ltot, 28.0, kw["nt"])
    assert np.abs(ds[[0, 2]]).min() > kw["nsymb"]                                   # more than a frame
    delay = np.sign(delay) * (np.abs(delay) % n)
    Hown = pipeline.wdm_cde_tables(256, 56e9, cb["lam"], Ltot, cb["t"]["Dch"], kw["slope"])
    Hsh = cde_transfer(256, 56e9, 1550.0e-9, Ltot, 17.0e-6, kw["slope"] * 1e-6)
    hp = _plan(1, **kw)
    try:
        ux, uy = hp.make_batch(1)
        tx = (ux.cpu().numpy().reshape(3, n).copy(), uy.cpu().numpy().reshape(3, n).copy())
        hp.fibre(ux, uy)
        hp.receive(ux, uy)
        torch.cuda.synchronize()
        eq = hp.eq[:3].cpu().numpy() / (4 * math.sqrt(2))
        assert np.array_equal(hp.rx_delay, delay) and np.array_equal(hp.cde_H, Hown)
        assert hp.rx_scale == pytest.approx(4 * math.sqrt(2) * math.exp(0.5 * hp.alphalin * kw["length"]), rel=1e-12)
    finally:
        hp.close()
    mid = slice(64, -64)
    for c in range(3):
        for pol in range(2):
            t2 = tx[pol][c][::half]
            own = wdm_rx_ref.linear_chain(tx[pol][c], cb["t"]["betat"][:, c], Ltot, half, delay[c], Hown[c], 128)
            shared = wdm_rx_ref.linear_chain(tx[pol][c], cb["t"]["betat"][:, c], Ltot, half, delay[c], Hsh, 128)
            f_own, f_sh = wdm_rx_ref.rel_rms(own[mid], t2[mid]), wdm_rx_ref.rel_rms(shared[mid], t2[mid])
            f_dev = wdm_rx_ref.rel_rms(eq[c, pol][mid], t2[mid])
            d = _relmax(eq[c, pol], own)
            print("channel %d pol %d: model own table %.4g, shared table %.4g (x %.1f); device %.4g, eq against the model %.3g"
                  % (c, pol, f_own, f_sh, f_sh / f_own, f_dev, d))
            if c != 1:
                assert f_sh >= 10 * f_own                  # a condition on the model, before the device is looked at
            assert d <= 1e-9
            assert abs(f_dev - f_own) <= 1e-9


# ----------------------------------------------------------- what must not change ---
def test_gpu_channel_one_channel_is_bit_identical(be):
    """nch = 1 with wdm_receiver='channel' against None: the field after fibre(), hp.rx, hp.eq, hp.sym and the counts are
    bit-identical (delay 0 is the two picks, one table is plx_cde_create's plan)."""
    import torch
    kw = dict(nsymb=256, nt=16, flag="g-s-", manakov="yes", pavg_mw=4.0, length=4e4, dphimax=2e-2, dzmax=1e4, cma_mu=1 / 300,
              freqavg=20, variants=2)
    got = []
    for opt in (None, "channel"):
        hp = _plan(2, wdm_receiver=opt, **kw)
        try:
            ux, uy = hp.make_batch(2, launch_scale=[1.0, 1.5])
            hp.fibre(ux, uy)
            fx, fy = ux.cpu().numpy().copy(), uy.cpu().numpy().copy()
            nc = hp.last_ncycle(2).copy()
            err = hp.receive(ux, uy).cpu().numpy().copy()
            cnt = hp.errors(2).cpu().numpy().copy()
            torch.cuda.synchronize()
            got.append((fx, fy, nc, hp.rx[:2].cpu().numpy().copy(), hp.eq[:2].cpu().numpy().copy(),
                        hp.sym[:2].cpu().numpy().copy(), err, cnt))
            if opt:
                assert list(hp.rx_delay) == [0] and list(hp.rx_delay_symbols) == [0.0]
        finally:
            hp.close()
    assert got[0][2].min() > 3
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)


def test_gpu_channel_campaign_is_keyed_by_realisation(be):
    """McCampaign with nch = 3 and the option, no random PMD, receiver noise on: collect returns 3 n counts (and EVM samples),
    channels innermost, and the same ones for one batch of 4 as for two batches of 2; ShardedBer.run on it raises its
    ValueError (one count per realisation)."""
    from polmux_amd import mc, pipeline
    cfg = pipeline.HotPathConfig(**dict(LINEAR, wdm_receiver="channel"))
    res = []
    for per in (4, 2):
        camp = pipeline.McCampaign(cfg, frames_per_call=per, noise_sigma=0.35)
        try:
            assert not camp.hp.pmd
            res.append(camp.collect(camp.launch([0, 1, 2, 3]), with_samples=True))
            if per == 2:
                sb = mc.ShardedBer(camp.simulate, camp.bits_per_realisation, dict(stop=[0.1, 95], nmin=1), per_rank_per_round=2)
                with pytest.raises(ValueError, match="one error count per realisation"):
                    sb.run(max_realisations=4)
        finally:
            camp.close()
    (a, va), (b, vb) = res
    print("campaign counts %s" % a.tolist())
    assert a.shape == (12,) and va.shape == (12,) and a.dtype == np.int64
    assert np.array_equal(a, b) and np.array_equal(va, vb)
    assert len(set(va.tolist())) == 12                                  # every realisation and channel has its own noise


def test_gpu_channel_with_manakov_xpm(be):
    """xpm_dualpol='manakov' (flag 'gpsx', manakov 'yes'), the route whose per-channel counts the option exists for: the field
    after fibre() is bit-identical with and without the option (it touches the receiver only), and the centre channel's
    hp.rx, whose delay is 0, is bit-identical too; the outer channels' differ."""
    import torch
    kw = dict(nsymb=256, nt=16, nch=3, flag="gpsx", manakov="yes", xpm_dualpol="manakov", pavg_mw=4.0, length=2e4, dphimax=2e-2,
              dzmax=1e4, nplates=6, cma_mu=1 / 300, freqavg=20, variants=3)
    got = []
    for opt in (None, "channel"):
        hp = _plan(2, wdm_receiver=opt, **kw)
        try:
            ux, uy = hp.make_batch(2, launch_scale=[1.0, 1.6])
            hp.fibre(ux, uy)
            fx, fy = ux.cpu().numpy().copy(), uy.cpu().numpy().copy()
            hp.receive(ux, uy)
            e = hp.errors(6).cpu().numpy()
            torch.cuda.synchronize()
            got.append((fx, fy, hp.rx[:6].cpu().numpy().copy(), e))
            if opt:
                delay = hp.rx_delay.copy()
        finally:
            hp.close()
    print("manakov xpm: delays %s samples, counts at sample 0 %s, per channel %s" % (delay.tolist(), got[0][3].tolist(), got[1][3].tolist()))
    assert delay[1] == 0 and delay[0] < 0 < delay[2]
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    a, b = got[0][2].reshape(2, 3, 2, -1), got[1][2].reshape(2, 3, 2, -1)
    assert np.array_equal(a[:, 1], b[:, 1])
    assert not np.array_equal(a[:, 0], b[:, 0]) and not np.array_equal(a[:, 2], b[:, 2])
