"""The LO frequency offset (plx_lo_detune_dev, plx_dsp_run_freq_dev, HotPathConfig(lo_detuning, lo_detuning_spread); DESIGN.md
section 8h) on the MI355X through the shipped library: the kernel cases of tests/lo_detune_ref.py and two at batch width, both
front ends against numpy and the table route of rxfront, the frequency estimate and the error counts against the host oracle
chain back to back and over 80 km, the keyed draws through McCampaign, and what must not change."""
import numpy as np
import pytest

from polmux_amd import _abi
from tests import lo_detune_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    b = _abi.get()
    assert b.path.endswith("polmux_amd/lib/libpolmux_hip.so")
    return ref.Dev(b)


def _sync():
    import torch
    torch.cuda.synchronize()


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ------------------------------------------------------------------ the kernels ---
@pytest.mark.parametrize("nfft,nfc,F,strides", [c + (ref.STRIDES,) for c in ref.KERNEL_CASES] + [(1 << 16, 16, 4, (1, 32))])
def test_gpu_lo_detune_against_numpy(be, nfft, nfc, F, strides):
    """tests/test_emu_lo_detune.py's kernel cases through the shipped library, and once at batch width (2^16 samples, 16
    channels, 4 frames: 2048 items of a d_phi launch, the whole grid)"""
    wu, wp = ref.check_kernel(be, nfft, nfc, F, strides)
    print("nfft %d, nfc %d, F %d: phasor %.3g of max, phase %.3g rad" % (nfft, nfc, F, wu, wp))


def test_gpu_lo_detune_2p20_largest_product(be):
    """2^20 samples, b = 2^19 - 1: (b mod nfft) (n + 1) reaches 2^39, beyond a 32-bit product; phase and phasor against numpy"""
    nfft, b = 1 << 20, (1 << 19) - 1
    r = np.random.default_rng(20)
    th = ref.theta_np([b], nfft)
    u0 = [np.concatenate([ref.cnormal(r, (1, nfft)), np.full((1, nfft), ref.SENT)]) for _ in range(2)]
    phi0 = np.full((2, nfft), np.nan)
    g = ref.detune(be, nfft, 1, 1, u=u0, sign=-1.0, bins=[[b]], phi=phi0)
    assert np.abs(g["phi"][0] - th[0]).max() <= 1e-12 and np.isnan(g["phi"][1]).all()
    assert len(np.unique(th[0])) == nfft                                   # b is odd: every residue once
    for got, src in ((g["ux"], u0[0]), (g["uy"], u0[1])):
        assert _relmax(got[0], src[0] * np.exp(-1j * th[0])) <= 1e-12 and np.all(got[1] == ref.SENT)
    assert g["bins"][0] == b


def test_gpu_lo_detune_argument_errors(be):
    ref.check_errors(be)


@pytest.mark.parametrize("Lin,freqavg", [(128, 500), (512, 5), (2048, 500)])
def test_gpu_dsp_freq_turns(be, Lin, freqavg):
    ref.check_freq(be, Lin, freqavg)


# ---------------------------------------------------------------- the front ends ---
SMALL = dict(nsymb=64, nt=16, pavg_mw=4.0, length=4e4, cma_mu=1 / 300, freqavg=20, dphimax=2e-2)
BIN64 = 28e9 / 64


def _plan(frames, **kw):
    from polmux_amd import pipeline
    return pipeline.HotPath(pipeline.HotPathConfig(**kw), max_frames=frames)


@pytest.mark.parametrize("extra", [False, True], ids=["detuning", "with_linewidth_and_lo_phase"])
def test_gpu_pick_rx_against_numpy(be, extra):
    """hp.rx with the option equals hp.rx without it times numpy's exp(-i theta) at the pick instants, to 1e-12 of max; once
    with lo_linewidth > 0 and an injected lo_phase beside it (the phase noise is in both plans)"""
    import torch
    F, keys = 3, [4, 90, 1 << 35]
    kw = dict(SMALL, lo_linewidth=1e-3) if extra else dict(SMALL)
    rxs, bins = [], None
    for opt in ({}, dict(lo_detuning=-2.5 * BIN64, lo_detuning_spread=3.5 * BIN64)):
        hp = _plan(F, **dict(kw, **opt))
        try:
            ux, uy = hp.make_batch(F)
            hp.fibre(ux, uy)
            lop = None
            if extra:
                lop = torch.from_numpy(np.cumsum(0.02 * np.random.default_rng(3).standard_normal((F, 1, hp.cfg.nfft)), 2)).cuda()
            hp.receive(ux, uy, noise_keys=keys, lo_phase=lop)
            _sync()
            rxs.append(hp.rx[:F].cpu().numpy().copy())
            if opt:
                bins = hp.lo_bins.cpu().numpy().copy()
                assert np.array_equal(bins, hp.lo_bins_host(keys).reshape(-1)) and (hp.lo_k0, hp.lo_K) == (-3, 3)
                assert len(set(bins.tolist())) > 1
            else:
                assert hp.lo_bins is None
        finally:
            hp.close()
    want = rxs[0] * ref.lo_at_pick(bins, 64 * 16, 8)[:, None, :]
    d = _relmax(rxs[1], want)
    print("pick, bins %s: %.3g of max" % (bins.tolist(), d))
    assert d <= 1e-12
    assert _relmax(rxs[1], rxs[0]) > 0.1                                   # (the offset is there)


@pytest.mark.parametrize("k", [3, -2])
def test_gpu_cohmix_rx_against_the_elo_table_route(be, k):
    """frontend='cohmix': hp.rx with lo_detuning = k bins against a plx_front plan whose elo table comes from
    rxfront._front_tables(..., lodetuning=...) -- the one-frame surface's route -- run on the same fields: 1e-12 of max (the
    two routes agree on the sign), and the same freq_turns, -k"""
    import torch
    from polmux_amd import rxfront
    F, hz = 2, (k + 0.5) * BIN64
    hp = _plan(F, **dict(SMALL, frontend="cohmix", lo_detuning=hz))
    tab = _plan(F, **dict(SMALL, frontend="cohmix"))
    try:
        assert (hp.lo_k0, hp.lo_K) == (k, 0)
        ux, uy = hp.make_batch(F)
        hp.fibre(ux, uy)
        vx, vy = ux.clone(), uy.clone()
        hp.receive(ux, uy)
        _sync()
        rx, turns = hp.rx[:F].cpu().numpy().copy(), hp.freq_turns(F).cpu().numpy().copy()
        assert hp.lo_bins.cpu().numpy().tolist() == [k] * F
        cfg, t = tab.cfg, tab.front_tables
        tab.bind_gstate()
        rp = dict(oftype=cfg.oftype, obw=cfg.obw, oord=cfg.oord, eftype=cfg.eftype, ebw=cfg.ebw, eord=cfg.eord,
                  lopower=cfg.lopower, lodetuning=hz)
        elo = rxfront._front_tables(1, rp, nfc=1)[1]
        assert np.ndim(elo) == 1 and np.abs(elo[0] - 10 ** (cfg.lopower / 20) * np.exp(2j * np.pi * k / cfg.nfft)) < 1e-12
        tab.front.close()
        tab.front = rxfront._Front(cfg.nfft, True, F, t["hopt"], elo, t["hel"], True, cfg.adcbits, t["decim"], t["fir"])
        # the receiver behind the table-route front end, with its frequency estimate read out: zero further bins
        tab.receive(vx, vy, lo_bins=torch.zeros((F, 1), dtype=torch.int32, device="cuda"))
        _sync()
        rx2, turns2 = tab.rx[:F].cpu().numpy().copy(), tab.freq_turns(F).cpu().numpy().copy()
    finally:
        hp.close()
        tab.close()
    d = _relmax(rx, rx2)
    print("cohmix, k = %d: %.3g of max, turns %s" % (k, d, turns.tolist()))
    assert d <= 1e-12
    assert np.array_equal(turns, turns2) and np.all(turns == -k)


@pytest.mark.parametrize("frontend", ["pick", "cohmix"])
def test_gpu_unchanged_when_off(be, frontend):
    """both options 0: rx, sym and err bit-identical to a config that does not name them"""
    outs = []
    for kw in ({}, dict(lo_detuning=0.0, lo_detuning_spread=0.0)):
        hp = _plan(3, **dict(SMALL, frontend=frontend, lo_linewidth=1e-3, **kw))
        try:
            ux, uy = hp.make_batch(3)
            hp.fibre(ux, uy, span_keys=[1, 2, 3])
            err = hp.receive(ux, uy, noise_sigma=0.1, noise_seed=5, noise_keys=[1, 2, 3])
            _sync()
            assert hp.lo_bins is None
            with pytest.raises(ValueError, match="freq_turns"):
                hp.freq_turns(3)
            outs.append((hp.rx[:3].cpu().numpy().copy(), hp.sym[:3].cpu().numpy().copy(), err.cpu().numpy().copy()))
        finally:
            hp.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------- the estimator and the error counts ---
def _received(oracle, bins, **kw):
    """make_batch -> fibre -> receive(lo_bins=bins) of len(bins) frames of a default-size plan (nsymb 1024, nt 32); returns
    (freq_turns, errors_resolved, device symbols, [(oracle symbols, oracle errors)] of the host chain on the same fields)"""
    import torch
    F = len(bins)
    hp = _plan(F, **dict(dict(nsymb=1024, nt=32, flag="g---"), **kw))
    try:
        ux, uy = hp.make_batch(F)
        hp.fibre(ux, uy)
        _sync()
        fx, fy = ux.cpu().numpy().copy(), uy.cpu().numpy().copy()
        hp.receive(ux, uy, lo_bins=torch.tensor(bins, dtype=torch.int32, device="cuda").reshape(F, 1))
        e = hp.errors_resolved(F).cpu().numpy()
        _sync()
        turns, sym = hp.freq_turns(F).cpu().numpy().copy(), hp.sym[:F].cpu().numpy().copy()
        assert hp.lo_bins.cpu().numpy().tolist() == list(bins)
        host = [ref.host_chain(oracle, hp.cfg, hp, fx[f], fy[f], bins[f]) for f in range(F)]
    finally:
        hp.close()
    return turns, e, sym, host


def test_gpu_back_to_back_estimator_range(be, oracle):
    """1 m of lossless fibre, 1024 symbols: injected bins 0, +-1, +-64, +-127 over 8 frames -- freq_turns == -b on both
    polarisations up to one bin short of the estimator's range nsymb / 8, no errors on the device and none in the host oracle
    chain on the same samples"""
    bins = [0, 1, -1, 64, -64, 127, -127, 0]
    turns, e, _, host = _received(oracle, bins, length=1.0, alphadB=0.0)
    print("back to back: turns %s, errors %s, oracle %s" % (turns.tolist(), e.tolist(), [h[1] for h in host]))
    assert np.array_equal(turns, -np.array(bins)[:, None] * np.ones((1, 2), np.int64))
    assert [h[1] for h in host] == [0] * 8
    assert e.tolist() == [0] * 8


def test_gpu_80km_linear_against_the_oracle_chain(be, oracle):
    """80 km of D = 17 ('g---'), CDE 256/128: bins 0, +-1, +-4, 16, 24 -- no errors on the device and none in the host oracle
    chain, the symbols against that chain to 1e-10 (the bar tests/test_gpu_phase_noise.py holds the same chain to), and the
    estimator reads -b to within one turn (measured: 1, 0, 2, -3, 4, -16, -24 on both polarisations -- behind 80 km and
    CDE_OFDE the sum the circularity fix rounds sits near a half turn, on symbols that agree with the oracle chain to 1e-13:
    the chain's own reading, not the kernel's; back to back it is exactly -b)"""
    bins = [0, 1, -1, 4, -4, 16, 24]
    turns, e, sym, host = _received(oracle, bins, fft_length=256, cde_L=128)
    d = [float(np.abs(sym[f].T - host[f][0]).max()) for f in range(len(bins))]
    print("80 km: turns %s, errors %s, oracle %s, symbols %s" % (turns.tolist(), e.tolist(), [h[1] for h in host],
                                                                   ["%.2g" % v for v in d]))
    assert [h[1] for h in host] == [0] * len(bins)
    assert e.tolist() == [0] * len(bins)
    assert max(d) <= 1e-10
    assert np.abs(turns + np.array(bins)[:, None]).max() <= 1


# ---------------------------------------------------------------- keyed draws ---
def test_gpu_keyed_draws_do_not_depend_on_batching(be):
    """lo_detuning_spread = 3.5 bins (K = 3): hp.lo_bins equals lo_bins_host(keys); a McCampaign over 12 realisations run in
    one call of 12 and in calls of 5 + 7 returns identical counts, bins and EVM samples"""
    from polmux_amd import pipeline
    cfg = pipeline.HotPathConfig(**dict(SMALL, lo_detuning=1.5 * BIN64, lo_detuning_spread=3.5 * BIN64, lo_linewidth=1e-3))
    camp = pipeline.McCampaign(cfg, 12, noise_sigma=0.3)
    try:
        hp = camp.hp
        assert (hp.lo_k0, hp.lo_K) == (1, 3)
        idx = list(range(100, 112))
        want = hp.lo_bins_host(idx).reshape(-1)
        assert want.min() >= -2 and want.max() <= 4 and len(set(want.tolist())) >= 4
        whole = camp.collect(camp.launch(idx), with_samples=True)
        b_whole = hp.lo_bins.cpu().numpy().copy()
        parts, b_parts = [], []
        for sub in (idx[:5], idx[5:]):
            parts.append(camp.collect(camp.launch(sub), with_samples=True))
            b_parts.append(hp.lo_bins.cpu().numpy().copy())
    finally:
        camp.close()
    assert np.array_equal(b_whole, want) and np.array_equal(np.concatenate(b_parts), want)
    np.testing.assert_array_equal(np.concatenate([p[0] for p in parts]), whole[0])
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), whole[1])
    assert whole[0].shape == (12,)


# ------------------------------------------------------ with the other features ---
COMB = dict(nsymb=256, nt=16, nch=3, chspacing=0.4, cma_mu=1 / 300, freqavg=20, variants=3, flag="g---", nspans=2)
SPACING = 456 / 256                                              # the comb's spacing in symbol rates (0.4 nm at 28 Gbaud, 256 symbols)
BINS3 = [[1, -2, 3], [-3, 2, 0]]


@pytest.mark.parametrize("kw", [dict(length=4e4, wdm_field="sepfields", wdm_receiver="channel"),
                                dict(length=4e4, wdm_field="unique", mux_filter=dict(ftype="ideal", bw=0.9 * SPACING),
                                     oftype="ideal", obw=0.9 * SPACING)], ids=["channel_receiver", "unique_field"])
def test_gpu_with_wdm_receivers(be, kw):
    """three channels, each channel's receiver with an LO offset of its own (injected; test_gpu_channel_end_to_end_linear's
    comb and, for 'unique', test_gpu_unique_end_to_end_linear's filters): every channel-frame counts 0 and its estimator
    reads minus its own bin to within one turn.
    The link is 2 x 40 km for both, 80 km of D = 17 in all: nothing estimates the offset in front of CDE_OFDE, which turns
    it into a delay in proportion to the accumulated dispersion, and 80 km is the link whose tolerance is known (clean up to
    24 bins of 1024 symbols = 0.66 GHz, one or two errors at 0.875 GHz).  The offsets here stay within 3 bins of 256 symbols
    = 0.33 GHz, half of that.  Over 2 x 80 km, where the same delay is twice as large, the 'unique' comb counted 0, 2, 0 /
    2, 0, 0 with these bins (the offsets -2 and -3)."""
    import torch
    hp = _plan(2, **dict(COMB, **kw))
    try:
        ux, uy = hp.make_batch(2)
        hp.fibre(ux, uy)
        hp.receive(ux, uy, lo_bins=torch.tensor(BINS3, dtype=torch.int32, device="cuda"))
        e = hp.errors(6).cpu().numpy()
        _sync()
        turns, bins = hp.freq_turns(6).cpu().numpy(), hp.lo_bins.cpu().numpy()
    finally:
        hp.close()
    flat = np.array(BINS3).reshape(-1)
    print("%s: errors %s, turns %s" % (kw["wdm_field"], e.tolist(), turns.tolist()))
    assert np.array_equal(bins, flat)
    assert e.tolist() == [0] * 6
    assert np.abs(turns + flat[:, None]).max() <= 1                       # (behind a dispersive link: see the 80 km test)
