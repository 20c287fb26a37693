"""GPU tests of laser phase noise (plx_phase_noise_dev, HotPathConfig(tx_linewidth, lo_linewidth)) and of the Monte-Carlo
scripts' differential decoding (plx_decide_count_dqpsk_dev, decoding='dqpsk') on the MI355X, against the numpy operators
of tests/test_phase_noise.py and the CPU oracle."""
import ctypes as C
import math

import numpy as np
import pytest

from polmux_amd import _abi
from tests.test_gpu_configs import _rx_oracle
from tests.test_phase_noise import SEED, np_phase, sigma_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return _abi.get()


def _gen(lib, nfft, nfc, keys, sig, tag):
    import torch
    F = len(keys)
    phi = torch.full((F, nfc, nfft), float("nan"), dtype=torch.float64, device="cuda")
    work = torch.empty(F * nfc * (-(-nfft // 2048)), dtype=torch.float64, device="cuda")
    kt = torch.as_tensor(np.asarray(keys, np.int64), device="cuda")
    s = np.ascontiguousarray(sig, dtype=float)
    lib.call("plx_phase_noise_dev", None, None, 1, nfft, 1.0, nfft, nfc, F, s.ctypes.data, SEED, kt.data_ptr(), tag, None,
             phi.data_ptr(), work.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return phi.cpu().numpy()


def test_generator_2p20_matches_restatement_and_batching(lib):
    """2^20 samples x 3 frames x 2 channels (512 workgroups per channel and pass) against the numpy restatement; a
    realisation's phase is bit-identical drawn alone or inside a batch"""
    n, keys, sig = 1 << 20, [11, 4242, 7], [sigma_of(1e-4, 64), sigma_of(3e-4, 64)]
    for tag in (_abi.PLX_PHASE_TX, _abi.PLX_PHASE_LO):
        phi = _gen(lib, n, 2, keys, sig, tag)
        ref = np_phase(n, 2, keys, sig, tag)
        sc = np.abs(ref).max()
        assert np.abs(phi - ref).max() <= 1e-12 * sc
        assert np.abs(phi[:, :, -1]).max() <= 1e-13 * sc and np.all(phi[:, :, 0] == 0)
        alone = _gen(lib, n, 2, [4242], sig, tag)
        np.testing.assert_array_equal(alone[0], phi[1])


def _cfg(frontend, **kw):
    from polmux_amd import pipeline
    return pipeline.HotPathConfig(nsymb=64, nt=16, pavg_mw=4.0, length=4e4, cma_mu=1 / 300, freqavg=20, dphimax=2e-2,
                                  frontend=frontend, **kw)


@pytest.mark.parametrize("frontend", ["pick", "cohmix"])
def test_zero_linewidth_is_bit_identical(lib, frontend):
    import torch
    from polmux_amd import pipeline
    outs = []
    for kw in ({}, dict(tx_linewidth=0.0, lo_linewidth=0.0, decoding="rotation")):
        hp = pipeline.HotPath(_cfg(frontend, **kw), max_frames=3)
        ux, uy = hp.make_batch(3)
        hp.fibre(ux, uy, span_keys=[1, 2, 3])
        err = hp.receive(ux, uy, noise_keys=[1, 2, 3])
        torch.cuda.synchronize()
        outs.append((hp.sym[:3].cpu().numpy(), err.cpu().numpy(), hp.errors(3).cpu().numpy()))
        hp.close()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


def test_cohmix_lo_phase_equals_one_frame_plans(lib):
    """plx_front_run_lo_dev with a per-frame LO phase equals, frame by frame, a one-frame rxfront._Front (RxPdmCohQpsk's
    route) whose elo carries that frame's phase as x.lophasenoise builds it, and oracle/front.py given the same elo"""
    import torch
    from oracle import front
    from polmux_amd import pipeline, rxfront
    cfg = _cfg("cohmix")
    hp = pipeline.HotPath(cfg, max_frames=3)
    n, F = cfg.nfft, 3
    r = np.random.default_rng(2)
    ux0 = r.standard_normal((F, n)) + 1j * r.standard_normal((F, n))
    uy0 = r.standard_normal((F, n)) + 1j * r.standard_normal((F, n))
    phi = np.cumsum(0.05 * r.standard_normal((F, n)), axis=1)
    t = hp.front_tables
    ux, uy = torch.from_numpy(ux0.copy()).cuda(), torch.from_numpy(uy0.copy()).cuda()
    out = hp.front.run(ux, uy, hp.front_shifts, lo_phase=torch.from_numpy(phi).cuda())
    got = out.cpu().numpy()
    for f in range(F):
        elo = t["elo"] * np.exp(1j * phi[f])
        one = rxfront._Front(n, True, 1, t["hopt"], elo, t["hel"], True, cfg.adcbits, t["decim"], t["fir"])
        a, b = torch.from_numpy(ux0[f:f + 1].copy()).cuda(), torch.from_numpy(uy0[f:f + 1].copy()).cuda()
        want = one.run(a, b, hp.front_shifts).cpu().numpy()[0]
        one.close()
        assert np.abs(got[f] - want).max() <= 1e-12 * np.abs(want).max()
        cur = front.receiver_cohmix(ux0[f], uy0[f], t["hopt"], elo, t["hel"], True)
        orc = front.rx_front(cur, True, cfg.adcbits, hp.front_shifts, t["decim"], t["fir"])
        assert np.abs(got[f] - orc.T).max() <= 1e-9 * np.abs(orc).max()
    hp.close()


@pytest.mark.parametrize("frontend", ["pick", "cohmix"])
def test_chain_with_injected_phases_vs_oracle(lib, frontend):
    """fibre + receiver with injected transmitter and LO phases against the oracle chain: the transmitter field rotated
    in numpy before plxo.matrix_ssfm, the LO phase in elo (cohmix) or on the picked samples (pick)"""
    import torch
    from oracle import plxo
    from polmux_amd import pipeline
    cfg = _cfg(frontend)
    F, n = 2, cfg.nfft
    hp = pipeline.HotPath(cfg, max_frames=F)
    r = np.random.default_rng(8)
    ptx = np.cumsum(0.03 * r.standard_normal((F, 1, n)), axis=2)
    plo = np.cumsum(0.03 * r.standard_normal((F, 1, n)), axis=2)
    ux, uy = hp.make_batch(F)
    hp.fibre(ux, uy, tx_phase=torch.from_numpy(ptx).cuda())
    torch.cuda.synchronize()
    field = ux.cpu().numpy()
    hp.receive(ux, uy, lo_phase=torch.from_numpy(plo).cuda())
    torch.cuda.synchronize()
    sym = hp.sym[:F].cpu().numpy()
    gam, betat, db1 = hp._keep
    for f in range(F):
        rot = np.exp(1j * ptx[f, 0])
        rc, _, _, ox, oy = plxo.matrix_ssfm(hp.tx_host[0] * rot, hp.tx_host[1] * rot, betat, db1, min(cfg.dzmax, cfg.length),
                                            cfg.dphimax, gam, hp.alphalin, cfg.length, 1, 0, hp.fls, [0.0], [0.0], [0.0])
        assert rc == 0 and np.abs(field[f] - ox[:, 0]).max() <= 1e-9 * np.abs(ox).max()
        ox, oy = ox[:, 0], oy[:, 0]
        if frontend == "cohmix":
            t0 = hp.front_tables
            hp.front_tables = dict(t0, elo=t0["elo"] * np.exp(1j * plo[f, 0]))
            ref, bits = _rx_oracle(plxo, cfg, hp, ox, oy)
            hp.front_tables = t0
        else:
            lo = np.exp(-1j * plo[f, 0])
            ref, bits = _rx_oracle(plxo, cfg, hp, ox * lo, oy * lo)
        assert np.abs(sym[f].T - ref).max() <= 1e-10
        got = plxo.samp2pat_coherent(np.angle(sym[f].T))
        np.testing.assert_array_equal(got, bits)
    hp.close()


def test_mc_campaign_dqpsk_sharding_and_clean_c1(lib):
    """McCampaign(decoding='dqpsk') counts through McRankShare are the same for world 1 and world 2; noise-free C1 frames
    with tx_linewidth = lo_linewidth = 1e-4 give zero errors with the differential decoding"""
    from polmux_amd import pipeline
    cfg = _cfg("pick", tx_linewidth=1e-3, lo_linewidth=1e-3, decoding="dqpsk")
    camp = pipeline.McCampaign(cfg, 4, noise_sigma=0.35)
    whole = pipeline.McRankShare(camp, 0, 1).simulate(range(6))
    parts = [pipeline.McRankShare(camp, k, 2).simulate(range(3)) for k in range(2)]
    np.testing.assert_array_equal(whole[0::2], parts[0])
    np.testing.assert_array_equal(whole[1::2], parts[1])
    assert whole.sum() > 0
    camp.close()
    c1 = pipeline.HotPathConfig(tx_linewidth=1e-4, lo_linewidth=1e-4, decoding="dqpsk")
    camp = pipeline.McCampaign(c1, 4)
    e = camp.simulate(range(4))
    camp.close()
    np.testing.assert_array_equal(e, np.zeros(4, np.int64))
