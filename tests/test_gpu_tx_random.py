"""GPU tests of the device transmitter (plx_tx_qpsk_dev, HotPathConfig(tx_data='random')) on the MI355X:
the kernels against the numpy chain of tests/test_tx_random.py, the receiver's per-frame counts against a host recount
with the host mirror's bits, and the Monte-Carlo campaign's counts under every batching and sharding of the indices."""
import numpy as np
import pytest

from polmux_amd import _abi, synth
from tests.test_phase_noise import dqpsk_count_host, rotation_count_host
from tests.test_tx_random import SEED, check_against_reference, reference_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return _abi.get()


def _tx(lib, nsymb, nt, nfc, keys, pavg=2.0, dq=True):
    import torch
    F, n = len(keys), nsymb * nt
    ux = torch.full((F, nfc, n), float("nan"), dtype=torch.complex128, device="cuda")
    uy = torch.full_like(ux, float("nan"))
    pat = torch.full((F, nfc, 4, nsymb), 7, dtype=torch.uint8, device="cuda")
    pdq = torch.full_like(pat, 7) if dq else None
    power = torch.full((F, nfc), float("nan"), dtype=torch.float64, device="cuda")
    kt = torch.as_tensor(np.asarray(keys, np.int64), device="cuda")
    drive = synth.qpsk_drive_tables(nt)
    lib.call("plx_tx_qpsk_dev", ux.data_ptr(), uy.data_ptr(), nsymb, nt, nfc, F, drive.ctypes.data, pavg, SEED, kt.data_ptr(),
             pat.data_ptr(), pdq.data_ptr() if dq else None, power.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [t.cpu().numpy() if t is not None else None for t in (ux, uy, pat, pdq, power)]


@pytest.mark.parametrize("nsymb,nt,nfc,keys", [(1024, 64, 1, [3, (1 << 32) + 17]), (64, 16, 3, [0, 9, 4])])
def test_kernels_match_numpy_chain_and_batching(lib, nsymb, nt, nfc, keys):
    got = _tx(lib, nsymb, nt, nfc, keys)
    check_against_reference(got, reference_batch(nsymb, nt, nfc, keys, 2.0))
    alone = _tx(lib, nsymb, nt, nfc, [keys[1]], dq=False)
    for i in (0, 1, 2, 4):
        np.testing.assert_array_equal(alone[i][0], got[i][1])


def _cfg(**kw):
    from polmux_amd import pipeline
    return pipeline.HotPathConfig(nsymb=256, nt=16, length=1e3, cma_mu=1 / 600, freqavg=20, tx_data="random", **kw)


def _recount(hp, ncf, bits):
    """(rotation, dqpsk) host counts of the symbols now in hp.sym against bits [ncf, nsymb, 4]"""
    sym = hp.sym[:ncf].cpu().numpy()
    rot = [rotation_count_host(sym[i], bits[i]) for i in range(ncf)]
    dq = [dqpsk_count_host(sym[i], [2 * bits[i][:, 0].astype(int) + bits[i][:, 1], 2 * bits[i][:, 2].astype(int) + bits[i][:, 3]])
          for i in range(ncf)]
    return np.array(rot), np.array(dq)


@pytest.mark.parametrize("nch,F", [(1, 6), (3, 2)])
def test_noise_free_frames_count_against_their_own_data(lib, nch, F):
    import torch
    from polmux_amd import pipeline
    hp = pipeline.HotPath(_cfg(nch=nch), F)
    keys = [7 + 3 * f for f in range(F)]
    ux, uy = hp.make_batch(F, data_keys=keys)
    assert tuple(ux.shape) == ((F, hp.cfg.nfft) if nch == 1 else (F, nch, hp.cfg.nfft))
    bits = hp.tx_bits_host(keys)                                      # [F, nch, nsymb, 4]
    assert bits.shape == (F, nch, 256, 4)
    flat = bits.reshape(F * nch, 256, 4)
    np.testing.assert_array_equal(hp.pat_frames.cpu().numpy(), flat.transpose(0, 2, 1))   # channel c = the mirror's chan
    assert len({flat[i].tobytes() for i in range(F * nch)}) == F * nch                  # every channel-frame its own data
    power = hp.tx_power.cpu().numpy()
    assert np.ptp(power) > 0                                          # ... and its own power, undone by its own gain
    np.testing.assert_allclose(hp.rx_gain.cpu().numpy().reshape(-1), np.sqrt(hp.power_mw / power), rtol=1e-14)
    hp.fibre(ux, uy)
    hp.receive(ux, uy)
    ncf = F * nch
    e_rot = hp.errors_resolved(ncf).cpu().numpy()
    e_dq = hp.errors_dqpsk(ncf).cpu().numpy()
    torch.cuda.synchronize()
    rot, dq = _recount(hp, ncf, flat)
    print("rotation", e_rot, rot, "dqpsk", e_dq, dq, "mean |symbol|", np.abs(hp.sym[:ncf].cpu().numpy()).mean())
    np.testing.assert_array_equal(e_rot, rot)
    np.testing.assert_array_equal(e_dq, dq)
    assert e_rot.max() <= 2 and e_dq.max() <= 2
    hp.close()


def test_campaign_counts_do_not_depend_on_batching_or_sharding(lib):
    """twelve noisy realisations in one batch, in ragged pipelined batches of five and one at a time: the same counts --
    a pattern, power or gain buffer reused under the receiver's stream would change them -- and through McRankShare"""
    from polmux_amd import pipeline
    cfg = _cfg(decoding="dqpsk")
    counts = {}
    for F in (12, 5, 1):
        camp = pipeline.McCampaign(cfg, F, noise_sigma=1.2)
        counts[F] = camp.simulate(list(range(12)))
        if F == 5:
            share = pipeline.McRankShare(camp, 1, 2).simulate(list(range(6)))
        half = camp.bits_per_realisation // 2
        camp.close()
    print("counts", counts, "share", share)
    np.testing.assert_array_equal(counts[5], counts[12])
    np.testing.assert_array_equal(counts[1], counts[12])
    np.testing.assert_array_equal(share, counts[12][1::2])
    assert np.count_nonzero(counts[12]) >= 6 and np.all(counts[12] < half)


def test_debruijn_batches_are_untouched(lib):
    from polmux_amd import pipeline
    hp = pipeline.HotPath(pipeline.HotPathConfig(nsymb=64, nt=16, variants=2), 3)
    assert hp.random is False
    ux, uy = hp.make_batch(3, data_keys=[5, 6, 7])
    for f in range(3):
        vx, vy, _ = hp.var_host[f % 2]
        np.testing.assert_array_equal(ux[f].cpu().numpy(), vx)
        np.testing.assert_array_equal(uy[f].cpu().numpy(), vy)
    assert hp.rx_gain is None and hp.batch_tensors() == []
    hp.close()
