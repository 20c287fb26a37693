"""GPU tests of the device Tx filter (plx_tx_bandlimit_dev, HotPathConfig(tx_filter=)) on the MI355X: the two
kernels of plx_txfilt.hip against pipeline.band_limit in numpy at every tile count, the batching property bit for bit, the
random-data transmitter with the filter against band_limit of the numpy chain, the de Bruijn route against the host route
(mux_filter), random data through a three-channel comb against a host recount, and the Monte-Carlo campaign under
reordering and ragged batching."""
import ctypes as C

import numpy as np
import pytest

from polmux_amd import _abi, synth
from polmux_amd.pipeline import band_limit
from polmux_amd.rxfront import myfilter
from tests.test_phase_noise import dqpsk_count_host, rotation_count_host
from tests.test_tx_filter import POWER_BAR, case, check_entry, ntiles
from tests.test_tx_random import SEED, reference_batch

pytestmark = pytest.mark.gpu

PLAN_BAR = 4e-14           # of max |u|: the transmitter's 1e-14 on the input plus the entry's 3e-14
SPACING = 456 / 256        # |s_1 - s_0| dFN of the comb below, in symbol rates (0.4 nm at 28 Gbaud, NSYMB 256)
# the COMB of tests/test_gpu_wdm_unique.py, restated, without its channel filter: the tests put tx_filter= or mux_filter= in
COMB = dict(nsymb=256, nt=16, nch=3, chspacing=0.4, cma_mu=1 / 300, freqavg=20, cma_taps=7, fft_length=256, cde_L=128,
            variants=3, wdm_field="unique", oftype="ideal", obw=0.9 * SPACING)
CHFILT = dict(ftype="ideal", bw=0.9 * SPACING)
LINEAR = dict(flag="g---", nspans=2, length=8e4, disp=17.0, pavg_mw=2.0)


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    b = _abi.get()
    assert b.path.endswith("polmux_amd/lib/libpolmux_hip.so")
    return b


class DevPlan:
    def __init__(self, lib, nfft, max_signals, h):
        self.lib, self.plan = lib, C.c_void_p()
        hr, hi = np.ascontiguousarray(h.real), np.ascontiguousarray(h.imag)
        lib.call("plx_filter_create", C.byref(self.plan), nfft, max_signals, hr.ctypes.data, hi.ctypes.data)

    def run(self, x, y, pavg=2.0):
        """plx_tx_bandlimit_dev on device copies of x, y [npairs, nfft] -> host (x, y, gain)"""
        import torch
        npairs, nfft = x.shape
        dx, dy = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda()      # (copies: the cases are read-only)
        gain = torch.full((npairs,), float("nan"), dtype=torch.float64, device="cuda")
        work = torch.full((npairs * ntiles(nfft),), float("nan"), dtype=torch.float64, device="cuda")
        self.lib.call("plx_tx_bandlimit_dev", self.plan, dx.data_ptr(), dy.data_ptr(), npairs, pavg, gain.data_ptr(),
                      work.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return dx.cpu().numpy(), dy.cpu().numpy(), gain.cpu().numpy()

    def close(self):
        self.lib.call("plx_filter_destroy", self.plan)


# a partial tile, two tiles, 32 tiles, the 512 tiles of the largest frame (two partials per thread in the second kernel)
@pytest.mark.parametrize("kind", ["random", "ideal"])
@pytest.mark.parametrize("nfft,npairs", [(256, 1), (4096, 5), (65536, 3), (1 << 20, 1)])
def test_gpu_entry_matches_band_limit(lib, nfft, npairs, kind):
    ref = case(nfft, npairs, kind)
    plan = DevPlan(lib, nfft, npairs, ref[2])
    try:
        gx, gy, gain = plan.run(ref[0], ref[1])
    finally:
        plan.close()
    check_entry(gx, gy, gain, ref)


@pytest.mark.parametrize("nfft", [4096, 65536])
def test_gpu_pair_in_a_batch_equals_the_pair_alone(lib, nfft):
    """pair 2 of a 5-pair call against the same pair alone on the same plan (max_signals 5): rows and gain bit for bit"""
    x, y, h = case(nfft, 5, "random")[:3]
    plan = DevPlan(lib, nfft, 5, h)
    try:
        bx, by, bg = plan.run(x, y)
        ax, ay, ag = plan.run(x[2:3], y[2:3])
    finally:
        plan.close()
    for a, b in ((ax[0], bx[2]), (ay[0], by[2]), (ag[0], bg[2])):
        assert np.array_equal(np.asarray(a).view(np.float64), np.asarray(b).view(np.float64))
    assert np.isfinite(bg).all() and bg[2] > 0


# ---------------------------------------------------------------------- the plan ---
def test_gpu_random_transmitter_with_filter_against_band_limit(lib):
    """HotPath(nsymb=64, nt=16, nch=3, tx_data='random', tx_filter=ideal 1.6): make_batch against band_limit of the numpy
    chain's frames, the power of every pair, the stop band, and everything the filter must leave alone"""
    import torch
    from polmux_amd import pipeline
    kw = dict(nsymb=64, nt=16, nch=3, tx_data="random")
    keys, bw, pavg = [0, 9, 4], 1.6, 2.0
    hp = pipeline.HotPath(pipeline.HotPathConfig(tx_filter=dict(ftype="ideal", bw=bw), **kw), 3)
    plain = pipeline.HotPath(pipeline.HotPathConfig(**kw), 3)
    try:
        ux, uy = hp.make_batch(3, data_keys=keys)
        px, py = plain.make_batch(3, data_keys=keys)
        torch.cuda.synchronize()
        assert tuple(ux.shape) == (3, 3, 1024)
        gx, gy = ux.cpu().numpy(), uy.cpu().numpy()
        rx, ry, _, _, _ = reference_batch(64, 16, 3, keys, pavg)
        fn = synth.fn_grid(64, 16)
        h = myfilter("ideal", fn, 0.5 * bw)
        wx, wy, wg = np.empty_like(rx), np.empty_like(ry), np.empty((3, 3))
        for f in range(3):
            for c in range(3):
                wx[f, c], wy[f, c] = band_limit(rx[f, c], ry[f, c], h, pavg)
                fx, fy = np.fft.ifft(np.fft.fft(rx[f, c]) * h), np.fft.ifft(np.fft.fft(ry[f, c]) * h)
                wg[f, c] = np.sqrt(pavg / np.mean(np.abs(fx) ** 2 + np.abs(fy) ** 2))
        scale = max(np.abs(wx).max(), np.abs(wy).max())
        ex, ey = np.abs(gx - wx).max() / scale, np.abs(gy - wy).max() / scale
        power = np.mean(np.abs(gx) ** 2 + np.abs(gy) ** 2, axis=-1)
        ep = np.abs(power / pavg - 1).max()
        eg = np.abs(hp.tx_gain.cpu().numpy().reshape(3, 3) / wg - 1).max()
        spec = np.abs(np.fft.fft(np.concatenate([gx, gy]).reshape(-1, 1024), axis=-1))
        stop = spec[:, np.abs(fn) > 0.5 * bw].max() / spec.max()
        print("field %.2e %.2e of max |u|, mean power %.2e, gain %.2e, stop band %.2e of the largest bin" % (ex, ey, ep, eg, stop))
        assert ex <= PLAN_BAR and ey <= PLAN_BAR
        assert ep <= POWER_BAR and eg <= POWER_BAR
        assert np.count_nonzero(np.abs(fn) > 0.5 * bw) > 0 and stop <= 1e-13
        assert np.abs(gx - px.cpu().numpy()).max() > 1e-3 * scale          # (the filter did change the field)
        # the patterns and the power after create_field are those of the plan without the filter
        for name in ("pat_frames", "dpat_frames", "tx_power"):
            assert np.array_equal(getattr(hp, name).cpu().numpy(), getattr(plain, name).cpu().numpy()), name
        assert np.array_equal(hp.rx_gain.cpu().numpy(), plain.rx_gain.cpu().numpy()) and hp.power_mw == plain.power_mw
        assert any(t is hp.tx_gain for t in hp.batch_tensors()) and len(hp.batch_tensors()) == len(plain.batch_tensors()) + 1
    finally:
        hp.close()
        plain.close()


def test_gpu_no_filter_is_the_transmitter_call(lib):
    """tx_filter=None: make_batch's fields are the direct output of plx_tx_qpsk_dev, bit for bit, and no gain is kept"""
    import torch
    from polmux_amd import pipeline
    keys = [0, 9, 4]
    hp = pipeline.HotPath(pipeline.HotPathConfig(nsymb=64, nt=16, nch=3, tx_data="random"), 3)
    try:
        ux, uy = hp.make_batch(3, data_keys=keys)
        assert hp.txfilt is None and hp.tx_gain is None and len(hp.batch_tensors()) == 4
        dx = torch.full((3, 3, 1024), float("nan"), dtype=torch.complex128, device="cuda")
        dy = torch.full_like(dx, float("nan"))
        pat = torch.empty((9, 4, 64), dtype=torch.uint8, device="cuda")
        power = torch.empty(9, dtype=torch.float64, device="cuda")
        kt = torch.as_tensor(np.asarray(keys, np.int64), device="cuda")
        drive = synth.qpsk_drive_tables(16)
        lib.call("plx_tx_qpsk_dev", dx.data_ptr(), dy.data_ptr(), 64, 16, 3, 3, drive.ctypes.data, 2.0, SEED, kt.data_ptr(),
                 pat.data_ptr(), None, power.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(ux.cpu().numpy().view(np.float64), dx.cpu().numpy().view(np.float64))
        assert np.array_equal(uy.cpu().numpy().view(np.float64), dy.cpu().numpy().view(np.float64))
        assert np.array_equal(hp.tx_power.cpu().numpy(), power.cpu().numpy())
    finally:
        hp.close()


def _through_the_link(frames, data_keys=None, **over):
    """(Tx fields of make_batch, error counts per channel-frame, hp.sym, mean EVM) of a batch of the comb over the linear link"""
    import torch
    from polmux_amd import pipeline
    kw = dict(COMB, **LINEAR)
    kw.update(over)
    hp = pipeline.HotPath(pipeline.HotPathConfig(**kw), max_frames=frames)
    try:
        ux, uy = hp.make_batch(frames, data_keys=data_keys)
        tx = (ux.cpu().numpy().copy(), uy.cpu().numpy().copy())
        hp.fibre(ux, uy)
        hp.receive(ux, uy)
        ncf = frames * hp.nch
        out = dict(tx=tx, rot=hp.errors_resolved(ncf).cpu().numpy(), dq=hp.errors_dqpsk(ncf).cpu().numpy(),
                   evm=hp.evm(ncf).cpu().numpy())
        torch.cuda.synchronize()
        out["sym"] = hp.sym[:ncf].cpu().numpy().copy()
        if data_keys is not None:
            out["bits"] = hp.tx_bits_host(data_keys).reshape(ncf, hp.cfg.nsymb, 4)
        return out
    finally:
        hp.close()


def test_gpu_debruijn_device_route_against_host_route(lib):
    """the comb's de Bruijn waveforms band-limited on the device at plan creation (tx_filter) against the host route
    (mux_filter, the yardstick, run here): make_batch within 4e-14 of max |u|, the same error counts per channel-frame"""
    host = _through_the_link(2, mux_filter=CHFILT)
    dev = _through_the_link(2, tx_filter=CHFILT)
    scale = max(np.abs(host["tx"][0]).max(), np.abs(host["tx"][1]).max())
    ex, ey = (np.abs(dev["tx"][i] - host["tx"][i]).max() / scale for i in range(2))
    print("de Bruijn, device against host band-limit: %.2e %.2e of max |u|; errors host %s device %s" %
          (ex, ey, host["rot"].tolist(), dev["rot"].tolist()))
    assert host["tx"][0].shape == (2, 3, 4096)
    assert ex <= PLAN_BAR and ey <= PLAN_BAR
    assert dev["rot"].shape == (6,) and np.array_equal(dev["rot"], host["rot"]) and np.array_equal(dev["dq"], host["dq"])


def _recount(sym, bits):
    """(rotation, dqpsk) host counts of symbols [ncf, 2, nsymb] against bits [ncf, nsymb, 4] (tests/test_gpu_tx_random.py)"""
    ncf = sym.shape[0]
    rot = [rotation_count_host(sym[i], bits[i]) for i in range(ncf)]
    dq = [dqpsk_count_host(sym[i], [2 * bits[i][:, 0].astype(int) + bits[i][:, 1], 2 * bits[i][:, 2].astype(int) + bits[i][:, 3]])
          for i in range(ncf)]
    return np.array(rot), np.array(dq)


def test_gpu_random_data_through_the_comb(lib):
    """two realisations of random data on the three-channel comb, band-limited on the device: the device counts equal a host
    recount of hp.sym against the mirror's bits, and a frame alone equals itself inside the batch, bit for bit.  The same two
    frames without the filter are run for the record: their mean EVM is printed, not asserted."""
    keys = [7, 10]
    rnd = dict(variants=1, tx_data="random")
    got = _through_the_link(2, data_keys=keys, tx_filter=CHFILT, **rnd)
    rot, dq = _recount(got["sym"], got["bits"])
    print("random comb with tx_filter: rotation %s / host %s, dqpsk %s / host %s" % (got["rot"].tolist(), rot.tolist(),
                                                                                      got["dq"].tolist(), dq.tolist()))
    assert np.array_equal(got["rot"], rot)
    assert np.array_equal(got["dq"], dq)
    alone = _through_the_link(1, data_keys=keys[1:], tx_filter=CHFILT, **rnd)
    assert np.array_equal(alone["sym"].view(np.float64), got["sym"][3:].view(np.float64))
    assert np.array_equal(alone["rot"], got["rot"][3:]) and np.array_equal(alone["dq"], got["dq"][3:])
    for i in range(2):
        assert np.array_equal(alone["tx"][i][0].view(np.float64), got["tx"][i][1].view(np.float64))
    bare = _through_the_link(2, data_keys=keys, **rnd)
    print("mean EVM of the two frames: %.6g with tx_filter, %.6g without (errors %s / %s)" %
          (got["evm"].mean(), bare["evm"].mean(), got["rot"].tolist(), bare["rot"].tolist()))


def _campaign_checks(a, va, b, vb, c, vc, order):
    assert a.shape == (24,) and b.shape == (24,) and va.shape == (24,)
    a, b, va, vb = a.reshape(8, 3), b.reshape(8, 3), va.reshape(8, 3), vb.reshape(8, 3)
    for i, r in enumerate(order):
        assert np.array_equal(b[i], a[r]) and np.array_equal(vb[i], va[r])
    for i, r in enumerate([7, 2, 5]):
        assert np.array_equal(c.reshape(3, 3)[i], a[r]) and np.array_equal(vc.reshape(3, 3)[i], va[r])
    assert len(set(va.reshape(-1).tolist())) == 24            # every realisation and channel has its own noise


def test_gpu_campaign_with_filter_is_keyed_by_realisation(lib):
    """McCampaign on the random-data comb with tx_filter and receiver noise: 8 realisations in batches of 4, reordered, and
    ragged ([7, 2, 5]): the same counts and EVM samples realisation for realisation"""
    from polmux_amd import pipeline
    kw = dict(COMB, variants=1, tx_data="random", tx_filter=CHFILT, **LINEAR)
    order = [4, 5, 6, 7, 0, 1, 2, 3]
    camp = pipeline.McCampaign(pipeline.HotPathConfig(**kw), frames_per_call=4, noise_sigma=0.35)
    try:
        a, va = camp.collect(camp.launch(list(range(8))), with_samples=True)
        b, vb = camp.collect(camp.launch(order), with_samples=True)
        c, vc = camp.collect(camp.launch([7, 2, 5]), with_samples=True)
    finally:
        camp.close()
    print("campaign counts %s, mean EVM %.4g" % (a.tolist(), va.mean()))
    _campaign_checks(a, va, b, vb, c, vc, order)
