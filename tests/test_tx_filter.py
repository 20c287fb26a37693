"""CPU tests (-m "not gpu") of the device Tx filter (plx_tx_bandlimit_dev, HotPathConfig(tx_filter=)): the
kernels of plx_txfilt.hip under the host emulator against pipeline.band_limit in numpy, the batching property bit for bit,
the H = 0 case, every refusal of the entry, and the host option's validation.  tests/test_gpu_tx_filter.py imports the
cases and their bars from here."""
import ctypes as C
import functools

import numpy as np
import pytest

from polmux_amd import _abi, synth
from polmux_amd.pipeline import band_limit
from polmux_amd.rxfront import myfilter

FIELD_BAR = 3e-14      # of max |reference|: the filter's 2e-14 plus the rounding of one sum, one square root, one multiply
POWER_BAR = 1e-13      # relative: the project's bar for a power (gain, and the mean power of every output pair)
TILE = 2048


def ntiles(nfft):
    return -(-nfft // TILE)


@functools.lru_cache(maxsize=None)
def case(nfft, npairs, kind, pavg=2.0):
    """(x, y [npairs, nfft], H [nfft], reference x, y, gain) -- computed once, shared, never written to.  kind 'random': a
    random complex table; 'ideal': myfilter('ideal', FN, 0.8) on the grid of nt = 16 samples per symbol."""
    rng = np.random.default_rng(1000 * npairs + nfft % 997 + (kind == "ideal"))
    x = rng.standard_normal((npairs, nfft)) + 1j * rng.standard_normal((npairs, nfft))
    y = rng.standard_normal((npairs, nfft)) + 1j * rng.standard_normal((npairs, nfft))
    x *= (1 + np.arange(npairs)).reshape(-1, 1)                    # every pair its own power, so its own gain
    if kind == "random":
        h = rng.standard_normal(nfft) + 1j * rng.standard_normal(nfft)
    else:
        h = np.asarray(myfilter("ideal", synth.fn_grid(nfft // 16, 16), 0.8), dtype=complex)
        assert 0 < np.count_nonzero(h) < nfft
    rx, ry, gain = np.empty_like(x), np.empty_like(y), np.empty(npairs)
    for p in range(npairs):
        fx, fy = np.fft.ifft(np.fft.fft(x[p]) * h), np.fft.ifft(np.fft.fft(y[p]) * h)
        gain[p] = np.sqrt(pavg / np.mean(np.abs(fx) ** 2 + np.abs(fy) ** 2))
        rx[p], ry[p] = band_limit(x[p], y[p], h, pavg)
    for a in (x, y, h, rx, ry, gain):
        a.setflags(write=False)
    return x, y, h, rx, ry, gain


def check_entry(gx, gy, gain, ref, pavg=2.0):
    """the bars of the issue on one call's output against case(...)"""
    _, _, _, rx, ry, rgain = ref
    scale = max(np.abs(rx).max(), np.abs(ry).max())
    ex, ey = np.abs(gx - rx).max() / scale, np.abs(gy - ry).max() / scale
    eg = np.abs(gain / rgain - 1).max()
    power = np.mean(np.abs(gx) ** 2 + np.abs(gy) ** 2, axis=-1)
    ep = np.abs(power / pavg - 1).max()
    print("field %.2e %.2e gain %.2e mean power %.2e" % (ex, ey, eg, ep))
    assert ex <= FIELD_BAR and ey <= FIELD_BAR
    assert eg <= POWER_BAR
    assert ep <= POWER_BAR
    assert len(set(np.round(gain, 6).tolist())) == gain.size        # (the pairs did have their own gains)


# ----------------------------------------------------------------- emulator helpers ---
@pytest.fixture(scope="module")
def emu():
    from tests import _emu
    return _emu.binding()


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class EmuPlan:
    def __init__(self, emu, nfft, max_signals, h):
        self.emu, self.plan = emu, C.c_void_p()
        hr, hi = np.ascontiguousarray(h.real), np.ascontiguousarray(h.imag)
        emu.call("plx_filter_create", C.byref(self.plan), nfft, max_signals, _vp(hr), _vp(hi))

    def run(self, x, y, pavg=2.0, with_gain=True):
        """plx_tx_bandlimit_dev on copies of x, y [npairs, nfft] -> (x, y, gain, work)"""
        npairs, nfft = x.shape
        gx, gy = np.array(x, dtype=np.complex128), np.array(y, dtype=np.complex128)
        gain = np.full(npairs, np.nan) if with_gain else None
        work = np.full(npairs * ntiles(nfft), np.nan)
        self.emu.call("plx_tx_bandlimit_dev", self.plan, _vp(gx), _vp(gy), npairs, pavg, _vp(gain), _vp(work), None)
        return gx, gy, gain, work

    def close(self):
        self.emu.call("plx_filter_destroy", self.plan)


# ----------------------------------------------------------------------------- tests ---
def test_abi_entry_point_declared():
    assert "plx_tx_bandlimit_dev" in _abi.SIGNATURES and len(_abi.SIGNATURES["plx_tx_bandlimit_dev"]) == 8


# a partial tile, exactly one tile, two tiles, many tiles; odd pair counts
@pytest.mark.parametrize("kind", ["random", "ideal"])
@pytest.mark.parametrize("nfft,npairs", [(256, 1), (2048, 3), (4096, 5), (65536, 2)])
def test_emu_entry_matches_band_limit(emu, nfft, npairs, kind):
    ref = case(nfft, npairs, kind)
    plan = EmuPlan(emu, nfft, npairs, ref[2])
    try:
        gx, gy, gain, work = plan.run(ref[0], ref[1])
    finally:
        plan.close()
    check_entry(gx, gy, gain, ref)
    # the tile partials are the sum's terms: they add up to nfft m_p = nfft pavg / k_p^2
    tot = work.reshape(npairs, -1).sum(1)
    np.testing.assert_allclose(tot, nfft * 2.0 / gain ** 2, rtol=1e-13)


def test_emu_pair_in_a_batch_equals_the_pair_alone(emu):
    """pair 2 of a 5-pair call against the same pair alone on the same plan: rows and gain bit for bit"""
    nfft = 4096
    x, y, h = case(nfft, 5, "random")[:3]
    plan = EmuPlan(emu, nfft, 5, h)
    try:
        bx, by, bg, _ = plan.run(x, y)
        ax, ay, ag, _ = plan.run(x[2:3], y[2:3])
        nx, ny, none, _ = plan.run(x[2:3], y[2:3], with_gain=False)      # d_gain NULL changes nothing else
    finally:
        plan.close()
    assert none is None
    for a, b in ((ax[0], bx[2]), (ay[0], by[2]), (ag[0], bg[2]), (nx[0], bx[2]), (ny[0], by[2])):
        assert np.array_equal(np.asarray(a).view(np.float64), np.asarray(b).view(np.float64))


def test_emu_zero_response_leaves_zero_rows_and_gain_zero(emu):
    nfft = 4096
    x, y = case(nfft, 5, "random")[:2]
    plan = EmuPlan(emu, nfft, 3, np.zeros(nfft, complex))
    try:
        gx, gy, gain, work = plan.run(x[:3], y[:3])
    finally:
        plan.close()
    assert np.all(gx == 0) and np.all(gy == 0)
    assert np.all(gain == 0)
    assert np.all(np.isfinite(gx.view(np.float64))) and np.all(np.isfinite(gy.view(np.float64))) and np.all(work == 0)


def test_emu_refusals(emu):
    nfft = 256
    plan = EmuPlan(emu, nfft, 2, np.ones(nfft, complex))
    x, y = np.ones((2, nfft), complex), np.ones((2, nfft), complex)
    gain, work = np.zeros(2), np.zeros(2)
    good = [plan.plan, _vp(x), _vp(y), 2, 2.0, _vp(gain), _vp(work), None]
    try:
        emu.call("plx_tx_bandlimit_dev", *good)
        bad = [(0, None), (1, None), (2, None), (6, None), (3, 0), (3, 3), (3, -1), (4, 0.0), (4, -1.0), (4, float("inf")),
               (4, float("-inf")), (4, float("nan"))]
        for pos, val in bad:
            a = list(good)
            a[pos] = val
            x0 = x.copy()
            with pytest.raises(_abi.PolmuxError, match="plx_tx_bandlimit_dev") as ei:
                emu.call("plx_tx_bandlimit_dev", *a)
            assert ei.value.code == _abi.PLX_ERR_ARG, (pos, val)
            assert np.array_equal(x, x0)                               # refused before anything is written
        a = list(good)
        a[5] = None                                                    # d_gain may be NULL
        emu.call("plx_tx_bandlimit_dev", *a)
    finally:
        plan.close()


# ---------------------------------------------------------------------- host options ---
UNIQUE = dict(nch=3, wdm_field="unique")


def test_check_tx_filter_accepts():
    from polmux_amd.pipeline import HotPathConfig, check_tx_filter
    assert HotPathConfig().tx_filter is None
    assert check_tx_filter(HotPathConfig()) is False
    ok = [dict(tx_filter=dict(ftype="ideal", bw=1.6)), dict(tx_filter=dict(ftype="gauss", bw=1.2, ord=3)),
          dict(tx_filter=dict(ftype="ideal", bw=np.float64(1.6))), dict(tx_filter=dict(ftype="ideal", bw=2)),
          dict(tx_filter=dict(ftype="ideal", bw=1.6), tx_data="random"),
          dict(tx_filter=dict(ftype="ideal", bw=1.6), tx_data="random", **UNIQUE),
          dict(tx_filter=dict(ftype="ideal", bw=1.6), **UNIQUE),
          dict(tx_filter=dict(ftype="ideal", bw=1.6), nch=3), dict(tx_filter=dict(ftype="ideal", bw=1.6), nch=3, tx_data="random")]
    from polmux_amd.pipeline import check_tx_options, check_wdm_options
    for kw in ok:
        cfg = HotPathConfig(**kw)
        assert check_tx_filter(cfg) is True
        check_wdm_options(cfg)                                         # ... and the other options do not object to it
        check_tx_options(cfg)


MALFORMED = ["ideal", ["ideal", 1.6], dict(bw=1.6), dict(ftype="ideal"), dict(ftype="ideal", bw=1.6, order=3), dict(),
             dict(ftype="ideal", bw=0), dict(ftype="ideal", bw=-1.0), dict(ftype="ideal", bw=float("inf")),
             dict(ftype="ideal", bw=float("nan")), dict(ftype="ideal", bw="1.6"), dict(ftype="ideal", bw=[1.6]),
             dict(ftype="ideal", bw=np.array([1.6, 1.6])), dict(ftype="ideal", bw=None), dict(ftype="ideal", bw=True),
             dict(ftype="ideal", bw=1.6j), dict(ftype=7, bw=1.6), dict(ftype=None, bw=1.6)]


def test_check_tx_filter_refuses_and_the_plan_refuses_before_any_device_use():
    from polmux_amd.pipeline import HotPath, HotPathConfig, check_tx_filter
    bad = [dict(tx_filter=tf) for tf in MALFORMED]
    bad += [dict(tx_filter=tf, tx_data="random", **UNIQUE) for tf in MALFORMED[:4]]
    bad.append(dict(tx_filter=dict(ftype="ideal", bw=1.6), mux_filter=dict(ftype="ideal", bw=1.6), **UNIQUE))
    for kw in bad:
        with pytest.raises(ValueError, match="tx_filter"):
            check_tx_filter(HotPathConfig(**kw))
        with pytest.raises(ValueError, match="tx_filter"):
            HotPath(HotPathConfig(**kw), 1)
    # mux_filter's own refusals are what they were: random data still refuses the host band-limit, and says where to go
    with pytest.raises(ValueError, match="tx_data") as ei:
        HotPath(HotPathConfig(tx_data="random", mux_filter=dict(ftype="ideal", bw=1.6), **UNIQUE), 1)
    assert "tx_filter" in str(ei.value)
    with pytest.raises(ValueError, match="mux_filter needs wdm_field='unique'"):
        HotPath(HotPathConfig(nch=3, mux_filter=dict(ftype="ideal", bw=1.6)), 1)
