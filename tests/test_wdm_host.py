"""Host side of the one-field WDM route, no library and no GPU: the option checks HotPath.__init__
makes through pipeline.check_wdm_options, the walk-off delay, and the multiplexer's channel filter."""
import math

import numpy as np
import pytest

from polmux_amd import pipeline
from polmux_amd.pipeline import HotPathConfig, check_wdm_options
from tests import wdm_ref


def test_defaults_are_the_separate_fields():
    cfg = HotPathConfig()
    assert cfg.wdm_field == "sepfields" and cfg.mux_filter is None
    assert check_wdm_options(cfg) is False
    assert check_wdm_options(HotPathConfig(nch=3, xpm_dualpol="manakov", flag="gpsx", manakov="yes")) is False
    assert check_wdm_options(HotPathConfig(equaliser="dbp")) is False


def test_unique_is_accepted():
    assert check_wdm_options(HotPathConfig(nch=3, wdm_field="unique")) is True
    assert check_wdm_options(HotPathConfig(nch=1, wdm_field="unique")) is True          # one channel: the one-channel path
    assert check_wdm_options(HotPathConfig(nch=3, wdm_field="unique", mux_filter=dict(ftype="ideal", bw=1.6))) is True
    assert check_wdm_options(HotPathConfig(nch=3, wdm_field="unique", mux_filter=dict(ftype="supergauss", bw=1.6, ord=3))) is True
    assert check_wdm_options(HotPathConfig(nch=3, wdm_field="unique", frontend="cohmix", decoding="dqpsk")) is True


@pytest.mark.parametrize("value", ["Unique", "sep", None, 1, ""])
def test_other_field_types_raise(value):
    with pytest.raises(ValueError, match="wdm_field must be 'sepfields' or 'unique'"):
        check_wdm_options(HotPathConfig(wdm_field=value))


def test_mux_filter_with_sepfields_raises():
    with pytest.raises(ValueError, match="mux_filter needs wdm_field='unique'"):
        check_wdm_options(HotPathConfig(nch=3, mux_filter=dict(ftype="ideal", bw=1.6)))
    with pytest.raises(ValueError, match="mux_filter needs wdm_field='unique'"):
        check_wdm_options(HotPathConfig(mux_filter=dict(ftype="gauss", bw=1.6)))


@pytest.mark.parametrize("mf", ["ideal", dict(bw=1.0), dict(ftype="ideal"), dict(ftype="ideal", bw=1.0, order=3),
                                dict(ftype="ideal", bw=0.0), dict(ftype="ideal", bw=float("nan")), dict(ftype="ideal", bw=[1.0, 2.0])])
def test_malformed_mux_filter_raises(mf):
    with pytest.raises(ValueError, match="mux_filter"):
        check_wdm_options(HotPathConfig(nch=3, wdm_field="unique", mux_filter=mf))


def test_unique_with_dbp_or_xpm_raises_naming_the_option():
    with pytest.raises(ValueError, match="equaliser='dbp'"):
        check_wdm_options(HotPathConfig(nch=3, wdm_field="unique", equaliser="dbp"))
    with pytest.raises(ValueError, match="xpm_dualpol"):
        check_wdm_options(HotPathConfig(nch=3, wdm_field="unique", xpm_dualpol="manakov", flag="gpsx", manakov="yes"))


def test_walkoff_delay():
    """The comb of the linear known answer (tests/test_emu_wdm.py: 3 channels 0.4 nm apart, 28 Gbaud, NSYMB 256, NT 16, D 17):
    shifts -456 / 0 / 456 bins; after 80 km the neighbours are -15.22 / +15.22 symbols away (-243 / +244 samples), after two
    spans -30.43 / +30.45 (-487 / +487).  The channel at the HIGHER frequency (negative shift: mux moves a channel by
    -s_c bins) arrives early in a fibre of D > 0.  Against D L dlambda from the textbook, with dlambda of the integer bin."""
    cb = wdm_ref.comb()
    assert list(cb["shift"]) == [-456, 0, 456] and cb["dfn"] == 1 / 256
    assert list(cb["delay"]) == [-243, 0, 244]
    np.testing.assert_allclose(cb["ds"], [-15.2163, 0.0, 15.2242], atol=2e-4)
    cb2 = wdm_ref.comb(nspans=2)
    assert list(cb2["delay"]) == [-487, 0, 487]
    np.testing.assert_allclose(cb2["ds"], 2 * cb["ds"], rtol=1e-14)
    # D L dlambda: the carrier of channel 0 is 456 bins = 456 / 256 * 28 GHz above the centre
    c, lam = 299792458.0, 1550.0
    dnu = 456 / 256 * 28.0                                   # GHz
    dlam = lam * lam / c * dnu                               # nm  (nm^2 GHz / (m/s) = 1e-18 m^2 1e9 / s / (m/s) = 1e-9 m)
    textbook = 17.0 * 80.0 * dlam * 1e-3 * 28.0              # ps/nm/km km nm -> ps; 1e-3 -> ns; times GHz -> symbols
    assert abs(abs(cb["ds"][0]) - textbook) < 2e-2 and abs(cb["ds"][2] - textbook) < 2e-2
    # the rounding is MATLAB's round (half away from zero), sign kept
    ds, d = pipeline.wdm_walkoff([1, -1], 1.0, 0.0, 1.0, 1.0, 2.5 / (2 * math.pi * 16), 16)
    assert list(ds * 16) == [-2.5, 2.5] and list(d) == [-3, 3]
    # slope changes b30 only: the outer channels move by different amounts
    cs = wdm_ref.comb(slope=0.06)
    assert cs["ds"][0] > cb["ds"][0] and cs["ds"][2] > cb["ds"][2] and cs["delay"][1] == 0


def test_band_limit_keeps_the_power_and_the_band():
    from polmux_amd import synth
    from polmux_amd.rxfront import myfilter
    fn = synth.fn_grid(64, 16)
    h = myfilter("ideal", fn, 0.5 * 1.6)
    vx, vy, _, _ = synth.pdm_qpsk_field(64, 16, 2.0)
    fx, fy = pipeline.band_limit(vx, vy, h, 2.0)
    assert np.mean(np.abs(fx) ** 2 + np.abs(fy) ** 2) == pytest.approx(2.0, rel=1e-13)
    out = np.abs(fn) > 0.8
    assert np.abs(np.fft.fft(fx)[out]).max() < 1e-9 * np.abs(np.fft.fft(fx)).max()
    assert np.abs(np.fft.fft(vx)[out]).max() > 1e-3 * np.abs(np.fft.fft(vx)).max()       # the unfiltered waveform has tails


def test_sharded_ber_refuses_per_channel_frame_counts():
    """mc.ShardedBer takes one count per realisation; the [n nch] vector of a 'unique' campaign with nch > 1 is refused with
    a message that says so (limits) instead of a shape error inside the exchange."""
    from polmux_amd import mc
    x = dict(stop=[0.1, 95], nmin=1)
    ok = mc.ShardedBer(lambda idx: np.full(len(idx), 3, np.int64), 1024, x, per_rank_per_round=4)
    ok.run(max_realisations=8)
    assert len(ok.counts) >= 4
    sb = mc.ShardedBer(lambda idx: np.zeros(3 * len(idx), np.int64), 1024, x, per_rank_per_round=4)
    with pytest.raises(ValueError, match="one error count per realisation"):
        sb.run(max_realisations=8)
