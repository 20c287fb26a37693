"""Host side of the per-channel 'sepfields' receiver (HotPathConfig(wdm_receiver='channel')): the walk-off
table, the per-channel CDE tables and the raises of check_config.  No GPU, no library."""
import numpy as np
import pytest

from polmux_amd import pipeline
from polmux_amd.rx import cde_transfer
from tests import wdm_rx_ref


def _matlab_round(v):
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def test_sepfields_walkoff_known_answers():
    """Three channels 0.4 nm apart, D = 17, 2 x 80 km, 28 Gbaud: delay_symbols = L SYMBOLRATE b1 (fiber.m:367 over two equal
    spans) is antisymmetric around the centre up to the lamc asymmetry of fiber.m:315 (lamc is the harmonic mean of the outer
    wavelengths, 1550 - 1.0e-4 nm here: every channel moves by ~ +0.008 symbols), its magnitude is the 'unique' route's
    30.4 symbols (D dlambda L = 17 x 0.4 x 160 ps = 1088 ps = 30.46 symbols of 35.7 ps), the channel at the shorter
    wavelength arrives early, and delay is MATLAB's round of delay_symbols nt."""
    cb = wdm_rx_ref.sep_comb(nch=3, chspacing=0.4, length=8e4)
    ds, delay = pipeline.sepfields_walkoff(cb["t"]["b1"], 2 * 8e4, 28.0, 16)
    assert ds.shape == (3,) and delay.shape == (3,) and delay.dtype == np.int64
    assert ds[0] < 0 < ds[2]
    assert abs(abs(ds[0]) - 30.46) < 0.05 and abs(abs(ds[2]) - 30.46) < 0.05
    assert abs(ds[1]) < 0.02 and abs(ds[0] + ds[2] - 2 * ds[1]) < 1e-3          # antisymmetric around the centre's own offset
    assert np.array_equal(delay, _matlab_round(ds * 16)) and list(delay) == [-487, 0, 488]
    assert np.all(np.abs(ds * 16 - delay) <= 0.5)
    # linear in the length: one span is half of it
    ds1, _ = pipeline.sepfields_walkoff(cb["t"]["b1"], 8e4, 28.0, 16)
    assert np.allclose(2 * ds1, ds, rtol=1e-15, atol=0)


def test_sepfields_walkoff_rounds_half_away_from_zero():
    """MATLAB's round: +-0.5 -> +-1, +-2.5 -> +-3 (numpy's rint would give 0 and +-2); b1 chosen so that the products are exact"""
    ds, delay = pipeline.sepfields_walkoff([0.5, -0.5, 2.5, -2.5, 1.5, -1.5, 0.25, -0.25, 0.0], 1.0, 1.0, 1)
    assert list(delay) == [1, -1, 3, -3, 2, -2, 0, 0, 0]
    ds, delay = pipeline.sepfields_walkoff([0.03125, -0.03125], 2.0, 0.5, 16)      # 0.5 samples of nt = 16
    assert list(ds) == [0.03125, -0.03125] and list(delay) == [1, -1]


def test_one_channel_has_no_delay_and_the_shared_table():
    """nch = 1: the delay is [0] and the stacked CDE table equals cde_transfer(...) at lam and disp, the table without the option, bit for bit"""
    cb = wdm_rx_ref.sep_comb(nch=1, slope=0.08)
    ds, delay = pipeline.sepfields_walkoff(cb["t"]["b1"], 16e4, 28.0, 16)
    assert list(delay) == [0] and abs(ds[0]) < 1e-9
    assert list(cb["lam"]) == [1550.0] and list(cb["t"]["Dch"]) == [17.0]
    H = pipeline.wdm_cde_tables(256, 56e9, cb["lam"], 16e4, cb["t"]["Dch"], 0.08)
    want = cde_transfer(256, 56e9, 1550.0 * 1e-9, 16e4, 17.0 * 1e-6, 0.08 * 1e-6)
    assert H.shape == (1, 256) and H.dtype == np.complex128 and H.flags["C_CONTIGUOUS"]
    assert np.array_equal(H[0], want)


def test_per_channel_tables_follow_dch_and_lambda():
    """channel c's table is cde_transfer at LAMBDA[c] and Dch[c] = disp + slope (LAMBDA[c] - lam) (fiber.m:336)"""
    cb = wdm_rx_ref.sep_comb(nch=3, chspacing=8.0, slope=0.09)
    assert np.allclose(cb["t"]["Dch"], [17 - 0.72, 17, 17 + 0.72], rtol=0, atol=1e-12)
    H = pipeline.wdm_cde_tables(256, 56e9, cb["lam"], 16e4, cb["t"]["Dch"], 0.09)
    assert H.shape == (3, 256)
    for c in range(3):
        assert np.array_equal(H[c], cde_transfer(256, 56e9, cb["lam"][c] * 1e-9, 16e4, cb["t"]["Dch"][c] * 1e-6, 0.09e-6))
    assert not np.array_equal(H[0], H[1]) and not np.array_equal(H[2], H[1])


def test_wdm_receiver_option_raises_without_a_gpu():
    cfg = pipeline.HotPathConfig
    assert cfg().wdm_receiver is None
    assert pipeline.check_config(cfg(nch=3, wdm_receiver="channel")) == (False, False, False)
    assert pipeline.check_config(cfg(nch=1, wdm_receiver="channel")) == (False, False, False)
    for bad in ("frame", "Channel", "", 1, True, ["channel"]):
        with pytest.raises(ValueError, match="wdm_receiver must be None or 'channel'"):
            pipeline.check_config(cfg(nch=3, wdm_receiver=bad))
    with pytest.raises(ValueError, match="wdm_field='unique'"):
        pipeline.check_config(cfg(nch=3, wdm_receiver="channel", wdm_field="unique"))
    with pytest.raises(ValueError, match="frontend='pick'"):
        pipeline.check_config(cfg(nch=3, wdm_receiver="channel", frontend="cohmix"))
    with pytest.raises(ValueError, match="equaliser='dbp'"):
        pipeline.check_config(cfg(nch=3, wdm_receiver="channel", equaliser="dbp"))


def test_abi_declares_the_two_entry_points():
    from polmux_amd import _abi
    assert len(_abi.SIGNATURES["plx_pick_wdm_dev"]) == 11 and len(_abi.SIGNATURES["plx_cde_create_wdm"]) == 6
