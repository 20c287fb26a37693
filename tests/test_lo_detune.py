"""Host side of the LO frequency offset (HotPathConfig(lo_detuning, lo_detuning_spread)): Hz to bins,
every raise and both warnings of check_config, and the host restatement of the device draw.  No GPU, no library."""
import math
import warnings

import numpy as np
import pytest

from polmux_amd import _abi, pipeline, synth

MINFREQ = 28.0e9 / 1024          # one bin of the default grid


def cfg(**kw):
    return pipeline.HotPathConfig(**kw)


def test_abi_declares_the_entry_points():
    assert len(_abi.SIGNATURES["plx_lo_detune_dev"]) == 17 and len(_abi.SIGNATURES["plx_dsp_run_freq_dev"]) == 6
    assert _abi.PLX_PHILOX_LO_DETUNE == 5 == synth.PHILOX_LO_DETUNE


@pytest.mark.parametrize("hz,k", [(0.0, 0), (0.999 * MINFREQ, 0), (1.5 * MINFREQ, 1), (-0.5 * MINFREQ, -1), (-1.5 * MINFREQ, -2),
                                  (100.25 * MINFREQ, 100), (-100.25 * MINFREQ, -101), (1e9, math.floor(1e9 / MINFREQ))])
def test_bins_from_hz_floor(hz, k):
    """k0 = floor(lo_detuning / minfreq), K = floor(lo_detuning_spread / minfreq): the reference's floor, towards -inf"""
    assert pipeline.lo_detune_bins(cfg(lo_detuning=hz))[0] == k
    if hz >= 0:
        assert pipeline.lo_detune_bins(cfg(lo_detuning_spread=hz))[1] == k
    c = cfg(nsymb=256, symbolrate=10.0, lo_detuning=2.5 * 10e9 / 256)
    assert pipeline.lo_detune_bins(c) == (2, 0)


@pytest.mark.parametrize("kw,what", [(dict(lo_detuning=float("nan")), "lo_detuning must be a finite scalar"),
                                     (dict(lo_detuning=float("inf")), "lo_detuning must be a finite scalar"),
                                     (dict(lo_detuning_spread=float("nan")), "lo_detuning_spread must be a finite scalar"),
                                     (dict(lo_detuning=[1.0, 2.0]), "lo_detuning must be a finite scalar"),
                                     (dict(lo_detuning="1e9"), "lo_detuning must be a finite scalar"),
                                     (dict(lo_detuning_spread=-1.0), "lo_detuning_spread must be >= 0"),
                                     (dict(nsymb=64, nt=4, lo_detuning_spread=128.5 * 28e9 / 64), "do not fit"),
                                     (dict(lo_detuning=3 * MINFREQ, equaliser="dbp"), "not with equaliser='dbp'"),
                                     (dict(lo_detuning_spread=3 * MINFREQ, equaliser="dbp"), "not with equaliser='dbp'")])
def test_check_config_raises(kw, what):
    with pytest.raises(ValueError, match=what):
        pipeline.check_config(cfg(**kw))


def test_check_config_accepts_and_keeps_its_return():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert pipeline.check_config(cfg()) == (False, False, False)
        assert pipeline.check_config(cfg(lo_detuning=-5.5 * MINFREQ, lo_detuning_spread=3.5 * MINFREQ)) == (False, False, False)
        assert pipeline.check_config(cfg(equaliser="dbp", lo_detuning=0.0, lo_detuning_spread=0.0)) == (False, False, False)
        # the largest spread a frame holds: 2 K + 1 = nfft - 1 (no estimator, so no range to warn about)
        pipeline.check_config(cfg(nsymb=64, nt=4, freqavg=0, lo_detuning_spread=127.5 * 28e9 / 64))


def test_warnings():
    with pytest.warns(UserWarning, match="below one frequency bin"):
        pipeline.check_config(cfg(lo_detuning=0.5 * MINFREQ))
    with pytest.warns(UserWarning, match="range of the QPSK frequency estimator"):
        pipeline.check_config(cfg(lo_detuning=128.5 * MINFREQ))                    # nsymb / 8 = 128
    with pytest.warns(UserWarning, match="range of the QPSK frequency estimator"):
        pipeline.check_config(cfg(lo_detuning=-120.5 * MINFREQ, lo_detuning_spread=7.5 * MINFREQ))   # |-121| + 7
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pipeline.check_config(cfg(lo_detuning=-120.5 * MINFREQ, lo_detuning_spread=6.5 * MINFREQ))   # 127: inside
        pipeline.check_config(cfg(lo_detuning=300.5 * MINFREQ, freqavg=0))          # no estimator: nothing to warn about


def test_lo_bins_host_draws():
    """synth.lo_detune_bins: k0 when K = 0; within k0 +- K; a pure function of (key, channel); channels differ; over 4096
    keys with K = 3 each of the 7 values occurs with a frequency within 4 standard errors of 1/7"""
    seed = pipeline.MASTER_SEED
    assert np.array_equal(synth.lo_detune_bins(seed, [3, 9], 4, -12, 0), np.full((2, 4), -12))
    keys = list(range(4096))
    b = synth.lo_detune_bins(seed, keys, 3, 5, 3)
    assert b.shape == (4096, 3) and b.dtype == np.int64 and b.min() == 2 and b.max() == 8
    again = synth.lo_detune_bins(seed, [77, 4000, 77], 3, 5, 3)
    assert np.array_equal(again[0], b[77]) and np.array_equal(again[1], b[4000]) and np.array_equal(again[2], b[77])
    assert (b[:, 0] != b[:, 1]).mean() > 0.7 and (b[:, 1] != b[:, 2]).mean() > 0.7     # (6/7 expected)
    p = 1 / 7
    se = math.sqrt(p * (1 - p) / 4096)
    for c in range(3):
        freq = np.array([(b[:, c] == v).mean() for v in range(2, 9)])
        assert np.abs(freq - p).max() <= 4 * se, (c, freq.tolist())
    assert not np.array_equal(synth.lo_detune_bins(seed + 1, keys[:64], 3, 5, 3), b[:64])   # the seed is part of the key
    big = synth.lo_detune_bins(seed, [(1 << 40) + 17, 17, -3], 2, 0, 1 << 18)
    assert not np.array_equal(big[0], big[1]) and np.all(np.abs(big) <= 1 << 18)
