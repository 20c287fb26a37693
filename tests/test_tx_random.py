"""CPU tests (-m "not gpu") of the device transmitter (plx_tx_qpsk_dev): the host mirror of the bit
definition against a restatement with the Philox of tests/test_phase_noise.py, the drive tables against the host Tx chain,
the kernels of plx_tx.hip under the host emulator against the numpy chain random bits -> electricsource_qpsk ->
qi_modulator -> mean-power normalisation, and every refusal.  tests/test_gpu_tx_random.py imports the numpy chain from
here."""
import ctypes as C

import numpy as np
import pytest

from polmux_amd import _abi, patterns, synth
from tests.test_phase_noise import np_philox

SEED = 20260101
M32 = np.uint64(0xFFFFFFFF)


# ----------------------------------------------------------------- numpy restatements ---
def np_bits(nsymb, seed, key, chan):
    """include/polmux_hip.h, plx_tx_qpsk_dev 'Bits', symbol by symbol: [nsymb, 4]"""
    with np.errstate(over="ignore"):
        s, k = np.uint64(seed), np.uint64(key)
        k0 = (s ^ k) & M32
        k1 = ((s >> np.uint64(32)) ^ ((k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32))) & M32
    out = np.empty((nsymb, 4), np.uint8)
    for m in range(nsymb):
        q = m >> 5
        r = np_philox([q & 0xFFFFFFFF], [q >> 32], [chan], [4], k0, k1)
        for st in range(4):
            out[m, st] = (int(r[st][0]) >> (m & 31)) & 1
    return out


def np_chain(bits, nt, pavg):
    """(ux, uy, power) of the host Tx chain on bits [nsymb, 4]: synth.pdm_qpsk_field with these bits for the de Bruijn ones"""
    carrier = np.sqrt(pavg)
    sx = synth.qi_modulator(carrier, synth.electricsource_qpsk(bits[:, 0], nt), synth.electricsource_qpsk(bits[:, 1], nt))
    sy = synth.qi_modulator(carrier, synth.electricsource_qpsk(bits[:, 2], nt), synth.electricsource_qpsk(bits[:, 3], nt))
    avge = np.mean(np.abs(sx) ** 2 + np.abs(sy) ** 2)
    k = np.sqrt(pavg / avge)
    return sx * k, sy * k, pavg * pavg / avge


def np_dqpsk(bits):
    """[4, nsymb]: patterns.pat_decoder(pat, 'dqpsk') of the X and Y quaternary patterns of bits [nsymb, 4]"""
    rows = []
    for c in (0, 2):
        pm = patterns.pat_decoder(2 * bits[:, c].astype(int) + bits[:, c + 1].astype(int), "dqpsk")[1]
        rows += [pm[:, 0], pm[:, 1]]
    return np.stack(rows).astype(np.uint8)


def reference_batch(nsymb, nt, nfc, keys, pavg, seed=SEED):
    """ux, uy [F, nfc, nfft], pat, dq [F, nfc, 4, nsymb], power [F, nfc] of the numpy chain on the mirror's bits"""
    F = len(keys)
    ux = np.empty((F, nfc, nsymb * nt), complex)
    uy = np.empty_like(ux)
    pat = np.empty((F, nfc, 4, nsymb), np.uint8)
    dq = np.empty_like(pat)
    power = np.empty((F, nfc))
    for f, key in enumerate(keys):
        for c in range(nfc):
            b = synth.random_qpsk_bits(nsymb, seed, key, c)
            ux[f, c], uy[f, c], power[f, c] = np_chain(b, nt, pavg)
            pat[f, c], dq[f, c] = b.T, np_dqpsk(b)
    return ux, uy, pat, dq, power


def check_against_reference(got, ref):
    """the bars of the issue: field <= 1e-14 of max |u| (three roundings), power <= 1e-13 relative, patterns equal"""
    ux, uy, pat, dq, power = got
    rx, ry, rpat, rdq, rpower = ref
    scale = max(np.abs(rx).max(), np.abs(ry).max())
    ex, ey = np.abs(ux - rx).max() / scale, np.abs(uy - ry).max() / scale
    ep = np.abs(power / rpower - 1).max()
    print("field %.2e %.2e power %.2e" % (ex, ey, ep))
    assert ex <= 1e-14 and ey <= 1e-14
    assert ep <= 1e-13
    np.testing.assert_array_equal(pat, rpat)
    if dq is not None:
        np.testing.assert_array_equal(dq, rdq)


# ----------------------------------------------------------------- emulator helpers ---
@pytest.fixture(scope="module")
def emu():
    from tests import _emu
    return _emu.binding()


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def emu_tx(emu, nsymb, nt, nfc, F, pavg=2.0, keys=None, dq=True, seed=SEED, drive=None):
    n = nsymb * nt
    ux, uy = np.full((F, nfc, 2 * n), np.nan), np.full((F, nfc, 2 * n), np.nan)
    pat = np.full((F, nfc, 4, nsymb), 7, np.uint8)
    pdq = np.full((F, nfc, 4, nsymb), 7, np.uint8) if dq else None
    power = np.full((F, nfc), np.nan)
    drive = synth.qpsk_drive_tables(nt) if drive is None else drive
    kt = np.asarray(keys, np.int64) if keys is not None else None
    emu.call("plx_tx_qpsk_dev", _vp(ux), _vp(uy), nsymb, nt, nfc, F, _vp(drive), pavg, seed, _vp(kt), _vp(pat), _vp(pdq),
             _vp(power), None)
    return ux.view(np.complex128), uy.view(np.complex128), pat, pdq, power


# ----------------------------------------------------------------------------- tests ---
def test_abi_entry_point_declared():
    assert "plx_tx_qpsk_dev" in _abi.SIGNATURES and _abi.PLX_PHILOX_TX_DATA == 4


@pytest.mark.parametrize("nsymb,key,chan", [(16, 0, 0), (96, 7, 0), (64, (1 << 32) + 5, 2), (128, 123456789012345, 1)])
def test_host_mirror_matches_restatement(nsymb, key, chan):
    got = synth.random_qpsk_bits(nsymb, SEED, key, chan)
    assert got.shape == (nsymb, 4) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, np_bits(nsymb, SEED, key, chan))


def test_host_mirror_streams_differ():
    a = synth.random_qpsk_bits(256, SEED, 3, 0)
    assert 0.35 < a.mean() < 0.65
    for other in (synth.random_qpsk_bits(256, SEED, 4, 0), synth.random_qpsk_bits(256, SEED, 3, 1),
                  synth.random_qpsk_bits(256, SEED + 1, 3, 0), synth.random_qpsk_bits(256, SEED, 3 + (1 << 32), 0)):
        assert 0.3 < np.mean(a != other) < 0.7
    assert 0.3 < np.mean(a[:, 0] != a[:, 1]) < 0.7


@pytest.mark.parametrize("nsymb,nt", [(16, 16), (32, 8), (64, 4), (128, 2), (64, 64), (32, 32)])
def test_drive_tables_reproduce_the_host_chain_bit_for_bit(nsymb, nt):
    """a drive[t][j] sigma for both quadratures IS qi_modulator(electricsource_qpsk(...)) before the normalisation"""
    pavg = 2.0
    bits = synth.random_qpsk_bits(nsymb, SEED, 11, 0)
    drive = synth.qpsk_drive_tables(nt)
    assert drive.shape == (2, nt) and drive.dtype == np.float64
    a = np.sqrt(pavg) / np.sqrt(2.0)
    j = np.tile(np.arange(nt), nsymb)
    w = []
    for s in range(4):
        b = bits[:, s].astype(int)
        t = np.repeat(b ^ np.roll(b, -1), nt)
        w.append((a * drive[t, j]) * np.repeat(2.0 * b - 1.0, nt))
    carrier = np.sqrt(pavg)
    sx = synth.qi_modulator(carrier, synth.electricsource_qpsk(bits[:, 0], nt), synth.electricsource_qpsk(bits[:, 1], nt))
    sy = synth.qi_modulator(carrier, synth.electricsource_qpsk(bits[:, 2], nt), synth.electricsource_qpsk(bits[:, 3], nt))
    np.testing.assert_array_equal(w[0] + 1j * w[1], sx)
    np.testing.assert_array_equal(w[2] + 1j * w[3], sy)


# (nsymb, nt, nfc, frames): half a word; one word, the circular neighbour inside it; two words, channels, a wave's run wider
# than a symbol; the smallest pulse; the largest table
SHAPES = [(16, 16, 1, 1), (32, 8, 1, 2), (64, 4, 3, 2), (128, 2, 1, 1), (64, 64, 2, 1)]


@pytest.mark.parametrize("nsymb,nt,nfc,F", SHAPES)
def test_emu_transmitter_matches_numpy_chain(emu, nsymb, nt, nfc, F):
    pavg = 2.0 if nt != 4 else 0.5
    got = emu_tx(emu, nsymb, nt, nfc, F, pavg)
    check_against_reference(got, reference_batch(nsymb, nt, nfc, list(range(F)), pavg))
    # |sin| <= 1: the unnormalised mean power is at most 2 pavg (both polarisations at full drive), so P >= pavg / 2 (short
    # pulses have no raised-cosine edge at all and sit on that bound)
    assert np.all(got[4] >= 0.5 * pavg * (1 - 1e-13))


def test_emu_keys_null_pattern_and_batch_independence(emu):
    nsymb, nt, nfc = 64, 4, 2
    keys = [5, (1 << 33) + 9, 0, 5]
    got = emu_tx(emu, nsymb, nt, nfc, 4, keys=keys)
    check_against_reference(got, reference_batch(nsymb, nt, nfc, keys, 2.0))
    for a in got:
        np.testing.assert_array_equal(a[0], a[3])                     # the same key at another position: the same frame
    assert np.any(got[2][0] != got[2][1]) and np.any(got[2][0, 0] != got[2][0, 1])
    # a frame alone is itself in a batch, bit for bit; without d_pat_dq nothing else changes
    alone = emu_tx(emu, nsymb, nt, nfc, 1, keys=[keys[1]], dq=False)
    assert alone[3] is None
    for i in (0, 1, 2, 4):
        np.testing.assert_array_equal(alone[i][0], got[i][1])
    # keys NULL: the frame index
    idx = emu_tx(emu, nsymb, nt, nfc, 1)
    np.testing.assert_array_equal(idx[0][0], got[0][2])
    np.testing.assert_array_equal(idx[2][0], got[2][2])


def test_emu_refusals(emu):
    good = dict(nsymb=32, nt=8, nfc=1, F=1, pavg=2.0)
    emu_tx(emu, **good)
    bad = [dict(nsymb=8), dict(nsymb=48), dict(nsymb=1 << 20, nt=2), dict(nt=1, nsymb=256), dict(nt=12), dict(nt=128, nsymb=16),
           dict(nsymb=16, nt=8), dict(nsymb=1 << 19, nt=4), dict(nfc=0), dict(nfc=65), dict(F=0), dict(pavg=0.0),
           dict(pavg=-1.0), dict(pavg=float("inf")), dict(pavg=float("nan"))]
    n, z, zb, one = 256, np.zeros(2 * 256), np.zeros(4 * 32, np.uint8), np.zeros(1)
    for b in bad:
        a = dict(good)
        a.update(b)
        drive = np.ones((2, max(a["nt"], 1)))
        with pytest.raises(_abi.PolmuxError, match="plx_tx_qpsk_dev") as ei:     # (refused before anything is written)
            emu.call("plx_tx_qpsk_dev", _vp(z), _vp(z), a["nsymb"], a["nt"], a["nfc"], a["F"], _vp(drive), a["pavg"], SEED, None,
                     _vp(zb), None, _vp(one), None)
        assert ei.value.code == _abi.PLX_ERR_ARG, b
    drive = synth.qpsk_drive_tables(8)
    for bd in (np.where(np.arange(16).reshape(2, 8) == 3, np.nan, drive), np.where(np.arange(16).reshape(2, 8) == 12, np.inf, drive),
               np.stack([np.zeros(8), drive[1]])):
        with pytest.raises(_abi.PolmuxError, match="drive") as ei:
            emu.call("plx_tx_qpsk_dev", _vp(z), _vp(z), 32, 8, 1, 1, _vp(np.ascontiguousarray(bd)), 2.0, SEED, None, _vp(zb), None,
                     _vp(one), None)
        assert ei.value.code == _abi.PLX_ERR_ARG
    args = [_vp(z), _vp(z), 32, 8, 1, 1, _vp(drive), 2.0, SEED, None, _vp(zb), None, _vp(one), None]
    for null in (0, 1, 6, 10, 12):
        a = list(args)
        a[null] = None
        with pytest.raises(_abi.PolmuxError, match="null argument"):
            emu.call("plx_tx_qpsk_dev", *a)
    assert n == 32 * 8


def test_host_option_refusals():
    from polmux_amd.pipeline import HotPath, HotPathConfig, check_tx_options
    assert check_tx_options(HotPathConfig()) is False
    assert check_tx_options(HotPathConfig(tx_data="random")) is True
    assert check_tx_options(HotPathConfig(tx_data="random", nch=3, wdm_field="unique", nt=64)) is True
    bad = [dict(tx_data="prbs"), dict(tx_data=None), dict(tx_data="random", variants=2),
           dict(tx_data="random", nch=3, wdm_field="unique", mux_filter=dict(ftype="gauss", bw=1.2)),
           dict(tx_data="random", nsymb=16, nt=128)]
    for kw in bad:
        with pytest.raises(ValueError, match="tx_data"):
            check_tx_options(HotPathConfig(**kw))
        with pytest.raises(ValueError, match="tx_data"):             # ... and the plan refuses before it touches a device
            HotPath(HotPathConfig(**kw), 1)
