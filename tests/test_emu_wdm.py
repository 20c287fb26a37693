"""The two kernels of the one-field WDM route (plx_wdm_mux_dev, plx_wdm_select_dev) under the host
emulator: against create_field('unique') restated in numpy, their bit-exact properties, and the linear known answer that pins
the sign of the phasor and of the walk-off delay."""
import numpy as np
import pytest

from polmux_amd._abi import PLX_ERR_ARG, PolmuxError
from tests import wdm_ref
from tests.wdm_ref import call_mux, call_select, cnormal


@pytest.fixture(scope="module")
def emu():
    from tests import _emu
    return _emu.binding()


@pytest.mark.parametrize("N,nch", [(256, 1), (256, 3), (4096, 5), (1024, 16)])
def test_emu_mux_against_create_field(emu, N, nch):
    """mux against ifft(sum_c roll(fft(s_c), -s_c)): 3 frames of complex normal samples, X and Y, shifts of both signs that
    include +-(N/2 - 1); once more with d_sy = NULL.  Bar: 1e-12 of max |u| (one operator on the emulator).
    Observed: 3.7e-16 / 3.3e-16 / 5.0e-16 / 4.8e-16 at (256, 1) / (256, 3) / (4096, 5) / (1024, 16)."""
    r = np.random.default_rng(100 + nch)
    shift = wdm_ref.edge_shifts(N, nch)
    assert shift.min() == -(N // 2 - 1) and (nch == 1 or shift.max() == N // 2 - 1)
    sx, sy = cnormal(r, (3, nch, N)), cnormal(r, (3, nch, N))
    ux, uy = call_mux(emu, sx, sy, shift)
    ex, ey = wdm_ref.mux_fft(sx, shift), wdm_ref.mux_fft(sy, shift)
    dx, dy = np.abs(ux - ex).max() / np.abs(ex).max(), np.abs(uy - ey).max() / np.abs(ey).max()
    print("mux (%d, %d): %.3g %.3g of max |u|" % (N, nch, dx, dy))
    assert dx <= 1e-12 and dy <= 1e-12
    ox, none = call_mux(emu, sx, None, shift)
    assert none is None and np.array_equal(ox, ux)


def test_emu_copy_and_round_trip(emu):
    """shift 0, one channel: mux and select are bit-identical copies.  select(mux(s)) of one channel at shift k, delay 0:
    1e-14 of max |s| (two correctly reduced phasors and two complex products).  Observed: at most 2.4e-16."""
    r = np.random.default_rng(7)
    N = 1024
    sx, sy = cnormal(r, (2, 1, N)), cnormal(r, (2, 1, N))
    ux, uy = call_mux(emu, sx, sy, [0])
    assert np.array_equal(ux, sx[:, 0]) and np.array_equal(uy, sy[:, 0])
    rx, ry = call_select(emu, ux, uy, [0])
    assert np.array_equal(rx, sx) and np.array_equal(ry, sy)
    rx, ry = call_select(emu, ux, uy, [0], [0])
    assert np.array_equal(rx, sx) and np.array_equal(ry, sy)
    for k in (1, -1, 37, -300, N // 2 - 1, -(N // 2 - 1)):
        ux, uy = call_mux(emu, sx, sy, [k])
        assert not np.array_equal(ux, sx[:, 0])
        rx, ry = call_select(emu, ux, uy, [k], [0])
        d = max(np.abs(rx - sx).max() / np.abs(sx).max(), np.abs(ry - sy).max() / np.abs(sy).max())
        print("round trip at shift %d: %.3g" % (k, d))
        assert d <= 1e-14


def test_emu_select_delay_is_a_roll(emu):
    """select with delay d equals np.roll(select with delay 0, -d) bit for bit, d of both signs: the phasor is taken at the
    source index."""
    r = np.random.default_rng(8)
    N, shift = 512, [-200, -3, 0, 77]
    ux, uy = cnormal(r, (2, N)), cnormal(r, (2, N))
    r0x, r0y = call_select(emu, ux, uy, shift, None)
    against = wdm_ref.select_np(ux, shift)
    assert np.abs(r0x - against).max() <= 1e-12 * np.abs(against).max()
    for delay in ([1, -1, 100, -100], [N - 1, -(N - 1), 0, 255], [-17, 17, -256, 3]):
        rx, ry = call_select(emu, ux, uy, shift, delay)
        for c, d in enumerate(delay):
            assert np.array_equal(rx[:, c], np.roll(r0x[:, c], -d, axis=-1)), (c, d)
            assert np.array_equal(ry[:, c], np.roll(r0y[:, c], -d, axis=-1)), (c, d)


def test_emu_frame_alone_equals_frame_in_batch(emu):
    r = np.random.default_rng(9)
    N, nch = 512, 6                               # six channels: the unrolled body of four and the tail of mux's loop
    shift, delay = wdm_ref.edge_shifts(N, nch), [5, -5, 0, 200, -511, 1]
    sx, sy = cnormal(r, (3, nch, N)), cnormal(r, (3, nch, N))
    ux, uy = call_mux(emu, sx, sy, shift)
    rx, ry = call_select(emu, ux, uy, shift, delay)
    for f in range(3):
        ax, ay = call_mux(emu, sx[f:f + 1], sy[f:f + 1], shift)
        assert np.array_equal(ax[0], ux[f]) and np.array_equal(ay[0], uy[f])
        bx, by = call_select(emu, ux[f:f + 1], uy[f:f + 1], shift, delay)
        assert np.array_equal(bx[0], rx[f]) and np.array_equal(by[0], ry[f])


@pytest.mark.parametrize("slope", [0.0, 0.06])
def test_emu_linear_known_answer(emu, slope):
    """Three channels 0.4 nm apart at 28 Gbaud (NSYMB 256, NT 16), band-limited with myfilter('ideal', FN, 0.45 spacing),
    mux, one linear step ifft(fft(u) exp(-i betat L)) over 80 km of D = 17 in numpy with the one-column betat of
    fiber_tables, select with the delays of pipeline.wdm_walkoff, and the same ideal filter on each selected channel (its
    neighbours are still beside it).  After taking out, in numpy, the channel's own dispersion and the sub-sample
    remainder of the walk-off, every channel equals its band-limited Tx waveform up to one constant phase (bar: 1e-11
    relative L2, an emulator propagation), and its cross-correlation with it peaks at lag 0.
    Observed: shifts -456 / 0 / 456 bins, delays -243 / 0 / 244 samples (-15.22 / 0 / 15.22 symbols; with slope 0.06
    -15.21 / 0 / 15.23); at worst 1.3e-14 on the outer channels and 8.0e-16 on the centre one, at either slope."""
    from polmux_amd import synth
    from polmux_amd.rxfront import myfilter
    cb = wdm_ref.comb(slope=slope)
    shift, delay = cb["shift"], cb["delay"]
    assert list(shift) == [-456, 0, 456]
    assert delay[0] < 0 < delay[2] and delay[1] == 0 and abs(abs(delay[0]) - 243) <= 2
    assert np.all(np.abs(cb["ds"] * cb["nt"] - delay) <= 0.5)
    h = myfilter("ideal", cb["fn"], 0.45 * cb["spacing"])
    tx = []
    for c in range(3):
        vx, vy, _, _ = synth.pdm_qpsk_field(256, 16, 2.0, 2 + 2 * c, 3 + 2 * c)
        tx.append((np.fft.ifft(np.fft.fft(vx) * h), np.fft.ifft(np.fft.fft(vy) * h)))
    sx = np.stack([t[0] for t in tx])[None]
    sy = np.stack([t[1] for t in tx])[None]
    ux, uy = call_mux(emu, sx, sy, shift)
    lin = np.exp(-1j * cb["t"]["betat"][:, 0] * cb["length"])
    ux, uy = np.fft.ifft(np.fft.fft(ux) * lin), np.fft.ifft(np.fft.fft(uy) * lin)
    rx, ry = call_select(emu, ux, uy, shift, delay)
    worst = 0.0
    for c in range(3):
        for got, ref in ((rx[0, c], sx[0, c]), (ry[0, c], sy[0, c])):
            got = np.fft.ifft(np.fft.fft(got) * h)      # the channel alone: its neighbours are still beside it after select
            e = wdm_ref.rel_l2_upto_phase(wdm_ref.undo_channel(got, cb, c), ref)
            lag = wdm_ref.xcorr_lag(wdm_ref.undo_channel(got, cb, c, remainder=False), ref)
            print("slope %g channel %d: %.3g relative L2, correlation peak at lag %d" % (slope, c, e, lag))
            worst = max(worst, e)
            assert lag == 0
            assert e <= 1e-11
    # without the compensation the neighbours are +-15 symbols away: the delay is doing the work
    r0x, _ = call_select(emu, ux, uy, shift, None)
    r0 = np.fft.ifft(np.fft.fft(r0x[0, 0]) * h)
    assert abs(wdm_ref.xcorr_lag(wdm_ref.undo_channel(r0, cb, 0, remainder=False), sx[0, 0]) - delay[0]) <= 1


def test_emu_argument_errors(emu):
    z = np.zeros(2 * 4 * 1024)
    o = np.zeros(2 * 4 * 1024)
    one = np.zeros(1, np.int64)

    def mux(nfft, nch, shift, sy=True):
        sh = np.asarray(shift, dtype=np.int64)
        emu.call("plx_wdm_mux_dev", wdm_ref.vp(z), wdm_ref.vp(z) if sy else None, wdm_ref.vp(o), wdm_ref.vp(o), nfft, nch, 1,
                 wdm_ref.vp(sh), None)

    def select(nfft, nch, shift, delay=None):
        sh = np.asarray(shift, dtype=np.int64)
        dl = np.asarray(delay, dtype=np.int64) if delay is not None else None
        emu.call("plx_wdm_select_dev", wdm_ref.vp(z), wdm_ref.vp(z), wdm_ref.vp(o), wdm_ref.vp(o), nfft, nch, 1, wdm_ref.vp(sh),
                 wdm_ref.vp(dl) if dl is not None else None, None)

    for call in (mux, select):
        for args, what in (((384, 1, [0]), "power of two"), ((128, 1, [0]), "power of two"), ((1 << 21, 1, [0]), "power of two"),
                           ((256, 0, one), "nch"), ((256, 65, [0] * 65), "nch"),
                           ((256, 1, [128]), "shift"), ((256, 1, [-128]), "shift"), ((256, 2, [0, 200]), "shift")):
            with pytest.raises(PolmuxError, match=what) as ei:
                call(*args)
            assert ei.value.code == PLX_ERR_ARG
    for d in (256, -256):
        with pytest.raises(PolmuxError, match="delay") as ei:
            select(256, 1, [0], [d])
        assert ei.value.code == PLX_ERR_ARG
    with pytest.raises(PolmuxError, match="both or neither") as ei:
        mux(256, 1, [0], sy=False)
    assert ei.value.code == PLX_ERR_ARG
    mux(256, 1, [127])                          # the largest offset is accepted
    select(256, 1, [-127], [255])


def test_emu_receiver_noise_call_is_keyed_per_realisation(emu):
    """The call HotPath.receive makes for noise_sigma with noise_keys on nch channel-frames per frame: plx_ampliflat_dev on
    rx viewed as [frames][nch][2 Lrx], one key per frame.  A realisation's noise is the same wherever its frame stands in
    a batch, and its channel-frames draw different streams."""
    L, nch = 512, 3

    def run(keys):
        F = len(keys)
        z, k, sig = np.zeros(F * nch * 2 * L * 2), np.asarray(keys, np.int64), np.full(nch, 0.35)
        emu.call("plx_ampliflat_dev", wdm_ref.vp(z), None, 2 * L, nch, F, 1.0, wdm_ref.vp(sig), None, 20260101, wdm_ref.vp(k), 1, 0, None)
        return z.view(np.complex128).reshape(F, nch, 2 * L)
    a, b = run([0, 1, 2, 3]), run([2, 0])
    assert np.array_equal(b[0], a[2]) and np.array_equal(b[1], a[0])
    assert not np.array_equal(a[0, 0], a[0, 1]) and not np.array_equal(a[0], a[1])
    assert abs(a.real.std() - 0.35) < 0.01 and abs(a.imag.std() - 0.35) < 0.01
