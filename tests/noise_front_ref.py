"""Cases and runners for the tests of the two stages between the fibre and the equaliser that a Monte-Carlo campaign's
bit-error rate rests on: the ASE / receiver-noise generator (plx_ampliflat_dev: k_ampliflat of plx_misc.hip, Philox-4x32-10
+ Box-Muller) against a numpy restatement of its draws, and the coherent front end (plx_front_run_dev, plx_front_run_lo_dev:
k_mix, k_absmax, k_decimate of plx_front.hip) at batch width against oracle/front.py frame by frame, and plx_pick_dev away
from offset 0.  The same cases run on two back ends, the host emulator (tests/test_emu_noise_front.py) and the shipped
library on device tensors (tests/test_gpu_noise_front.py); the checks are written once, here.

Every buffer a call writes reaches one frame past what the call may write and is NaN first: the guard frame must still
be NaN afterwards and nothing written may be NaN.  The front end's input fields have a NaN frame in FRONT of frame 0 as
well, so that a sample read from before a frame's start shows as a NaN.  Every frame, channel and polarisation has its own input."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.test_emu_kernels import _front_case, _front_desc
from tests.test_phase_noise import SEED, np_normals
from tests.wdm_rx_ref import Dev, Host, cnormal, nan, vp  # noqa: F401  (the back ends are shared with the receiver's cases)

DRAW_BAR = 1e-13                 # absolute per unit sigma: rad <= 8.7, a few ulp in log and sincos give a few 1e-15
SEED_HI = (0x2545F491 << 32) | SEED          # a seed whose high word is not zero
KEYS3 = [5, 2 ** 32 + 5, 2 ** 40 + 123]      # keys 2^32 apart: they differ in the high key word only
CUR_BAR, SAMP_BAR, FLIP_AT, FLIP_CAP = 1e-11, 1e-14, 1e-9, 2e-3     # the bars of test_front_end_vs_oracle


class Measured:
    """the figures the tests print (profiles/noise_front_tests.md is made from them): (back end, case, what) -> value"""
    rows = {}

    @classmethod
    def put(cls, be, case, what, value):
        name = type(be).__name__ if not isinstance(be, str) else be
        cls.rows[(name, case, what)] = max(value, cls.rows.get((name, case, what), 0.0))
        print("MEASURED %s %s %s %.3g" % (name, case, what, value))


# ------------------------------------------------------------------ the draws ---
def unit_np(n, nfc, keys, seed):
    """the unit complex normal draws [F, 2, nfc, n] of k_ampliflat: counter (k lo, k hi, channel, polarisation 0/1), key
    (seed, frame key); the cos branch is the real part, the sin branch the imaginary part"""
    out = np.empty((len(keys), 2, nfc, n), complex)
    for f, key in enumerate(keys):
        for pol in range(2):
            for c in range(nfc):
                cs, sn = np_normals(n, c, pol, seed, int(key))
                out[f, pol, c].real, out[f, pol, c].imag = cs, sn
    return out


def ase_np(n, nfc, keys, seed, sigma, asex=1, asey=1):
    """sigma[c] (cos branch + i sin branch) of plx_ampliflat_dev's generator, [F, 2, nfc, n]; zero where a polarisation is off"""
    sigma = np.broadcast_to(np.asarray(sigma, dtype=float), (nfc,))
    out = unit_np(n, nfc, keys, seed) * sigma[None, None, :, None]
    for pol, on in enumerate((asex, asey)):
        if not on:
            out[:, pol] = 0
    return out


def scaled(u, gain):
    """sqrt(gain) u as cscale forms it: each part times the real factor, bit for bit"""
    return (np.ascontiguousarray(u).view(np.float64) * math.sqrt(gain)).view(np.complex128)


def _all_nan(a):
    return bool(np.isnan(np.ascontiguousarray(a).view(np.float64)).all())


def call_ampliflat(be, ux, uy, gain, sigma, seed, keys, asex=1, asey=1, noise=None):
    """plx_ampliflat_dev in place on ux, uy [F, nfc, n] (uy None: d_uy null; sigma None: null; keys None: d_keys null; noise
    [F, 2 nfc, n]: the injected route) -> the host copies [F, nfc, n] (None for a null uy); the buffers hold a NaN frame F"""
    F, nfc, n = ux.shape
    bufs = []
    for u in (ux, uy):
        b = None
        if u is not None:
            b = nan((F + 1, nfc, n))
            b[:F] = u
            b = be.up(b)
        bufs.append(b)
    sg = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64)
    kt = None if keys is None else be.up(np.asarray(keys, dtype=np.int64))
    nz = None if noise is None else be.up(noise)
    be.b.call("plx_ampliflat_dev", be.ptr(bufs[0]), be.ptr(bufs[1]), n, nfc, F, float(gain), None if sg is None else vp(sg),
              be.ptr(nz), seed, be.ptr(kt), asex, asey, be.stream)
    outs = []
    for b in bufs:
        h = None
        if b is not None:
            h = be.down(b)
            assert _all_nan(h[F]) and not np.isnan(h[:F]).any()
            h = h[:F]
        outs.append(h)
    return outs


def check_draws(be, case, n, nfc, F, keys, seed, gain, sigma, dual=True, asex=1, asey=1):
    """one shape of plx_ampliflat_dev's generator against the restatement: (1) on a zero field the output IS sigma times the
    draw -- DRAW_BAR per unit sigma, and exactly zero where sigma or the polarisation is off; (2) on a field of its own per
    frame, channel and polarisation, field plus noise to 1e-13 (sigma + max|sqrt(gain) u|) (the last multiply-add may be
    contracted), and sqrt(gain) u bit for bit where sigma or the polarisation is off.  Returns the outputs of (2) and the field."""
    r = np.random.default_rng(n + 131 * nfc + F)
    sigma = np.asarray(sigma, dtype=float)
    unit = unit_np(n, nfc, range(F) if keys is None else keys, seed)
    on = [bool(asex), bool(asey)]
    zero = np.zeros((F, nfc, n), complex)
    got = call_ampliflat(be, zero, zero if dual else None, gain, sigma, seed, keys, asex, asey)
    worst = 0.0
    for pol in range(2 if dual else 1):
        for c in range(nfc):
            if sigma[c] == 0 or not on[pol]:
                assert not got[pol][:, c].any(), (case, pol, c)
            else:
                worst = max(worst, np.abs(got[pol][:, c] - sigma[c] * unit[:, pol, c]).max() / sigma[c])
    Measured.put(be, case, "draws, per unit sigma", worst)
    assert worst <= DRAW_BAR, (case, worst)
    u = [cnormal(r, (F, nfc, n)), cnormal(r, (F, nfc, n)) if dual else None]
    got = call_ampliflat(be, u[0], u[1], gain, sigma, seed, keys, asex, asey)
    worst = 0.0
    for pol in range(2 if dual else 1):
        su = scaled(u[pol], gain)
        for c in range(nfc):
            if sigma[c] == 0 or not on[pol]:
                assert np.array_equal(got[pol][:, c], su[:, c]), (case, pol, c)
            else:
                e = np.abs(got[pol][:, c] - (su[:, c] + sigma[c] * unit[:, pol, c])).max() / (sigma[c] + np.abs(su).max())
                worst = max(worst, e)
    Measured.put(be, case, "field plus noise, of sigma + max|field|", worst)
    assert worst <= DRAW_BAR, (case, worst)
    return got, u


def sigmas(nfc):
    """nfc distinct sigmas, one of them 0"""
    s = 0.2 + 0.05 * np.arange(nfc)
    s[nfc // 2] = 0.0
    return s


def check_a1_a2(be, nfc):
    """A1 (nfc = 33: the device sigma table) and A2 (32, 31: the by-value table's boundary): n = 1000 is no multiple of 256 and
    no power of two, the keys differ in their high word, the seed has a high word, one sigma is 0"""
    check_draws(be, "A1" if nfc > 32 else "A2 nfc=%d" % nfc, 1000, nfc, 3, KEYS3, SEED_HI, 2.25, sigmas(nfc))


def check_a3(be):
    """A3: n = 70000 > 65536 = 256 blocks of 256 threads: the second pass of the grid-stride loop; d_keys null: the frame
    index is the key"""
    check_draws(be, "A3", 70000, 2, 2, None, SEED, 2.25, [0.3, 0.5])


def check_a4(be):
    """A4: 65 frames under a shuffled range of keys, then three of them alone: a realisation's noise is bit-identical alone or
    anywhere in a batch, and frames with different keys differ"""
    n, nfc, F = 2048, 2, 65
    keys = (np.random.default_rng(65).permutation(F) + 1000).tolist()
    assert all(k != f for f, k in enumerate(keys))
    got, u = check_draws(be, "A4", n, nfc, F, keys, SEED, 2.25, [0.3, 0.5])
    for pol in range(2):
        assert len({got[pol][f, 0, :4].tobytes() for f in range(F)}) == F
    for f in (0, 31, 64):
        alone = call_ampliflat(be, u[0][f:f + 1], u[1][f:f + 1], 2.25, [0.3, 0.5], SEED, [keys[f]])
        for pol in range(2):
            assert np.array_equal(alone[pol][0], got[pol][f]), (f, pol)


def check_a5(be):
    """A5: 'asex' only, 'asey' only, d_uy null, sigma null, gain 0: the polarisation that is off equals sqrt(gain) u bit for bit"""
    n, nfc, F, keys, sig = 512, 2, 2, [11, 2 ** 32 + 11], [0.3, 0.5]
    check_draws(be, "A5 asex", n, nfc, F, keys, SEED, 2.25, sig, asex=1, asey=0)
    check_draws(be, "A5 asey", n, nfc, F, keys, SEED, 2.25, sig, asex=0, asey=1)
    check_draws(be, "A5 uy null", n, nfc, F, keys, SEED, 2.25, sig, dual=False)
    check_draws(be, "A5 gain 0", n, nfc, F, keys, SEED, 0.0, sig)
    r = np.random.default_rng(5)
    ux, uy = cnormal(r, (F, nfc, n)), cnormal(r, (F, nfc, n))
    gx, gy = call_ampliflat(be, ux, uy, 2.25, None, SEED, keys)
    assert np.array_equal(gx, scaled(ux, 2.25)) and np.array_equal(gy, scaled(uy, 2.25))


def check_a6(be):
    """A6: the injected route, d_noise [frame][X cols | Y cols][nfft] with its own values per frame, polarisation and column"""
    n, nfc, F, gain = 512, 3, 3, 2.25
    r = np.random.default_rng(6)
    ux, uy, noise = cnormal(r, (F, nfc, n)), cnormal(r, (F, nfc, n)), cnormal(r, (F, 2 * nfc, n))
    sig = np.array([0.3, 0.5, 0.7])
    got = call_ampliflat(be, ux, uy, gain, sig, 0, None, noise=noise)
    worst = 0.0
    for pol, u in enumerate((ux, uy)):
        su = scaled(u, gain)
        want = su + sig[None, :, None] * noise[:, pol * nfc:(pol + 1) * nfc]
        worst = max(worst, (np.abs(got[pol] - want).max(-1).max(0) / (sig + np.abs(su).max())).max())
    Measured.put(be, "A6", "field plus noise, of sigma + max|field|", worst)
    assert worst <= DRAW_BAR


def check_a7(be):
    """A7: the call HotPath._rx_noise makes: rx [F, nch, 2 Lrx] as one 'polarisation' of nch columns, d_uy null, unit gain,
    asey = 0, keyed per frame"""
    check_draws(be, "A7", 2 * 512, 3, 4, [7, 2 ** 33 + 7, 0, 2 ** 40], 5, 1.0, np.full(3, 0.35), dual=False, asex=1, asey=0)


def distribution():
    """The statistics of the restatement's streams, each in units of its standard error at N = 2^17: both quadratures of the
    streams (channel, pol, key) below at SEED -> dict(mean, variance, skewness, kurtosis, lag1, cross) of worst |value| / s.e."""
    N = 1 << 17
    seqs = []
    for c, pol, key in ((0, 0, 11), (0, 1, 11), (1, 0, 11), (0, 0, 12), (0, 0, 2 ** 32 + 11)):
        seqs += list(np_normals(N, c, pol, SEED, key))
    x = np.stack(seqs)
    m, v = x.mean(1), x.var(1)
    z = (x - m[:, None]) / np.sqrt(v)[:, None]
    cc = np.corrcoef(x)
    return dict(mean=np.abs(m).max() * math.sqrt(N), variance=np.abs(v - 1).max() / math.sqrt(2 / N),
                skewness=np.abs((z ** 3).mean(1)).max() / math.sqrt(6 / N),
                kurtosis=np.abs((z ** 4).mean(1) - 3).max() / math.sqrt(24 / N),
                lag1=np.abs((z[:, :-1] * z[:, 1:]).mean(1)).max() * math.sqrt(N),
                cross=np.abs(cc[np.triu_indices(len(seqs), 1)]).max() * math.sqrt(N))


# ------------------------------------------------------------ the front end ---
def _off(be, h, nbytes):
    p = be.ptr(h)
    return C.c_void_p((p.value if isinstance(p, C.c_void_p) else p) + nbytes)


class FrontPlan:
    """a plx_front plan made from _front_desc(...) and run on host frames through either back end"""

    def __init__(self, be, n, dual, frames, hopt, hel, elo, balanced, bits, r, fir):
        self.be, self.n, self.dual, self.frames = be, n, dual, frames
        self.oracle = dict(hopt=hopt, hel=hel, elo=elo, balanced=balanced, bits=bits, r=r, fir=fir)
        self.desc = _front_desc(n, dual, frames, hopt, hel, elo, balanced, bits, r, fir)
        self.plan = C.c_void_p()
        be.b.call("plx_front_create", C.byref(self.plan), C.byref(self.desc))
        self.nout = be.b.lib.plx_front_out_len(self.plan)
        assert self.nout == -(-n // r)

    def close(self):
        self.be.b.call("plx_front_destroy", self.plan)

    def run(self, fx, fy, shifts, lophase=None):
        """fx, fy [F, n] -> (photocurrents x, y [F, n] complex I + jQ, samples [F, npol, nout]).  The fields sit between two
        NaN frames, the samples have a NaN frame behind them: the guards must stay NaN, nothing written may be NaN"""
        be, n, F, npol = self.be, self.n, fx.shape[0], self.dual + 1
        bufs = []
        for u in (fx, fy)[:npol]:
            b = nan((F + 2, n))
            b[1:F + 1] = u
            bufs.append(be.up(b))
        out = be.up(nan((F + 1, npol, self.nout)))
        sh = (C.c_int64 * 2)(*shifts)
        px, py = _off(be, bufs[0], 16 * n), _off(be, bufs[1], 16 * n) if self.dual else None
        if lophase is None:
            be.b.call("plx_front_run_dev", self.plan, px, py, F, sh, be.ptr(out), be.stream)
        else:
            lo = be.up(np.ascontiguousarray(lophase, dtype=np.float64))
            be.b.call("plx_front_run_lo_dev", self.plan, px, py, F, sh, be.ptr(lo), be.ptr(out), be.stream)
        o = be.down(out)
        assert _all_nan(o[F]) and not np.isnan(o[:F]).any()
        cur = []
        for b in bufs:
            h = be.down(b)
            assert _all_nan(h[0]) and _all_nan(h[F + 1]) and not np.isnan(h[1:F + 1]).any()
            cur.append(h[1:F + 1])
        return cur[0], (cur[1] if self.dual else None), o[:F]

    def check(self, case, fx, fy, shifts, lophase=None, skip=(), full=True, bits=None):
        """run, then every frame against oracle/front.py with the bars of test_front_end_vs_oracle: photocurrents within
        CUR_BAR of their maximum, samples within SAMP_BAR of the oracle continued from the device's own currents, and against
        the all-oracle chain a share of samples off by more than FLIP_AT below FLIP_CAP (taken over the case's frames; full =
        False: not compared).  skip: frames the oracle cannot state (an all-zero frame: its ADC divides 0 by 0)."""
        from oracle import front
        o, be, dual = self.oracle, self.be, bool(self.dual)
        cx, cy, out = self.run(fx, fy, shifts, lophase)
        sh = [shifts[0], shifts[1] if dual else shifts[0]]
        wc = ws = 0.0
        flips = total = 0
        for f in range(fx.shape[0]):
            if f in skip:
                continue
            elo = o["elo"] if lophase is None else o["elo"] * np.exp(1j * lophase[f])
            want = front.receiver_cohmix(fx[f], fy[f] if dual else None, o["hopt"], elo, o["hel"], bool(o["balanced"]))
            got = np.stack([cx[f].real, cx[f].imag] + ([cy[f].real, cy[f].imag] if dual else []), 1)
            ec = np.abs(got - want).max() / np.abs(want).max()
            rx = front.rx_front(got, dual, o["bits"], sh, o["r"], o["fir"])
            es = np.abs(out[f].T - rx).max() / np.abs(rx).max()
            wc, ws = max(wc, ec), max(ws, es)
            assert ec < CUR_BAR, (case, f, ec)
            assert es <= SAMP_BAR, (case, f, es)
            if full:
                fl = front.rx_front(want, dual, o["bits"], sh, o["r"], o["fir"])
                flips += int(np.sum(np.abs(out[f].T - fl) > FLIP_AT * np.abs(fl).max()))
                total += fl.size
        Measured.put(be, case, "photocurrents, of max", wc)
        Measured.put(be, case, "samples vs oracle from device currents, of max", ws)
        if full:
            Measured.put(be, case, "share of samples off the all-oracle chain by > 1e-9", flips / total)
            print("MEASURED %s %s flips %d of %d" % (type(be).__name__, case, flips, total))
            assert flips / total < FLIP_CAP, (case, flips, total)
        return cx, cy, out


def front_frames(n, amps, seed):
    """len(amps) frames of both polarisations, each with its own content: amps[f] (the base waveform rolled and turned by
    its own amount + its own noise); -> (fx, fy [F, n], hopt, hel, elo table)"""
    assert n % 16 == 0
    _, ux, uy, hopt, hel, elo = _front_case(n // 16, 16)
    r = np.random.default_rng(seed)
    amps = np.asarray(amps, dtype=float)
    F = len(amps)
    fx = np.stack([amps[f] * (np.roll(ux, 5 * f + 1) * np.exp(0.3j * f) + 0.1 * cnormal(r, n)) for f in range(F)])
    fy = np.stack([amps[f] * (np.roll(uy, -3 * f - 2) * np.exp(-0.2j * f) + 0.1 * cnormal(r, n)) for f in range(F)])
    return fx, fy, hopt, hel, elo


B1_ZERO = 17
# a real scalar LO: the four diode squares of a zero field are then the same number whatever the compiler contracts, so
# that an all-zero frame gives exactly zero balanced currents (with a complex LO they are x x + y y and y y + x x)
B1_LO = 1.25


def b1_frames():
    from polmux_amd import rxfront
    amps = 10 ** np.linspace(-1.5, 1.5, 65)
    amps[B1_ZERO] = 0.0
    fx, fy, hopt, hel, _ = front_frames(256, amps, 1)
    assert not fx[B1_ZERO].any() and not fy[B1_ZERO].any()
    return fx, fy, hopt, hel, rxfront.fir1_lowpass(16, 1.0 / 8)


def check_b1_b2(be):
    """B1: 65 frames on a 66-frame plan, n = 256, dual, balanced, 5 bits, r = 8, 17-tap fir1_lowpass, shifts (-13, 21), an
    amplitude ladder of 10^(-1.5 .. 1.5) -- every frame's ADC full scale (d_max[frame]) differs from the others' by many
    quantisation steps -- and one all-zero frame, whose output is exactly zero through k_decimate's M > 0 guard.
    B2: the same plan straight afterwards on 3 frames of small amplitudes: no maximum survives from the larger batch."""
    fx, fy, hopt, hel, fir = b1_frames()
    p = FrontPlan(be, 256, 1, 66, hopt, hel, B1_LO, 1, 5, 8, fir)
    try:
        cx, cy, out = p.check("B1", fx, fy, (-13, 21), skip=(B1_ZERO,))
        assert not out[B1_ZERO].any() and not cx[B1_ZERO].any() and not cy[B1_ZERO].any()
        top = np.array([max(np.abs(cx[f].view(float)).max(), np.abs(cy[f].view(float)).max()) for f in range(65)])
        assert top.max() > 500 * top[top > 0].min()                    # the full scales really differ
        gx, gy = front_frames(256, [1e-3, 3e-3, 2e-3], 2)[:2]
        p.check("B2", gx, gy, (-13, 21))
    finally:
        p.close()


def check_b3(be):
    """B3: n = 4096, one polarisation (d_uy null), normal photodiodes, no ADC, r = 1 (the one-tap path), an LO table with
    detuning and 1.5 dB, 5 frames"""
    fx, fy, hopt, hel, elo = front_frames(4096, [1.0, 0.5, 2.0, 1.5, 0.8], 3)
    p = FrontPlan(be, 4096, 0, 5, hopt, hel, elo, 0, 0, 1, None)
    try:
        p.check("B3", fx, None, (-13, 0))
    finally:
        p.close()


B4_FIRS = [(3, 17), (2, 1), (8, 63), (16, 17)]


def check_b4(be, r, ntaps):
    """B4: random ASYMMETRIC taps (a reversed tap order shows), nout = ceil(n / r) with r = 3 not dividing n, the 63-tap
    maximum (the odd reflection covers 31 samples at both ends), one tap with r > 1, shifts with |shift| >= n and n - 1"""
    n = 256
    fx, fy, hopt, hel, elo = front_frames(n, [1.0, 0.6, 1.7, 1.2], 4)
    fir = np.random.default_rng(ntaps + r).standard_normal(ntaps)
    fir /= np.abs(fir).sum()
    assert ntaps == 1 or np.abs(fir - fir[::-1]).max() > 0.1 * np.abs(fir).max()
    p = FrontPlan(be, n, 1, 4, hopt, hel, elo, 1, 5, r, fir)
    try:
        for shifts in ((n + 5, -(2 * n + 3)), (0, n - 1)):
            p.check("B4 r=%d ntaps=%d" % (r, ntaps), fx, fy, shifts)
    finally:
        p.close()


def check_b5(be):
    """B5: d_lophase [F][n], its own random walk per frame, on 65 frames: k_mix's frame offset; the oracle is given
    elo exp(i phi_f)"""
    from polmux_amd import rxfront
    F, n = 65, 256
    fx, fy, hopt, hel, elo = front_frames(n, 1.0 + 0.01 * np.arange(F), 5)
    r = np.random.default_rng(55)
    phi = np.cumsum(0.05 * r.standard_normal((F, n)), 1) + r.uniform(-3, 3, (F, 1))
    p = FrontPlan(be, n, 1, F, hopt, hel, elo, 1, 5, 8, rxfront.fir1_lowpass(16, 1.0 / 8))
    try:
        p.check("B5", fx, fy, (-13, 21), lophase=phi)
    finally:
        p.close()


def check_b6(be, bits):
    """B6: four of B1's frames at adcbits 1 and 30, the ends of the level count 1u << bits; compared only with the oracle
    continued from the device's own currents (at 30 bits a step of the all-oracle chain is below FLIP_AT)"""
    fx, fy, hopt, hel, fir = b1_frames()
    sel = [0, 21, 43, 64]
    p = FrontPlan(be, 256, 1, 4, hopt, hel, B1_LO, 1, bits, 8, fir)
    try:
        p.check("B6 bits=%d" % bits, fx[sel], fy[sel], (-13, 21), full=False)
    finally:
        p.close()


# ------------------------------------------------------------------- the pick ---
def check_pick_dev(be):
    """C: plx_pick_dev away from offset 0: out[s][i] = scale in[s][offset + i stride], bit-exact against numpy's gather, the
    pitch padding and the row behind the last stay NaN, selections out of range by one refuse with PLX_ERR_ARG"""
    from polmux_amd._abi import PLX_ERR_ARG, PolmuxError
    n_in, nsig, scale = 1000, 130, 1.0 / 3.0
    x = cnormal(np.random.default_rng(8), (nsig, n_in))
    dx = be.up(x)

    def pick(offset, stride, n_out, pitch, out=None):
        p = pitch or n_out
        dout = be.up(nan((nsig + 1, p))) if out is None else out
        be.b.call("plx_pick_dev", be.ptr(dx), be.ptr(dout), n_in, n_out, offset, stride, scale, nsig, pitch, be.stream)
        return be.down(dout)

    for offset, stride, n_out, pitch in ((0, 1, 1000, 0), (7, 3, 331, 400), (999, 1, 1, 5)):
        got = pick(offset, stride, n_out, pitch)
        want = (np.ascontiguousarray(x[:, offset + np.arange(n_out) * stride]).view(np.float64) * scale).view(np.complex128)
        assert np.array_equal(got[:nsig, :n_out], want), (offset, stride)
        assert _all_nan(got[:nsig, n_out:]) and _all_nan(got[nsig])
    spare = be.up(nan((nsig + 1, 1001)))
    for offset, stride, n_out, pitch in ((0, 1, 1001, 0), (1, 1, 1000, 0), (7, 3, 332, 400), (10, 3, 331, 400), (1000, 1, 1, 5),
                                         (-1, 1, 1, 5), (7, 3, 331, 330)):
        with pytest.raises(PolmuxError) as ei:
            pick(offset, stride, n_out, pitch, out=spare)
        assert ei.value.code == PLX_ERR_ARG, (offset, stride, n_out, pitch)
    assert _all_nan(be.down(spare))
    pick(9, 3, 331, 400, out=spare)                # the last selections in range are accepted
    pick(0, 1, 1000, 1001, out=spare)
