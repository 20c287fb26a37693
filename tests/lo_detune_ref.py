"""numpy restatements and shared cases for the tests of the LO frequency offset (plx_lo_detune_dev, plx_dsp_run_freq_dev,
HotPathConfig(lo_detuning, lo_detuning_spread)): one case table and runner for the two back ends (host
emulator, shipped library), and the host side of the receiver chain the GPU tests compare with."""
import ctypes as C

import numpy as np

from polmux_amd import synth
from polmux_amd._abi import PLX_ERR_ARG, DspParams, PolmuxError
from tests.wdm_rx_ref import Dev, Host, cnormal  # noqa: F401  (the back ends are this module's as well)

SEED = 20260101
SENT = 7.0 + 7.0j            # what a sample the call may not touch holds before and after
KERNEL_CASES = [(256, 1, 3), (256, 64, 2), (4096, 5, 2)]
STRIDES = (1, 2, 16)


def theta_np(bins, nfft):
    """theta[f][c][n] = 2 pi (((b mod nfft) (n + 1)) mod nfft) / nfft for bins [F, nfc] -> [F, nfc, nfft]"""
    bm = np.asarray(bins, dtype=np.int64) % nfft                         # numpy's % is the floored one: [0, nfft)
    m = (bm[..., None] * np.arange(1, nfft + 1, dtype=np.int64)) % nfft    # below 2^40: exact in int64
    return 2 * np.pi * m / nfft


def edge_bins(nfft, count, rep):
    """`count` injected offsets, set `rep`: 0, +-1, +-(nfft/2 - 1), nfft/2 and values beyond +-nfft (reduced modulo nfft)"""
    pool = [0, 1, -1, nfft // 2 - 1, -(nfft // 2 - 1), nfft // 2, nfft + 3, -(2 * nfft + 5), 3 * nfft, 17, -(nfft - 1)]
    return np.array([pool[(rep * count + i) % len(pool)] for i in range(count)], dtype=np.int32), len(pool)


def detune(be, nfft, nfc, F, u=None, two=True, stride=1, pitch=None, sign=1.0, k0=0, K=0, keys=None, bins=None, phi=None,
           acc=0, bins_out=True, seed=SEED):
    """one plx_lo_detune_dev call -> dict(ux, uy, phi, bins) of what it left (host arrays; every buffer one channel-frame
    longer than the call may write).  u: (ux, uy) host [F nfc + 1, pitch]; phi: host [F nfc + 1, nfft]."""
    CF = F * nfc
    dux = be.up(u[0]) if u is not None else None
    duy = be.up(u[1]) if u is not None and two else None
    dphi = be.up(phi) if phi is not None else None
    dbo = be.up(np.full(CF + 1, -12345, np.int32)) if bins_out else None
    dbi = be.up(np.ascontiguousarray(bins, dtype=np.int32).reshape(-1)) if bins is not None else None
    dk = be.up(np.ascontiguousarray(keys, dtype=np.int64)) if keys is not None else None
    be.b.call("plx_lo_detune_dev", be.ptr(dux), be.ptr(duy), stride, pitch if pitch is not None else nfft // stride,
              float(sign), nfft, nfc, F, k0, K, seed, be.ptr(dk), be.ptr(dbi), be.ptr(dphi), acc, be.ptr(dbo), be.stream)
    return dict(ux=be.down(dux) if dux is not None else None, uy=be.down(duy) if duy is not None else None,
                phi=be.down(dphi) if dphi is not None else None, bins=be.down(dbo) if dbo is not None else None)


def _targets(rng, CF, nj, pitch):
    """(ux, uy) [CF + 1, pitch]: random where the call works, SENT in the pitch's tail and in the guard channel-frame"""
    out = []
    for _ in range(2):
        u = np.full((CF + 1, pitch), SENT)
        u[:CF, :nj] = cnormal(rng, (CF, nj))
        out.append(u)
    return out


def _check_apply(got, u0, th, stride, sign, CF, nj, what):
    want = u0[:CF, :nj] * np.exp(1j * sign * th[:, ::stride])
    d = np.abs(got[:CF, :nj] - want).max() / np.abs(u0[:CF, :nj]).max()
    assert d <= 1e-12, (what, d)
    assert np.all(got[:CF, nj:] == SENT) and np.all(got[CF] == SENT), what


def check_kernel(be, nfft, nfc, F, strides=STRIDES, seed=5):
    """plx_lo_detune_dev against theta_np on every route: injected bins (every edge value), the phasor at each stride and
    either sign on two polarisations and on one, d_phi written over NaN and accumulated onto a random buffer, d_bins_out
    exact; then the generated draws against synth.lo_detune_bins.  Returns the largest phasor and phase differences."""
    r = np.random.default_rng(seed + nfft + 3 * nfc)
    CF = F * nfc
    worst_u = worst_p = 0.0
    _, npool = edge_bins(nfft, CF, 0)
    seen = set()
    for rep in range(-(-npool // CF)):
        bins, _ = edge_bins(nfft, CF, rep)
        seen.update(bins.tolist())
        th = theta_np(bins, nfft)                                         # [CF, nfft]
        for k, stride in enumerate(strides):
            sign = 1.0 if (k + rep) % 2 == 0 else -1.0
            nj = nfft // stride
            pitch = nj + 3
            u0 = _targets(r, CF, nj, pitch)
            phi0 = np.full((CF + 1, nfft), np.nan)
            g = detune(be, nfft, nfc, F, u=u0, stride=stride, pitch=pitch, sign=sign, bins=bins.reshape(F, nfc), phi=phi0)
            for got, src in ((g["ux"], u0[0]), (g["uy"], u0[1])):
                _check_apply(got, src, th, stride, sign, CF, nj, (rep, stride, sign))
                worst_u = max(worst_u, np.abs(got[:CF, :nj] - src[:CF, :nj] * np.exp(1j * sign * th[:, ::stride])).max()
                              / np.abs(src[:CF, :nj]).max())
            assert np.isnan(g["phi"][CF]).all()
            dp = np.abs(g["phi"][:CF] - th).max()
            worst_p = max(worst_p, dp)
            assert dp <= 1e-12, (rep, stride, dp)
            assert np.array_equal(g["bins"][:CF], bins) and g["bins"][CF] == -12345
        # the other sign at the first stride, one polarisation, no d_phi (the tiles then cover the target samples alone)
        stride = strides[0]
        nj = nfft // stride
        u0 = _targets(r, CF, nj, nj)
        g = detune(be, nfft, nfc, F, u=u0, two=False, stride=stride, sign=-1.0 if rep % 2 == 0 else 1.0,
                   bins=bins.reshape(F, nfc), bins_out=False)
        _check_apply(g["ux"], u0[0], th, stride, -1.0 if rep % 2 == 0 else 1.0, CF, nj, "one polarisation")
        assert g["uy"] is None
        # accumulate onto a random buffer; nothing else asked for
        phi0 = np.full((CF + 1, nfft), np.nan)
        phi0[:CF] = r.uniform(-50, 50, (CF, nfft))
        g = detune(be, nfft, nfc, F, bins=bins.reshape(F, nfc), phi=phi0, acc=1, bins_out=False)
        assert np.isnan(g["phi"][CF]).all()
        assert np.abs(g["phi"][:CF] - (phi0[:CF] + th)).max() <= 1e-12      # (one rounding of a sum below 64: 4e-15)
    assert {0, 1, -1, nfft // 2 - 1, -(nfft // 2 - 1), nfft // 2, nfft + 3, -(2 * nfft + 5)} <= seen
    check_draws(be, nfft, nfc, F)
    return worst_u, worst_p


def check_draws(be, nfft, nfc, F):
    """the generated offsets against the host restatement, exactly: with keys (one of them beyond 32 bits, one negative),
    with NULL keys (the frame index), with K = 0, and through the phase they produce"""
    keys = [5, (1 << 40) + 17, -3, 77][:F]
    for k0, K in ((0, 3), (-7, nfft // 2 - 1), (11, 0), (2, 1)):
        want = synth.lo_detune_bins(SEED, keys, nfc, k0, K)
        assert want.shape == (F, nfc) and np.all(np.abs(want - k0) <= K)
        phi0 = np.full((F * nfc + 1, nfft), np.nan)
        g = detune(be, nfft, nfc, F, k0=k0, K=K, keys=keys, phi=phi0)
        assert np.array_equal(g["bins"][:F * nfc], want.reshape(-1)), (k0, K)
        assert np.abs(g["phi"][:F * nfc] - theta_np(want.reshape(-1), nfft)).max() <= 1e-12
        g = detune(be, nfft, nfc, F, k0=k0, K=K, keys=None)               # nothing but d_bins_out
        assert np.array_equal(g["bins"][:F * nfc], synth.lo_detune_bins(SEED, range(F), nfc, k0, K).reshape(-1))
    if nfc > 1:                                                            # the channel is a word of the counter
        assert len(set(synth.lo_detune_bins(SEED, keys[:1], nfc, 0, nfft // 2 - 1)[0].tolist())) > 1


def check_errors(be):
    """every PLX_ERR_ARG of plx_lo_detune_dev, and the largest arguments it accepts"""
    import pytest
    u = np.zeros((2, 256), complex)
    p8 = np.zeros(2 * 256 + 1)

    def call(nfft=256, nfc=1, F=1, ux=u, uy=None, stride=1, pitch=256, k0=0, K=0, bins=None, phi=None, bins_out=False):
        dux = be.up(ux) if ux is not None else None
        duy = be.up(uy) if uy is not None else None
        dbi = be.up(np.asarray(bins, np.int32)) if bins is not None else None
        dbo = be.up(np.zeros(64, np.int32)) if bins_out else None
        pp = phi
        if phi is not None and not isinstance(phi, C.c_void_p):
            keep = be.up(phi)
            pp = be.ptr(keep)
        be.b.call("plx_lo_detune_dev", be.ptr(dux), be.ptr(duy), stride, pitch, 1.0, nfft, nfc, F, k0, K, SEED, None,
                  be.ptr(dbi), pp, 0, be.ptr(dbo), be.stream)

    for kw, what in ((dict(nfft=128), "power of two"), (dict(nfft=384), "power of two"), (dict(nfft=1 << 21), "power of two"),
                     (dict(nfc=0), "nfc outside"), (dict(nfc=65), "nfc outside"), (dict(F=0), "no frames"),
                     (dict(ux=None), "nothing to write"), (dict(ux=None, uy=u, bins_out=True), "d_uy needs d_ux"),
                     (dict(stride=0), "stride must divide"), (dict(stride=3), "stride must divide"),
                     (dict(stride=2, pitch=127), "stride must divide"), (dict(pitch=255), "stride must divide"),
                     (dict(K=-1), "kspread"), (dict(K=128), "kspread"), (dict(k0=(1 << 30) + 1), "k0"),
                     (dict(k0=-(1 << 30) - 1), "k0")):
        with pytest.raises(PolmuxError, match=what) as ei:
            call(**kw)
        assert ei.value.code == PLX_ERR_ARG, kw
    if isinstance(be, Host):                     # a misaligned d_phi (a host pointer can be formed without touching it)
        base = be.ptr(be.up(p8)).value
        with pytest.raises(PolmuxError, match="16-byte aligned") as ei:
            call(ux=None, phi=C.c_void_p(base + 8 if base % 16 == 0 else base))
        assert ei.value.code == PLX_ERR_ARG
    call(K=127)                                  # 2 K + 1 = nfft - 1
    call(k0=1 << 30, ux=None, bins_out=True)
    call(K=999, bins=[4])                        # the injected route ignores k0 and kspread
    call(stride=256, pitch=1)


# ------------------------------------------------------ the frequency read-out ---
def dsp_params(**kw):
    p = DspParams()
    d = dict(workatbaudrate=0, applynlr=0, nlralpha=0.0, power_mw=2.0, applypol=0, polmethod=1, cma_mu=1 / 40, cma_taps=7,
             cma_txpolars=2, cma_phizero=0.0, easi_mu=1 / 40, easi_txpolars=2, easi_phizero=0.0, modorder=2, freqavg=500,
             phasavg=3, poworder=2)
    d.update(kw)
    for k, v in d.items():
        setattr(p, k, v)
    p.cma_R[0], p.cma_R[1] = 1.0, 1.0
    return p


def expected_turns(b, nsymb):
    """what the QPSK estimator makes of a carrier b bins off: -b inside its range nsymb / 8, aliased by nsymb / 4 just beyond"""
    b = np.asarray(b, dtype=np.int64)
    return np.where(np.abs(b) < nsymb // 8, -b, -(b - np.sign(b) * (nsymb // 4)))


def check_freq(be, Lin, freqavg=500):
    """plx_dsp_run_freq_dev on clean QPSK whose carrier turns b times over the frame: d_turns == -b for b = 0, +-1, 3,
    +-(nsymb/8 - 1) and the aliased value at nsymb/8 + 1; the second column carries -b.  The symbols are bit-identical to
    plx_dsp_run_dev's; the frame beyond nframes is left alone; freqavg = 0 stores zeros."""
    L = Lin // 2
    bins = np.array([0, 1, -1, 3, L // 8 - 1, -(L // 8 - 1), L // 8 + 1], dtype=np.int64)
    F, Fmax = len(bins), len(bins) + 1
    r = np.random.default_rng(Lin)
    m = np.arange(L)
    x = cnormal(r, (F, 2, Lin))                                           # (the odd samples are dropped by the plan)
    for f, b in enumerate(bins):
        for c, bc in enumerate((b, -b)):
            a = np.exp(1j * (np.pi / 4 + np.pi / 2 * r.integers(0, 4, L)))
            x[f, c, ::2] = a * np.exp(-2j * np.pi * bc * m / L + 0.3j * (f + 1)) * 4 * np.sqrt(2.0)
    want = np.stack([expected_turns(bins, L), expected_turns(-bins, L)], 1)
    out = {}
    for fa in (freqavg, 0):
        p = dsp_params(freqavg=fa)
        plan = C.c_void_p()
        be.b.call("plx_dsp_create", C.byref(plan), Lin, 2, Fmax, C.byref(p))
        try:
            din = be.up(x)
            d0, d1 = be.up(np.full((Fmax, 2, L), np.nan + 0j)), be.up(np.full((Fmax, 2, L), np.nan + 0j))
            dt = be.up(np.full((Fmax, 2), -99, np.int32))
            be.b.call("plx_dsp_run_dev", plan, be.ptr(din), be.ptr(d0), F, be.stream)
            be.b.call("plx_dsp_run_freq_dev", plan, be.ptr(din), be.ptr(d1), F, be.ptr(dt), be.stream)
            s0, s1, t = be.down(d0), be.down(d1), be.down(dt)
            d2 = be.up(np.full((Fmax, 2, L), np.nan + 0j))                # a NULL d_turns is plx_dsp_run_dev
            be.b.call("plx_dsp_run_freq_dev", plan, be.ptr(din), be.ptr(d2), F, None, be.stream)
            s2 = be.down(d2)
        finally:
            be.b.call("plx_dsp_destroy", plan)
        assert not np.isnan(s0[:F]).any() and np.isnan(s0[F]).all() and np.isnan(s1[F]).all()
        assert np.array_equal(s0[:F], s1[:F]) and np.array_equal(s0[:F], s2[:F])
        assert np.all(t[F] == -99)
        out[fa] = t[:F]
    assert np.array_equal(out[freqavg], want), (out[freqavg].tolist(), want.tolist())
    assert np.all(out[0] == 0)
    return out[freqavg]


# ------------------------------------------------- the receiver chain on the host ---
def lo_at_pick(bins, nfft, half):
    """exp(-i theta) at the 2-sps pick instants i half: [len(bins), 2 nsymb]"""
    return np.exp(-1j * theta_np(np.asarray(bins).reshape(-1), nfft)[:, ::half])


def host_chain(plxo, cfg, hp, ox, oy, b):
    """the oracle chain on one frame's field (ox, oy) with the LO b bins off, applied before the pick: the 2-sps pick,
    cde_ofde, dsp_pdm_coh_qpsk; returns (symbols [nsymb, 2], errors with the rotations and the swap resolved)"""
    from tests.test_gpu_configs import _rx_oracle
    lo = np.exp(-1j * theta_np([b], cfg.nfft)[0])
    ref, _ = _rx_oracle(plxo, cfg, hp, ox * lo, oy * lo)
    return ref, resolved_errors(plxo, ref, hp.bits)


def resolved_errors(plxo, sym, bits):
    """HotPath.errors_resolved on the host: per polarisation the minimum over the four pi/2 rotations, summed, then the
    minimum over the polarisation swap; sym [nsymb, 2], bits [nsymb, 4]"""
    best = []
    for tx in (bits, np.concatenate([bits[:, 2:], bits[:, :2]], 1)):
        tot = 0
        for p in range(2):
            tot += min(int((plxo.samp2pat_coherent(np.angle(sym[:, p:p + 1] * 1j ** k)) != tx[:, 2 * p:2 * p + 2]).sum())
                       for k in range(4))
        best.append(tot)
    return min(best)
