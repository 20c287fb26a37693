"""CPU tests (-m "not gpu") of laser phase noise and differential decoding: a numpy restatement of the device phase
generator (Philox-4x32-10 + Box-Muller, cumsum, Brownian bridge; include/polmux_hip.h, plx_phase_noise_dev), the kernels
of plx_phase.hip and k_decide_dqpsk under the host emulator against it and against the host composition samp2pat ->
pat_decoder -> ex20 swap, and lasersource's options against lasersource.m restated.  tests/test_gpu_phase_noise.py
imports the numpy operators from here."""
import ctypes as C
import math

import numpy as np
import pytest

from polmux_amd import _abi, patterns
from polmux_amd.rx import samp2pat

M32 = np.uint64(0xFFFFFFFF)
SEED = 20260101


# ----------------------------------------------------------------- numpy restatements ---
def np_philox(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on uint64 arrays holding 32-bit words (plx_philox.h)"""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def np_normals(n, chan, tag, seed, key):
    """the Box-Muller pair (cos, sin branch) of sample k < n, channel chan, counter word 3 = tag, key (seed, key)"""
    with np.errstate(over="ignore"):
        seed, key = np.uint64(seed), np.uint64(key)
        k0 = (seed ^ key) & M32
        k1 = ((seed >> np.uint64(32)) ^ ((key * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32))) & M32
    k = np.arange(n, dtype=np.uint64)
    r = np_philox(k & M32, k >> np.uint64(32), np.full(n, chan, np.uint64), np.full(n, tag, np.uint64), k0, k1)
    u1 = (((r[0] << np.uint64(21)) ^ (r[1] >> np.uint64(11))).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    u2 = (((r[2] << np.uint64(21)) ^ (r[3] >> np.uint64(11))).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)


def np_phase(nfft, nfc, keys, sigma, tag, seed=SEED):
    """phi_b [F, nfc, nfft] of plx_phase_noise_dev's generator: inc[0] = 0, inc[k] = sigma n[k], cumsum, bridge"""
    sigma = np.broadcast_to(np.asarray(sigma, dtype=float), (nfc,))
    out = np.empty((len(keys), nfc, nfft))
    kk = np.arange(nfft)
    for f, key in enumerate(keys):
        for c in range(nfc):
            inc = sigma[c] * np_normals(nfft, c, tag, seed, key)[0]
            inc[0] = 0.0
            phi = np.cumsum(inc)
            out[f, c] = phi - kk / (nfft - 1) * phi[-1]
    return out


def sigma_of(linewidth, nt):
    return math.sqrt(2 * math.pi * linewidth / nt)


def dqpsk_count_host(sym, pat_tx):
    """ex20_coherent_polmux.m:155-173 on one frame: sym [2, L] complex, pat_tx [L] x 2 quaternary transmitted patterns.
    samp2pat 'coherent' -> pat_decoder(binary) per polarisation -> ex20's swap rule -> errors of the four bit streams."""
    ph = np.angle(sym).T                                             # [L, 2]
    pm_hat = samp2pat(dict(rec="coherent"), None, ph)                # [L, 4]
    hx = patterns.pat_decoder(pm_hat[:, 0:2], "dqpsk", dict(binary=True))[1]
    hy = patterns.pat_decoder(pm_hat[:, 2:4], "dqpsk", dict(binary=True))[1]
    rx = np.concatenate([patterns.pat_decoder(p, "dqpsk")[1] for p in pat_tx], 1)
    hat = np.concatenate([hx, hy], 1)
    if np.sum(rx[:, 0:2] != hat[:, 2:4]) < np.sum(rx[:, 0:2] != hat[:, 0:2]):
        hat = np.concatenate([hat[:, 2:4], hat[:, 0:2]], 1)
    return int(np.sum(hat != rx))


def rotation_count_host(sym, bits):
    """HotPath.errors_resolved's rule on one frame: min over swap of the sum over polarisations of the minimum over the
    four pi/2 rotations, against the raw transmitted bits [L, 4]"""
    best = []
    for swap in (False, True):
        b = bits[:, [2, 3, 0, 1]] if swap else bits
        tot = 0
        for p in range(2):
            tot += min(int(np.sum(samp2pat(dict(rec="coherent"), None, np.angle(sym[p] * 1j ** k).reshape(-1, 1)) != b[:, 2 * p:2 * p + 2]))
                       for k in range(4))
        best.append(tot)
    return min(best)


def dqpsk_frames(L, nframes, seed=3):
    """synthetic received symbols [F, 2, L] and their transmitted bits [F, L, 4] / quaternary patterns [F, 2, L]:
    every global rotation, a pi/2 cycle slip mid-frame, exchanged polarisations, a few symbol errors, per-frame data.
    Returns also the mask of the slipped frames."""
    r = np.random.default_rng(seed)
    bits = r.integers(0, 2, (nframes, L, 4)).astype(np.uint8)
    sym = np.empty((nframes, 2, L), complex)
    slipped = np.zeros(nframes, bool)
    for f in range(nframes):
        for p in range(2):
            first, second = bits[f, :, 2 * p], bits[f, :, 2 * p + 1]
            # the quadrant samp2pat decides (first, second) for: first <=> Re > 0, second <=> Im > 0
            s = (np.where(first, 1.0, -1.0) + 1j * np.where(second, 1.0, -1.0)) / math.sqrt(2)
            s = s * np.exp(1j * 0.2 * r.standard_normal(L))
            sym[f, p] = s * 1j ** ((f + p) % 4)                      # global rotation per polarisation
        if f % 3 == 1:                                               # cycle slip: the second half turned by pi/2
            sym[f, :, L // 2:] *= 1j
            slipped[f] = True
        if f % 2 == 1:                                               # the receiver exchanged X and Y
            sym[f] = sym[f, ::-1].copy()
    quat = np.stack([2 * bits[:, :, 0] + bits[:, :, 1], 2 * bits[:, :, 2] + bits[:, :, 3]], 1)
    return sym, bits, quat, slipped


def expected_dqpsk_pat(quat):
    """[F, 4, L] uint8 of pat_decoder(pat, 'dqpsk') for the X and Y quaternary patterns of each frame"""
    out = []
    for q in quat:
        px = patterns.pat_decoder(q[0], "dqpsk")[1]
        py = patterns.pat_decoder(q[1], "dqpsk")[1]
        out.append(np.stack([px[:, 0], px[:, 1], py[:, 0], py[:, 1]]))
    return np.ascontiguousarray(np.stack(out).astype(np.uint8))


# ----------------------------------------------------------------- emulator helpers ---
@pytest.fixture(scope="module")
def emu():
    from tests import _emu
    return _emu.binding()


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _work(nfft, nfc, F):
    return np.zeros(F * nfc * (-(-nfft // 2048)))


def emu_phase(emu, nfft, nfc, keys, sigma, tag, u=None, stride=1, pitch=None, sign=1.0, phi_in=None, out=True):
    F = len(keys)
    sig = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, float), (nfc,)))
    kt = np.asarray(keys, dtype=np.int64)
    phi = np.full((F, nfc, nfft), np.nan) if out else None
    work = _work(nfft, nfc, F)
    ux = uy = None
    if u is not None:
        ux, uy = (np.array(v, dtype=np.complex128).view(np.float64) for v in u)
    emu.call("plx_phase_noise_dev", _vp(ux), _vp(uy), stride, pitch or nfft // stride, sign, nfft, nfc, F,
             _vp(sig) if phi_in is None else None, SEED, _vp(kt) if phi_in is None else None, tag, _vp(phi_in), _vp(phi),
             _vp(work) if phi_in is None else None, None)
    res = [phi]
    if u is not None:
        res += [ux.view(np.complex128).reshape(u[0].shape), uy.view(np.complex128).reshape(u[1].shape)]
    return res


# ----------------------------------------------------------------------------- tests ---
def test_abi_entry_points_declared():
    for name in ("plx_phase_noise_dev", "plx_front_run_lo_dev", "plx_decide_count_dqpsk_dev"):
        assert name in _abi.SIGNATURES
    assert (_abi.PLX_PHASE_TX, _abi.PLX_PHASE_LO) == (2, 3)


def test_restatement_reproduces_ampliflat_draws_and_tags_differ(emu):
    """With counter word 0 the restatement IS ampliflat's ASE stream (X polarisation, real part) -- so the documented
    layout is the device's -- and with the seed and key of an ampliflat call the phase draws (tags 2, 3) differ from
    every ASE draw of both polarisations."""
    n, key, seed = 4096, 77, SEED
    z, zy = np.zeros(2 * n), np.zeros(2 * n)
    kt, one = np.array([key], np.int64), np.ones(1)
    emu.call("plx_ampliflat_dev", _vp(z), _vp(zy), n, 1, 1, 1.0, _vp(one), None, seed, _vp(kt), 1, 1, None)
    ase = np.concatenate([z.view(np.complex128), zy.view(np.complex128)])
    cx, sx = np_normals(n, 0, 0, seed, key)
    np.testing.assert_allclose(z.view(np.complex128).real, cx, rtol=0, atol=1e-13)
    np.testing.assert_allclose(z.view(np.complex128).imag, sx, rtol=0, atol=1e-13)
    pool = np.concatenate([ase.real, ase.imag])
    for tag in (_abi.PLX_PHASE_TX, _abi.PLX_PHASE_LO):
        c, _ = np_normals(n, 0, tag, seed, key)
        assert np.intersect1d(np.round(c, 12), np.round(pool, 12)).size == 0
        assert abs(np.corrcoef(c, cx)[0, 1]) < 0.1
    tx, lo = np_normals(n, 0, 2, seed, key)[0], np_normals(n, 0, 3, seed, key)[0]
    assert abs(np.corrcoef(tx, lo)[0, 1]) < 0.1


@pytest.mark.parametrize("nfft,nfc", [(256, 3), (4096, 1), (65536, 3)])
def test_emu_generator_matches_restatement(emu, nfft, nfc):
    keys = [5, 123456789012, 5][: 2 if nfc == 3 else 3]
    sig = [sigma_of(1e-3, 16) * (1 + c) for c in range(nfc)]
    for tag in (_abi.PLX_PHASE_TX, _abi.PLX_PHASE_LO):
        phi, = emu_phase(emu, nfft, nfc, keys, sig, tag)
        ref = np_phase(nfft, nfc, keys, sig, tag)
        scale = np.abs(ref).max()
        assert np.abs(phi - ref).max() <= 1e-12 * scale
        assert np.abs(phi[:, :, -1]).max() <= 1e-13 * scale and np.all(phi[:, :, 0] == 0)   # bridge end points
    if len(keys) == 3:
        np.testing.assert_array_equal(phi[0], phi[2])                                      # same key, same draw
    assert not np.allclose(phi[0], phi[1])


def test_emu_rotation_routes(emu):
    """(a) transmitter: both polarisations times exp(+i phi_b); the 2-sps pick route: every stride-th sample of a
    [frame][channel][2][L] buffer times exp(-i phi_b); (c) the injected phase."""
    nfft, nfc, keys = 4096, 2, [3, 9]
    r = np.random.default_rng(1)
    ux = r.standard_normal((2, nfc, nfft)) + 1j * r.standard_normal((2, nfc, nfft))
    uy = r.standard_normal((2, nfc, nfft)) + 1j * r.standard_normal((2, nfc, nfft))
    sig = [0.02, 0.05]
    phi, ox, oy = emu_phase(emu, nfft, nfc, keys, sig, _abi.PLX_PHASE_TX, u=(ux, uy))
    ref = np_phase(nfft, nfc, keys, sig, _abi.PLX_PHASE_TX)
    np.testing.assert_allclose(ox, ux * np.exp(1j * ref), rtol=0, atol=1e-12)
    np.testing.assert_allclose(oy, uy * np.exp(1j * ref), rtol=0, atol=1e-12)
    # the pick route: rx [F nfc][2][L], L = nfft / stride, pol Y at +L
    stride = 16
    L = nfft // stride
    rx = r.standard_normal((2 * nfc, 2, L)) + 1j * r.standard_normal((2 * nfc, 2, L))
    buf = np.ascontiguousarray(rx).view(np.float64).copy()
    sg = np.ascontiguousarray(sig, dtype=float)
    kt = np.asarray(keys, np.int64)
    work = _work(nfft, nfc, 2)
    emu.call("plx_phase_noise_dev", _vp(buf), C.c_void_p(buf.ctypes.data + L * 16), stride, 2 * L, -1.0, nfft, nfc, 2,
             _vp(sg), SEED, _vp(kt), _abi.PLX_PHASE_LO, None, None, _vp(work), None)
    lo = np_phase(nfft, nfc, keys, sig, _abi.PLX_PHASE_LO)[:, :, ::stride].reshape(2 * nfc, 1, L)
    np.testing.assert_allclose(buf.view(np.complex128).reshape(rx.shape), rx * np.exp(-1j * lo), rtol=0, atol=1e-12)
    # injected phase (any values, no bridge)
    pin = np.ascontiguousarray(r.uniform(-50, 50, (2, nfc, nfft)))
    _, ix, iy = emu_phase(emu, nfft, nfc, keys, sig, _abi.PLX_PHASE_TX, u=(ux, uy), phi_in=pin, out=False)
    np.testing.assert_allclose(ix, ux * np.exp(1j * pin), rtol=0, atol=1e-12)
    np.testing.assert_allclose(iy, uy * np.exp(1j * pin), rtol=0, atol=1e-12)


def test_emu_phase_argument_checks(emu):
    z = np.zeros(2 * 512)
    bad = [dict(nfft=384), dict(nfft=128), dict(nfc=65), dict(tag=0), dict(sigma=-1.0), dict(stride=3)]
    for b in bad:
        a = dict(nfft=512, nfc=1, tag=2, sigma=0.1, stride=1)
        a.update(b)
        sg, work = np.full(max(a["nfc"], 1), a["sigma"]), np.zeros(64)
        with pytest.raises(_abi.PolmuxError):
            emu.call("plx_phase_noise_dev", _vp(z), None, a["stride"], a["nfft"], 1.0, a["nfft"], a["nfc"], 1,
                     _vp(sg), SEED, None, a["tag"], None, None, _vp(work), None)
    one = np.ones(1)
    with pytest.raises(_abi.PolmuxError, match="d_work"):
        emu.call("plx_phase_noise_dev", _vp(z), None, 1, 512, 1.0, 512, 1, 1, _vp(one), SEED, None, 2, None, None, None, None)


def test_emu_dqpsk_count_equals_host_composition(emu):
    L, F = 512, 12
    sym, bits, quat, slipped = dqpsk_frames(L, F)
    pat = expected_dqpsk_pat(quat)
    s = np.ascontiguousarray(sym).view(np.float64)
    err = np.full(F, -1, np.int64)
    emu.call("plx_decide_count_dqpsk_dev", _vp(s), L, 2, F, _vp(pat), 4 * L, _vp(err), None)
    host = np.array([dqpsk_count_host(sym[f], quat[f]) for f in range(F)])
    np.testing.assert_array_equal(err, host)
    assert host.max() > 0                                           # the symbol noise makes a few errors
    rot = np.array([rotation_count_host(sym[f], bits[f]) for f in range(F)])
    assert np.all(rot[slipped] > host[slipped]) and np.all(rot[slipped] > L // 4)
    assert np.all(host[slipped] <= host[~slipped].max() + 8)        # a slip costs the symbols next to it, not the frame
    # one pattern shared by all frames (stride 0)
    e0 = np.full(F, -1, np.int64)
    emu.call("plx_decide_count_dqpsk_dev", _vp(s), L, 2, F, _vp(np.ascontiguousarray(pat[0])), 0, _vp(e0), None)
    np.testing.assert_array_equal(e0, [dqpsk_count_host(sym[f], quat[0]) for f in range(F)])


def test_dqpsk_expected_matches_pat_decoder():
    from polmux_amd import synth
    from polmux_amd.pipeline import dqpsk_expected
    px, bx = synth.pattern_debruijn(256, 2, 4)
    py, by = synth.pattern_debruijn(256, 3, 4)
    got = dqpsk_expected(np.concatenate([bx, by], 1))
    want = np.concatenate([patterns.pat_decoder(px, "dqpsk")[1], patterns.pat_decoder(py, "dqpsk")[1]], 1).T
    np.testing.assert_array_equal(got, want)


# ----------------------------------------------------------------------- lasersource ---
def _reference_lasersource_phase(nfft, nch, nt, linewidth, rng):
    """lasersource.m:182-192 restated loop for loop (1-based MATLAB indices kept in the comments)"""
    lw = np.broadcast_to(np.asarray(linewidth, float), (nch,))
    fn = np.sqrt(2 * np.pi * lw / nt)[None, :] * rng.standard_normal((nfft, nch))
    fn.flat[0] = 0.0                                                 # freq_noise(1) = 0: linear index 1
    pn = np.cumsum(fn, axis=0)
    lin = pn.T.reshape(-1).copy()                                    # column-major linear view
    n = max(pn.shape)
    for k in range(1, n + 1):                                        # for nnoise = 1:length(phase_noise)
        lin[k - 1] = lin[k - 1] - (k - 1) / (n - 1) * lin[-1]        # ... - (nnoise-1)/(length-1)*phase_noise(end)
    return lin.reshape(nch, nfft).T


@pytest.mark.parametrize("nch", [1, 3])
def test_lasersource_linewidth_follows_reference(nch):
    import polmux_amd as px
    nsymb, nt = 64, 8
    px.reset_all(nsymb, nt, nch)
    lw = 1e-3 if nch == 1 else [1e-3, 2e-3, 5e-4]
    E = px.lasersource(2.0, 1550.0, 0.4, dict(linewidth=lw), rng=np.random.default_rng(9))
    ph = _reference_lasersource_phase(nsymb * nt, nch, nt, lw, np.random.default_rng(9))
    np.testing.assert_allclose(E, np.sqrt(2.0) * np.exp(1j * ph), rtol=0, atol=1e-12)
    assert E.shape == (nsymb * nt, nch)
    assert abs(np.angle(E[0, 0])) == 0.0
    if nch == 1:
        assert abs(np.angle(E[-1, 0])) < 1e-12                       # bridged: both ends at zero
    else:
        assert np.all(np.angle(E[0, 1:]) != 0)                       # freq_noise(1) zeroes column 1 only
        assert abs(np.angle(E[-1, -1])) > 1e-6                       # the other columns are not bridged
        np.testing.assert_allclose(np.angle(E[-1, 0]) % (2 * np.pi),
                                   (ph[-1, 0]) % (2 * np.pi), atol=1e-12)


def test_lasersource_options_and_errors():
    import polmux_amd as px
    px.reset_all(32, 8, 1)
    E0 = px.lasersource(1.0, 1550.0)
    np.testing.assert_array_equal(E0, np.ones((256, 1)))
    np.testing.assert_array_equal(px.lasersource(1.0, 1550.0, None, dict(linewidth=0.0)), E0)
    pn = np.linspace(0, 3, 256)
    np.testing.assert_allclose(px.lasersource(1.0, 1550.0, None, dict(pnoise=pn))[:, 0], np.exp(1j * pn), atol=1e-15)
    for k in ("n0", "anoise", "single"):
        with pytest.raises(ValueError, match="not supported"):
            px.lasersource(1.0, 1550.0, None, {k: 1})
    with pytest.raises(ValueError, match="does not exist"):
        px.lasersource(1.0, 1550.0, None, dict(linewdth=1e-3))
    px.reset_all(32, 8, 2)
    with pytest.raises(ValueError, match="linewidth length"):
        px.lasersource(1.0, 1550.0, 0.4, dict(linewidth=[1e-3, 1e-3, 1e-3]))


def test_hotpath_config_checks():
    from polmux_amd.pipeline import HotPath, HotPathConfig
    for kw in (dict(tx_linewidth=-1e-3), dict(lo_linewidth=float("inf")), dict(decoding="gray")):
        with pytest.raises(ValueError):
            HotPath(HotPathConfig(nsymb=16, nt=16, **kw), 1)
