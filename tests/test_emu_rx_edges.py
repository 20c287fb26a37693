"""Shape edges of the receiver kernels (polmux_amd/csrc/plx_rx.hip) against the CPU oracle.

Every case runs twice on the same seeded inputs: under the host emulator (tests/emu, CPU) and, with -m gpu, through the
hipcc-built library on the MI355X.  Output buffers reach one frame (or signal) beyond what the call may write and are
filled with NaN or a marker first: an unwritten frame or a write past the last one fails.  Bars: CDE, CPE and decisions
as test_gpu_parity.py (1e-11, bit-exact); the CMA driver loop 1e-9 with pass counts equal."""
import ctypes as C

import numpy as np
import pytest

from polmux_amd._abi import PLX_ERR_ARG, PLX_ERR_UNSUPPORTED, DspParams, PolmuxError


class _Host:
    """emulator: device pointers are host pointers"""
    stream = None

    def __init__(self, b):
        self.b = b

    def up(self, a):
        return np.array(a, order="C", copy=True)

    def ptr(self, h):
        return None if h is None else C.c_void_p(h.ctypes.data)

    def down(self, h):
        return np.array(h, copy=True)


class _Dev:
    def __init__(self, b):
        import torch
        self.torch, self.b = torch, b

    def up(self, a):
        return self.torch.from_numpy(np.array(a, order="C", copy=True)).cuda()

    def ptr(self, h):
        return None if h is None else h.data_ptr()

    def down(self, h):
        self.torch.cuda.synchronize()
        return h.cpu().numpy()

    @property
    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module", params=["emu", pytest.param("lib", marks=pytest.mark.gpu)])
def be(request):
    if request.param == "emu":
        from tests import _emu
        return _Host(_emu.binding())
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from polmux_amd import _abi
    b = _abi.get()
    assert b.path.endswith("polmux_amd/lib/libpolmux_hip.so")
    return _Dev(b)


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _nan(shape):
    return np.full(shape, np.nan + 1j * np.nan)


# ======================================================================= CDE ===
# N 4 .. 4096 (2048 and 4096: H read from global memory, one block per workgroup); L = N (no overlap), L = 2; nx = N and
# nx = k L +- 1 (a last block that is one sample short of full, or holds one sample)
@pytest.mark.parametrize("N,L,nx", [(4, 4, 4), (4, 4, 13), (4, 2, 7), (4, 2, 9), (16, 2, 33), (2048, 2048, 2048),
                                    (2048, 1024, 3071), (2048, 1024, 3073), (4096, 4096, 4096), (4096, 4096, 4097),
                                    (4096, 2048, 6143)])
def test_cde_apply_edges(be, oracle, N, L, nx):
    nsig = 3
    r = np.random.default_rng(1000 * N + nx)
    x = r.standard_normal((nsig, nx)) + 1j * r.standard_normal((nsig, nx))
    H = np.exp(1j * r.uniform(-np.pi, np.pi, N)) * r.uniform(0.5, 1.5, N)     # every bin distinct: a misplaced bin shows
    Hi = np.ascontiguousarray(H).view(np.float64)
    plan = C.c_void_p()
    be.b.call("plx_cde_create", C.byref(plan), N, L, _vp(Hi))
    try:
        dx, dy = be.up(x), be.up(_nan((nsig + 1, nx)))
        be.b.call("plx_cde_apply_dev", plan, be.ptr(dx), be.ptr(dy), nx, nsig, be.stream)
        y = be.down(dy)
    finally:
        be.b.call("plx_cde_destroy", plan)
    assert np.isnan(y[nsig]).all()
    for k in range(nsig):
        ref, rc = oracle.overlap_both_trans(x[k], H, L)
        assert rc == 0
        np.testing.assert_allclose(y[k], ref, rtol=0, atol=1e-11)


@pytest.mark.parametrize("N,L,code,msg", [(8192, 4096, PLX_ERR_UNSUPPORTED, "power of two in \\[4, 4096\\]"),
                                          (96, 48, PLX_ERR_UNSUPPORTED, "power of two"),
                                          (2, 2, PLX_ERR_UNSUPPORTED, "power of two"),
                                          (16, 7, PLX_ERR_UNSUPPORTED, "N-L must be even"),
                                          (4096, 4095, PLX_ERR_UNSUPPORTED, "N-L must be even"),
                                          (15, 5, PLX_ERR_ARG, "H must be even length"),           # CDE_OFDE.m:73-74
                                          (16, 0, PLX_ERR_ARG, "L must be > 0"),                   # :77-78
                                          (16, 17, PLX_ERR_ARG, "shorter than filter length")])    # :79-80
def test_cde_rejections(be, N, L, code, msg):
    H = np.ones(2 * N)
    plan = C.c_void_p(1234)
    with pytest.raises(PolmuxError, match=msg) as e:
        be.b.call("plx_cde_create", C.byref(plan), N, L, _vp(H))
    assert e.value.code == code
    assert not plan.value


def test_cde_rejects_signal_shorter_than_filter(be):
    H = np.ones(2 * 64)
    plan = C.c_void_p()
    be.b.call("plx_cde_create", C.byref(plan), 64, 32, _vp(H))
    try:
        dx = be.up(np.zeros(63, complex))
        with pytest.raises(PolmuxError, match="Signal must be longer or equal filter") as e:     # :83-84
            be.b.call("plx_cde_apply_dev", plan, be.ptr(dx), be.ptr(dx), 63, 1, be.stream)
        assert e.value.code == PLX_ERR_ARG
    finally:
        be.b.call("plx_cde_destroy", plan)


# =============================================================== CMA driver ===
def _mixed_qpsk(L, seed, noise=0.05, th=0.4):
    r = np.random.default_rng(seed)
    a = np.exp(1j * (np.pi / 4 + np.pi / 2 * r.integers(0, 4, (L, 2))))
    J = np.array([[np.cos(th), np.sin(th) * np.exp(0.3j)], [-np.sin(th) * np.exp(-0.3j), np.cos(th)]])
    return a @ J + noise * (r.standard_normal((L, 2)) + 1j * r.standard_normal((L, 2)))


def _frames(L, F, seed):
    """F frames with their own input (seed, noise, mixing) and their own initial centre-tap matrix M"""
    xs, Ms = [], []
    for f in range(F):
        xs.append(_mixed_qpsk(L, seed + f, noise=0.02 + 0.03 * f, th=0.15 + 0.2 * f))
        phi, psi = 0.1 + 0.25 * f, 0.4 * f - 0.3
        Ms.append(np.array([[np.cos(phi), np.sin(phi) * np.exp(1j * psi)], [-np.sin(phi) * np.exp(-1j * psi), np.cos(phi)]]))
    return xs, Ms


def _cma_vs_oracle(be, oracle, xs, Ms, taps, mu):
    """plx_poldemux_dev (CMA driver) on all frames at once; y, h and passes of every frame against oracle.cmapolardemux.
    R1 != R2, so that an exchange of the two output rows shows."""
    F, L = len(xs), xs[0].shape[0]
    R = np.array([1.0, 1.2])
    dx = be.up(np.stack([v.T for v in xs]))                          # [frame][2][L]
    dM = be.up(np.stack([m.reshape(4) for m in Ms]))
    dy, dh = be.up(_nan((F + 1, 2, L))), be.up(_nan((F + 1, 2, 2, taps)))
    dp = be.up(np.full(F + 1, -7, np.int32))
    be.b.call("plx_poldemux_dev", 1, be.ptr(dx), be.ptr(dy), L, F, taps, mu, _vp(R), be.ptr(dM), be.ptr(dh), be.ptr(dp),
              be.stream)
    y, h, passes = be.down(dy), be.down(dh), be.down(dp)
    assert np.isnan(y[F]).all() and np.isnan(h[F]).all() and passes[F] == -7     # nothing past the last frame
    assert np.isfinite(y[:F]).all() and np.isfinite(h[:F]).all()
    for f in range(F):
        oy, h1, h2, n = oracle.cmapolardemux(xs[f], Ms[f], taps, mu, R)
        assert passes[f] == n, f
        np.testing.assert_allclose(y[f].T, oy, rtol=0, atol=1e-9)
        np.testing.assert_allclose(h[f, 0].T, h1, rtol=0, atol=1e-9)
        np.testing.assert_allclose(h[f, 1].T, h2, rtol=0, atol=1e-9)
    return passes[:F]


# k_cma16: L = 16 .. 41 is 2 .. 5 chunks of 8 symbols, with and without a tail, with and without interior chunks
# (0 < k < nchunks - 2); mu keeps the pass budget 50 ceil(1/(L mu)) at 100
@pytest.mark.parametrize("taps", [1, 3, 5, 7])
@pytest.mark.parametrize("L", [16, 17, 23, 24, 25, 31, 32, 33, 40, 41])
def test_cma16_chunk_edges(be, oracle, L, taps):
    xs, Ms = _frames(L, 3, 100 * L + taps)
    _cma_vs_oracle(be, oracle, xs, Ms, taps, 0.55 / L)


# below 16 samples the driver takes the generic k_cma: L = 15, and the shortest frame the taps allow (taps/2 + 1)
@pytest.mark.parametrize("taps", [1, 3, 5, 7])
@pytest.mark.parametrize("short", [False, True])
def test_cma_short_frames_take_generic_kernel(be, oracle, taps, short):
    L = taps // 2 + 1 if short else 15
    xs, Ms = _frames(L, 3, 7 * L + taps)
    _cma_vs_oracle(be, oracle, xs, Ms, taps, (0.2 if short else 0.55) / L)


# k_cma group widths: 9 taps -> 16 lanes, 17 -> 32, 33 and 63 -> 64 (a whole wave per frame)
@pytest.mark.parametrize("taps,L,mu", [(9, 24, 1 / 48), (17, 24, 1 / 48), (33, 40, 1 / 150), (63, 40, 1 / 200)])
def test_cma_group_widths(be, oracle, taps, L, mu):
    xs, Ms = _frames(L, 3, taps)
    _cma_vs_oracle(be, oracle, xs, Ms, taps, mu)


def test_cma_65_taps_unsupported(be):
    L = 40
    dx = be.up(np.zeros((1, 2, L), complex))
    dy = be.up(np.zeros((1, 2, L), complex))
    dM = be.up(np.eye(2, dtype=complex).reshape(1, 4))
    R = np.array([1.0, 1.0])
    with pytest.raises(PolmuxError, match="at most 64 taps") as e:
        be.b.call("plx_poldemux_dev", 1, be.ptr(dx), be.ptr(dy), L, 1, 65, 1e-3, _vp(R), be.ptr(dM), None, None, be.stream)
    assert e.value.code == PLX_ERR_UNSUPPORTED


# ============================================================ CPE (DSP plan) ===
def _dsp_params(**kw):
    p = DspParams()
    d = dict(workatbaudrate=0, applynlr=0, nlralpha=0.0, power_mw=2.0, applypol=0, polmethod=1, cma_mu=1 / 40,
             cma_taps=7, cma_txpolars=2, cma_phizero=0.0, easi_mu=1 / 40, easi_txpolars=2, easi_phizero=0.0,
             modorder=2, freqavg=20, phasavg=3, poworder=2)
    d.update(kw)
    for k, v in d.items():
        setattr(p, k, v)
    p.cma_R[0], p.cma_R[1] = 1.0, 1.0
    return p


# carrier recovery alone (no demultiplexing): the LDS route up to L = 1320, global scratch from 1321 on; a boxcar of
# 2*70+1 = 141 taps over a 64-symbol frame (wraps twice); no averaging at all; modorder 1 (BPSK, no pi/4 offset); one
# column; an odd Lin (decimates to (Lin+1)/2); the nonlinear rotation over one column
@pytest.mark.parametrize("Lin,ncol,kw", [(2640, 2, dict()), (2642, 2, dict()), (34, 2, dict()), (128, 2, dict(phasavg=70)),
                                         (256, 2, dict(freqavg=0, phasavg=0)), (256, 2, dict(modorder=1)),
                                         (256, 1, dict()), (129, 2, dict()), (256, 1, dict(applynlr=1, nlralpha=0.05))],
                         ids=["L1320_lds", "L1321_global", "L17", "boxcar_wraps_twice", "no_averaging", "modorder1", "ncol1",
                              "odd_Lin", "nlr_ncol1"])
def test_cpe_through_dsp_plan(be, oracle, Lin, ncol, kw):
    F, Fmax = 3, 4
    p = _dsp_params(**kw)
    L = (Lin + 1) // 2
    r = np.random.default_rng(Lin + 10 * ncol + 100 * p.modorder + p.phasavg)
    ins = []
    for f in range(F):
        if p.modorder == 1:
            a = r.choice([-1.0, 1.0], (L, ncol)).astype(complex)
        else:
            a = np.exp(1j * (np.pi / 4 + np.pi / 2 * r.integers(0, 4, (L, ncol))))
        n = np.arange(L)[:, None]
        ph = 2 * np.pi * (1 + f) / L * n + 0.3 + 0.7 * f + np.cumsum(0.01 * r.standard_normal((L, 1)), 0)   # offset + walk
        s = a * np.exp(1j * ph) + 0.05 * (r.standard_normal((L, ncol)) + 1j * r.standard_normal((L, ncol)))
        x = r.standard_normal((Lin, ncol)) + 1j * r.standard_normal((Lin, ncol))
        x[::2] = s * 4 * np.sqrt(2.0)
        ins.append(x)
    plan = C.c_void_p()
    be.b.call("plx_dsp_create", C.byref(plan), Lin, ncol, Fmax, C.byref(p))
    try:
        assert be.b.lib.plx_dsp_out_len(plan) == L
        din, dout = be.up(np.stack([x.T for x in ins])), be.up(_nan((Fmax, ncol, L)))
        be.b.call("plx_dsp_run_dev", plan, be.ptr(din), be.ptr(dout), F, be.stream)
        out = be.down(dout)
    finally:
        be.b.call("plx_dsp_destroy", plan)
    assert np.isnan(out[F:]).all()
    op = oracle.dsp_params(power_mw=2.0, applynlr=bool(p.applynlr), nlralpha=p.nlralpha, modorder=p.modorder,
                           freqavg=p.freqavg, phasavg=p.phasavg, poworder=p.poworder)
    for f in range(F):
        ref = oracle.dsp_pdm_coh_qpsk(ins[f], op)
        assert ref.shape == (L, ncol)
        np.testing.assert_allclose(out[f].T, ref, rtol=0, atol=1e-11)


# ================================================================ decisions ===
@pytest.mark.parametrize("L", [1, 255, 257])
@pytest.mark.parametrize("ncol", [1, 2])
def test_decide_per_frame_patterns(be, oracle, ncol, L):
    """plx_decide_count_frames_dev with pat_frame_stride > 0 (what HotPath uses with variants > 1): frame f counts against
    the pattern block at f * stride bytes; the stride here is padded past the block, so it must be taken as given."""
    F = 3
    r = np.random.default_rng(10 * L + ncol)
    sym = np.exp(1j * r.uniform(-np.pi, np.pi, (F, ncol, L))) * r.uniform(0.5, 1.5, (F, ncol, L))
    stride = 2 * ncol * L + 5
    patbuf = r.integers(0, 2, F * stride).astype(np.uint8)
    pats = [patbuf[f * stride: f * stride + 2 * ncol * L].reshape(2 * ncol, L) for f in range(F)]
    dsym, dpat = be.up(sym), be.up(patbuf)
    dhat = be.up(np.full((F + 1, 2 * ncol, L), 7, np.uint8))
    derr = be.up(np.full((F + 1) * ncol, -1, np.int64))
    be.b.call("plx_decide_count_frames_dev", be.ptr(dsym), L, ncol, F, be.ptr(dpat), stride, be.ptr(dhat), be.ptr(derr),
              be.stream)
    hat, err = be.down(dhat), be.down(derr)
    assert (hat[F] == 7).all() and (err[F * ncol:] == -1).all()
    counts = []
    for f in range(F):
        want = oracle.samp2pat_coherent(np.angle(sym[f].T)).T                # [2 ncol][L]
        np.testing.assert_array_equal(hat[f], want)
        for c in range(ncol):
            counts.append(int((want[2 * c: 2 * c + 2] != pats[f][2 * c: 2 * c + 2]).sum()))
    assert err[: F * ncol].tolist() == counts
    if L > 1:      # the per-frame patterns matter: against frame 0's pattern the counts are different ones
        shared = [int((oracle.samp2pat_coherent(np.angle(sym[f].T)).T[2 * c: 2 * c + 2] != pats[0][2 * c: 2 * c + 2]).sum())
                  for f in range(F) for c in range(ncol)]
        assert shared != counts


def test_decide_without_pattern_or_without_hat(be, oracle):
    F, ncol, L = 2, 2, 130
    r = np.random.default_rng(8)
    sym = np.exp(1j * r.uniform(-np.pi, np.pi, (F, ncol, L)))
    pat = r.integers(0, 2, (2 * ncol, L)).astype(np.uint8)
    dsym, dpat = be.up(sym), be.up(pat)
    want = [oracle.samp2pat_coherent(np.angle(sym[f].T)).T for f in range(F)]
    # no pattern: decisions only, counts of zero
    dhat, derr = be.up(np.full((F, 2 * ncol, L), 7, np.uint8)), be.up(np.full(F * ncol, -1, np.int64))
    be.b.call("plx_decide_count_frames_dev", be.ptr(dsym), L, ncol, F, None, 0, be.ptr(dhat), be.ptr(derr), be.stream)
    hat, err = be.down(dhat), be.down(derr)
    for f in range(F):
        np.testing.assert_array_equal(hat[f], want[f])
    assert err.tolist() == [0] * (F * ncol)
    # no decisions: counts only
    derr = be.up(np.full(F * ncol, -1, np.int64))
    be.b.call("plx_decide_count_frames_dev", be.ptr(dsym), L, ncol, F, be.ptr(dpat), 0, None, be.ptr(derr), be.stream)
    err = be.down(derr)
    assert err.tolist() == [int((want[f][2 * c: 2 * c + 2] != pat[2 * c: 2 * c + 2]).sum()) for f in range(F) for c in range(ncol)]


def test_decide_symbols_on_the_axes(be, oracle):
    """Symbols exactly on the decision boundaries, signed zeros included: atan2(+0, -1) = pi, atan2(-0, -1) = -pi;
    bit-exact against samp2pat (samp2pat.m:61-66) on numpy's angle of the same values."""
    vals = np.array([1.0, -1.0, 0.0, -0.0, 0.5, -2.0, 1e-300, -1e-300])
    re, im = np.meshgrid(vals, vals)
    sym = np.empty(re.size, complex)
    sym.real, sym.imag = re.reshape(-1), im.reshape(-1)
    L = sym.size
    assert np.signbit(sym.imag).sum() > 0 and np.signbit(sym.real).sum() > 0
    s2 = np.stack([sym, sym[::-1]])[None]                                     # [1 frame][2][L]
    dsym = be.up(s2)
    dhat = be.up(np.full((1, 4, L), 7, np.uint8))
    be.b.call("plx_decide_count_frames_dev", be.ptr(dsym), L, 2, 1, None, 0, be.ptr(dhat), None, be.stream)
    hat = be.down(dhat)[0]
    want = oracle.samp2pat_coherent(np.angle(s2[0].T)).T
    np.testing.assert_array_equal(hat, want)
    k = np.flatnonzero((sym.real == -1.0) & (sym.imag == 0))
    assert sorted(hat[1, k].tolist()) == [0, 1]          # the sign of the zero decides the second bit on the negative axis


def test_evm_one_column(be):
    F, L = 3, 257
    r = np.random.default_rng(12)
    sym = np.exp(1j * (np.pi / 4 + np.pi / 2 * r.integers(0, 4, (F, 1, L)))) + 0.15 * (r.standard_normal((F, 1, L)) + 1j * r.standard_normal((F, 1, L)))
    sym[0, 0, :4] = [0.0, -0.0, 1j * 0.5, -0.3]                               # on the axes: x >= 0 and y > 0 decide
    d = be.up(sym)
    out = be.up(np.full(F + 1, np.nan))
    be.b.call("plx_evm_dev", be.ptr(d), L, 1, F, be.ptr(out), be.stream)
    got = be.down(out)
    assert np.isnan(got[F])
    hat = (np.where(sym.real >= 0, 1, -1) + 1j * np.where(sym.imag > 0, 1, -1)) / np.sqrt(2)
    np.testing.assert_allclose(got[:F], (np.abs(sym - hat) ** 2).mean(axis=(1, 2)), rtol=1e-13)
