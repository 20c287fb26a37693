"""numpy restatements and shared cases for the tests of the per-channel 'sepfields' receiver (HotPathConfig(wdm_receiver=
'channel')): the pick with a delay per channel, the CDE with a table per channel, the two back ends
(host emulator, shipped library) the same cases run on, and the linear model of fibre -> pick -> CDE."""
import ctypes as C

import numpy as np


def vp(a):
    return C.c_void_p(a.ctypes.data)


class Host:
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


class Dev:
    """the hipcc-built library on device tensors"""

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


def cnormal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def nan(shape):
    return np.full(shape, np.nan + 1j * np.nan)


# ------------------------------------------------------------------------ pick ---
def pick_np(ux, uy, n_out, stride, scale, nch, delay):
    """rx[cf][p][i] = scale * u_p[cf][(i stride + delay[cf % nch]) mod nfft]; ux, uy [CF, nfft] -> [CF, 2, n_out]"""
    CF, nfft = ux.shape
    d = np.asarray(delay, dtype=np.int64)[np.arange(CF) % nch]
    idx = (np.arange(n_out, dtype=np.int64)[None, :] * stride + d[:, None]) % nfft
    return np.stack([np.take_along_axis(ux, idx, 1), np.take_along_axis(uy, idx, 1)], 1) * scale


def call_pick_wdm(be, dux, duy, nfft, n_out, stride, scale, nch, F, delay):
    """plx_pick_wdm_dev on uploaded ux, uy [F nch, nfft] -> host rx [F nch + 1, 2, n_out]: the output is NaN first and
    reaches one channel-frame beyond what the call may write"""
    drx = be.up(nan((F * nch + 1, 2, n_out)))
    dl = np.ascontiguousarray(delay, dtype=np.int64)
    be.b.call("plx_pick_wdm_dev", be.ptr(dux), be.ptr(duy), be.ptr(drx), nfft, n_out, stride, float(scale), nch, F, vp(dl),
              be.stream)
    return be.down(drx)


def call_pick_two(be, dux, duy, nfft, n_out, stride, scale, CF):
    """the two plx_pick_dev calls of HotPath._front_end that the one launch replaces -> host rx [CF + 1, 2, n_out]"""
    drx = be.up(nan((CF + 1, 2, n_out)))
    base = be.ptr(drx)
    base = base.value if isinstance(base, C.c_void_p) else base
    for pol, src in enumerate((dux, duy)):
        be.b.call("plx_pick_dev", be.ptr(src), C.c_void_p(base + pol * n_out * 16), nfft, n_out, 0, stride, float(scale), CF,
                  2 * n_out, be.stream)
    return be.down(drx)


def edge_delays(nfft, nch, k):
    """delay sets of both signs that include 0, +-1 and +-(nfft - 1): set k of 2 for nch channels"""
    pool = [0, 1, -1, nfft - 1, -(nfft - 1), 17, -17, nfft // 2, -(nfft // 2) - 3]
    if nch == 1:
        return [pool[k]]                      # (one channel: one edge value per call, k over the first five)
    return [pool[(k * 3 + c) % len(pool)] * (1 if (c // len(pool)) % 2 == 0 else -1) for c in range(nch)]


def check_pick(be, nfft, nch, F, strides, seed=1):
    """the pick against numpy's gather, bit for bit (a copy times one scale), with the properties that pin it: all-zero
    delays equal the two plx_pick_dev calls, delay d equals np.roll(delay 0, -d) before the stride; returns nothing"""
    r = np.random.default_rng(seed + nfft + 7 * nch)
    CF = F * nch
    ux, uy = cnormal(r, (CF, nfft)), cnormal(r, (CF, nfft))
    dux, duy = be.up(ux), be.up(uy)
    scale = 1.0 / 3.0                          # (not a power of two: the product rounds)
    seen = set()
    for stride in strides:
        n_out = nfft // stride
        zero = call_pick_wdm(be, dux, duy, nfft, n_out, stride, scale, nch, F, [0] * nch)
        assert np.isnan(zero[CF]).all()
        assert np.array_equal(zero[:CF], pick_np(ux, uy, n_out, stride, scale, nch, [0] * nch))
        two = call_pick_two(be, dux, duy, nfft, n_out, stride, scale, CF)
        assert np.array_equal(zero[:CF], two[:CF])
        for k in range(5 if nch == 1 else 2):
            delay = edge_delays(nfft, nch, k)
            seen.update(delay)
            got = call_pick_wdm(be, dux, duy, nfft, n_out, stride, scale, nch, F, delay)
            assert np.isnan(got[CF]).all()
            assert np.array_equal(got[:CF], pick_np(ux, uy, n_out, stride, scale, nch, delay)), (stride, delay)
            if stride == 1:                    # the sign: reading at n + d is a roll of the output by -d
                for cf in range(CF):
                    assert np.array_equal(got[cf], np.roll(zero[cf], -delay[cf % nch], axis=-1)), (cf, delay)
    assert {0, 1, -1, nfft - 1, -(nfft - 1)} <= seen


def check_pick_errors(be):
    from polmux_amd._abi import PLX_ERR_ARG, PolmuxError
    import pytest
    z = be.up(np.zeros((2, 256), complex))
    o = be.up(np.zeros((2, 2, 256), complex))

    def call(nfft=256, n_out=128, stride=2, nch=1, F=1, delay=(0,), ux=z, uy=z, rx=o, nodelay=False):
        dl = np.ascontiguousarray(delay, dtype=np.int64)
        be.b.call("plx_pick_wdm_dev", be.ptr(ux), be.ptr(uy), be.ptr(rx), nfft, n_out, stride, 1.0, nch, F,
                  None if nodelay else vp(dl), be.stream)

    for kw, what in ((dict(nch=0), "nch"), (dict(nch=65, delay=[0] * 65), "nch"), (dict(delay=[256]), "delay"),
                     (dict(delay=[-256]), "delay"), (dict(nch=2, delay=[0, 300]), "delay"), (dict(n_out=129), "n_out \\* stride"),
                     (dict(n_out=256, stride=2), "n_out \\* stride"), (dict(n_out=0), "n_out \\* stride"),
                     (dict(stride=0), "n_out \\* stride"), (dict(F=0), "nframes"), (dict(F=65536), "nframes"),
                     (dict(nfft=0), "nfft"), (dict(ux=None), "null"), (dict(uy=None), "null"), (dict(rx=None), "null"),
                     (dict(nodelay=True), "null")):
        with pytest.raises(PolmuxError, match=what) as ei:
            call(**kw)
        assert ei.value.code == PLX_ERR_ARG, kw
    call(delay=[255])                              # the largest delays are accepted
    call(delay=[-255])
    call(n_out=256, stride=1)


# ------------------------------------------------------------------------- CDE ---
def unit_tables(rng, nch, N):
    """random unit-modulus tables [nch, N], every bin distinct: a row served by the wrong table or a misplaced bin shows"""
    return np.exp(1j * rng.uniform(-np.pi, np.pi, (nch, N)))


def cde_apply(be, create, args, dx, nrows, nx):
    """one plan made by `create`(&plan, *args), applied to the uploaded rows dx [nrows, nx] -> host y [nrows + 1, nx]"""
    plan = C.c_void_p()
    be.b.call(create, C.byref(plan), *args)
    try:
        dy = be.up(nan((nrows + 1, nx)))
        be.b.call("plx_cde_apply_dev", plan, be.ptr(dx), be.ptr(dy), nx, nrows, be.stream)
        return be.down(dy)
    finally:
        be.b.call("plx_cde_destroy", plan)


def check_cde_tables(be, N, L, nx, nch, rpc, nrows, seed=3):
    """a plx_cde_create_wdm plan: every row equals, bit for bit, the same row through a one-table plx_cde_create plan built
    from that row's table, table (r / rpc) % nch; returns the output [nrows, nx]"""
    r = np.random.default_rng(seed + N)
    x = cnormal(r, (nrows, nx))
    H = unit_tables(r, nch, N)
    Hi = np.ascontiguousarray(H).view(np.float64)
    dx = be.up(x)
    y = cde_apply(be, "plx_cde_create_wdm", (N, L, vp(Hi), nch, rpc), dx, nrows, nx)
    assert np.isnan(y[nrows]).all() and not np.isnan(y[:nrows]).any()
    tab = (np.arange(nrows) // rpc) % nch
    assert nch == 1 or len(set(tab.tolist())) == nch
    for c in range(nch):
        Hc = np.ascontiguousarray(H[c]).view(np.float64)
        one = cde_apply(be, "plx_cde_create", (N, L, vp(Hc)), dx, nrows, nx)
        rows = np.nonzero(tab == c)[0]
        assert np.array_equal(y[rows], one[rows]), c
        others = np.nonzero(tab != c)[0]
        assert all(not np.array_equal(y[k], one[k]) for k in others)      # (the tables differ: the check is not vacuous)
    return y[:nrows]


def check_cde_errors(be):
    from polmux_amd._abi import PLX_ERR_ARG, PLX_ERR_UNSUPPORTED, PolmuxError
    import pytest
    H = np.ones(2 * 3 * 64)
    for args, code, what in (((64, 32, vp(H), 0, 2), PLX_ERR_ARG, "nch must be in \\[1, 64\\]"),
                             ((64, 32, vp(H), 65, 2), PLX_ERR_ARG, "nch must be in \\[1, 64\\]"),
                             ((64, 32, vp(H), 3, 0), PLX_ERR_ARG, "rows_per_channel must be >= 1"),
                             ((15, 5, vp(H), 3, 2), PLX_ERR_ARG, "H must be even length"),
                             ((16, 0, vp(H), 3, 2), PLX_ERR_ARG, "L must be > 0"),
                             ((16, 17, vp(H), 3, 2), PLX_ERR_ARG, "shorter than filter length"),
                             ((8192, 4096, vp(H), 1, 2), PLX_ERR_UNSUPPORTED, "power of two in \\[4, 4096\\]"),
                             ((16, 7, vp(H), 3, 2), PLX_ERR_UNSUPPORTED, "N-L must be even")):
        plan = C.c_void_p(1234)
        with pytest.raises(PolmuxError, match=what) as ei:
            be.b.call("plx_cde_create_wdm", C.byref(plan), *args)
        assert ei.value.code == code and not plan.value
    with pytest.raises(PolmuxError, match="plx_cde_create_wdm: null argument") as ei:
        be.b.call("plx_cde_create_wdm", C.byref(C.c_void_p()), 64, 32, None, 3, 2)
    assert ei.value.code == PLX_ERR_ARG


# ------------------------------------------------- the linear chain in numpy ---
def overlap_save(x, H, L):
    """OverlapBothTrans (CDE_OFDE.m:88-124) in numpy: x [nx], H [N] on the fftshift-ordered grid"""
    N, nx = H.size, x.size
    B2 = (N - L) // 2
    nb = -(-nx // L)
    xe = np.concatenate([np.zeros(B2, complex), x, np.zeros(nb * L + N - nx, complex)])
    Hs = np.fft.ifftshift(H)
    y = np.concatenate([np.fft.ifft(np.fft.fft(xe[b * L:b * L + N]) * Hs)[B2:B2 + L] for b in range(nb)])
    return y[:nx]


def linear_chain(tx, betat_c, total_length, half, delay, H, L):
    """one polarisation of one channel: ifft(fft(tx) exp(-i betat L)) -> the 2-sps pick at i half + delay -> overlap-save
    with H (lossless and unit scale: the spans' loss is restored by the amplifiers and the receiver scale)"""
    u = np.fft.ifft(np.fft.fft(tx) * np.exp(-1j * betat_c * total_length))
    n = tx.size
    return overlap_save(u[(np.arange(n // half) * half + int(delay)) % n], H, L)


def rel_rms(a, b):
    return np.sqrt(np.mean(np.abs(a - b) ** 2) / np.mean(np.abs(b) ** 2))


def sep_comb(nsymb=256, nt=16, nch=3, chspacing=0.4, lam=1550.0, symbolrate=28.0, length=8e4, disp=17.0, slope=0.0):
    """fiber_tables of a 'sepfields' comb of nch columns ('g---'), on GSTATE as HotPath sets it while the tables are formed
    (restored on return): dict(t, lam [nch] in nm, fn)"""
    from polmux_amd import synth
    from polmux_amd.fiber import fiber_tables
    from polmux_amd.gstate import GSTATE
    names = ("NSYMB", "NT", "NCH", "SYMBOLRATE", "FN", "LAMBDA")
    saved = {k: getattr(GSTATE, k) for k in names}
    try:
        GSTATE.NSYMB, GSTATE.NT, GSTATE.NCH, GSTATE.SYMBOLRATE = nsymb, nt, nch, symbolrate
        GSTATE.FN = fn = synth.fn_grid(nsymb, nt)
        GSTATE.LAMBDA = lamv = lam + chspacing * (np.arange(nch) - (nch - 1) / 2)
        x = {"length": length, "alphadB": 0.2, "aeff": 80.0, "n2": 2.7e-20, "lambda": lam, "disp": disp, "slope": slope}
        t = fiber_tables(x, [1, 0, 0, 0], nch, 0.0)
    finally:
        for k, v in saved.items():
            setattr(GSTATE, k, v)
    return dict(t=t, lam=np.atleast_1d(lamv), fn=np.asarray(fn, dtype=float))
