"""Cases and one runner for the tests of the fibre propagator away from the suite's one operating point (alphadB = 0.2,
dphimax 5e-3 ... 2e-2, dzmax 1e4 ... 2e4, the nonlinear-phase rule picking every step): a lossless fibre (the alphalin == 0
arms of nextstep and of Leff, ssfm_ctrl.h), the loss-limited step (dl >= 1: dz = dzmax), steps of a large nonlinear phase
(the full-range sincos of the fused sweep with GVD on), a step that loses several dB, many waveplate trunks in one step
through the phasor tables (30 < trunks <= tmax <= 64), a batch whose frames sit in different regimes and one with an
all-zero frame.  The same cases run on two back ends, the host emulator (tests/test_emu_fibre_regimes.py) and the shipped
library on device tensors (tests/test_gpu_fibre_regimes.py); the checks are written once, here.

Every case is compared with the oracle: ncycle equal, the first step to 1e-12 relative, the field to the back end's bar.
That a case really sits in the regime it is named after is computed from its inputs and the oracle's steps, never from
the library under test."""
import ctypes as C
import math

import numpy as np
import pytest

from polmux_amd import synth
from polmux_amd._abi import PLX_SSFM_SHARE_DEVICE
from tests.test_emu_kernels import _desc, _tables
from tests.wdm_rx_ref import Dev, Host, vp  # noqa: F401  (the back ends are shared with the receiver's cases)

GAM = [1.3e-6]
ALPHA = 4.6e-5                  # 0.2 dB/km
EMU_BAR = 1e-11                 # of max|u|: the bar of tests/test_emu_kernels.py
GPU_BAR = 1e-9                  # FIELD_RTOL of tests/test_gpu_parity.py
FULL_RANGE = 0.0625             # rad: where the Kerr step of the fused sweep leaves the Taylor form (ssfm_colx.hip)

# id -> fls, L, alphalin, dzmax, dphimax, pavg, nplates, manakov; steps: the oracle's ncycle at n = 256 and 4096 (measured
# on the oracle alone, asserted of the oracle before anything is compared with it); regime: what the case is there for
CASES = {
    "R1": dict(fls=[1, 0, 1, 0], L=1.5e3, alpha=0.0, dzmax=4e2, dph=5e-3, pavg=6.0, steps={256: 4, 4096: 5}),
    "R1m": dict(fls=[1, 0, 1, 0], L=1.5e3, alpha=0.0, dzmax=4e2, dph=5e-3, pavg=6.0, manakov=1, steps={256: 4, 4096: 4}),
    "R2": dict(fls=[1, 0, 1, 0], L=8e4, alpha=ALPHA, dzmax=2e4, dph=5e-3, pavg=0.05, steps={256: 4, 4096: 4},
               regime="loss", firstdz=2e4),
    "R3": dict(fls=[1, 0, 1, 0], L=6e4, alpha=ALPHA, dzmax=2e4, dph=0.3, pavg=6.0, steps={256: 3, 4096: 3}, regime="phase"),
    "R4": dict(fls=[1, 0, 1, 0], L=3e3, alpha=2.3e-3, dzmax=1e3, dph=5e-3, pavg=6.0, steps={256: 3, 4096: 3},
               regime="strongloss"),
    "R5": dict(fls=[1, 1, 1, 0], L=1.5e3, alpha=0.0, dzmax=4e2, dph=5e-3, pavg=6.0, nplates=7, steps={256: 4, 4096: 4}),
    "R6": dict(fls=[1, 1, 1, 0], L=1.5e3, alpha=ALPHA, dzmax=4e2, dph=5e-3, pavg=6.0, nplates=40, steps={256: 4, 4096: 4}),
    "R7": dict(fls=[1, 0, 1, 0], L=3e2, alpha=ALPHA, dzmax=4e2, dph=5e-3, pavg=0.5, steps={256: 1, 4096: 1}),
    "R8": dict(fls=[1, 1, 0, 0], L=3e3, alpha=ALPHA, dzmax=3e3, dph=math.inf, pavg=6.0, nplates=60, steps={256: 1, 4096: 1},
               regime="trunks"),
    "R9": dict(fls=[1, 1, 1, 0], L=3e3, alpha=0.0, dzmax=1.5e3, dph=0.5, pavg=6.0, nplates=120, steps={256: 2, 4096: 2},
               regime="trunks"),
    "R10": dict(fls=[1, 1, 1, 0], L=3e4, alpha=ALPHA, dzmax=1e4, dph=0.3, pavg=6.0, nplates=9, manakov=1,
                steps={256: 3, 4096: 3}, regime="phase"),
    "R11": dict(fls=[1, 0, 1, 0], L=3e3, alpha=ALPHA, dzmax=1e3, dph=math.inf, pavg=6.0, steps={256: 3, 4096: 3}),
    # R3 and R10 at a power where the phase rule, not dzmax, picks the first step: one radian at the peak.  At 0.3 rad and
    # below the Taylor form is still good to a^10 / 10! = 1.6e-12, inside either bar, so that a threshold set too high would
    # pass R3 and R10; at 1 rad the same term is 2.8e-7
    "R12": dict(fls=[1, 0, 1, 0], L=6e4, alpha=ALPHA, dzmax=2e4, dph=1.0, pavg=60.0, steps={256: 4, 4096: 5}, regime="radian"),
    "R13": dict(fls=[1, 1, 1, 0], L=3e4, alpha=ALPHA, dzmax=1e4, dph=1.0, pavg=120.0, nplates=9, manakov=1,
                steps={256: 6, 4096: 7}, regime="radian"),
}
# batches: one plan, every frame against the oracle on its own.  loss: the frames whose steps come from dl >= 1
BATCHES = {
    "B1": dict(fls=[1, 0, 1, 0], L=6e4, alpha=ALPHA, dzmax=2e4, dph=5e-3, pavg=[0.02, 0.5, 8.0, 0.1, 30.0],
               steps={256: [3, 7, 123, 3, 493], 4096: [3, 8, 161, 3, 654]}, loss=[0, 3]),
    "B2": dict(fls=[1, 0, 1, 0], L=3e3, alpha=ALPHA, dzmax=1e3, dph=5e-3, pavg=[6.0, 6.0, 3.0], zero=1,
               steps={256: [8, 3, 4], 4096: [9, 3, 5]}, loss=[]),
}
NT = {256: 16, 4096: 64, 65536: 64}          # 256: the small path; 4096: the smallest fused frame (p1 = 8); 65536: 256 x 256
LARGE = ["R1", "R3", "R5", "R9", "R10", "R12", "R13"]      # the cases that also run on the production geometry (GPU only)

# scalar plans through plx_scalar_ssfm: (fls) x (alphalin, dphimax, dzmax, steps)
SCALAR_GAM = [1.2e-6, 1.3e-6, 1.1e-6]
SCALAR_L = 1.5e3
SCALAR_FLS = {"g-sx": [1, 0, 1, 1], "g-s-": [1, 0, 1, 0], "g--x": [1, 0, 0, 1]}
# rule -> alphalin, dphimax, dzmax, steps, power of channel 0.  'phase' takes dzmax at every step, and at 6 (1 + k) mW
# (half of it in the one polarisation a scalar field is) its strongest channel turns by 0.010 rad in the first step:
# below FULL_RANGE.  'fullrange' is the same fibre at a hundred times the power and dphimax = 1: one radian in the first
# step, where the Taylor form would be wrong by 2.8e-7 (see R12)
SCALAR_RULES = {"lossless": (0.0, 5e-3, 4e2, 5, 6.0), "phase": (ALPHA, 0.3, 1e3, 2, 6.0), "fullrange": (ALPHA, 1.0, 1e3, {"g-sx": 3, "g-s-": 2, "g--x": 3}, 600.0)}


class Measured:
    """worst relative field error per case (printed by the tests: profiles/fibre_regimes.md is made from it)"""
    rows = {}

    @classmethod
    def put(cls, key, err):
        cls.rows[key] = max(err, cls.rows.get(key, 0.0))
        print("fibre regimes %s: worst field error / max|u| = %.2e" % (key, err))


def _field(n, pavg):
    return synth.pdm_qpsk_field(n // NT[n], NT[n], pavg, 2, 3)[:2]


def _plates(rng, nplates):
    """one frame's waveplates, drawn as _brf of tests/test_gpu_parity.py"""
    return tuple(np.ascontiguousarray(b) for b in (rng.random(nplates) * 2 * np.pi - np.pi, rng.random(nplates) * np.pi - np.pi / 2,
                                                   0.5 * np.arcsin(rng.random(nplates) * 2 - 1)))


def leff(alpha, dz):
    return dz if alpha == 0 else (1 - math.exp(-alpha * dz)) / alpha


_ORACLE = {}


def matrix_inputs(oracle, cid, n):
    """fields, tables, waveplates and the oracle's result of every frame of case / batch `cid` at n samples, computed once
    and shared (read-only) by the tests of both plan forms: dict(c, F, fields, brf, betat, db1, ref=[(fd, nc, ox, oy, dz)])"""
    key = (cid, n)
    if key in _ORACLE:
        return _ORACLE[key]
    c = dict(CASES[cid] if cid in CASES else BATCHES[cid])
    c.setdefault("nplates", 1)
    c.setdefault("manakov", 0)
    pavgs = c["pavg"] if isinstance(c["pavg"], list) else [c["pavg"]]
    F = len(pavgs)
    betat, db1 = _tables(n, NT[n], c["fls"], c["nplates"])
    fields = [_field(n, p) for p in pavgs]
    if c.get("zero") is not None:
        fields[c["zero"]] = tuple(np.zeros_like(v) for v in fields[c["zero"]])
    rng = np.random.default_rng(11)
    brf = [_plates(rng, c["nplates"]) if c["fls"][1] else (np.zeros(1),) * 3 for _ in range(F)]
    ref = []
    for f in range(F):
        rc, fd, nc, ox, oy, dz = oracle.matrix_ssfm(fields[f][0], fields[f][1], betat, db1, c["dzmax"], c["dph"], GAM, c["alpha"],
                                                    c["L"], c["nplates"], c["manakov"], c["fls"], *brf[f], return_dz=True)
        assert rc == 0
        ref.append((fd, nc, ox[:, 0], oy[:, 0], dz))
    for v in fields + brf:
        for a in v:
            a.setflags(write=False)
    _ORACLE[key] = dict(c=c, F=F, fields=fields, brf=brf, betat=betat, db1=db1, ref=ref)
    return _ORACLE[key]


def check_regime(cid, n, inp):
    """the case is where its name says, from the inputs and the oracle's steps alone; and the oracle's step counts are the
    recorded ones (n = 256 and 4096)"""
    c, ref = inp["c"], inp["ref"]
    want = c["steps"].get(n)
    if want is not None:
        assert [r[1] for r in ref] == (want if isinstance(want, list) else [want])
    pmax = [GAM[0] * (np.abs(fx) ** 2 + np.abs(fy) ** 2).max() for fx, fy in inp["fields"]]     # fiber.m:694-698 at z = 0
    if c.get("regime") == "loss" or c.get("loss"):
        for f in range(inp["F"]):
            lossy = c.get("regime") == "loss" or f in c["loss"]
            if c.get("zero") == f:
                continue
            assert (c["alpha"] * c["dph"] / pmax[f] >= 1) == lossy, f            # dl >= 1: the step is dzmax (fiber.m:700-702)
            if lossy:
                assert ref[f][0] == c["dzmax"]
    if "firstdz" in c:
        assert ref[0][0] == c["firstdz"]
    if c.get("regime") in ("phase", "radian"):    # Kerr phase at the frame's peak in the first step
        assert ref[0][1] > 1 and pmax[0] * leff(c["alpha"], ref[0][0]) >= (FULL_RANGE if c["regime"] == "phase" else 0.99)
    if c.get("regime") == "strongloss":           # a full step loses several dB
        assert 10 * math.log10(math.e) * c["alpha"] * ref[0][0] > 3.0
    if c.get("regime") == "trunks":               # the trunks of a step go through the phasor tables, and there are many
        lcorr = c["L"] / c["nplates"]
        tmax = math.ceil(c["dzmax"] / lcorr) + 2
        k = np.arange(n)
        m = np.where(k < n // 2, k, k - n)
        assert np.allclose(inp["db1"][:, 0], inp["db1"][1, 0] * m, rtol=0, atol=1e-14 * abs(inp["db1"][1, 0]) * n)   # (tables: db1 linear)
        assert tmax <= 64
        for dz in ref[0][4]:
            assert 30 < math.ceil(dz / lcorr) and math.ceil(dz / lcorr) + 1 <= tmax


def plan_run(be, inp, n, form, tune=None, log=0, replay=None):
    """one plan of the case's descriptor in the given form ('default': what plx_ssfm_create builds; 'three': the three-sweep
    step of PLX_SSFM_SHARE_DEVICE; 'notab': the default without the trunk phasor tables), all frames propagated in one call
    -> (info[8], firstdz [F], ncycle [F], ux [F, n], uy [F, n], logged steps per frame or None)"""
    c, F = inp["c"], inp["F"]
    d = _desc(n, 1, 1, c["fls"], c["L"], c["alpha"], GAM, c["dzmax"], c["dph"], inp["betat"], inp["db1"], nplates=c["nplates"],
              manakov=c["manakov"], frames=F)
    plan = C.c_void_p()
    if form == "notab":
        tune.setenv("PLX_SSFM_NO_PMD_TAB", "1")
    try:
        be.b.call("plx_ssfm_create_ex", C.byref(plan), C.byref(d), PLX_SSFM_SHARE_DEVICE if form == "three" else 0)
    finally:
        if form == "notab":
            tune.delenv("PLX_SSFM_NO_PMD_TAB")
    try:
        info = (C.c_int32 * 8)()
        be.b.call("plx_ssfm_info", plan, info)
        if c["fls"][1]:
            db0, th, ep = (np.ascontiguousarray(np.stack([b[k] for b in inp["brf"]])) for k in range(3))
            be.b.call("plx_ssfm_set_birefringence", plan, vp(db0), vp(th), vp(ep), F)
        if log:
            be.b.call("plx_ssfm_log_steps", plan, log)
        if replay is not None:
            assert F == 1
            rp = np.ascontiguousarray(replay, dtype=float)
            be.b.call("plx_ssfm_set_step_sequence", plan, vp(rp), rp.size)
        dux = be.up(np.stack([f[0] for f in inp["fields"]]))
        duy = be.up(np.stack([f[1] for f in inp["fields"]]))
        be.b.call("plx_ssfm_propagate_dev", plan, be.ptr(dux), be.ptr(duy), F, be.stream)
        gx, gy = be.down(dux), be.down(duy)
        fd, nc = np.zeros(F), np.zeros(F, np.int32)
        be.b.call("plx_ssfm_results", plan, F, vp(fd), vp(nc))
        steps = None
        if log:
            steps = []
            for f in range(F):
                s = np.zeros(log)
                be.b.call("plx_ssfm_step_sequence", plan, f, vp(s), log)
                steps.append(s[:nc[f]])
    finally:
        be.b.call("plx_ssfm_destroy", plan)
    return list(info), fd, nc, gx, gy, steps


def _err(g, o):
    return np.abs(g - o).max() / np.abs(o).max()


def check_form(info, n, form):
    """the plan is the one the test is about (plx_ssfm_info): the fused column sweep from 4096 samples up by default, three
    sweeps where asked for and on the small path; 65536 samples: the 256 x 256 split with the register-form rows k_row256r"""
    assert info[0] == (1 if (n >= 4096 and form in ("default", "notab")) else 0), (info, form)
    if n >= 4096:
        assert info[1] == 8
    if n == 65536:
        assert info[2] == 8 and info[6] == 64, info


def run_matrix(be, oracle, cid, n, bar, forms, tune=None):
    """case / batch `cid` at n samples in every plan form of `forms` against the oracle (and the forms against each other)"""
    inp = matrix_inputs(oracle, cid, n)
    c, F, ref = inp["c"], inp["F"], inp["ref"]
    check_regime(cid, n, inp)
    e0 = [sum(float((np.abs(v) ** 2).sum()) for v in fr) for fr in inp["fields"]]
    got = {}
    for form in forms:
        info, fd, nc, gx, gy, _ = plan_run(be, inp, n, form, tune)
        check_form(info, n, form)
        assert np.isfinite(gx).all() and np.isfinite(gy).all()
        worst = 0.0
        for f in range(F):
            ofd, onc, ox, oy, odz = ref[f]
            assert nc[f] == onc, (cid, form, f, nc[f], onc)        # a mismatch is a bug to find, not a tolerance to widen
            assert fd[f] == pytest.approx(ofd, rel=1e-12)
            if c.get("zero") == f:
                assert not ox.any() and not oy.any() and not gx[f].any() and not gy[f].any()    # stays exactly zero
                continue
            ex, ey = _err(gx[f], ox), _err(gy[f], oy)
            if max(ex, ey) >= bar and F == 1:
                ex, ey = _under_one_sequence(be, inp, n, form, tune, odz, oracle)
            worst = max(worst, ex, ey)
            assert ex < bar and ey < bar, (cid, form, f, ex, ey)
            if c["alpha"] == 0:                                    # every operator is unitary (not through the oracle)
                e1 = float((np.abs(gx[f]) ** 2).sum() + (np.abs(gy[f]) ** 2).sum())
                assert e1 == pytest.approx(e0[f], rel=1e-12)
        Measured.put("%s %s n=%d %s" % (type(be).__name__, cid, n, form), worst)
        got[form] = (gx, gy)
    names = list(got)
    for other in names[1:]:
        for f in range(F):
            if c.get("zero") == f:
                continue
            for p in range(2):
                assert np.abs(got[other][p][f] - got[names[0]][p][f]).max() < bar * np.abs(ref[f][2 + p]).max(), (cid, other, f)
    if "notab" in got:                                             # (the tables were in use: the switch selects other arithmetic)
        assert not np.array_equal(got["notab"][0], got["default"][0])
    return got


def _under_one_sequence(be, inp, n, form, tune, odz, oracle):
    """DESIGN.md, 'Conditioning of the step rule': the device's own steps are each within 1e-12 relative of the oracle's, and
    under the oracle's sequence the field is compared again -> (ex, ey)"""
    c = inp["c"]
    _, _, nc, _, _, steps = plan_run(be, inp, n, form, tune, log=len(odz) + 8)
    assert len(steps[0]) == len(odz)
    assert np.all(np.abs(steps[0] - odz) <= 1e-12 * np.abs(odz))
    _, _, nc, gx, gy, _ = plan_run(be, inp, n, form, tune, replay=odz)
    rc, fd, onc, ox, oy = oracle.matrix_ssfm(inp["fields"][0][0], inp["fields"][0][1], inp["betat"], inp["db1"], c["dzmax"], c["dph"],
                                             GAM, c["alpha"], c["L"], c["nplates"], c["manakov"], c["fls"], *inp["brf"][0], replay_dz=odz)
    assert rc == 0 and nc[0] == onc
    return _err(gx[0], ox[:, 0]), _err(gy[0], oy[:, 0])


# ---------------------------------------------------------------- scalar plans ---
def scalar_field(n, nfc, pavg0):
    return np.asfortranarray(np.stack([synth.pdm_qpsk_field(n // NT[n], NT[n], pavg0 * (1 + k), 2 + k, 5 + k)[0] for k in range(nfc)], 1))


def run_scalar(b, oracle, n, flag, rule, bar):
    """three 'sepfields' channels of powers pavg0 (1 + k) through plx_scalar_ssfm (host arrays on either back end)"""
    nfc, fls = 3, SCALAR_FLS[flag]
    alpha, dph, dzm, steps, pavg0 = SCALAR_RULES[rule]
    betat, db1 = _tables(n, NT[n], fls, 1, nfc)
    u = scalar_field(n, nfc, pavg0)
    ofd, onc, ou = oracle.scalar_ssfm(u, betat, dzm, dph, SCALAR_GAM, alpha, SCALAR_L, fls)
    assert onc == (steps[flag] if isinstance(steps, dict) else steps)
    pmax = max(g * (np.abs(u[:, k]) ** 2).max() for k, g in enumerate(SCALAR_GAM))
    print("scalar %s %s n=%d: Kerr phase of the first step at the peak %.3f rad" % (flag, rule, n, pmax * leff(alpha, ofd)))
    if rule == "fullrange":
        assert pmax * leff(alpha, ofd) >= 0.99
    d = _desc(n, nfc, 0, fls, SCALAR_L, alpha, SCALAR_GAM, dzm, dph, betat, db1)
    ur, ui = np.asfortranarray(u.real.copy()), np.asfortranarray(u.imag.copy())
    fd, nc = C.c_double(), C.c_int32()
    b.call("plx_release_all")
    try:
        b.call("plx_scalar_ssfm", vp(ur), vp(ui), C.byref(d), C.byref(fd), C.byref(nc))
    finally:
        b.call("plx_release_all")
    g = ur + 1j * ui
    assert nc.value == onc and fd.value == pytest.approx(ofd, rel=1e-12)
    e = _err(g, ou)
    Measured.put("scalar %s %s n=%d" % (flag, rule, n), e)
    assert e < bar
    if alpha == 0:
        assert float((np.abs(g) ** 2).sum()) == pytest.approx(float((np.abs(u) ** 2).sum()), rel=1e-12)


def adaptive_case():
    """the frame of test_emu_adaptive_ssfm (tests/test_emu_kernels.py): 512 samples, two channels with XPM"""
    n, nt, nfc, L = 512, 8, 2, 0.5e4
    fls = [1, 0, 1, 1]
    betat, db1 = _tables(n, nt, fls, 1, nfc)
    u = np.asfortranarray(np.stack([synth.pdm_qpsk_field(n // nt, nt, 6.0, 2 + k, 5 + k)[0] for k in range(nfc)], 1))
    return n, nfc, L, fls, betat, db1, u, [1.2e-6, 1.3e-6]


def run_adaptive_lossless(b, oracle, bar):
    """plx_scalar_ssfm_adaptive(tolflag = 2) in a lossless fibre: ncycle and nrej the oracle's (29 and 7).  (No energy check
    here: every accepted step ends in Richardson's combination 4/3 uh - 1/3 u (fiber.m:1003-1008), which is not unitary --
    the oracle's own energy moves by 1.0e-8 over these 29 steps.)"""
    n, nfc, L, fls, betat, db1, u, gam = adaptive_case()
    d = _desc(n, nfc, 0, fls, L, 0.0, gam, L, math.inf, betat, db1)
    ur, ui = np.asfortranarray(u.real.copy()), np.asfortranarray(u.imag.copy())
    fd, nc, nr = C.c_double(), C.c_int32(), C.c_int32()
    b.call("plx_release_all")
    try:
        b.call("plx_scalar_ssfm_adaptive", vp(ur), vp(ui), C.byref(d), 2, 1e-6, 0.9, C.byref(fd), C.byref(nc), C.byref(nr))
    finally:
        b.call("plx_release_all")
    ofd, onc, onrej, ou = oracle.scalar_a_ssfm(u, betat, L, math.inf, gam, 0.0, L, 1e-6, 0.9, fls)
    assert (onc, onrej) == (29, 7)
    assert (nc.value, nr.value) == (onc, onrej) and fd.value == pytest.approx(ofd, rel=1e-12)
    g = ur + 1j * ui
    e = _err(g, ou)
    Measured.put("adaptive lossless", e)
    assert e < bar


def check_dphiadapt_refused_lossless(b):
    """x.dphiadapt in a lossless fibre: the correction of fiber.m:607 is 0/0 (the reference returns a field of NaN); the
    library refuses, leaves the field alone and says why"""
    from polmux_amd._abi import PLX_ERR_REFERENCE, PolmuxError
    n, nfc, L, fls, betat, db1, u, gam = adaptive_case()
    d = _desc(n, nfc, 0, fls, L, 0.0, gam, L, 2e-2, betat, db1)
    ur, ui = np.asfortranarray(u.real.copy()), np.asfortranarray(u.imag.copy())
    fd, nc, nr = C.c_double(), C.c_int32(), C.c_int32()
    with pytest.raises(PolmuxError, match="fiber.m:607") as ei:
        b.call("plx_scalar_ssfm_adaptive", vp(ur), vp(ui), C.byref(d), 1, 1e-6, 0.9, C.byref(fd), C.byref(nc), C.byref(nr))
    assert ei.value.code == PLX_ERR_REFERENCE
    assert np.array_equal(ur + 1j * ui, u)
