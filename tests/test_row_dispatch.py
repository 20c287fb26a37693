"""Which row pass a plan builds (the resolver of ssfm_plan.hip), pinned for every frame length 2^8 ... 2^20 over scalar, dual
and dual-with-PMD plans (a linear db1: the trunk phasor tables), at the default tuning and under each single-field override
the suite uses.  Plans are created and asked (plx_ssfm_info); nothing is launched.  An entry is (info[1], info[2], info[6],
info[7]) = (log2 N1, log2 N2, row-pass workgroup size, row-pass form), or the error a refused creation reports.  The
tables are literals: a change of the dispatch has to change them knowingly.  info[0], info[3] and info[4] are not pinned
(occupancy differs between the emulator and the GPU)."""
import ctypes as C

import numpy as np
import pytest

from polmux_amd import _abi
from polmux_amd._abi import SsfmDesc

LOGS = range(8, 21)
KINDS = ("scalar", "dual", "pmd")
UNSUPPORTED = "PLX_ERR_UNSUPPORTED"
OVERRIDES = [{"rowr": 0}, {"rowsm": 2}, {"rowg_split": 0}, {"row256_split": 0}, {"row4k_split": 0}, {"no_row_split": 1},
             {"short_rows": 1}, {"no_pmd_tab": 1}]

# EXPECTED[tuning][kind][log2 nfft - 8]
EXPECTED = {
    "default": {
        "scalar": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 64, 2), (8, 6, 64, 2), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "dual": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "pmd": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 512, 0)],
    },
    "rowr=0": {
        "scalar": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 128, 0), (8, 9, 128, 0), (8, 10, 128, 0), (8, 11, 256, 0), (8, 12, 256, 1)],
        "dual": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 128, 0), (8, 9, 128, 0), (8, 10, 256, 0), (8, 11, 256, 1), (8, 12, 256, 1)],
        "pmd": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 128, 0), (8, 9, 128, 0), (8, 10, 256, 0), (8, 11, 256, 1), (8, 12, 512, 0)],
    },
    "rowsm=2": {
        "scalar": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 64, 2), (8, 6, 64, 2), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "dual": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 64, 2), (8, 6, 64, 2), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "pmd": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 512, 0)],
    },
    "rowg_split=0": {
        "scalar": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 64, 2), (8, 6, 64, 2), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "dual": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "pmd": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 512, 0)],
    },
    "row256_split=0": {
        "scalar": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 64, 2), (8, 6, 64, 2), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "dual": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "pmd": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 512, 0)],
    },
    "row4k_split=0": {
        "scalar": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 64, 2), (8, 6, 64, 2), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "dual": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "pmd": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 512, 0)],
    },
    "no_row_split=1": {
        "scalar": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 64, 2), (8, 6, 64, 2), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (9, 11, 256, 2)],
        "dual": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (9, 11, 256, 2)],
        "pmd": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (9, 11, 256, 2)],
    },
    "short_rows=1": {
        "scalar": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 64, 2), (8, 6, 64, 2), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (9, 11, 256, 2)],
        "dual": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (9, 11, 256, 2)],
        "pmd": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (9, 11, 256, 2)],
    },
    "no_pmd_tab=1": {
        "scalar": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 64, 2), (8, 6, 64, 2), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "dual": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 64, 2), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 256, 1)],
        "pmd": [(4, 4, 128, 0), (5, 4, 128, 0), (6, 4, 128, 0), (7, 4, 128, 0), (8, 4, 128, 0), (8, 5, 128, 0), (8, 6, 128, 0), (8, 7, 128, 0), (8, 8, 64, 0), (8, 9, 256, 2), (8, 10, 256, 2), (8, 11, 256, 2), (8, 12, 512, 0)],
    },
}


def _key(fields):
    return ",".join("%s=%d" % kv for kv in sorted(fields.items())) or "default"


def _desc(lg, kind):
    n = 1 << lg
    d = SsfmDesc()
    d.nfft, d.nfc, d.dual_pol, d.max_frames = n, 1, int(kind != "scalar"), 1
    for i, f in enumerate([1, int(kind == "pmd"), 1, 0]):
        d.fls[i] = f
    d.dzmaxt, d.dphimaxt, d.alphalin, d.length, d.nplates, d.manakov = 1e3, 5e-3, 4.6e-5, 1e4, 4, 0
    m = np.fft.fftfreq(n, 1.0 / n)                         # the signed frequency index: db1 linear in it (fiber.m:358)
    d._keep = (np.array([1.3e-6]), np.zeros(n), 0.01 * m)
    d.gam, d.betat, d.db1 = (a.ctypes.data for a in d._keep)
    return d


def observe(lib, lg, kind, fields):
    d = _desc(lg, kind)
    tuning = lib.tuning(**fields)
    plan = C.c_void_p()
    rc = lib.lib.plx_ssfm_create_tuned(C.byref(plan), C.byref(d), 0, C.byref(tuning))
    if rc == _abi.PLX_ERR_UNSUPPORTED:
        return UNSUPPORTED
    assert rc == _abi.PLX_OK, lib.last_error()
    info = (C.c_int32 * 8)()
    try:
        lib.call("plx_ssfm_info", plan, info)
    finally:
        lib.call("plx_ssfm_destroy", plan)
    return (info[1], info[2], info[6], info[7])


def _check(lib, fields):
    want = EXPECTED[_key(fields)]
    got = {kind: [observe(lib, lg, kind, fields) for lg in LOGS] for kind in KINDS}
    for kind in KINDS:
        for lg, g, w in zip(LOGS, got[kind], want[kind]):
            assert g == w, "%s plan of 2^%d samples, tuning %s: %r, recorded %r" % (kind, lg, _key(fields), g, w)


@pytest.fixture(scope="module")
def emu():
    from tests import _emu
    return _emu.binding()


@pytest.mark.parametrize("fields", [{}] + OVERRIDES, ids=_key)
def test_row_dispatch_emulator_build(emu, fields):
    """every frame length and plan kind, at the default tuning and under each single-field override"""
    _check(emu, fields)


def test_row_dispatch_refuses_4096_point_rows_without_the_split(emu):
    """a refusal is behaviour too.  no_row_split alone never meets it (it also caps the rows at 2048 points: the (9, 11)
    entries above); with the 256-row tile forced as well, the dual plans of 2^20 samples are refused and the scalar one is not"""
    fields = {"no_row_split": 1, "p1": 8}
    assert observe(emu, 20, "scalar", fields) == (8, 12, 256, 1)
    assert observe(emu, 20, "dual", fields) == UNSUPPORTED
    assert observe(emu, 20, "pmd", fields) == UNSUPPORTED


@pytest.mark.gpu
def test_row_dispatch_gpu_build():
    """the library the product loads resolves the same row pass at the default tuning"""
    _check(_abi.get(), {})
