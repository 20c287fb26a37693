"""The fibre propagator away from the suite's one operating point on the MI355X: the shipped library on device tensors against
the oracle, with the cases and checks of tests/fibre_regimes_ref.py (the emulated form is tests/test_emu_fibre_regimes.py).
What the emulator cannot show is the gfx950 build itself in these regimes: the device log / exp of the out-of-line step
controller at alphalin = 0 and at dl >= 1, the full-range sincos through the exchange buffer, the LDS copy of the control
record, and the 256 x 256 production geometry (k_colx16 + k_row256r), which the emulator does not run fused."""
import numpy as np
import pytest

from tests import fibre_regimes_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from polmux_amd import _abi
    b = _abi.get()
    assert b.path.endswith("polmux_amd/lib/libpolmux_hip.so")
    return R.Dev(b)


def _forms(cid, n):
    forms = ["default"] + (["three"] if n >= 4096 else [])
    return forms + (["notab"] if R.CASES.get(cid, {}).get("regime") == "trunks" else [])


@pytest.mark.parametrize("cid,n", [(c, n) for n in (256, 4096) for c in R.CASES] + [(c, 65536) for c in R.LARGE])
def test_gpu_fibre_regime(be, oracle, tune, cid, n):
    """one frame per regime: ncycle, first step (1e-12) and field (1e-9) against the oracle; fused and three-sweep plans of one
    case within the same bar of each other; lossless cases conserve the energy to 1e-12"""
    R.run_matrix(be, oracle, cid, n, R.GPU_BAR, _forms(cid, n), tune)


@pytest.mark.parametrize("bid,n", [("B1", 256), ("B1", 4096), ("B2", 256), ("B2", 4096), ("B2", 65536)])
def test_gpu_fibre_regime_batch(be, oracle, bid, n):
    """one plan, five frames in different regimes (two of them on dl >= 1) or three with an all-zero one: every frame against
    the oracle on its own; the zero frame stays exactly zero"""
    R.run_matrix(be, oracle, bid, n, R.GPU_BAR, _forms(bid, n))


@pytest.mark.parametrize("rule", list(R.SCALAR_RULES))
@pytest.mark.parametrize("flag", list(R.SCALAR_FLS))
@pytest.mark.parametrize("n", [256, 4096])
def test_gpu_scalar_regime(be, oracle, n, flag, rule):
    R.run_scalar(be.b, oracle, n, flag, rule, R.GPU_BAR)


def test_gpu_adaptive_step_lossless(be, oracle):
    R.run_adaptive_lossless(be.b, oracle, R.GPU_BAR)


def test_gpu_dphiadapt_refused_in_a_lossless_fibre(be):
    """through the C ABI, and through fiber(): the library's error is fiber()'s exception and the field is left alone"""
    import polmux_amd as px
    from polmux_amd import synth
    from polmux_amd._abi import PLX_ERR_REFERENCE, PolmuxError
    from polmux_amd.gstate import GSTATE, to_host_field
    R.check_dphiadapt_refused_lossless(be.b)
    px.reset_all(64, 16, 1)
    GSTATE.SYMBOLRATE = 28.0
    px.lasersource(1.5, 1550.0)
    px.create_field("sepfields", synth.pdm_qpsk_field(64, 16, 3.0)[0], None, dict(power="average"))
    u0 = to_host_field(GSTATE.FIELDX)
    x = dict(length=1e3, alphadB=0.0, aeff=80.0, n2=2.7e-20, disp=17.0, slope=0.0, ltol=1e-6, dphiadapt=True, dphimax=2e-2, dzmax=5e2)
    x["lambda"] = 1550.0
    with pytest.raises(PolmuxError, match="fiber.m:607") as ei:
        px.fiber(x, "g-s-")
    assert ei.value.code == PLX_ERR_REFERENCE
    assert np.array_equal(to_host_field(GSTATE.FIELDX), u0)
