"""The fibre propagator away from the suite's one operating point, kernel sources under the host emulator against the oracle:
the cases and the checks are tests/fibre_regimes_ref.py's.  256 samples take the small path, 4096 the fused column sweep
(and, asked for, the three-sweep step); the 256 x 256 geometry runs on the GPU only (tests/test_gpu_fibre_regimes.py)."""
import pytest

from tests import fibre_regimes_ref as R


@pytest.fixture(scope="module")
def be():
    from tests import _emu
    return R.Host(_emu.binding())


def _forms(cid, n):
    forms = ["default"] + (["three"] if n >= 4096 else [])
    return forms + (["notab"] if R.CASES.get(cid, {}).get("regime") == "trunks" else [])


@pytest.mark.parametrize("n", [256, 4096])
@pytest.mark.parametrize("cid", list(R.CASES))
def test_emu_fibre_regime(be, oracle, tune, cid, n):
    """one frame per regime (lossless, loss-limited step, radians of Kerr phase per step, a step of several dB, many trunks
    through the phasor tables, dzmax > L, dphimax = inf): ncycle, first step and field against the oracle, in every plan form"""
    R.run_matrix(be, oracle, cid, n, R.EMU_BAR, _forms(cid, n), tune)


@pytest.mark.parametrize("n", [256, 4096])
@pytest.mark.parametrize("bid", list(R.BATCHES))
def test_emu_fibre_regime_batch(be, oracle, bid, n):
    """one plan, frames in different regimes (B1: two of five on dl >= 1, 3 to 654 steps) or one of them all zero (B2: Pmax = 0,
    leffn = inf; it stays exactly zero): every frame against the oracle on its own.  (B1 is the slow one here: 654 lock-step
    steps of the emulated fused sweep at n = 4096, and as many of three sweeps: about two minutes.)"""
    R.run_matrix(be, oracle, bid, n, R.EMU_BAR, _forms(bid, n))


@pytest.mark.parametrize("rule", list(R.SCALAR_RULES))
@pytest.mark.parametrize("flag", list(R.SCALAR_FLS))
@pytest.mark.parametrize("n", [256, 4096])
def test_emu_scalar_regime(be, oracle, n, flag, rule):
    """a three-channel scalar plan (SPM and XPM, each alone and together) in a lossless fibre, at dphimax = 0.3 and at one radian
    per step"""
    R.run_scalar(be.b, oracle, n, flag, rule, R.EMU_BAR)


def test_emu_adaptive_step_lossless(be, oracle):
    R.run_adaptive_lossless(be.b, oracle, R.EMU_BAR)


def test_emu_dphiadapt_refused_in_a_lossless_fibre(be):
    R.check_dphiadapt_refused_lossless(be.b)
