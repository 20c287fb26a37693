"""The ASE / receiver-noise generator (plx_ampliflat_dev), the coherent front end at batch width (plx_front_run_dev,
plx_front_run_lo_dev) and plx_pick_dev under the host emulator: the cases of tests/noise_front_ref.py, which
tests/test_gpu_noise_front.py runs through the shipped library, and the statistics of the restated noise streams."""
import pytest

from tests import noise_front_ref as ref


@pytest.fixture(scope="module")
def be():
    from tests import _emu
    return ref.Host(_emu.binding())


# ---------------------------------------------------------------- A: the draws ---
@pytest.mark.parametrize("nfc", [33, 32, 31])
def test_emu_ampliflat_draws_sigma_table(be, nfc):
    ref.check_a1_a2(be, nfc)


def test_emu_ampliflat_draws_second_grid_pass_null_keys(be):
    ref.check_a3(be)


def test_emu_ampliflat_draws_alone_or_in_a_batch(be):
    ref.check_a4(be)


def test_emu_ampliflat_one_polarisation_null_arguments(be):
    ref.check_a5(be)


def test_emu_ampliflat_injected_noise_layout(be):
    ref.check_a6(be)


def test_emu_ampliflat_receiver_noise_call(be):
    ref.check_a7(be)


def test_restated_noise_streams_are_standard_normal_and_independent():
    """Mean, variance, skewness, excess kurtosis, lag-1 autocorrelation and every pairwise correlation of both quadratures of
    five streams that differ in channel, polarisation, key and high key word, N = 2^17 each: all within 4 standard errors.
    On the restatement alone: the device equals it draw for draw by the tests above and in tests/test_gpu_noise_front.py."""
    d = ref.distribution()
    for k, v in d.items():
        ref.Measured.put("numpy", "distribution", k + ", standard errors", v)
    assert all(v < 4.0 for v in d.values()), d


# ----------------------------------------------------------- B: the front end ---
def test_emu_front_amplitude_ladder_then_smaller_batch(be):
    ref.check_b1_b2(be)


def test_emu_front_single_polarisation_lo_table(be):
    ref.check_b3(be)


@pytest.mark.parametrize("r,ntaps", ref.B4_FIRS)
def test_emu_front_asymmetric_fir_and_large_shifts(be, r, ntaps):
    ref.check_b4(be, r, ntaps)


def test_emu_front_lo_phase_per_frame(be):
    ref.check_b5(be)


@pytest.mark.parametrize("bits", [1, 30])
def test_emu_front_adc_level_count_ends(be, bits):
    ref.check_b6(be, bits)


# ---------------------------------------------------------------- C: the pick ---
def test_emu_pick_dev_offset_stride_pitch(be):
    ref.check_pick_dev(be)
