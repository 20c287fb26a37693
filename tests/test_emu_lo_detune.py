"""The two entry points of the LO frequency offset (plx_lo_detune_dev, plx_dsp_run_freq_dev) under the
host emulator: the cases of tests/lo_detune_ref.py, which tests/test_gpu_lo_detune.py runs through the shipped library."""
import pytest

from tests import lo_detune_ref as ref


@pytest.fixture(scope="module")
def be():
    from tests import _emu
    return ref.Host(_emu.binding())


@pytest.mark.parametrize("nfft,nfc,F", ref.KERNEL_CASES)
def test_emu_lo_detune_against_numpy(be, nfft, nfc, F):
    """theta = 2 pi (((b mod nfft) (n + 1)) mod nfft) / nfft against numpy at strides 1, 2 and 16 and either sign: the
    phasor on two polarisations and on one to 1e-12 of max |u|, d_phi written over NaN and accumulated onto a random buffer
    to 1e-12, d_bins_out exact; injected bins 0, +-1, +-(nfft/2 - 1), nfft/2 and beyond +-nfft; the pitch's tail and a guard
    channel-frame untouched; the generated draws (keys, a key beyond 32 bits, NULL keys, K = 0) equal to the host
    restatement synth.lo_detune_bins."""
    wu, wp = ref.check_kernel(be, nfft, nfc, F)
    print("nfft %d, nfc %d, F %d: phasor %.3g of max, phase %.3g rad" % (nfft, nfc, F, wu, wp))


def test_emu_lo_detune_argument_errors(be):
    ref.check_errors(be)


@pytest.mark.parametrize("Lin,freqavg", [(128, 500), (512, 5), (2048, 500)])
def test_emu_dsp_freq_turns(be, Lin, freqavg):
    """64, 256 and 1024 symbols of clean QPSK b bins off: d_turns == -b inside nsymb / 8, the aliased -(b - nsymb / 4) at
    nsymb / 8 + 1, zeros with freqavg = 0, and symbols bit-identical to plx_dsp_run_dev"""
    t = ref.check_freq(be, Lin, freqavg)
    print("Lin %d: turns %s" % (Lin, t.tolist()))
