"""The ASE / receiver-noise generator (plx_ampliflat_dev), the coherent front end at batch width (plx_front_run_dev,
plx_front_run_lo_dev) and plx_pick_dev on the MI355X through the shipped library: the cases of tests/noise_front_ref.py
(tests/test_emu_noise_front.py runs them under the host emulator), and the noise HotPath.receive and HotPath.fibre add --
what McCampaign draws -- against the restatement of the generator."""
import numpy as np
import pytest

from tests import noise_front_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from polmux_amd import _abi
    b = _abi.get()
    assert b.path.endswith("polmux_amd/lib/libpolmux_hip.so")
    return ref.Dev(b)


# ---------------------------------------------------------------- A: the draws ---
@pytest.mark.parametrize("nfc", [33, 32, 31])
def test_gpu_ampliflat_draws_sigma_table(be, nfc):
    ref.check_a1_a2(be, nfc)


def test_gpu_ampliflat_draws_second_grid_pass_null_keys(be):
    ref.check_a3(be)


def test_gpu_ampliflat_draws_alone_or_in_a_batch(be):
    ref.check_a4(be)


def test_gpu_ampliflat_one_polarisation_null_arguments(be):
    ref.check_a5(be)


def test_gpu_ampliflat_injected_noise_layout(be):
    ref.check_a6(be)


def test_gpu_ampliflat_receiver_noise_call(be):
    ref.check_a7(be)


# ------------------------------------------------- A: through the pipeline ---
def _plan(frames, **kw):
    from polmux_amd import pipeline
    return pipeline.HotPath(pipeline.HotPathConfig(**dict(dict(nsymb=64, nt=16, cma_mu=1 / 300, freqavg=20), **kw)),
                            max_frames=frames)


def _noise_bar(case, diff, want, sigma, field):
    """diff = (noisy - noiseless) against want = sigma * draws: DRAW_BAR relative to sigma + max|field|"""
    e = np.abs(diff - want).max() / (sigma + np.abs(field).max())
    ref.Measured.put("Dev", case, "added noise, of sigma + max|field|", e)
    assert diff.shape == want.shape and e <= ref.DRAW_BAR, (case, e)


@pytest.mark.parametrize("nch", [1, 3])
def test_gpu_receive_adds_the_restated_noise(be, nch):
    """hp.receive (pick front end) on the same fibre output without and with noise_sigma = 0.35, noise_seed = 5, noise_keys =
    [7, 2^33 + 7]: hp.rx differs by 0.35 ase_np(2 Lrx, nch, keys, 5): a channel-frame [X | Y] is one column of 2 Lrx samples,
    the nch channel-frames of a frame are the columns of its key."""
    import torch
    keys, sig = [7, 2 ** 33 + 7], 0.35
    kw = dict(variants=2) if nch == 1 else dict(variants=6, nch=3, wdm_field="sepfields", flag="g---")
    hp = _plan(2, **kw)
    try:
        ux, uy = hp.make_batch(2)
        hp.fibre(ux, uy)
        hp.receive(ux, uy)
        torch.cuda.synchronize()
        quiet = hp.rx[:2 * nch].cpu().numpy().copy()
        hp.receive(ux, uy, noise_sigma=sig, noise_seed=5, noise_keys=keys)
        torch.cuda.synchronize()
        noisy = hp.rx[:2 * nch].cpu().numpy().copy()
        L2 = 2 * hp.Lrx
    finally:
        hp.close()
    assert quiet.shape == (2 * nch, 2, L2 // 2) and len({quiet[k].tobytes() for k in range(2 * nch)}) == 2 * nch
    want = ref.ase_np(L2, nch, keys, 5, sig, 1, 0)[:, 0].reshape(2 * nch, 2, L2 // 2)
    _noise_bar("receive nch=%d" % nch, noisy - quiet, want, sig, quiet)


def _fibre(nspans, nf, keys, inject_first_zero=False):
    """the field after hp.fibre of two distinct frames with rx_amp (an amplifier behind every span) -> (x, y [2, nfft], sigma)"""
    import torch
    from polmux_amd.ampliflat import ase_sigma
    hp = _plan(2, variants=2, nspans=nspans, rx_amp=True, span_nf_db=nf)
    try:
        ux, uy = hp.make_batch(2)
        inj = None
        if inject_first_zero:     # the first amplifier adds sigma * 0, the second draws from the generator
            inj = [torch.zeros((2, 2, hp.cfg.nfft), dtype=torch.complex128, device=hp.dev), None]
        hp.fibre(ux, uy, span_keys=keys, inject_noise=inj)
        torch.cuda.synchronize()
        sigma = None if nf is None else float(ase_sigma(nf, np.exp(hp.alphalin * hp.cfg.length), 1)[0])
        return ux.cpu().numpy().copy(), uy.cpu().numpy().copy(), sigma
    finally:
        hp.close()


def test_gpu_fibre_amplifier_adds_the_restated_ase(be):
    """hp.fibre at nspans = 1, rx_amp = True, span_keys = [3, 9], without and with a noise figure: the fields differ by
    ase_sigma(...) ase_np(nfft, 1, keys, MASTER_SEED) on both polarisations.  Two spans, the first amplifier given zeros to
    inject: the difference from the noiseless run is the second amplifier's draw, under the seed MASTER_SEED + 7919 * 1."""
    from polmux_amd.pipeline import MASTER_SEED
    keys = [3, 9]
    for nspans in (1, 2):
        qx, qy, _ = _fibre(nspans, None, keys)
        nx, ny, sigma = _fibre(nspans, 5.0, keys, inject_first_zero=nspans == 2)
        assert sigma > 1e-4 * np.abs(qx).max() and not np.array_equal(qx[0], qx[1])
        want = ref.ase_np(qx.shape[-1], 1, keys, MASTER_SEED + 7919 * (nspans - 1), sigma)[:, :, 0]
        _noise_bar("fibre nspans=%d x" % nspans, nx - qx, want[:, 0], sigma, qx)
        _noise_bar("fibre nspans=%d y" % nspans, ny - qy, want[:, 1], sigma, qy)


# ----------------------------------------------------------- B: the front end ---
def test_gpu_front_amplitude_ladder_then_smaller_batch(be):
    ref.check_b1_b2(be)


def test_gpu_front_single_polarisation_lo_table(be):
    ref.check_b3(be)


@pytest.mark.parametrize("r,ntaps", ref.B4_FIRS)
def test_gpu_front_asymmetric_fir_and_large_shifts(be, r, ntaps):
    ref.check_b4(be, r, ntaps)


def test_gpu_front_lo_phase_per_frame(be):
    ref.check_b5(be)


@pytest.mark.parametrize("bits", [1, 30])
def test_gpu_front_adc_level_count_ends(be, bits):
    ref.check_b6(be, bits)


# ---------------------------------------------------------------- C: the pick ---
def test_gpu_pick_dev_offset_stride_pitch(be):
    ref.check_pick_dev(be)
