"""The two kernels of the per-channel 'sepfields' receiver (plx_pick_wdm_dev, plx_cde_create_wdm) under
the host emulator: the pick against numpy's gather and the CDE with a table per channel against one-table plans, both bit for
bit, and the error returns."""
import pytest

from tests import wdm_rx_ref


@pytest.fixture(scope="module")
def be():
    from tests import _emu
    return wdm_rx_ref.Host(_emu.binding())


@pytest.mark.parametrize("nfft,nch,F", [(256, 1, 3), (256, 3, 3), (256, 64, 2), (4096, 5, 2)])
def test_emu_pick_wdm_against_numpy(be, nfft, nch, F):
    """rx[cf][p][i] = scale u_p[cf][(i stride + delay[c]) mod nfft] against numpy's gather at strides 1, 2 and 32 with
    n_out stride = nfft, delays of both signs that include 0, +-1 and +-(nfft - 1), the output NaN first and one channel-frame
    longer than the call may write.  Bit-exact: a copy times one scale.  All-zero delays equal the two plx_pick_dev calls the
    launch replaces, and delay d equals np.roll(delay 0, -d) before the stride (the sign)."""
    wdm_rx_ref.check_pick(be, nfft, nch, F, (1, 2, 32))


def test_emu_pick_wdm_argument_errors(be):
    wdm_rx_ref.check_pick_errors(be)


@pytest.mark.parametrize("N,L,nx", [(4, 2, 13), (256, 128, 643), (2048, 1024, 5123)])
def test_emu_cde_per_channel_tables(be, N, L, nx):
    """Random unit-modulus tables, nch = 3, rows_per_channel = 2, 12 rows (the channel index wraps), nx no multiple of L, at
    the smallest FFT, an LDS-staged table and a table read from global memory: every row equals the same row through a
    one-table plx_cde_create plan built from that row's table, bit for bit."""
    assert nx % L != 0
    wdm_rx_ref.check_cde_tables(be, N, L, nx, 3, 2, 12)


def test_emu_cde_one_table_is_plx_cde_create(be):
    """nch = 1 (any rows_per_channel): the plan of plx_cde_create, bit for bit"""
    wdm_rx_ref.check_cde_tables(be, 256, 128, 643, 1, 2, 5)


def test_emu_cde_create_wdm_argument_errors(be):
    wdm_rx_ref.check_cde_errors(be)
