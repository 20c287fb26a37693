"""The host side of pipeline.HotPath: every option is refused by check_config before anything is created, the per-frame
keys have one home (frame_keys), and a constructor that fails half way releases the plans it has made.  The CPU tests use
no library; the GPU tests create plans and launch nothing."""
import re

import numpy as np
import pytest

from polmux_amd import _abi, pipeline
from polmux_amd.pipeline import HotPath, HotPathConfig, check_config, frame_keys
from tests.test_tx_filter import MALFORMED

SMALL = dict(nsymb=64, nt=16, pavg_mw=4.0, length=4e4, cma_mu=1 / 300, freqavg=20, dphimax=2e-2)

# (options, what the message names, does check_config see it -- or only the host steps of the constructor behind it)
BAD = [(dict(frontend="heterodyne"), "frontend must be", True),
       (dict(equaliser="mlse"), "equaliser must be", True),
       (dict(decoding="gray"), "decoding must be", True),
       (dict(xpm_dualpol="yes"), "xpm_dualpol must be", True),
       (dict(tx_linewidth=-1e-4), "tx_linewidth must be", True),
       (dict(lo_linewidth=float("nan")), "lo_linewidth must be", True),
       (dict(tx_linewidth=np.array([1e-4, 1e-4])), "tx_linewidth must be", True),
       (dict(equaliser="dbp", frontend="cohmix"), "needs frontend='pick'", True),
       (dict(equaliser="dbp", xpm_dualpol="manakov", nch=3, flag="gpsx", manakov="yes"), "no XPM backpropagation", True),
       (dict(nch=3, wdm_field="unique", chspacing=2.0), "samples per symbol is too small", False),   # 4 nm = 17.8 symbol rates > nt
       (dict(flag="gx"), "wrong flag", False)]


@pytest.fixture
def no_library(monkeypatch):
    """a machine without a GPU: whoever asks for the library has gone too far"""
    def get():
        raise AssertionError("the library was asked for before the options were checked")
    monkeypatch.setattr(_abi, "get", get)


@pytest.mark.parametrize("kw,match,in_check", BAD, ids=[b[1] for b in BAD])
def test_every_bad_option_is_refused_before_anything_is_created(no_library, kw, match, in_check):
    cfg = HotPathConfig(**dict(SMALL, **kw))
    if in_check:
        with pytest.raises(ValueError, match=match):
            check_config(cfg)
    else:
        assert check_config(cfg) == (cfg.wdm_field == "unique", False, False)
    with pytest.raises(ValueError, match=match):
        HotPath(cfg, 1)


def test_check_config_returns_what_the_constructor_needs():
    assert check_config(HotPathConfig()) == (False, False, False)
    f = dict(ftype="ideal", bw=1.6)
    assert check_config(HotPathConfig(nch=3, wdm_field="unique", tx_data="random", tx_filter=f)) == (True, True, True)
    assert check_config(HotPathConfig(nch=3, wdm_field="unique", mux_filter=f)) == (True, False, False)
    assert check_config(HotPathConfig(tx_filter=f, frontend="cohmix", decoding="dqpsk")) == (False, False, True)


@pytest.mark.parametrize("mf", MALFORMED, ids=[repr(m)[:40] for m in MALFORMED])
def test_mux_filter_is_held_to_tx_filters_rules(no_library, mf):
    cfg = HotPathConfig(**dict(SMALL, nsymb=256, nch=3, wdm_field="unique", mux_filter=mf))
    for check in (pipeline.check_wdm_options, check_config, lambda c: HotPath(c, 1)):
        with pytest.raises(ValueError, match="mux_filter"):
            check(cfg)


def test_frame_keys():
    assert frame_keys(None, 3, "span_keys") is None
    want = np.array([0, 1, 2], dtype=np.int64)
    for keys in (range(3), [0, 1, 2], want, np.array([0, 9, 1, 9, 2, 9], dtype=np.int64)[::2], (k for k in range(3))):
        got = frame_keys(keys, 3, "span_keys")
        assert got.dtype == np.int64 and got.flags.c_contiguous and got.shape == (3,) and np.array_equal(got, want)
    assert frame_keys([(1 << 32) + 17], 1, "data_keys")[0] == (1 << 32) + 17
    assert frame_keys([], 0, "data_keys").shape == (0,)
    for what in ("data_keys", "span_keys", "noise_keys"):
        for n in (2, 4, 0):
            with pytest.raises(ValueError, match=r"%s must hold one key per frame \(3\), not %d" % (what, n)):
                frame_keys(list(range(n)), 3, what)


def test_one_master_seed():
    from tests.test_tx_random import SEED
    assert pipeline.MASTER_SEED == SEED == 20260101


# ------------------------------------------------------------------------------ on the MI355X ---
class _Recorder:
    """the real binding behind a proxy that writes down every call (plans made and destroyed with their handles) and
    itself refuses the call named `fail` -- the GPU is not asked to fail"""

    def __init__(self, real, fail=None):
        self.real, self.fail, self.calls, self.made, self.gone = real, fail, [], [], []

    def call(self, name, *args):
        self.calls.append(name)
        if name == self.fail:
            raise _abi.PolmuxError(_abi.PLX_ERR_HIP, "%s: refused by the test" % name)
        rc = self.real.call(name, *args)
        if "_create" in name:
            self.made.append((re.sub("_create.*", "", name), args[0]._obj.value))
        elif name.endswith("_destroy"):
            self.gone.append((name[:-len("_destroy")], getattr(args[0], "value", args[0])))
        return rc

    def __getattr__(self, name):
        return getattr(self.real, name)


@pytest.fixture
def recorder(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    rec = _Recorder(_abi.get())
    monkeypatch.setattr(_abi, "get", lambda: rec)
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("fail,kw,kinds", [("plx_dsp_create", {}, ["plx_ssfm", "plx_cde"]),
                                           ("plx_filter_create", dict(nsymb=256, nch=3, wdm_field="unique"),
                                            ["plx_ssfm", "plx_cde", "plx_dsp"])])
def test_a_failing_constructor_releases_its_plans(recorder, fail, kw, kinds):
    recorder.fail = fail
    with pytest.raises(_abi.PolmuxError, match="refused by the test"):
        HotPath(HotPathConfig(**dict(SMALL, **kw)), 2)
    assert [k for k, _ in recorder.made] == kinds and all(h for _, h in recorder.made)
    assert sorted(recorder.gone) == sorted(recorder.made)              # each once, with the handle that was created
    assert recorder.calls[-len(kinds):] == [k + "_destroy" for k in kinds]   # ... and nothing after the failure but that


@pytest.mark.gpu
def test_close_is_idempotent_and_releases_everything_once(recorder):
    hp = HotPath(HotPathConfig(**dict(SMALL, nsymb=256, nch=3, wdm_field="unique")), 2)
    hp.close()
    hp.close()
    assert sorted(recorder.gone) == sorted(recorder.made) and len(recorder.made) == 4


@pytest.mark.gpu
def test_wrong_length_keys_are_refused_before_any_launch(recorder):
    for extra, what in ((dict(nspans=2, span_nf_db=5), "span_keys"), (dict(tx_linewidth=1e-4), "span_keys"),
                        (dict(lo_linewidth=1e-4), "noise_keys")):
        hp = HotPath(HotPathConfig(**dict(SMALL, **extra)), 2)
        try:
            ux, uy = hp.make_batch(2)
            before = list(recorder.calls)
            with pytest.raises(ValueError, match=r"span_keys must hold one key per frame \(2\), not 1"):
                hp.fibre(ux, uy, span_keys=[0])
            with pytest.raises(ValueError, match=r"span_keys must hold one key per frame \(2\), not 3"):
                hp.fibre(ux, uy, span_keys=[0, 1, 2])
            with pytest.raises(ValueError, match=r"noise_keys must hold one key per frame \(2\), not 1"):
                hp.receive(ux, uy, noise_sigma=0.1, noise_seed=1, noise_keys=[0])
            assert recorder.calls == before, what
        finally:
            hp.close()
