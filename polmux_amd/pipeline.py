"""Batched, device-resident hot path: fibre -> (pick to 2 sps) -> CDE_OFDE ->
DspPdmCohQpsk (CMA + carrier recovery) -> decisions/error count.

This is what bench.py times and what the Monte-Carlo runner shards.  It is the
chain of Run_my_PDM_QPSK.m:122-193 minus the analogue front end
(receiver_cohmix + decimate, SURVEY 8f-1, "next"): the harness takes the
symbol-centre and mid-symbol samples of the propagated field directly.  Every
stage is a call into libpolmux_hip through the resident tier of the C ABI;
torch only owns the HBM buffers and the stream.
"""
import ctypes as C
import math
import warnings

import numpy as np

from . import _abi, synth
from .ampliflat import ase_sigma
from .fiber import fiber_tables, parse_flag
from .gstate import GSTATE, unique_field_shifts
from .rx import cde_transfer, dsp_params_struct
from .rxfront import myfilter

MASTER_SEED = 20260101      # of every counter-based generator: data, birefringence, ASE, laser phase, receiver noise


def dqpsk_expected(bits):
    """[4, nsymb] uint8: pat_decoder(pat, 'dqpsk') of the quaternary X and Y patterns behind bits [nsymb x 4] (the
    de Bruijn (first, second) pairs of synth.pdm_qpsk_field, pat = 2 first + second), ex20_coherent_polmux.m:124-125"""
    from . import patterns
    out = []
    for c in (0, 2):
        _, pm = patterns.pat_decoder(2 * bits[:, c].astype(int) + bits[:, c + 1].astype(int), "dqpsk")
        out += [pm[:, 0], pm[:, 1]]
    return np.ascontiguousarray(np.stack(out).astype(np.uint8))


def _u01(keys):
    """splitmix64 finaliser of uint64 keys -> doubles in [0, 1) (53 bits)."""
    with np.errstate(over="ignore"):
        z = keys + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


class HotPathConfig:
    """Run_my_PDM_QPSK-style parameters (BASELINE config C1 by default)."""

    def __init__(self, nsymb=1024, nt=64, symbolrate=28.0, pavg_mw=2.0, lam=1550.0, flag="g-s-",
                 length=8e4, alphadB=0.2, aeff=80.0, n2=2.7e-20, disp=17.0, slope=0.0, dphimax=5e-3, dzmax=2e4,
                 dgd=0.1, nplates=100, manakov="no", nspans=1, fft_length=256, cde_L=128, applypol=True,
                 polmethod="cma", cma_taps=7, cma_mu=1 / 6000, freqavg=500, phasavg=3, poworder=2,
                 frontend="pick", oftype="gauss", obw=1.9, oord=3, eftype="bessel5", ebw=0.65, eord=4, lopower=0.0,
                 adcbits=5, span_nf_db=None, rx_amp=False, variants=1, nch=1, chspacing=0.4, share_device=False,
                 equaliser="cde", dbp_steps=4, dbp_xi=1.0, tx_linewidth=0.0, lo_linewidth=0.0, decoding="rotation",
                 xpm_dualpol=None, wdm_field="sepfields", mux_filter=None, tx_data="debruijn",
                 tx_filter=None, wdm_receiver=None, lo_detuning=0.0, lo_detuning_spread=0.0):
        """frontend: 'pick' = 2-sps sampling supplied by the harness; 'cohmix' = the reference's own
        receiver_cohmix + ADC + decimate chain (RxPdmCohQpsk.m, Run_my_PDM_QPSK.m:52-73 defaults) on the device.
        nspans > 1: every span but the last is followed by an in-line flat amplifier restoring its loss
        (ampliflat(G,'gain'), noiseless or with noise figure span_nf_db and ASE keyed per frame); the last span's loss is
        undone in the receiver scale, as for one span -- unless rx_amp: then the last span is followed by an amplifier as
        well (gain = span loss, ASE from span_nf_db), the `fiber(...); ampliflat(Gerbio,'gain',ampli)` of
        ex20_coherent_polmux.m:147-148 / ex24_pmd.m:86-87, and the receiver sees the amplified, noise-loaded field.
        variants: number of distinct Tx waveforms (de Bruijn seed pairs s+1, s+2 as Run_my_PDM_QPSK.m:104-105 does per
        channel); frame f carries variant f % variants, with its own transmitted bits for the error count.
        nch > 1: a frame is a 'sepfields' WDM field of nch columns (create_field.m:17-18, ex10_wdm.m:9-11; BASELINE
        config[2]) chspacing nm apart around lam: the channels share the step length (fiber.m:694-698) and each keeps its
        own walk-off and gamma (fiber.m:326-328); channel c of frame f carries variant (f nch + c) % variants, and every
        channel has its own receiver (receiver_cohmix.m:104-125 picks the column).
        share_device: the fibre plan takes the barrier-free three-sweep step (plx_ssfm_create_ex, PLX_SSFM_SHARE_DEVICE): a
        frame that is the whole grid of the fused sweep (2^20 samples, 16 channels) can then propagate beside the receiver of
        the previous batch on another stream (the fused sweep would wait for its frame's workgroups to be co-resident).
        equaliser: 'cde' = CDE_OFDE (overlap-save dispersion compensation); 'dbp' = digital backpropagation of the nspans
        spans on the 2-sps samples (polmux_amd.dbp, plx_dbp_apply_dev) with dbp_steps uniform steps per span and dbp_xi
        of the nonlinearity, using the reference wavelength's D, S and gamma (WDM channel-frames as well); 'pick' front
        end only (the cohmix LO/ADC chain is not proportional to the field).
        tx_linewidth, lo_linewidth: laser linewidths normalised to the symbol rate (lasersource.m options.linewidth,
        receiver_cohmix.m x.lolinewidth): every realisation gets its own Wiener phase per laser, drawn on the device
        (plx_phase_noise_dev) and keyed by the realisation keys; one transmitter laser per channel feeds both
        polarisations, and the LO of a channel's receiver multiplies the hybrid's LO field (cohmix) or acts as exp(-i phi)
        on the picked 2-sps samples (pick).  0: no phase noise, nothing is launched.
        decoding: 'rotation' = errors_resolved's minimum over the pi/2 rotations and the polarisation swap; 'dqpsk' = the
        Monte-Carlo scripts' differential decoding of both patterns plus ex20's swap rule (errors_dqpsk); McCampaign counts
        with it.
        xpm_dualpol: None = the reference's behaviour (an 'x' flag on dual-polarisation 'sepfields' frames raises its
        "not yet implemented"); 'manakov' = cross-phase modulation between the nch channels in the Manakov form (DESIGN.md
        section 8c, PLX_SSFM_XPM_MANAKOV) with flag 'gpsx' / '-psx' / 'gp-x' / '-p-x' and manakov='yes'; not with
        equaliser='dbp', which has no XPM backpropagation.
        wdm_field: 'sepfields' = one column per channel (above); 'unique' = the frame is ONE dual-polarisation field carrying
        every channel at its carrier offset (create_field.m:165-199), which sees the whole Kerr nonlinearity of the comb
        (SPM, XPM and four-wave mixing) -- DESIGN.md section 8d: multiplexed on the device (plx_wdm_mux_dev), propagated by a
        one-column plan at the centre wavelength, and split back into channel-frames with the walk-off delay taken out
        (plx_wdm_select_dev) in front of the receivers; with the 'pick' front end every channel-frame then passes the
        optical filter (oftype, obw, oord), which isolates it from its neighbours.  Not with equaliser='dbp', not with
        xpm_dualpol.
        mux_filter: None, or dict(ftype=, bw=, ord=) -- the multiplexer's channel filter, 'unique' only: every Tx waveform
        is band-limited once on the host, ifft(fft(v) myfilter(ftype, FN, 0.5 bw, ord)) (bw two-sided, in symbol rates,
        like obw), and rescaled to pavg_mw.  None is the reference's create_field: nothing is filtered.
        tx_data: 'debruijn' = every frame carries one of `variants` de Bruijn waveforms synthesised once on the host;
        'random' = every realisation draws its own data on the device (plx_tx_qpsk_dev): make_batch
        generates the batch's fields, transmitted patterns and per-realisation power, keyed by its data_keys (channel c of a
        frame is counter word 2), and the receiver normalises each channel-frame by its own power and counts against its own
        patterns; HotPath.tx_bits_host states any realisation's data on the host.  variants = 1, no mux_filter, nt <= 64.
        tx_filter: None, or dict(ftype=, bw=[, ord=]) -- the transmitter's channel filter on the DEVICE (plx_tx_bandlimit_dev,
        DESIGN.md section 8f), with both tx_data and both wdm_field values and any nch: every channel-frame is band-limited,
        ifft(fft(v) myfilter(ftype, FN, 0.5 bw, ord)) (bw two-sided, in symbol rates: mux_filter's table), and rescaled to
        pavg_mw by its OWN mean power.  tx_data='random': on every batch, behind plx_tx_qpsk_dev on make_batch's stream and
        with no read-back; 'debruijn': on the `variants` waveforms once, when the plan is made.  The patterns, tx_power,
        rx_gain and power_mw are what they are without the filter.  Not together with mux_filter (the host route).  None:
        nothing is launched.
        wdm_receiver: None = every channel-frame of a 'sepfields' frame is picked from sample 0 and equalised with the ONE
        CDE response at lam and disp (the error counts of the outer channels of nch > 1 frames then mean nothing: the fibre
        gives each channel its own walk-off and its own beta2); 'channel' = every channel-frame is received at its own
        channel's delay (sepfields_walkoff of fiber_tables' b1: GSTATE.DELAY of fiber.m:366-368, taken out as
        RxPdmCohQpsk.m:130-151 does with x.delay = 'theory') and equalised with its own channel's dispersion (Dch of
        fiber.m:336 at GSTATE.LAMBDA[c]) -- DESIGN.md section 8g: one plx_pick_wdm_dev launch instead of the two plx_pick_dev
        calls, and a plx_cde_create_wdm plan.  The LO phase keeps being applied at the instants i nt/2: it is a Wiener
        process with stationary increments, so its statistics on the shifted samples are the same.  McCampaign then returns
        a count per channel-frame, [len(indices) * nch], as for 'unique'.  nch = 1: the delay is 0 and the table is the one
        of wdm_receiver=None, bit for bit.  'sepfields' with frontend='pick' and equaliser='cde' only.
        lo_detuning, lo_detuning_spread: the LO's frequency offset from its channel's carrier in Hz (receiver_cohmix.m
        x.lodetuning).  With minfreq = symbolrate 1e9 / nsymb, k0 = floor(lo_detuning / minfreq) (the
        reference's floor, :191-192, also for negative values) and K = floor(lo_detuning_spread / minfreq): the LO of every
        channel-frame sits k0 + d bins off, d uniform on -K .. K, drawn on the device (plx_lo_detune_dev) under the keys the
        LO's phase noise uses (noise_keys, or the frame index) and the channel -- a realisation's offset does not depend on
        batching or sharding; HotPath.lo_bins_host states it on the host.  The LO multiplies the hybrid's LO field (cohmix)
        or acts as exp(-i theta) on the picked 2-sps samples (pick); the frequency estimator of DspPdmCohQpsk follows it
        while |k0| + K < nsymb / 8, and HotPath.freq_turns reads its estimate out.  Not with equaliser='dbp'.  Both 0:
        nothing is launched."""
        self.__dict__.update(locals())
        del self.__dict__["self"]

    @property
    def nfft(self):
        return self.nsymb * self.nt


def _check_filter(name, f):
    """the raises of a channel-filter option `name` = dict(ftype=, bw=[, ord=]) (mux_filter, tx_filter)"""
    if not isinstance(f, dict) or "ftype" not in f or "bw" not in f or set(f) - {"ftype", "bw", "ord"}:
        raise ValueError("%s must be None or dict(ftype=..., bw=...[, ord=...])" % name)
    try:
        bw = float(f["bw"]) if np.ndim(f["bw"]) == 0 and not isinstance(f["bw"], (bool, str, bytes)) else math.nan
    except (TypeError, ValueError):
        bw = math.nan
    if not (math.isfinite(bw) and bw > 0):
        raise ValueError("%s: bw must be a finite scalar > 0 (two-sided, in symbol rates)" % name)
    if not isinstance(f["ftype"], str):
        raise ValueError("%s: ftype must be a filter name of myfilter" % name)


def check_wdm_options(cfg):
    """The raises of HotPathConfig's wdm_field / mux_filter (needs no GPU); returns True for a 'unique' field."""
    field, mf = cfg.wdm_field, cfg.mux_filter
    if not isinstance(field, str) or field not in ("sepfields", "unique"):
        raise ValueError("wdm_field must be 'sepfields' or 'unique'")
    if mf is not None:
        _check_filter("mux_filter", mf)
        if field == "sepfields":
            raise ValueError("mux_filter needs wdm_field='unique' (it would change the 'sepfields' frames)")
    if field == "unique":
        if cfg.equaliser == "dbp":
            raise ValueError("wdm_field='unique' has no digital backpropagation: not with equaliser='dbp'")
        if cfg.xpm_dualpol:
            raise ValueError("wdm_field='unique' carries the channels' cross-phase modulation in its one field: not with xpm_dualpol")
    return field == "unique"


def check_tx_filter(cfg):
    """The raises of HotPathConfig's tx_filter (needs no GPU); returns True when the device band-limit is asked for."""
    if cfg.tx_filter is None:
        return False
    _check_filter("tx_filter", cfg.tx_filter)
    if cfg.mux_filter is not None:
        raise ValueError("tx_filter is the device route of the channel filter and mux_filter the host route: not both")
    return True


def check_tx_options(cfg):
    """The raises of HotPathConfig's tx_data (needs no GPU); returns True for the device transmitter ('random')."""
    td = cfg.tx_data
    if not isinstance(td, str) or td not in ("debruijn", "random"):
        raise ValueError("tx_data must be 'debruijn' or 'random'")
    if td == "random":
        if int(cfg.variants) != 1:
            raise ValueError("tx_data='random' draws every frame's data itself: not with variants != 1")
        if cfg.mux_filter is not None:
            raise ValueError("tx_data='random' has no multiplexer filter (mux_filter is the host band-limit; tx_filter is the device one): "
                             "not with mux_filter")
        if cfg.nt > 64:
            raise ValueError("tx_data='random' needs nt <= 64 (the drive tables of plx_tx_qpsk_dev)")
    return td == "random"


def lo_detune_bins(cfg):
    """(k0, K): lo_detuning and lo_detuning_spread in bins of minfreq = symbolrate 1e9 / nsymb, both floored as
    receiver_cohmix.m:191-192 floors x.lodetuning (towards -inf: -0.5 bins is bin -1)"""
    minfreq = cfg.symbolrate * 1e9 / cfg.nsymb
    return math.floor(float(cfg.lo_detuning) / minfreq), math.floor(float(cfg.lo_detuning_spread) / minfreq)


def check_lo_detuning(cfg):
    """The raises and warnings of HotPathConfig's lo_detuning / lo_detuning_spread (needs no GPU); returns True when
    either is non-zero."""
    for name in ("lo_detuning", "lo_detuning_spread"):
        v = getattr(cfg, name)
        if isinstance(v, (bool, str, bytes)) or np.ndim(v) != 0 or not math.isfinite(float(v)):
            raise ValueError("%s must be a finite scalar (Hz)" % name)
    if float(cfg.lo_detuning_spread) < 0:
        raise ValueError("lo_detuning_spread must be >= 0 (Hz)")
    if not (float(cfg.lo_detuning) or float(cfg.lo_detuning_spread)):
        return False
    if cfg.equaliser == "dbp":
        raise ValueError("lo_detuning / lo_detuning_spread: not with equaliser='dbp' (backpropagating a displaced spectrum is "
                         "wrong, and no frequency estimator runs in front of DBP)")
    k0, K = lo_detune_bins(cfg)
    if 2 * K + 1 > cfg.nfft:
        raise ValueError("lo_detuning_spread: the 2 K + 1 = %d offsets do not fit the %d bins of a frame" % (2 * K + 1, cfg.nfft))
    if abs(k0) > 2 ** 30:
        raise ValueError("lo_detuning: more than 2^30 bins")
    if float(cfg.lo_detuning) and k0 == 0:       # receiver_cohmix.m:193-196
        warnings.warn("lo_detuning is below one frequency bin (symbolrate / nsymb): the LO detuning is set to 0 bins")
    if cfg.freqavg > 0 and abs(k0) + K >= cfg.nsymb / 8:
        warnings.warn("LO offsets up to %d bins reach the range of the QPSK frequency estimator, nsymb / 8 = %g bins: "
                      "beyond it the estimate aliases by nsymb / 4" % (abs(k0) + K, cfg.nsymb / 8))
    return True


def check_config(cfg):
    """Every raise of HotPathConfig's options (needs no GPU, no library, no torch); returns (unique, random, txfilt_on)."""
    unique, random, txfilt_on = check_wdm_options(cfg), check_tx_options(cfg), check_tx_filter(cfg)
    check_lo_detuning(cfg)
    if cfg.equaliser not in ("cde", "dbp"):
        raise ValueError("equaliser must be 'cde' or 'dbp'")
    if cfg.equaliser == "dbp" and cfg.frontend != "pick":
        raise ValueError("equaliser='dbp' needs frontend='pick' (the cohmix LO/ADC chain is not proportional to the field)")
    for name in ("tx_linewidth", "lo_linewidth"):
        v = getattr(cfg, name)
        if not (np.ndim(v) == 0 and math.isfinite(float(v)) and float(v) >= 0):
            raise ValueError("%s must be a finite scalar >= 0 (normalised to the symbol rate)" % name)
    if cfg.decoding not in ("rotation", "dqpsk"):
        raise ValueError("decoding must be 'rotation' or 'dqpsk'")
    if cfg.xpm_dualpol not in (None, "manakov"):
        raise ValueError("xpm_dualpol must be None or 'manakov'")
    if cfg.xpm_dualpol and cfg.equaliser == "dbp":
        raise ValueError("equaliser='dbp' has no XPM backpropagation: not with xpm_dualpol")
    if cfg.frontend not in ("pick", "cohmix"):
        raise ValueError("frontend must be 'pick' or 'cohmix'")
    if cfg.wdm_receiver is not None:
        if not isinstance(cfg.wdm_receiver, str) or cfg.wdm_receiver != "channel":
            raise ValueError("wdm_receiver must be None or 'channel'")
        if unique:
            raise ValueError("wdm_receiver='channel' is for 'sepfields' frames: wdm_field='unique' takes its walk-off out in "
                             "plx_wdm_select_dev")
        if cfg.frontend == "cohmix":
            raise ValueError("wdm_receiver='channel' needs frontend='pick' (the cohmix ADC/FIR gather takes one shift per "
                             "polarisation)")
        if cfg.equaliser == "dbp":
            raise ValueError("wdm_receiver='channel' needs equaliser='cde' (equaliser='dbp' has no per-channel betat)")
    return unique, random, txfilt_on


def frame_keys(keys, nframes, what):
    """None, or the keys as a contiguous int64 array of exactly nframes entries (the kernels read keys[f] of every frame)"""
    if keys is None:
        return None
    k = np.ascontiguousarray(keys if isinstance(keys, np.ndarray) else list(keys), dtype=np.int64).reshape(-1)
    if k.size != nframes:
        raise ValueError("%s must hold one key per frame (%d), not %d" % (what, nframes, k.size))
    return k


def wdm_walkoff(shifts, beta2, b30, total_length, symbolrate, dfn, nt):
    """Walk-off of the channels of a 'unique' field after total_length metres: (delay_symbols, delay).  Channel c sits at
    Om_c = -2 pi symbolrate dfn s_c (where plx_wdm_mux_dev put it: on an integer bin, not at its unrounded wavelength);
    delay_symbols = total_length symbolrate (beta2 Om_c + b30 Om_c^2 / 2) with the one-column beta2, b30 of fiber_tables;
    delay = MATLAB's round(delay_symbols nt) in samples: plx_wdm_select_dev reads the field at n + delay[c]."""
    om = -2 * math.pi * symbolrate * dfn * np.asarray(shifts, dtype=float)
    ds = total_length * symbolrate * (beta2 * om + 0.5 * b30 * om * om)
    v = ds * nt
    return ds, (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def sepfields_walkoff(b1, total_length, symbolrate, nt):
    """Walk-off of the channels of a 'sepfields' frame after total_length metres: (delay_symbols, delay).  b1 is
    fiber_tables(...)["b1"], the array whose omega beta1 term is in the fibre's betat; delay_symbols[c] = total_length
    symbolrate b1[c] (GSTATE.DELAY of fiber.m:367, summed over equal spans); delay = MATLAB's round(delay_symbols nt) in
    samples, half away from zero, with wdm_walkoff's sign: the receiver reads the field at n + delay[c]."""
    ds = float(total_length) * float(symbolrate) * np.atleast_1d(np.asarray(b1, dtype=float))
    v = ds * nt
    return ds, (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def wdm_cde_tables(N, fs, lam_nm, total_length, Dch, slope):
    """[nch, N] complex: channel c's CDE_OFDE response cde_transfer(N, fs, lam_nm[c] 1e-9, total_length, Dch[c] 1e-6,
    slope 1e-6), Dch = fiber_tables(...)["Dch"] (fiber.m:336): what plx_cde_create_wdm takes"""
    return np.ascontiguousarray(np.stack([cde_transfer(N, fs, float(l) * 1e-9, total_length, float(d) * 1e-6, slope * 1e-6)
                                          for l, d in zip(np.atleast_1d(lam_nm), np.atleast_1d(Dch))]))


def band_limit(vx, vy, h, pavg_mw):
    """the multiplexer's channel filter on one Tx waveform: ifft(fft(v) h), rescaled to the average power pavg_mw"""
    fx, fy = np.fft.ifft(np.fft.fft(vx) * h), np.fft.ifft(np.fft.fft(vy) * h)
    k = math.sqrt(pavg_mw / np.mean(np.abs(fx) ** 2 + np.abs(fy) ** 2))
    return fx * k, fy * k


class HotPath:
    def __init__(self, cfg, max_frames):
        self.unique, self.random, self.txfilt_on = check_config(cfg)
        self.lo_k0, self.lo_K = lo_detune_bins(cfg)      # the LO's offset in bins: k0 + a draw on -K .. K per channel-frame
        self.detune = bool(float(cfg.lo_detuning) or float(cfg.lo_detuning_spread))
        # every handle and optional component, so that close() can run on a half-built plan
        self.ssfm = self.cde = self.dsp = self.chfilt = self.txfilt = self.dbp = self.front = None
        self.cfg = cfg
        self.F = int(max_frames)
        nch = self.nch = int(cfg.nch)
        self.CF = self.F * nch                           # channel-frames: what the receiver's plans count
        self.nfc = 1 if self.unique else nch             # columns of the fibre plan: a 'unique' field is one
        self.power_mw = None                             # (the transmitter sets it, and GSTATE.POWER with it)
        self.bind_gstate()
        # --- host side of fiber(): flag, conversions (fiber.m:157-251); the host steps that can still raise ---
        x = {"length": cfg.length, "alphadB": cfg.alphadB, "aeff": cfg.aeff, "n2": cfg.n2, "lambda": cfg.lam,
             "disp": cfg.disp, "slope": cfg.slope, "dphimax": cfg.dphimax, "dzmax": min(cfg.dzmax, cfg.length)}
        self.fls, dphimaxt, dzmaxt = parse_flag(cfg.flag, self.nfc, x)
        if self.unique:    # the comb as one field: carrier offsets in bins (create_field.m:181-184; raises when NT is too small)
            self.wdm_shift = np.ascontiguousarray(unique_field_shifts(), dtype=np.int64)
        import torch
        self.torch = torch
        self.lib = _abi.get()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        try:
            t = self._build_fibre(x, dphimaxt, dzmaxt)
            self._build_tx()
            self._build_rx(t)
        except BaseException:
            self.close()
            raise

    def _filter_plan(self, h, nsig):
        """plx_filter_create: a plan that multiplies the spectra of up to nsig signals of nfft samples by the complex table h"""
        h = np.asarray(h, dtype=complex)
        hr, hi = np.ascontiguousarray(h.real), np.ascontiguousarray(h.imag)
        plan = C.c_void_p()
        self.lib.call("plx_filter_create", C.byref(plan), self.cfg.nfft, nsig, hr.ctypes.data, hi.ctypes.data)
        return plan

    def _build_fibre(self, x, dphimaxt, dzmaxt):
        """the fibre plan (fiber.m:274-362: tables, PMD draw); returns fiber_tables' dict"""
        cfg, nfc = self.cfg, self.nfc
        self.pmd = self.fls[1] == 1
        nplates = self.nplates = cfg.nplates if self.pmd else 1
        dgdrms = math.sqrt(3 * math.pi / 8) * cfg.dgd / math.sqrt(nplates) if self.pmd else 0.0   # fiber.m:277
        t = fiber_tables(x, self.fls, nfc, dgdrms)        # (one column: the centre wavelength lamc and its gamma, as fiber())
        self.alphalin = t["alphalin"]
        d = _abi.SsfmDesc()
        d.nfft, d.nfc, d.dual_pol, d.max_frames = cfg.nfft, nfc, 1, self.F
        for i in range(4):
            d.fls[i] = self.fls[i]
        d.dzmaxt, d.dphimaxt, d.alphalin, d.length = dzmaxt, dphimaxt, t["alphalin"], cfg.length
        d.nplates, d.manakov = nplates, int(str(cfg.manakov).lower() == "yes")
        self._keep = (np.ascontiguousarray(t["gam"]), t["betat"], t["db1"])
        d.gam, d.betat, d.db1 = (a.ctypes.data for a in self._keep)
        self.ssfm = C.c_void_p()
        self.lib.call("plx_ssfm_create_ex", C.byref(self.ssfm), C.byref(d), (_abi.PLX_SSFM_SHARE_DEVICE if cfg.share_device else 0)
                      | (_abi.PLX_SSFM_XPM_MANAKOV if cfg.xpm_dualpol else 0))
        self._profiling = False
        if self.pmd:   # Monte-Carlo style: an independent random birefringence draw per frame (fiber.m:274-276)
            self.set_random_pmd(range(self.F))
        return t

    def _build_tx(self):
        """the transmitter (host, once: Run_my_PDM_QPSK.m:101-117): waveforms, patterns, the device Tx filter, the drive tables"""
        torch, cfg, nch = self.torch, self.cfg, self.nch
        # the default waveform, and further ones (other de Bruijn seeds): heterogeneous batches whose frames differ in data
        maxseed = cfg.nsymb * (cfg.nsymb - 1) // 4
        seeds = [()] + [((2 + 2 * v) % maxseed, (3 + 2 * v) % maxseed) for v in range(1, max(1, int(cfg.variants)))]
        fields = [synth.pdm_qpsk_field(cfg.nsymb, cfg.nt, cfg.pavg_mw, *sd) for sd in seeds]
        self.bits, self.power_mw = fields[0][2:]
        assert all(abs(f[3] - self.power_mw) <= 1e-9 * self.power_mw for f in fields)   # de Bruijn sequences share their statistics
        GSTATE.POWER = np.full(nch, self.power_mw)
        self.pat = torch.from_numpy(np.ascontiguousarray(self.bits.T.astype(np.uint8))).to(self.dev)   # [4, nsymb]
        self.var_host = [f[:3] for f in fields]
        mf, tf = cfg.mux_filter, cfg.tx_filter
        if mf is not None:                               # the multiplexer's channel filter (host, once per plan)
            hmux = myfilter(mf["ftype"], GSTATE.FN, 0.5 * float(mf["bw"]), mf.get("ord"))
            self.var_host = [band_limit(vx, vy, hmux, cfg.pavg_mw) + (vb,) for vx, vy, vb in self.var_host]
        self.nvar = len(self.var_host)
        self._txfilt_work = self.tx_gain = None
        if self.txfilt_on:                               # the transmitter's channel filter (device)
            npairs = self.CF if self.random else self.nvar
            self.txfilt = self._filter_plan(myfilter(tf["ftype"], GSTATE.FN, 0.5 * float(tf["bw"]), tf.get("ord")), npairs)
            # tile partials of the power sum: the plan's, touched only on the stream make_batch runs on
            self._txfilt_work = torch.empty(npairs * (-(-cfg.nfft // 2048)), dtype=torch.float64, device=self.dev)
            if not self.random:                          # the V waveforms, once: tx_host / var_host hold what is read back
                dx = torch.from_numpy(np.stack([v[0] for v in self.var_host])).to(self.dev)
                dy = torch.from_numpy(np.stack([v[1] for v in self.var_host])).to(self.dev)
                self.lib.call("plx_tx_bandlimit_dev", self.txfilt, dx.data_ptr(), dy.data_ptr(), self.nvar, float(cfg.pavg_mw),
                              None, self._txfilt_work.data_ptr(), self.stream())
                hx, hy = dx.cpu().numpy(), dy.cpu().numpy()
                self.var_host = [(hx[v], hy[v], self.var_host[v][2]) for v in range(self.nvar)]
                self.lib.call("plx_filter_destroy", self.txfilt)
                self.txfilt = self._txfilt_work = None
        self.tx_host = self.var_host[0][:2]
        self.tx = torch.from_numpy(np.stack(self.tx_host)).to(self.dev)      # [2, n]
        self.per_frame = self.nvar > 1 or self.random    # every channel-frame is counted against its own patterns
        if self.random:                                  # the device transmitter: its tables; make_batch fills the rest
            self.tx_drive = synth.qpsk_drive_tables(cfg.nt)
            self.pat_frames = self.dpat_frames = self.tx_power = None
        self._batch, self.rx_gain = [], None             # the current batch's own tensors, its per-frame receiver scale (make_batch)
        if self.nvar > 1:
            self.tx_var = torch.from_numpy(np.stack([np.stack([v[0], v[1]]) for v in self.var_host])).to(self.dev)   # [V, 2, n]
            pv = np.stack([np.ascontiguousarray(v[2].T.astype(np.uint8)) for v in self.var_host])               # [V, 4, nsymb]
            self.pat_frames = torch.from_numpy(pv[np.arange(self.CF) % self.nvar].copy()).to(self.dev)         # [F nch, 4, nsymb]
        # pat_decoder(pat, 'dqpsk') of each variant's transmitted X and Y patterns (ex20_coherent_polmux.m:124-125)
        dv = np.stack([dqpsk_expected(v[2]) for v in self.var_host])                                          # [V, 4, nsymb]
        self.dpat = torch.from_numpy(dv[0]).to(self.dev)
        if self.nvar > 1:
            self.dpat_frames = torch.from_numpy(dv[np.arange(self.CF) % self.nvar].copy()).to(self.dev)

    def _build_rx(self, t):
        """the receiver: a comb's walk-off (from fiber_tables' t; 'unique', or 'sepfields' with wdm_receiver='channel') and
        'unique' field, CDE / DBP, DSP, front end, buffers"""
        torch, cfg, nch, n = self.torch, self.cfg, self.nch, self.cfg.nfft
        if self.unique:    # the walk-off select takes out, and the plan-owned field the fibre works on
            self.wdm_delay_symbols, self.wdm_delay = wdm_walkoff(self.wdm_shift, float(t["beta2"][0]), float(t["b30"]),
                                                                 cfg.nspans * cfg.length, cfg.symbolrate,
                                                                 GSTATE.FN[1] - GSTATE.FN[0], cfg.nt)
            self.wx = torch.empty((self.F, n), dtype=torch.complex128, device=self.dev)
            self.wy = torch.empty_like(self.wx)
        self._phase_work = {}                            # tile sums of the phase generator, per laser (allocated on use)
        self._lo_buf = None                              # [F nch, nfft] LO phase of the cohmix route (allocated on use)
        self._lo_bins = self._turns = None               # the last receive()'s LO offsets [CF] and frequency estimates [CF, 2]
        self._detuned = 0                                # channel-frames of the last receive() if its LO was detuned
        self.Lrx = 2 * cfg.nsymb
        fs = 2 * cfg.symbolrate * 1e9                                         # Run_my_PDM_QPSK.m:66,149
        N = min(cfg.fft_length, self.Lrx)
        self.cde = C.c_void_p()
        if cfg.wdm_receiver == "channel":
            # every channel at its own delay and with its own dispersion.  The walk-off may exceed a
            # frame (config[2]: ~1 140 symbols of 1 024): the frame is periodic, so the delay is taken modulo nfft here
            self.rx_delay_symbols, delay = sepfields_walkoff(t["b1"] if nch > 1 else np.zeros(1), cfg.nspans * cfg.length,
                                                             cfg.symbolrate, cfg.nt)
            self.rx_delay = np.ascontiguousarray(np.sign(delay) * (np.abs(delay) % n), dtype=np.int64)
            self.cde_H = wdm_cde_tables(N, fs, np.atleast_1d(GSTATE.LAMBDA), cfg.length * cfg.nspans, t["Dch"], cfg.slope)
            Hi = np.ascontiguousarray(self.cde_H).view(np.float64)
            self.lib.call("plx_cde_create_wdm", C.byref(self.cde), N, cfg.cde_L, Hi.ctypes.data, nch, 2)
        else:
            H = cde_transfer(N, fs, cfg.lam * 1e-9, cfg.length * cfg.nspans, cfg.disp * 1e-6, cfg.slope * 1e-6)
            Hi = np.ascontiguousarray(H).view(np.float64)
            self.lib.call("plx_cde_create", C.byref(self.cde), N, cfg.cde_L, Hi.ctypes.data)
        dsp = dict(workatbaudrate=False, applynlr=False, applypol=cfg.applypol, polmethod=cfg.polmethod,
                   cmaparams=dict(R=[1, 1], mu=cfg.cma_mu, taps=cfg.cma_taps, txpolars=2, phizero=0),
                   easiparams=dict(mu=cfg.cma_mu, txpolars=2, phizero=0), modorder=2, freqavg=cfg.freqavg,
                   phasavg=cfg.phasavg, poworder=cfg.poworder)
        self.dsp_p = dsp_params_struct(dsp, self.power_mw)
        self.dsp = C.c_void_p()
        self.lib.call("plx_dsp_create", C.byref(self.dsp), self.Lrx, 2, self.CF, C.byref(self.dsp_p))
        # receive scale: undo the span loss and bring symbols to the 4*sqrt(P) full scale that
        # DspPdmCohQpsk divides by (DspPdmCohQpsk.m:22-23, "2* -> see receiver_cohmix")
        self.rx_scale = 4.0 * math.sqrt(self.power_mw) / math.sqrt(self.power_mw / 2.0)
        if cfg.equaliser == "dbp":
            # the 2-sps samples are the field after the receiver's amplifier (physical with rx_amp, else folded into
            # rx_scale below) times this full-scale factor times rx_gain: DBP's scale maps them back to sqrt(mW)
            from .dbp import DbpPlan, dbp_betat, dbp_desc
            self.dbp_scale = 1.0 / self.rx_scale
            gam_ref = 2 * math.pi * cfg.n2 / (cfg.lam * cfg.aeff) * 1e18                      # fiber.m:325 at lambda
            bt = dbp_betat(self.Lrx, fs, cfg.lam * 1e-9, cfg.disp * 1e-6, cfg.slope * 1e3) * self.fls[0]
            self.dbp = DbpPlan(dbp_desc(self.Lrx, self.CF, cfg.nspans, cfg.dbp_steps, str(cfg.manakov).lower() == "yes",
                                        cfg.length, self.alphalin, gam_ref, cfg.dbp_xi, bt))
            self._dbp_sc = torch.full((self.CF,), self.dbp_scale, dtype=torch.float64, device=self.dev)
        if not cfg.rx_amp:
            self.rx_scale *= math.exp(0.5 * self.alphalin * cfg.length)
        if cfg.frontend == "cohmix":
            from . import rxfront
            rp = dict(oftype=cfg.oftype, obw=cfg.obw, oord=cfg.oord, eftype=cfg.eftype, ebw=cfg.ebw, eord=cfg.eord,
                      lopower=cfg.lopower)
            hopt, elo, hel, post_delay, _ = rxfront._front_tables(1, rp, nfc=nch)
            # in-line amplifier restoring the span loss, folded into the optical filter table (no extra sweep)
            if not cfg.rx_amp:
                hopt = hopt * math.exp(0.5 * self.alphalin * cfg.length)
            r = cfg.nt // 2                                                    # RxPdmCohQpsk.m:49-53, 2 samples/symbol
            delay = rxfront.evaldelay(cfg.oftype, cfg.obw * 0.5) + rxfront.evaldelay(cfg.eftype, cfg.ebw) + post_delay
            self.front_shifts = [rxfront._mround(-delay * cfg.nt)] * 2         # 'theory' delay, RxPdmCohQpsk.m:124-137
            self.front_tables = dict(hopt=hopt, elo=elo, hel=hel, fir=rxfront.fir1_lowpass(16, 1.0 / r), decim=r)
            self.front = rxfront._Front(n, True, self.CF, hopt, elo, hel, True, cfg.adcbits, r, self.front_tables["fir"])
        elif self.unique and nch > 1:
            # the pick has no optical filter of its own: a channel-frame cut out of the one field still has its neighbours
            # beside it in the spectrum (one channel has none: nch = 1 is the one-channel path)
            self.chfilt_h = np.asarray(myfilter(cfg.oftype, GSTATE.FN, 0.5 * cfg.obw, cfg.oord), dtype=complex)
            self.chfilt = self._filter_plan(self.chfilt_h, self.CF)
        self.rx = torch.empty((self.CF, 2, self.Lrx), dtype=torch.complex128, device=self.dev)
        self.eq = torch.empty_like(self.rx)
        self.sym = torch.empty((self.CF, 2, cfg.nsymb), dtype=torch.complex128, device=self.dev)
        self.err = torch.zeros((self.CF, 2), dtype=torch.int64, device=self.dev)

    def close(self):
        for name, h in (("plx_ssfm_destroy", self.ssfm), ("plx_cde_destroy", self.cde), ("plx_dsp_destroy", self.dsp),
                        ("plx_filter_destroy", self.chfilt), ("plx_filter_destroy", self.txfilt)):
            if h:
                self.lib.call(name, h)
        self.ssfm = self.cde = self.dsp = self.chfilt = self.txfilt = None
        if self.dbp is not None:
            self.dbp.close()
            self.dbp = None
        if self.front is not None:
            self.front.close()
            self.front = None

    # ------------------------------------------------------------------ inputs ---
    def make_batch(self, nframes, launch_scale=None, data_keys=None):
        """Synthetic inputs -> (ux, uy), each [F, n] complex128 ([F, nch, n] for 'sepfields' WDM frames): channel c of
        frame f carries Tx waveform (f nch + c) % variants, with an optional per-frame launch-power scaling (power sweep;
        the receiver then normalises each frame by its own launch power, as a per-run GSTATE.POWER does in
        DspPdmCohQpsk.m:22-23).
        tx_data='random': one plx_tx_qpsk_dev call draws the data of frame f under data_keys[f] (the frame index when
        None) and fills, beside the fields, NEW tensors self.pat_frames, self.dpat_frames [F nch, 4, nsymb] and self.tx_power
        [F nch] -- the current batch's; rx_gain = sqrt(power_mw / tx_power) is formed on the device.  Nothing is read back.
        With tx_filter the same call is followed by plx_tx_bandlimit_dev on the F nch pairs (before any launch_scale), which
        leaves its gains in a NEW tensor self.tx_gain [F nch].
        A caller that runs the receiver on another stream record_stream()s batch_tensors() there, as it does ux, uy."""
        torch = self.torch
        nch, n = self.nch, self.cfg.nfft
        ncf = nframes * nch
        self._batch = []
        if self.random:
            ux, uy = self._tx_random(nframes, data_keys)
        elif self.nvar > 1:
            idx = torch.arange(ncf, device=self.dev) % self.nvar
            ux = self.tx_var[idx, 0].contiguous()
            uy = self.tx_var[idx, 1].contiguous()
        else:
            ux = self.tx[0].unsqueeze(0).repeat(ncf, 1).contiguous()
            uy = self.tx[1].unsqueeze(0).repeat(ncf, 1).contiguous()
        # tx_data='random': each channel-frame normalised by its own power after create_field (its GSTATE.POWER)
        self.rx_gain = torch.sqrt(self.power_mw / self.tx_power).reshape(-1, 1, 1) if self.random else None
        if launch_scale is not None:
            ls = np.repeat(np.asarray(launch_scale, dtype=float).reshape(-1), nch)
            k = torch.as_tensor(np.sqrt(ls), device=self.dev).reshape(-1, 1)
            ux, uy = ux * k, uy * k
            g = torch.as_tensor(1.0 / np.sqrt(ls), device=self.dev).reshape(-1, 1, 1)             # per channel-frame
            self.rx_gain = g if self.rx_gain is None else self.rx_gain * g
        if self.rx_gain is not None:
            self._batch.append(self.rx_gain)
        if nch > 1:
            ux, uy = ux.view(nframes, nch, n), uy.view(nframes, nch, n)
        return ux, uy

    def _tx_random(self, nframes, data_keys):
        """the device transmitter for one batch: fresh fields, patterns and power (never a plan-owned buffer written again:
        the receiver of the previous batch may still be reading its own on another stream)"""
        torch = self.torch
        cfg, nch = self.cfg, self.nch
        ncf = nframes * nch
        ux = torch.empty((ncf, cfg.nfft), dtype=torch.complex128, device=self.dev)
        uy = torch.empty_like(ux)
        self.pat_frames = torch.empty((ncf, 4, cfg.nsymb), dtype=torch.uint8, device=self.dev)
        self.dpat_frames = torch.empty_like(self.pat_frames)
        self.tx_power = torch.empty(ncf, dtype=torch.float64, device=self.dev)
        kt = self._keys_dev(frame_keys(data_keys, nframes, "data_keys"))
        self.lib.call("plx_tx_qpsk_dev", ux.data_ptr(), uy.data_ptr(), cfg.nsymb, cfg.nt, nch, nframes,
                      self.tx_drive.ctypes.data, float(cfg.pavg_mw), MASTER_SEED, kt.data_ptr() if kt is not None else None,
                      self.pat_frames.data_ptr(), self.dpat_frames.data_ptr(), self.tx_power.data_ptr(), self.stream())
        self._batch += [self.pat_frames, self.dpat_frames, self.tx_power]
        if self.txfilt:        # band-limit every channel-frame and bring it back to pavg_mw by its own mean power
            self.tx_gain = torch.empty(ncf, dtype=torch.float64, device=self.dev)
            self.lib.call("plx_tx_bandlimit_dev", self.txfilt, ux.data_ptr(), uy.data_ptr(), ncf, float(cfg.pavg_mw),
                          self.tx_gain.data_ptr(), self._txfilt_work.data_ptr(), self.stream())
            self._batch.append(self.tx_gain)
        return ux, uy

    def _keys_dev(self, keys):
        """frame_keys' array on the device (None for None)"""
        return None if keys is None else self.torch.as_tensor(keys, device=self.dev)

    def batch_tensors(self):
        """the tensors make_batch made for the current batch beside ux, uy (patterns, power, receiver gain)"""
        return list(self._batch)

    def tx_bits_host(self, keys):
        """[len(keys), nch, nsymb, 4] uint8: the data tx_data='random' transmits in the realisations `keys` (the host mirror
        synth.random_qpsk_bits; columns X first, X second, Y first, Y second)"""
        return np.stack([np.stack([synth.random_qpsk_bits(self.cfg.nsymb, MASTER_SEED, int(k), c) for c in range(self.nch)])
                         for k in keys])

    def lo_bins_host(self, keys):
        """[len(keys), nch] int64: the LO offsets in bins that lo_detuning / lo_detuning_spread give the realisations `keys`
        (the host mirror synth.lo_detune_bins of plx_lo_detune_dev's draw)"""
        return synth.lo_detune_bins(MASTER_SEED, keys, self.nch, self.lo_k0, self.lo_K)

    @property
    def lo_bins(self):
        """int32 device tensor [CF]: the LO offset in bins of every channel-frame of the last receive() (None if its LO was
        not detuned)"""
        return self._lo_bins[:self._detuned] if self._detuned else None

    def freq_turns(self, F):
        """int32 device tensor [F, 2]: round((omega(end) - omega(1)) / 2 pi) of the frequency estimator (DspPdmCohQpsk.m:
        52-55) on both polarisations of the first F channel-frames of the last receive() -- minus the LO's offset in bins
        while that is within the estimator's range.  Read out only when the LO was detuned (plx_dsp_run_freq_dev)."""
        if not self._detuned:
            raise ValueError("freq_turns: the last receive() ran without lo_detuning, lo_detuning_spread or lo_bins")
        return self._turns[:F]

    def set_random_pmd(self, seeds):
        """brf draws of fiber.m:274-276, one independent set per frame, keyed by the realisation index alone (a
        counter-based generator: splitmix64 of (master seed, realisation, plate, stream) -> U[0,1)), so any batching
        or sharding of the indices gives the same waveplates.  Uploaded stream-ordered, without a device sync."""
        np_ = self.nplates
        r = np.asarray(list(seeds), dtype=np.uint64).reshape(-1, 1, 1)
        plate = np.arange(np_, dtype=np.uint64).reshape(1, -1, 1)
        stream = np.arange(3, dtype=np.uint64).reshape(1, 1, 3)
        with np.errstate(over="ignore"):       # uint64 arithmetic wraps by design
            keys = (np.uint64(MASTER_SEED) * np.uint64(0x9E3779B97F4A7C15) + r) * np.uint64(0xD1342543DE82EF95) \
                + plate * np.uint64(3) + stream
        u = _u01(keys)
        db0 = np.ascontiguousarray(u[:, :, 0] * 2 * math.pi - math.pi)
        th = np.ascontiguousarray(u[:, :, 1] * math.pi - 0.5 * math.pi)
        ep = np.ascontiguousarray(0.5 * np.arcsin(u[:, :, 2] * 2 - 1))
        self.lib.call("plx_ssfm_set_birefringence_dev", self.ssfm, db0.ctypes.data, th.ctypes.data, ep.ctypes.data, db0.shape[0],
                      self.stream())
        return db0, th, ep

    # ------------------------------------------------------------------- stages ---
    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def fibre(self, ux, uy, span_keys=None, inject_noise=None, tx_phase=None):
        """ux, uy: [F, n] (or [F, nch, n]) complex128 device tensors ([frame][channel][nfft]), propagated in place.
        span_keys: per-frame keys of the amplifiers' ASE streams (realisation indices).  inject_noise: optional list,
        one entry per amplifier, of [F, 2, n] complex128 device tensors used INSTEAD of the device generator
        (ampliflat's options.noise, ampliflat.m:123-129: the parity route).
        tx_phase: optional [F, nch, n] float64 device tensor, the transmitter lasers' phase used INSTEAD of the
        cfg.tx_linewidth generator (keyed by span_keys, or the frame index): both polarisations *= exp(+i phi).
        wdm_field='unique': the same contract -- the channels of ux, uy (after their lasers' phase) are multiplexed into the
        plan's one field self.wx, self.wy [F, n], the spans and amplifiers work on that, and on return channel c of frame f
        in ux, uy holds that channel cut back out at baseband with its walk-off taken out (not yet filtered: its
        neighbours are still beside it in the spectrum); self.wx[:F], self.wy[:F] keep the one field."""
        F = ux.shape[0]
        self._rows = self._steps = 0
        cfg = self.cfg
        keys, kt = frame_keys(span_keys, F, "span_keys"), None
        if tx_phase is not None or cfg.tx_linewidth > 0:      # lasersource.m:182-192: one laser feeds X and Y
            self._phase(ux.data_ptr(), uy.data_ptr(), 1, cfg.nfft, 1.0, F, keys, _abi.PLX_PHASE_TX, cfg.tx_linewidth,
                        tx_phase)
        px, py = ux.data_ptr(), uy.data_ptr()
        if self.unique:
            px, py = self.wx.data_ptr(), self.wy.data_ptr()
            self.lib.call("plx_wdm_mux_dev", ux.data_ptr(), uy.data_ptr(), px, py, cfg.nfft, self.nch, F,
                          self.wdm_shift.ctypes.data, self.stream())
        namp = 0
        for span in range(cfg.nspans):
            self.lib.call("plx_ssfm_propagate_dev", self.ssfm, px, py, F, self.stream())
            rows, steps = C.c_int64(), C.c_int64()
            self.lib.call("plx_ssfm_stats", self.ssfm, C.byref(rows), C.byref(steps))
            self._rows += rows.value
            self._steps += steps.value
            if span + 1 < cfg.nspans or cfg.rx_amp:   # in-line amplifier (ampliflat.m), stays on the device
                gain = math.exp(self.alphalin * cfg.length)
                sig = None
                if cfg.span_nf_db is not None:
                    sig = np.ascontiguousarray(ase_sigma(cfg.span_nf_db, gain, self.nfc), dtype=float)
                if kt is None:       # uploaded once per call: every amplifier reads the same keys
                    kt = self._keys_dev(keys)
                inj = inject_noise[namp] if inject_noise is not None else None
                self.lib.call("plx_ampliflat_dev", px, py, cfg.nfft, self.nfc, F, gain,
                              sig.ctypes.data if sig is not None else None, inj.data_ptr() if inj is not None else None,
                              (MASTER_SEED + 7919 * span) & (2 ** 64 - 1),
                              kt.data_ptr() if kt is not None else None, 1, 1, self.stream())
                namp += 1
        if self.unique:
            self.lib.call("plx_wdm_select_dev", px, py, ux.data_ptr(), uy.data_ptr(), cfg.nfft, self.nch, F,
                          self.wdm_shift.ctypes.data, self.wdm_delay.ctypes.data, self.stream())

    def _phase(self, pu, pv, stride, pitch, sign, F, keys, tag, linewidth, phi_in, phi_out=None):
        """one plx_phase_noise_dev call on F frames of nch channels: the injected phi_in, or the generator keyed by keys"""
        torch = self.torch
        n, nch = self.cfg.nfft, self.nch
        if phi_in is not None:
            self._phase_shape(phi_in, F)
            self.lib.call("plx_phase_noise_dev", pu, pv, stride, pitch, sign, n, nch, F, None, 0, None, tag,
                          phi_in.data_ptr(), None, None, self.stream())
            return
        need = self.F * nch * (-(-n // 2048))
        work = self._phase_work.get(tag)        # one per laser: the LO's may run on the receiver's stream beside the Tx's
        if work is None:
            work = self._phase_work[tag] = torch.empty(need, dtype=torch.float64, device=self.dev)
        sig = np.full(nch, math.sqrt(2 * math.pi * float(linewidth) / self.cfg.nt))
        kt = self._keys_dev(frame_keys(keys, F, "keys"))
        self.lib.call("plx_phase_noise_dev", pu, pv, stride, pitch, sign, n, nch, F, sig.ctypes.data, MASTER_SEED,
                      kt.data_ptr() if kt is not None else None, tag, None, phi_out, work.data_ptr(), self.stream())

    def _phase_shape(self, phi, F):
        n = self.cfg.nfft
        if tuple(phi.shape) != (F, self.nch, n) or phi.dtype != self.torch.float64 or not phi.is_contiguous():
            raise ValueError("an injected phase must be a contiguous float64 tensor [F, nch, nfft] = [%d, %d, %d]" % (F, self.nch, n))

    def errors_dqpsk(self, F):
        """Per-frame bit errors as the Monte-Carlo scripts count them (ex20_coherent_polmux.m:155-173): decisions of the
        symbols now in self.sym, differentially decoded and compared with pat_decoder(pat, 'dqpsk') of the transmitted
        patterns after ex20's polarisation-swap rule.  One device call; returns an int64 tensor [F]."""
        out = self.torch.empty(F, dtype=self.torch.int64, device=self.dev)
        pat, stride = (self.dpat_frames, 4 * self.cfg.nsymb) if self.per_frame else (self.dpat, 0)
        self.lib.call("plx_decide_count_dqpsk_dev", self.sym.data_ptr(), self.cfg.nsymb, 2, F, pat.data_ptr(), stride,
                      out.data_ptr(), self.stream())
        return out

    def errors(self, F):
        """per-frame errors by cfg.decoding: errors_resolved ('rotation') or errors_dqpsk ('dqpsk')"""
        return self.errors_dqpsk(F) if self.cfg.decoding == "dqpsk" else self.errors_resolved(F)

    def receive(self, ux, uy, noise_sigma=0.0, noise_seed=None, side_stream=None, noise_keys=None, lo_phase=None,
                lo_bins=None):
        """Front end (2-sps pick, or receiver_cohmix + ADC + decimate), CDE, DSP, decisions.  Returns err [F,2] (device).
        Receiver noise (sigma per quadrature on the 2-sps samples, an ASE stand-in) comes from the device Philox
        generator of plx_ampliflat_dev keyed by (noise_seed, noise_keys[frame] or frame): with noise_keys = the
        realisation indices the noise of a realisation does not depend on batching or sharding.
        With side_stream the whole receiver is enqueued on that stream behind the fibre of this batch, so
        the latency-bound CMA recurrence overlaps the HBM-bound fibre sweeps of the NEXT batch.
        lo_phase: optional [F, nch, n] float64 device tensor, the LO phase of each channel's receiver used INSTEAD of the
        cfg.lo_linewidth generator (keyed by noise_keys, or the frame index).
        lo_bins: optional [F, nch] int32 device tensor, the LO's frequency offset of each channel's receiver in bins used
        INSTEAD of cfg.lo_detuning / lo_detuning_spread (the parity route; not with equaliser='dbp')."""
        if side_stream is not None and self.overlap_ok():
            torch = self.torch
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream())
            side_stream.wait_event(ready)
            with torch.cuda.stream(side_stream):
                return self.receive(ux, uy, noise_sigma, noise_seed, None, noise_keys, lo_phase, lo_bins)
        F = ux.shape[0] * self.nch             # channel-frames: every channel of a 'sepfields' frame has its own receiver
        cfg, st, rx = self.cfg, self.stream(), self.rx[:F]
        if self.nch > 1:
            ux, uy = ux.view(F, cfg.nfft), uy.view(F, cfg.nfft)
        Ff = F // self.nch                     # frames (the phase tensors are [Ff, nch, nfft])
        keys = frame_keys(noise_keys, Ff, "noise_keys")
        detuned = self.detune or lo_bins is not None
        if detuned:
            self._detune_buffers(lo_bins, Ff)
        self._detuned = F if detuned else 0
        self._front_end(ux, uy, rx, F, Ff, keys, lo_phase, lo_bins)
        if self.rx_gain is not None and self.front is None:   # launch-power ladder: each frame normalised by its own power
            rx.mul_(self.rx_gain[:F])
        if noise_sigma:
            self._rx_noise(rx, F, Ff, noise_sigma, noise_seed, keys)
        if self.dbp is not None:
            sc = self._dbp_sc[:F]
            if self.rx_gain is not None:     # launch-power ladder: rx carries each frame's own gain
                sc = (sc / self.rx_gain[:F].reshape(-1)).contiguous()
                self._dbp_sc_keep = sc       # alive until the kernel has run
            self.dbp.apply(rx, self.eq, sc, st)
        else:
            self.lib.call("plx_cde_apply_dev", self.cde, rx.data_ptr(), self.eq.data_ptr(), self.Lrx, 2 * F, st)
        if detuned:                            # the same DSP, with the frequency estimate of every column read out
            self.lib.call("plx_dsp_run_freq_dev", self.dsp, self.eq.data_ptr(), self.sym.data_ptr(), F, self._turns.data_ptr(), st)
        else:
            self.lib.call("plx_dsp_run_dev", self.dsp, self.eq.data_ptr(), self.sym.data_ptr(), F, st)
        return self._decide_count(F)

    def _detune_buffers(self, lo_bins, Ff):
        """the plan's buffers of a detuned receive() (allocated on use), and the checks of an injected lo_bins"""
        torch = self.torch
        if lo_bins is not None:
            if self.dbp is not None:
                raise ValueError("lo_bins: not with equaliser='dbp'")
            if tuple(lo_bins.shape) != (Ff, self.nch) or lo_bins.dtype != torch.int32 or not lo_bins.is_contiguous() \
                    or lo_bins.device != self.dev:
                raise ValueError("injected lo_bins must be a contiguous int32 device tensor [F, nch] = [%d, %d]" % (Ff, self.nch))
        if self._lo_bins is None:
            self._lo_bins = torch.zeros(self.CF, dtype=torch.int32, device=self.dev)
            self._turns = torch.zeros((self.CF, 2), dtype=torch.int32, device=self.dev)

    def _lo_detune(self, pu, pv, stride, pitch, sign, Ff, keys, lo_bins, phi, accumulate):
        """one plx_lo_detune_dev call on Ff frames of nch channels: the injected lo_bins, or k0 + the draw keyed by keys;
        the offsets go to self._lo_bins"""
        kt = None if lo_bins is not None else self._keys_dev(keys)
        self.lib.call("plx_lo_detune_dev", pu, pv, stride, pitch, sign, self.cfg.nfft, self.nch, Ff, self.lo_k0, self.lo_K,
                      MASTER_SEED, kt.data_ptr() if kt is not None else None,
                      lo_bins.data_ptr() if lo_bins is not None else None, phi, int(accumulate), self._lo_bins.data_ptr(),
                      self.stream())

    def _front_end(self, ux, uy, rx, F, Ff, keys, lo_phase, lo_bins=None):
        """rx [F, 2, Lrx] <- the 2-sps samples of the channel-frames ux, uy [F, nfft]: cohmix, or (channel filter +) pick + LO.
        wdm_receiver='channel': the pick reads every channel-frame at its own channel's delay; the LO phase stays at the
        instants i half (a Wiener process has stationary increments: the same statistics on the shifted samples)."""
        cfg, st, half = self.cfg, self.stream(), self.cfg.nt // 2
        lo = lo_phase is not None or cfg.lo_linewidth > 0
        detuned = self.detune or lo_bins is not None
        if self.front is not None and detuned:
            # the detuned LO of receiver_cohmix.m:197-203, :227: Elo[cf] = Elo exp(i (theta[cf] + phi_b[cf])) -- the Wiener
            # phase (generated, or an injected one copied in) is in the plan's buffer first and theta is added to it
            if self.rx_gain is not None:
                ux.mul_(self.rx_gain[:F, :, 0])
                uy.mul_(self.rx_gain[:F, :, 0])
            if self._lo_buf is None:
                self._lo_buf = self.torch.empty((self.CF, cfg.nfft), dtype=self.torch.float64, device=self.dev)
            lop = self._lo_buf
            if lo_phase is not None:
                self._phase_shape(lo_phase, Ff)
                lop[:F].copy_(lo_phase.view(F, cfg.nfft))
            elif lo:
                self._phase(None, None, 1, cfg.nfft, 1.0, Ff, keys, _abi.PLX_PHASE_LO, cfg.lo_linewidth, None, lop.data_ptr())
            self._lo_detune(None, None, 1, cfg.nfft, 1.0, Ff, keys, lo_bins, lop.data_ptr(), lo)
            self.front.run(ux, uy, self.front_shifts, out=rx, lo_phase=lop)
        elif self.front is not None:           # receiver_cohmix + ADC + decimate; ux, uy are consumed
            if self.rx_gain is not None:       # launch-power ladder: each frame normalised by its own power
                ux.mul_(self.rx_gain[:F, :, 0])
                uy.mul_(self.rx_gain[:F, :, 0])
            lop = lo_phase
            if lo_phase is not None:
                self._phase_shape(lo_phase, Ff)
            elif lo:                           # Elo[f] = Elo exp(i phi_b[f]) (receiver_cohmix.m:223): phi_b of every channel-frame
                if self._lo_buf is None:
                    self._lo_buf = self.torch.empty((self.CF, cfg.nfft), dtype=self.torch.float64, device=self.dev)
                lop = self._lo_buf
                self._phase(None, None, 1, cfg.nfft, 1.0, Ff, keys, _abi.PLX_PHASE_LO, cfg.lo_linewidth, None,
                            lop.data_ptr())
            self.front.run(ux, uy, self.front_shifts, out=rx, lo_phase=lop)
        else:
            if self.chfilt is not None:        # 'unique': the optical filter isolates the channel; ux, uy are consumed
                for src in (ux, uy):
                    self.lib.call("plx_filter_apply_dev", self.chfilt, src.data_ptr(), F, st)
            if cfg.wdm_receiver == "channel":  # rx[cf][pol][i] = scale * u_pol[cf][(i*half + rx_delay[c]) mod nfft], one launch
                self.lib.call("plx_pick_wdm_dev", ux.data_ptr(), uy.data_ptr(), rx.data_ptr(), cfg.nfft, self.Lrx, half,
                              self.rx_scale, self.nch, Ff, self.rx_delay.ctypes.data, st)
            else:
                for pol, src in enumerate((ux, uy)):   # rx[f][pol][i] = scale * u_pol[f][i*half]
                    self.lib.call("plx_pick_dev", src.data_ptr(), rx.data_ptr() + pol * self.Lrx * 16, cfg.nfft, self.Lrx, 0,
                                  half, self.rx_scale, F, 2 * self.Lrx, st)
            if lo:                             # the LO at the pick instants: rx[f][pol][i] *= exp(-i phi_b[f][i half])
                self._phase(rx.data_ptr(), rx.data_ptr() + self.Lrx * 16, half, 2 * self.Lrx, -1.0, Ff, keys,
                            _abi.PLX_PHASE_LO, cfg.lo_linewidth, lo_phase)
            if detuned:                        # its frequency offset there: rx[cf][pol][i] *= exp(-i theta[cf][i half])
                self._lo_detune(rx.data_ptr(), rx.data_ptr() + self.Lrx * 16, half, 2 * self.Lrx, -1.0, Ff, keys, lo_bins,
                                None, False)

    def _rx_noise(self, rx, F, Ff, noise_sigma, noise_seed, keys):
        """noise of sigma per quadrature on the 2-sps samples rx [F, 2, Lrx], keyed by (noise_seed, keys[frame] or channel-frame)"""
        kt, nf, ncol = self._keys_dev(keys), F, 1
        if kt is not None:
            # one key per FRAME (realisation): the nch channel-frames of a frame are the columns of one ampliflat frame,
            # so each draws its own stream (the column is a word of the Philox counter) under its realisation's key
            nf, ncol = Ff, self.nch
        sig = np.full(ncol, float(noise_sigma))
        # one channel-frame of rx = [X | Y] contiguous: a single-"polarisation" ampliflat column with unit gain
        self.lib.call("plx_ampliflat_dev", rx.data_ptr(), None, 2 * self.Lrx, ncol, nf, 1.0, sig.ctypes.data, None,
                      int(noise_seed or 0) & (2 ** 64 - 1), kt.data_ptr() if kt is not None else None, 1, 0, self.stream())

    def _decide_count(self, F, swap=False):
        """the view self.err[:F] ([F, 2]) of the symbols now in self.sym against the transmitted bits (tributaries exchanged if swap)"""
        cfg, st = self.cfg, self.stream()
        pat = self.pat_frames[:F] if self.per_frame else self.pat
        if swap:
            pat = self.torch.cat([pat[..., 2:, :], pat[..., :2, :]], -2).contiguous()
        self._pat_keep = pat              # alive until the kernel has run
        if self.per_frame:
            self.lib.call("plx_decide_count_frames_dev", self.sym.data_ptr(), cfg.nsymb, 2, F, pat.data_ptr(), 4 * cfg.nsymb,
                          None, self.err.data_ptr(), st)
        else:
            self.lib.call("plx_decide_count_dev", self.sym.data_ptr(), cfg.nsymb, 2, F, pat.data_ptr(), None,
                          self.err.data_ptr(), st)
        return self.err[:F]

    def _min_over_rotations(self, F, swap, base):
        """err [F, 2]: minimum of the counts over the four pi/2 rotations of base, a clone of self.sym[:F] (the caller restores it)"""
        best = None
        for k in range(4):
            self.sym[:F] = base * (1j ** k)
            e = self._decide_count(F, swap).clone()
            best = e if best is None else self.torch.minimum(best, e)
        return best

    def errors_resolved(self, F):
        """Per-frame bit errors after resolving what a blind receiver cannot know: the pi/2 phase
        ambiguity of the Viterbi&Viterbi estimate (per polarisation) and which CMA output carries which
        transmitted tributary (the pol-swap check of ex20_coherent_polmux.m:160-173).  Eight calls of
        the device decision/count kernel; returns an int64 tensor [F]."""
        base = self.sym[:F].clone()
        best = [self._min_over_rotations(F, swap, base).sum(1) for swap in (False, True)]
        self.sym[:F] = base
        return self.torch.minimum(best[0], best[1])

    def evm(self, F):
        """per-frame error-vector magnitude (mean |s - s_hat|^2) of the symbols now in self.sym: float64 tensor [F]"""
        out = self.torch.empty(F, dtype=self.torch.float64, device=self.dev)
        self.lib.call("plx_evm_dev", self.sym.data_ptr(), self.cfg.nsymb, 2, F, out.data_ptr(), self.stream())
        return out

    def errors_min_over_rotations(self, F):
        """Resolve the pi/2 ambiguity of the blind phase estimate per polarisation (host-side
        convenience for BER sanity; the reference's scripts use differential decoding instead)."""
        base = self.sym[:F].clone()
        best = self._min_over_rotations(F, False, base)
        self.sym[:F] = base
        return best

    def run(self, ux, uy, noise_sigma=0.0, noise_seed=None):
        self.fibre(ux, uy)
        return self.receive(ux, uy, noise_sigma, noise_seed)

    def profile(self, on):
        """per-kernel HIP-event timing of the step loop (plx_ssfm_profile); read with kernel_times() after fibre()"""
        self._profiling = bool(on)
        self.lib.call("plx_ssfm_profile", self.ssfm, int(bool(on)))

    def kernel_times(self):
        """(ms[4], active launches[4]) accumulated over the fibre() calls since the previous call of this method: column sweep
        that starts a step, k_row, k_col_inv, control (plx_ssfm_kernel_times: the event intervals are read lazily)"""
        ms, nl = np.zeros(4), np.zeros(4, np.int64)
        if self._profiling:
            self.lib.call("plx_ssfm_kernel_times", self.ssfm, ms.ctypes.data, nl.ctypes.data)
        return ms, nl

    def last_ncycle(self, F):
        """ncycle (fiber.m:431) of each frame of the last propagate call"""
        nc = np.zeros(F, np.int32)
        self.lib.call("plx_ssfm_results", self.ssfm, F, None, nc.ctypes.data)
        return nc

    def utilisation(self):
        """(frame-steps with work, frame slots of the device's active list, frame slots the launches covered) of the last
        propagate call"""
        v = [C.c_int64(), C.c_int64(), C.c_int64()]
        self.lib.call("plx_ssfm_utilisation", self.ssfm, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def info(self):
        """plx_ssfm_info of the fibre plan: [fused, log2 N1, log2 N2, fused grid, column tiles per frame, ...]"""
        info = (C.c_int32 * 8)()
        self.lib.call("plx_ssfm_info", self.ssfm, info)
        return list(info)

    def fused(self):
        return bool(self.info()[0])

    def bind_gstate(self):
        """GSTATE as this plan's grid and comb need it (another HotPath built meanwhile has set its own)."""
        cfg = self.cfg
        GSTATE.NSYMB, GSTATE.NT, GSTATE.NCH = cfg.nsymb, cfg.nt, self.nch
        GSTATE.SYMBOLRATE = cfg.symbolrate
        GSTATE.FN = synth.fn_grid(cfg.nsymb, cfg.nt)
        GSTATE.LAMBDA = cfg.lam + cfg.chspacing * (np.arange(self.nch) - (self.nch - 1) / 2)      # lasersource.m: equally spaced comb
        if self.power_mw is not None:    # (known once the transmitter is built)
            GSTATE.POWER = np.full(self.nch, self.power_mw)

    def tx_columns(self):
        """Tx field of ONE frame as MATLAB holds it: (ux, uy), each [nfft x nch] (column c = variant c % variants)"""
        cols = [self.var_host[c % self.nvar] for c in range(self.nch)]
        return (np.asfortranarray(np.stack([c[0] for c in cols], 1)), np.asfortranarray(np.stack([c[1] for c in cols], 1)))

    def row_kernel(self):
        """name of the kernel that serves the step's row pass (for reports)"""
        info = self.info()
        if info[6] == 64:
            return "k_row256r" if info[2] == 8 else "k_rowsm"    # (rows of 32 / 64 / 128 points)
        if info[7] == 2:
            return "k_rowreg"                                     # rows of 512 / 1024 / 2048 points, register form
        if info[2] == 12:
            return "k_row4k" if info[7] else "k_row4k<pair>"     # (PMD: both polarisations of a row in one workgroup)
        return "k_row"

    def overlap_ok(self):
        """May a second stream (the receiver of the previous batch) share the GPU with fibre()?  The fused column sweep needs
        the tiles of a frame co-resident; when ONE frame takes more than half of the grid (2^19- and 2^20-sample frames)
        a long-running receiver kernel that holds registers on every CU keeps the frame's second half from being placed
        until it ends: the two serialise (or the barrier times out).  Such plans run the receiver on the fibre's stream."""
        info = self.info()
        return (not info[0]) or 2 * info[4] <= info[3]

    def ssfm_stats(self):
        """(row-pass launches, sample-steps) of the last fibre() call, summed over its frame groups"""
        return self._rows, self._steps


def _concat(parts, dtype):
    """the parts of a campaign's result side by side (an empty result for no part)"""
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


class _Simulate:
    def simulate(self, indices, keep=None):
        """Error counts (pol swap and pi/2 ambiguities resolved, ex20_coherent_polmux.m:160-173) of the realisations
        `indices`.  keep(i0, idx, ux, uy): optional callback after the fibre + amplifier of each batch (tests read the
        field back there)."""
        return self.collect(self.launch(indices, keep))


class McCampaign(_Simulate):
    """Monte-Carlo BER over random PMD + ASE realisations (the ex20-style loop around ber_estimate,
    with ex24's random-birefringence fibre): realisation r gets its own birefringence draw and its own
    noise, both keyed by r alone, so any sharding of the indices over GPUs gives the same counts.

    ASE: with cfg.rx_amp the span is followed by ampliflat(Gerbio,'gain',{f: cfg.span_nf_db}) as in
    ex20_coherent_polmux.m:147-148 (device Philox stream keyed by r, or `noise_provider(indices)` -> host array
    [n, 2, nfft] complex, the options.noise injection of ampliflat.m:123-129, for parity tests); `noise_sigma`
    additionally (or instead) loads the 2-sps receiver samples, the cheap stand-in used by small tests."""

    def __init__(self, cfg, frames_per_call, noise_sigma=0.0, noise_provider=None):
        self.hp = HotPath(cfg, frames_per_call)
        self.F = frames_per_call
        self.sigma = noise_sigma
        self.noise_provider = noise_provider
        self._rx_stream = None

    @property
    def bits_per_realisation(self):
        return 4 * self.hp.cfg.nsymb

    def launch(self, indices, keep=None):
        """Enqueue the realisations `indices` and return a handle WITHOUT waiting for the receiver: the fibre runs on the
        current stream (plx_ssfm_propagate_dev returns when its data-dependent step loop has ended), the receiver and the
        error counts go to a second stream, so the receiver of this batch overlaps the fibre of the next one (the CMA is
        latency-bound: ~25 ms whatever the batch size).  collect(handle) -> int64 error counts."""
        import torch
        hp = self.hp
        if self._rx_stream is None:
            self._rx_stream = torch.cuda.Stream()
        out = []
        for i0 in range(0, len(indices), self.F):
            idx = list(indices[i0:i0 + self.F])
            n = len(idx)
            if hp.pmd:
                hp.set_random_pmd(idx)
            ux, uy = hp.make_batch(n, data_keys=idx)
            inj = None
            if self.noise_provider is not None:
                inj = [torch.from_numpy(np.ascontiguousarray(self.noise_provider(idx))).to(hp.dev)]
            hp.fibre(ux, uy, span_keys=idx, inject_noise=inj)
            if keep is not None:
                keep(i0, idx, ux, uy)
            # ONE stream for the receiver and everything that reads its outputs (hp.sym, hp.err): the side stream when the
            # plan may share the GPU with the next fibre, the fibre's own stream otherwise (receive() would fall back to
            # it by itself, and the EVM / error kernels must follow the DSP in stream order)
            rxs = self._rx_stream if hp.overlap_ok() else torch.cuda.current_stream()
            side = rxs if rxs is self._rx_stream else None
            hp.receive(ux, uy, self.sigma, MASTER_SEED, side, idx)   # receiver noise keyed by realisation index
            with torch.cuda.stream(rxs):
                # a 'unique' comb, or 'sepfields' with wdm_receiver='channel': a count per channel-frame, [n nch], channels innermost
                ncf = n * hp.nch if hp.unique or hp.cfg.wdm_receiver == "channel" else n
                v = hp.evm(ncf)            # a continuous per-realisation sample (mc_estimate) beside the error count
                e = hp.errors(ncf)
                if side is not None:
                    ux.record_stream(rxs); uy.record_stream(rxs)
                    for t in hp.batch_tensors():      # this batch's patterns, power and gain: the next batch makes its own
                        t.record_stream(rxs)
                done = torch.cuda.Event()
                done.record(rxs)
            out.append((e, v, done))
        return out

    def collect(self, handle, with_samples=False):
        """int64 error counts of a launch() handle (and, with_samples, the float64 EVM samples beside them); with
        wdm_field='unique' or wdm_receiver='channel' one per channel-frame: [len(indices) * nch], the channels of a realisation
        side by side"""
        res, smp = [], []
        for e, v, done in handle or []:
            done.synchronize()             # the counts were formed on the receiver's stream
            res.append(e.cpu().numpy())
            smp.append(v.cpu().numpy())
        return (_concat(res, np.int64), _concat(smp, np.float64)) if with_samples else _concat(res, np.int64)

    def close(self):
        self.hp.close()


class McRankShare(_Simulate):
    """The share ONE rank of `world` has in a campaign, run on its own: local index i stands for realisation rank + world * i
    (realisation r on GPU r mod world).  launch / collect / simulate of the wrapped campaign or pool."""

    def __init__(self, camp, rank, world):
        self.camp, self.rank, self.world = camp, int(rank), int(world)

    def _map(self, indices):
        return [self.rank + self.world * int(i) for i in indices]

    def launch(self, indices, keep=None):
        return self.camp.launch(self._map(indices), keep)

    def collect(self, handle, with_samples=False):
        return self.camp.collect(handle, with_samples)


class McCampaignPool(_Simulate):
    """`n` McCampaign instances taking the rounds of a campaign in turn, each with its own plans, receiver buffers and
    receiver stream: the receivers of up to n rounds are in flight at once (ShardedBer.run(depth=n - 1)).  A noise-loaded
    realisation's CMA runs all of its 299 passes -- ~58 ms of a serial recurrence whatever the batch size -- while its
    fibre takes a few ms: with one receiver in flight a round of 128 realisations is latency-bound on that."""

    def __init__(self, cfg, frames_per_call, n=2, noise_sigma=0.0, noise_provider=None, split=False):
        """split: ONE round is dealt over all n instances (contiguous parts, launched back to back, collected in order) instead
        of the rounds taking turns: the receivers of a round's parts run beside each other and the round still ends in ONE
        exchange -- what a rank of a strong-scaling run does with its fixed share (bench.py, mc.strong_scaling_rank_share)."""
        self.camps = [McCampaign(cfg, frames_per_call, noise_sigma, noise_provider) for _ in range(max(1, int(n)))]
        self._turn = 0
        self.split = bool(split)

    @property
    def bits_per_realisation(self):
        return self.camps[0].bits_per_realisation

    @property
    def hp(self):
        return self.camps[0].hp

    def launch(self, indices, keep=None):
        if self.split:
            idx = list(indices)
            per = -(-len(idx) // len(self.camps))
            return [(i, c.launch(idx[i * per:(i + 1) * per], keep)) for i, c in enumerate(self.camps) if idx[i * per:(i + 1) * per]]
        i = self._turn % len(self.camps)
        self._turn += 1
        return i, self.camps[i].launch(indices, keep)

    def collect(self, handle, with_samples=False):
        if self.split:
            parts = [self.camps[i].collect(h, True) for i, h in handle]
            counts, smp = _concat([p[0] for p in parts], np.int64), _concat([p[1] for p in parts], np.float64)
            return (counts, smp) if with_samples else counts
        i, h = handle
        return self.camps[i].collect(h, with_samples)

    def close(self):
        for c in self.camps:
            c.close()
