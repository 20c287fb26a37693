# dev tool: CRC32 of what the batched hot path (pipeline.HotPath, McCampaign, McCampaignPool) computes for a fixed set of
# configurations that between them take every branch of its host code.  Only the public surface is used, so the same file
# runs on the commit before and the commit after a host-side refactoring, which must reproduce every line bit for bit.
#   usage: python scripts/hotpath_crc.py > crc.txt ; diff against the file of the other commit (same built library)
import os, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
import torch
from polmux_amd import pipeline

F, FMAX = 3, 4
SMALL = dict(nsymb=64, nt=16, pavg_mw=4.0, length=4e4, cma_mu=1 / 300, freqavg=20, dphimax=2e-2)   # 1024 samples: one partial tile
COMB = dict(SMALL, nsymb=256, nch=3, wdm_field="unique")         # the 0.4 nm comb on bins +-456; 4096 samples: two tiles
FILT = dict(ftype="ideal", bw=1.6)
CASE3 = dict(SMALL, flag="gps-", nplates=5, nspans=2, span_nf_db=5, rx_amp=True)


def crc(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


def hot(name, cfg, batch=None, pmd=None, fibre=None, receive=None):
    hp = pipeline.HotPath(pipeline.HotPathConfig(**cfg), FMAX)
    try:
        if pmd is not None:
            hp.set_random_pmd(pmd)
        ux, uy = hp.make_batch(F, **(batch or {}))
        hp.fibre(ux, uy, **(fibre or {}))
        torch.cuda.synchronize()
        line = "ux %s uy %s" % (crc(ux), crc(uy))
        nc = hp.last_ncycle(F)
        err = hp.receive(ux, uy, **(receive or {}))
        ncf = err.shape[0]
        torch.cuda.synchronize()
        line += " sym %s err %s" % (crc(hp.sym[:ncf]), crc(err))
        line += " errors %s evm %s ncycle %s" % (crc(hp.errors(ncf)), crc(hp.evm(ncf)), nc.tolist())
    finally:
        hp.close()
    print("%-28s %s" % (name, line), flush=True)


def campaign(name, camp):
    try:
        counts, evm = camp.collect(camp.launch(list(range(7))), with_samples=True)
    finally:
        camp.close()
    print("%-28s counts %s %s evm %s" % (name, crc(counts), counts.tolist(), crc(evm)), flush=True)


hot("1 defaults", SMALL)
hot("2 variants dqpsk", dict(SMALL, variants=3, decoding="dqpsk"))
hot("3 pmd spans ase", CASE3, pmd=[5, 9, 2], fibre=dict(span_keys=[5, 9, 2]))
hot("4 cohmix linewidths noise", dict(SMALL, frontend="cohmix", tx_linewidth=1e-4, lo_linewidth=1e-4),
    receive=dict(noise_sigma=0.05, noise_seed=11, noise_keys=[3, 1, 4]))
# (plx_dbp_create wants 2 nsymb >= 256, the de Bruijn sequence a power of four)
hot("5 dbp ladder", dict(SMALL, nsymb=256, equaliser="dbp"), batch=dict(launch_scale=[0.5, 1, 2]))
hot("6 manakov xpm", dict(SMALL, nch=3, xpm_dualpol="manakov", flag="gpsx", manakov="yes"))
hot("7 unique pick txfilter", dict(COMB, tx_filter=FILT))
hot("8 unique random cohmix", dict(COMB, tx_data="random", tx_filter=FILT, frontend="cohmix"), batch=dict(data_keys=[7, 8, 9]))
hot("9 unique muxfilter", dict(COMB, mux_filter=FILT))
hot("10 random ladder", dict(SMALL, tx_data="random"), batch=dict(launch_scale=[0.5, 1, 2]))
MC = pipeline.HotPathConfig(**dict(CASE3, tx_data="random"))
campaign("11 campaign", pipeline.McCampaign(MC, frames_per_call=3, noise_sigma=0.05))
campaign("12 pool split", pipeline.McCampaignPool(MC, frames_per_call=3, n=2, noise_sigma=0.05, split=True))
