// ssfm_plan.h -- the propagator's plan object (library-internal).
#pragma once
#include "ssfm_kernels.h"
#include <vector>

using plxs::FrameCtl;
using plxs::SsfmArgs;

// One resolved row-pass launch: what launch_row needs besides the arguments and the number of frame-channels FC.  A plan
// holds one per use, resolved once at creation (resolve_rows, ssfm_plan.hip: one clause per kernel family).
enum RowFamily { ROW_GENERAL, ROW_SM, ROW_256, ROW_REG, ROW_4K };   // k_row, k_rowsm, k_row256r, k_rowreg, k_row4k
struct RowPass {
    plxs::sweep_kernel_t kern = nullptr;
    RowFamily family = ROW_GENERAL;
    unsigned threads = 0;          // workgroup size
    unsigned gx = 0;               // grid.x per frame-channel
    size_t lds = 0;                // dynamic LDS
    bool fold = false;             // grid (gx * FC) -- the kernel decodes row, frame-channel (and polarisation) itself -- not (gx, FC)
    bool single = false;           // dual plan through a one-polarisation kernel: the arguments rewritten to dual = 0, R = 1
    bool twice = false;            // ... one launch per polarisation (ux = uy on the second) instead of both in one grid
};
// Who launches the row pass.  The argument state of each use is fixed, so the kernel is too:
enum RowUse {
    ROW_STEP,                      // the step loop: the plan's own pmd and trunk phasor tables, force = 0, no hmul, no umat
    ROW_TABLE,                     // plx_ssfm_filter_dev with a multiplier table, plx_ssfm_linear_dev: force = 1, pmd = 0, no umat
    ROW_MATRIX,                    // plx_ssfm_filter_dev with matrix tables (dual plans): force = 1, pmd = 0, umat couples the polarisations
    ROW_USES
};

struct plx_ssfm {
    plx_ssfm_desc d;
    int p, p1, p2;
    size_t N;
    SsfmArgs a;
    double *d_betat = nullptr, *d_db1 = nullptr, *d_gam = nullptr, *d_brf = nullptr, *d_psum = nullptr;
    cplx *d_tpass = nullptr, *d_tw1 = nullptr, *d_tw2 = nullptr, *d_ctab = nullptr;
    FrameCtl *d_ctl = nullptr;
    unsigned long long *d_umax = nullptr;
    int *d_ndone = nullptr;   // [0] frames done, [1] abort word, [2] frames in the active list, [3] its running sum over the steps
    int *h_ndone = nullptr;   // pinned copy of the four words
    int *d_active = nullptr;  // [max_frames] active list (k_compact)
    hipEvent_t ev = nullptr;  // completion of the last read-back of d_ndone
    std::vector<FrameCtl> h_ctl;
    int brf_sets = 0;
    size_t lds_col = 0;
    cplx *d_e1 = nullptr, *d_e2 = nullptr;   // per-frame, per-trunk row / column phasors of PMD plans with a linear db1 (k_pmd_tab)
    unsigned long long *d_slots = nullptr;   // slot barrier of the fused column sweep: [launch parity][frame][tile]
    unsigned long long *d_mbox = nullptr;    // [teams][frames + 4] mailboxes of the fused column sweep's teams, then the two claim counters
    size_t mbox_bytes = 0;
    int fused = 0, fused_grid = 0, tiles_pf = 0;
    uint32_t flags = 0;                      // plx_ssfm_create_ex
    int xpm_dual = 0;                        // PLX_SSFM_XPM_MANAKOV on a multi-channel dual-polarisation plan: k_stokes_sum + k_col_fwd_xpm, d_psum holds the record
    int barrier_timeouts = 0;                // propagate calls of this plan that ended in a frame-barrier time-out (it then takes the three-sweep step
                                             // until plx_ssfm_barrier_timeouts(..., rearm) -- the gateway tier re-arms its cached plans itself)
    int calls_unfused = 0, rearm_after = 16; // gateway tier: three-sweep calls since the last time-out / how many of them before the fused step is tried again
    double *d_dzlist = nullptr, *d_dzlog = nullptr;   // diagnostics: replayed / logged step sequences
    int dzlist_cap = 0;
    int col_threads = 512;         // workgroup size of k_col_fwd / k_col_inv
    RowPass row[ROW_USES];         // the row pass of each use
    cplx *d_tw2c = nullptr, *d_twmid = nullptr;   // k_rowreg's compact twiddle table; k_rowsm's / k_rowreg's mid twiddles
    int tw_compact = 0;            // 4096-point rows: compact twiddle table in d_tw2, register-blocked row pass k_row4k
    double *h_brf[2] = {nullptr, nullptr}; // pinned staging of the waveplate tables
    hipEvent_t brf_ev[2] = {nullptr, nullptr};
    int brf_slot = 0;
    int64_t row_launches = 0, sample_steps = 0;
    int64_t slots_launched = 0, slots_listed = 0, frame_steps = 0;   // utilisation accounting of the last propagate
    // optional per-kernel timing of the step loop (plx_ssfm_profile): one event between consecutive launches
    int profile = 0;
    // The intervals are read LATER -- while the next call's first launches run, or when the times are asked for: some 160
    // hipEventElapsedTime calls per propagate would otherwise sit between two calls with the GPU idle (~2 ms per 110 ms).
    struct ProfRun { std::vector<hipEvent_t> ev; std::vector<int> cls, step; int maxnc = 0; bool fused = false; };
    std::vector<hipEvent_t> evfree;          // events not in use
    std::vector<ProfRun> prof_pending;       // finished step loops whose intervals have not been read yet
    double k_ms[4] = {0, 0, 0, 0};           // accumulated since the last plx_ssfm_kernel_times
    int64_t k_launches[4] = {0, 0, 0, 0};
};

// The linear step x = ifft(fft(x) .* exp(-i betat dz)) on one frame of `base`'s plan (lin_step, fiber.m:771-773) with the
// step length forced from the launch: the three transform sweeps through the row-pass dispatch of the step loop and the
// filter (ssfm_plan.hip: ROW_TABLE), scalar plans only.  The host-driven adaptive scheme (ssfm_gateway.hip) calls it; a
// failed launch is PLX_ERR_HIP.
PLX_HIDDEN int plx_ssfm_linear_dev(plx_ssfm *P, const SsfmArgs &base, cplx *d_x, double dz, hipStream_t st);

static const double kInv2Pi = 0.15915494309189533577;
