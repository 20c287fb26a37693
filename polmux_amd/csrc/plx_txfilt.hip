// plx_txfilt.hip -- the transmitter's channel filter on the device: pipeline.band_limit per realisation.
//
//   x_p = ifft(fft(x_p) H), y_p likewise      (the two passes of plx_filter_apply_dev over the X rows and the Y rows)
//   m_p = (1 / nfft) sum_n (|x_p[n]|^2 + |y_p[n]|^2);   k_p = sqrt(pavg / m_p);   x_p *= k_p, y_p *= k_p
//
// for every (X, Y) pair p of a batch, with no read-back.  The sum takes the structure of plx_phase.hip: tiles of 2048 samples,
//   k_txf_tile_power   one partial per (pair, tile) in d_work[p ntiles + t]: a thread's eight samples in ascending order, then
//                      block_sum -- the same order in every workgroup
//   k_txf_scale        every workgroup of a pair adds the pair's <= 512 partials in the same order (thread j takes partials j
//                      and j + 256, then block_sum), forms k_p and scales its own tile
// so m_p depends on nfft and the pair's samples alone -- not on npairs, not on the pair's place in the batch, not on the grid
// -- and no floating-point atomic is involved.  Both kernels are streams: 32 B read per sample pair in the first, 64 B read
// and written in the second.  A complex128 sample IS the 16-byte access; consecutive lanes take consecutive samples, so a wave
// instruction covers 1 KiB of one row, and a thread's sixteen loads are issued before the first is used.
// The (pair, tile) index is a flat work item that a one-dimensional grid of at most kMaxGrid workgroups strides over: no grid
// dimension grows with npairs.
#include "plx_internal.h"

#include <cmath>

namespace {

constexpr int kThreads = 256, kPer = 8, kTile = kThreads * kPer;
constexpr int kMaxGrid = 2048;   // 256 CUs x 8 workgroups: the rest of a large batch is strided over

struct TxFiltArgs {
    cplx *ux, *uy;            // [npairs][nfft]
    double *work;             // [npairs][ntiles]
    double *gain;             // [npairs] (may be null)
    int64_t nfft, nwork;      // nwork = npairs ntiles
    int ntiles;
    double pavg;
};

// sum over the workgroup, the same order in every workgroup (red: 4 doubles of LDS) -- plx_phase.hip's
__device__ __forceinline__ double block_sum(double v, double *red)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kThreads) void k_txf_tile_power(TxFiltArgs a)
{
    PLX_DYN_LDS(lds);
    double *red = (double *)lds;
    const int tid = threadIdx.x;
    for (int64_t w = blockIdx.x; w < a.nwork; w += gridDim.x) {
        const int64_t p = w / a.ntiles, t0 = (w - p * a.ntiles) * kTile;
        const int64_t left = a.nfft - t0;
        const int ns = (int)(left < kTile ? left : kTile);     // samples of this tile (nfft < 2048: the one partial tile)
        const cplx *x = a.ux + (size_t)p * a.nfft + t0, *y = a.uy + (size_t)p * a.nfft + t0;
        cplx vx[kPer], vy[kPer];
#pragma unroll
        for (int s = 0; s < kPer; s++) {
            const int i = s * kThreads + tid;
            const bool in = i < ns;
            vx[s] = in ? x[i] : make_double2(0.0, 0.0);
            vy[s] = in ? y[i] : make_double2(0.0, 0.0);
        }
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < kPer; s++)
            acc += (vx[s].x * vx[s].x + vx[s].y * vx[s].y) + (vy[s].x * vy[s].x + vy[s].y * vy[s].y);
        acc = block_sum(acc, red);
        if (tid == 0) a.work[w] = acc;
    }
}

__global__ __launch_bounds__(kThreads) void k_txf_scale(TxFiltArgs a)
{
    PLX_DYN_LDS(lds);
    double *red = (double *)lds;
    const int tid = threadIdx.x;
    for (int64_t w = blockIdx.x; w < a.nwork; w += gridDim.x) {
        const int64_t p = w / a.ntiles, t = w - p * a.ntiles, t0 = t * kTile;
        const int64_t left = a.nfft - t0;
        const int ns = (int)(left < kTile ? left : kTile);
        cplx *x = a.ux + (size_t)p * a.nfft + t0, *y = a.uy + (size_t)p * a.nfft + t0;
        cplx vx[kPer], vy[kPer];
#pragma unroll
        for (int s = 0; s < kPer; s++) {       // the tile's loads go out ahead of the partials' reduction
            const int i = s * kThreads + tid;
            const bool in = i < ns;
            vx[s] = in ? x[i] : make_double2(0.0, 0.0);
            vy[s] = in ? y[i] : make_double2(0.0, 0.0);
        }
        const double *ts = a.work + (size_t)p * a.ntiles;
        double tot = 0.0;
        for (int j = tid; j < a.ntiles; j += kThreads) tot += ts[j];
        tot = block_sum(tot, red);
        const double m = tot / (double)a.nfft, k = sqrt(a.pavg / m);
        // H removed everything (or the rows were not finite): the rows stay as filtered, the gain reads 0, no NaN is made
        const bool live = m > 0.0 && m < __builtin_huge_val() && k < __builtin_huge_val();
        if (t == 0 && tid == 0 && a.gain) a.gain[p] = live ? k : 0.0;
        if (!live) continue;                   // (uniform over the workgroup)
#pragma unroll
        for (int s = 0; s < kPer; s++) {
            const int i = s * kThreads + tid;
            if (i >= ns) break;
            x[i] = cscale(vx[s], k);
            y[i] = cscale(vy[s], k);
        }
    }
}

} // namespace

extern "C" int plx_tx_bandlimit_dev(plx_filter *P, double *d_ux, double *d_uy, int npairs, double pavg_mw, double *d_gain,
                                    double *d_work, void *stream)
{
    if (!P || !d_ux || !d_uy || !d_work) PLX_FAIL(PLX_ERR_ARG, "plx_tx_bandlimit_dev: null argument");
    if (npairs < 1 || npairs > P->max_sig) PLX_FAIL(PLX_ERR_ARG, "plx_tx_bandlimit_dev: npairs outside [1, max_signals]");
    if (!std::isfinite(pavg_mw) || !(pavg_mw > 0)) PLX_FAIL(PLX_ERR_ARG, "plx_tx_bandlimit_dev: pavg_mw must be finite and > 0");
    int rc = plx_ssfm_filter_dev(P->fft, (cplx *)d_ux, nullptr, P->d_h, npairs, stream);   // = plx_filter_apply_dev
    if (rc == PLX_OK) rc = plx_ssfm_filter_dev(P->fft, (cplx *)d_uy, nullptr, P->d_h, npairs, stream);
    if (rc != PLX_OK) return rc;
    int p1 = 0, p2 = 0;
    plx_ssfm_geometry(P->fft, &p1, &p2);
    TxFiltArgs a;
    a.ux = (cplx *)d_ux; a.uy = (cplx *)d_uy; a.work = d_work; a.gain = d_gain;
    a.nfft = (int64_t)1 << (p1 + p2);
    a.ntiles = (int)((a.nfft + kTile - 1) / kTile);
    a.nwork = (int64_t)npairs * a.ntiles;
    a.pavg = pavg_mw;
    const dim3 grid((unsigned)(a.nwork < kMaxGrid ? a.nwork : kMaxGrid));
    PLX_LAUNCH(k_txf_tile_power, grid, dim3(kThreads), 4 * sizeof(double), stream, a);
    PLX_LAUNCH(k_txf_scale, grid, dim3(kThreads), 4 * sizeof(double), stream, a);
    PLX_HIP(hipGetLastError());
    return PLX_OK;
}
