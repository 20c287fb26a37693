// plx_wdm.hip -- a WDM comb as ONE field: the multiplexer of create_field('unique') (create_field.m:165-199)
// restated in the time domain, and the channel selection of receiver_cohmix.m:104-125 with the walk-off delay taken out.
//   mux      u[f][n]    = sum_{c < nch} s[f][c][n] * W(s_c n)                      W(k) = exp(-i 2 pi (k mod N) / N)
//   select   r[f][c][n] = u[f][m] * conj(W(s_c m)),  m = (n + delay[c]) mod N      the phasor at the SOURCE index m
// Both are streaming kernels: one lane per sample (16-B loads and stores, consecutive lanes on consecutive samples), the
// channels of a sample in the lane's loop.  The phase s_c n is reduced modulo N in integers (N is a power of two, so the
// 32-bit product may wrap) and becomes an exact number of turns k / N for cexp_neg_turns: no error grows with n.
//
// The receiver of 'sepfields' frames with per-channel timing: the 2-sps pick of every channel-frame at its own
// channel's walk-off delay,
//   pick     rx[cf][p][i] = scale * u_p[cf][(i stride + delay[c]) mod N],  cf = f nch + c
// one lane per output sample (one 16-B load, one 16-B store), both polarisations and all channel-frames in one launch.
#include "../../include/polmux_hip.h"
#include "plx_common.h"

#define WDM_MAXCH 64
#define WDM_CH 4          // channels whose loads are issued before any arithmetic (as k_stokes_sum's STOKES_CH)

namespace {

struct WdmArgs {
    cplx *cx, *cy;               // [frame][nch][nfft]: the channels (mux reads them, select writes them); cy NULL: X only
    cplx *ux, *uy;               // [frame][nfft]: the one field
    unsigned nfft, mask;         // N, N - 1
    int nch;
    double inv_n;                // 1 / N (exact)
    unsigned shift[WDM_MAXCH];   // s_c mod N, in [0, N)
    unsigned delay[WDM_MAXCH];   // delay[c] mod N, in [0, N)
};

// W(s n): s, n < N <= 2^20; the product modulo 2^32 is the product modulo N after the mask
__device__ __forceinline__ cplx wdm_phasor(unsigned s, unsigned n, unsigned mask, double inv_n)
{
    return cexp_neg_turns((double)((s * n) & mask) * inv_n);
}

__global__ __launch_bounds__(256) void k_wdm_mux(WdmArgs a)
{
    const int f = blockIdx.y;
    const size_t N = a.nfft;
    const bool dual = a.cy != nullptr;
    const cplx *sx = a.cx + (size_t)f * a.nch * N, *sy = dual ? a.cy + (size_t)f * a.nch * N : nullptr;
    for (unsigned n = blockIdx.x * blockDim.x + threadIdx.x; n < a.nfft; n += gridDim.x * blockDim.x) {
        cplx ax = make_double2(0, 0), ay = make_double2(0, 0);
        int k = 0;
        for (; k + WDM_CH <= a.nch; k += WDM_CH) {
            cplx xv[WDM_CH], yv[WDM_CH];
#pragma unroll
            for (int j = 0; j < WDM_CH; j++) {
                xv[j] = sx[(size_t)(k + j) * N + n];
                yv[j] = dual ? sy[(size_t)(k + j) * N + n] : make_double2(0, 0);
            }
#pragma unroll
            for (int j = 0; j < WDM_CH; j++) { pin(xv[j]); pin(yv[j]); }
#pragma unroll
            for (int j = 0; j < WDM_CH; j++) {
                const unsigned s = a.shift[k + j];
                cplx px = xv[j], py = yv[j];
                if (s != 0) {                        // (wave-uniform; a carrier at the centre is copied, not multiplied by 1)
                    const cplx w = wdm_phasor(s, n, a.mask, a.inv_n);
                    px = cmul(px, w);
                    py = cmul(py, w);
                }
                ax = (k + j) ? cadd(ax, px) : px;    // the sum starts FROM channel 0: one channel at shift 0 is a copy to the bit
                ay = (k + j) ? cadd(ay, py) : py;
            }
        }
        for (; k < a.nch; k++) {
            const unsigned s = a.shift[k];
            cplx px = sx[(size_t)k * N + n], py = dual ? sy[(size_t)k * N + n] : make_double2(0, 0);
            if (s != 0) {
                const cplx w = wdm_phasor(s, n, a.mask, a.inv_n);
                px = cmul(px, w);
                py = cmul(py, w);
            }
            ax = k ? cadd(ax, px) : px;
            ay = k ? cadd(ay, py) : py;
        }
        a.ux[(size_t)f * N + n] = ax;
        if (dual) a.uy[(size_t)f * N + n] = ay;
    }
}

// One lane per SOURCE sample m: u[m] is read once and serves every channel; channel c's copy lands at n = m - delay[c]
// (consecutive lanes still write consecutive samples, the wrap apart).
__global__ __launch_bounds__(256) void k_wdm_select(WdmArgs a)
{
    const int f = blockIdx.y;
    const size_t N = a.nfft;
    const bool dual = a.cy != nullptr;
    cplx *rx = a.cx + (size_t)f * a.nch * N, *ry = dual ? a.cy + (size_t)f * a.nch * N : nullptr;
    for (unsigned m = blockIdx.x * blockDim.x + threadIdx.x; m < a.nfft; m += gridDim.x * blockDim.x) {
        const cplx u = a.ux[(size_t)f * N + m], v = dual ? a.uy[(size_t)f * N + m] : make_double2(0, 0);
        for (int c = 0; c < a.nch; c++) {
            const unsigned s = a.shift[c];
            const size_t n = (m + a.nfft - a.delay[c]) & a.mask;
            cplx px = u, py = v;
            if (s != 0) {
                const cplx w = wdm_phasor(s, m, a.mask, a.inv_n);
                px = cmulc(px, w);
                py = cmulc(py, w);
            }
            rx[(size_t)c * N + n] = px;
            if (dual) ry[(size_t)c * N + n] = py;
        }
    }
}

struct PickWdmArgs {
    const cplx *ux, *uy;         // [channel-frame][nfft]
    cplx *rx;                    // [channel-frame][2][n_out]
    unsigned nfft, n_out, stride;
    int nch;
    double scale;
    unsigned delay[WDM_MAXCH];   // delay[c] mod nfft, in [0, nfft)
};

// grid (ceil(n_out / 256), 2, channel-frames): i stride < nfft and delay < nfft, so one subtraction wraps the source index
__global__ __launch_bounds__(256) void k_pick_wdm(PickWdmArgs a)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_out) return;
    const unsigned p = blockIdx.y, cf = blockIdx.z;
    unsigned m = i * a.stride + a.delay[cf % (unsigned)a.nch];
    if (m >= a.nfft) m -= a.nfft;
    const cplx *u = p ? a.uy : a.ux;
    a.rx[((size_t)cf * 2 + p) * a.n_out + i] = cscale(u[(size_t)cf * a.nfft + m], a.scale);
}

// the checks both calls share; fills the argument block
int wdm_args(const char *who, WdmArgs &a, const void *cx, const void *cy, const void *ux, const void *uy, int64_t nfft,
             int32_t nch, int nframes, const int64_t *shift, const int64_t *delay)
{
    const std::string w(who);
    if (!cx || !ux || !shift) PLX_FAIL(PLX_ERR_ARG, w + ": null argument");
    if ((cy == nullptr) != (uy == nullptr)) PLX_FAIL(PLX_ERR_ARG, w + ": the Y channels and the Y field go together (both or neither)");
    if (nfft < 256 || nfft > ((int64_t)1 << 20) || (nfft & (nfft - 1))) PLX_FAIL(PLX_ERR_ARG, w + ": nfft must be a power of two in [256, 2^20]");
    if (nch < 1 || nch > WDM_MAXCH) PLX_FAIL(PLX_ERR_ARG, w + ": nch must be in [1, 64]");
    if (nframes < 1 || nframes > 65535) PLX_FAIL(PLX_ERR_ARG, w + ": nframes must be in [1, 65535]");
    a.cx = (cplx *)cx; a.cy = (cplx *)cy; a.ux = (cplx *)ux; a.uy = (cplx *)uy;
    a.nfft = (unsigned)nfft; a.mask = (unsigned)nfft - 1; a.nch = nch; a.inv_n = 1.0 / (double)nfft;
    for (int c = 0; c < WDM_MAXCH; c++) a.shift[c] = a.delay[c] = 0;
    for (int c = 0; c < nch; c++) {
        if (shift[c] <= -nfft / 2 || shift[c] >= nfft / 2) PLX_FAIL(PLX_ERR_ARG, w + ": |shift[c]| must be below nfft/2 (the carrier leaves the grid)");
        a.shift[c] = (unsigned)((shift[c] + nfft) & (nfft - 1));
        if (delay) {
            if (delay[c] <= -nfft || delay[c] >= nfft) PLX_FAIL(PLX_ERR_ARG, w + ": |delay[c]| must be below nfft");
            a.delay[c] = (unsigned)((delay[c] + nfft) & (nfft - 1));
        }
    }
    return PLX_OK;
}

unsigned wdm_grid(int64_t nfft)
{
    const int64_t g = nfft / 256;
    return (unsigned)(g > 1024 ? 1024 : g);
}

} // namespace

extern "C" int plx_wdm_mux_dev(const double *d_sx, const double *d_sy, double *d_ux, double *d_uy, int64_t nfft, int32_t nch,
                               int nframes, const int64_t *shift, void *stream)
{
    WdmArgs a;
    const int rc = wdm_args("plx_wdm_mux_dev", a, d_sx, d_sy, d_ux, d_uy, nfft, nch, nframes, shift, nullptr);
    if (rc) return rc;
    PLX_LAUNCH(k_wdm_mux, dim3(wdm_grid(nfft), (unsigned)nframes), dim3(256), 0, stream, a);
    PLX_HIP(hipGetLastError());
    return PLX_OK;
}

extern "C" int plx_wdm_select_dev(const double *d_ux, const double *d_uy, double *d_rx, double *d_ry, int64_t nfft, int32_t nch,
                                  int nframes, const int64_t *shift, const int64_t *delay, void *stream)
{
    WdmArgs a;
    const int rc = wdm_args("plx_wdm_select_dev", a, d_rx, d_ry, d_ux, d_uy, nfft, nch, nframes, shift, delay);
    if (rc) return rc;
    PLX_LAUNCH(k_wdm_select, dim3(wdm_grid(nfft), (unsigned)nframes), dim3(256), 0, stream, a);
    PLX_HIP(hipGetLastError());
    return PLX_OK;
}

extern "C" int plx_pick_wdm_dev(const double *d_ux, const double *d_uy, double *d_rx, int64_t nfft, int64_t n_out, int64_t stride,
                                double scale, int32_t nch, int nframes, const int64_t *delay, void *stream)
{
    const std::string w("plx_pick_wdm_dev");
    if (!d_ux || !d_uy || !d_rx || !delay) PLX_FAIL(PLX_ERR_ARG, w + ": null argument");
    if (nfft < 1 || nfft > ((int64_t)1 << 30)) PLX_FAIL(PLX_ERR_ARG, w + ": nfft must be in [1, 2^30]");
    if (nch < 1 || nch > WDM_MAXCH) PLX_FAIL(PLX_ERR_ARG, w + ": nch must be in [1, 64]");
    if (nframes < 1 || (int64_t)nframes * nch > 65535) PLX_FAIL(PLX_ERR_ARG, w + ": nframes * nch must be in [1, 65535]");
    if (n_out < 1 || stride < 1 || n_out > nfft || stride > nfft || n_out * stride > nfft)
        PLX_FAIL(PLX_ERR_ARG, w + ": selection out of range (n_out * stride must not exceed nfft)");
    PickWdmArgs a;
    a.ux = (const cplx *)d_ux; a.uy = (const cplx *)d_uy; a.rx = (cplx *)d_rx;
    a.nfft = (unsigned)nfft; a.n_out = (unsigned)n_out; a.stride = (unsigned)stride; a.nch = nch; a.scale = scale;
    for (int c = 0; c < WDM_MAXCH; c++) a.delay[c] = 0;
    for (int c = 0; c < nch; c++) {
        if (delay[c] <= -nfft || delay[c] >= nfft) PLX_FAIL(PLX_ERR_ARG, w + ": |delay[c]| must be below nfft");
        a.delay[c] = (unsigned)((delay[c] + nfft) % nfft);
    }
    PLX_LAUNCH(k_pick_wdm, dim3((unsigned)((n_out + 255) / 256), 2, (unsigned)(nframes * nch)), dim3(256), 0, stream, a);
    PLX_HIP(hipGetLastError());
    return PLX_OK;
}
