// plx_detune.hip -- the local oscillator's frequency offset on the device: receiver_cohmix.m:188-200 (x.lodetuning) with
// an offset of its own per (frame key, channel).
//
//   b = d_bins_in[f nfc + c], or k0 + d with d uniform on -kspread .. kspread from ONE Philox-4x32-10 call
//       (plx_philox.h), counter (0, 0, c, PLX_PHILOX_LO_DETUNE): d = ((r0 * (2 kspread + 1)) >> 32) - kspread
//   theta[n] = 2 pi (((b mod nfft) (n + 1)) mod nfft) / nfft                 (1-based, as receiver_cohmix.m:197)
//
// The product is reduced modulo nfft in 64-bit integers (both factors are below 2^20 + 1: it fits 41 bits), so theta carries
// ONE rounding whatever n and b.  One launch: a one-dimensional grid of at most 2048 workgroups strides over (channel-frame,
// tile) items of 2048 samples.  With d_phi the tiles cover the nfft samples of theta (two consecutive samples = 16 bytes per
// lane, consecutive lanes on consecutive pairs) and the phasor is applied to the samples of the tile that fall on the stride;
// without it the tiles cover the nfft / stride target samples alone.
#include "plx_internal.h"
#include "plx_philox.h"

namespace {

constexpr int kThreads = 256, kTile = 2048, kMaxGrid = 2048;

struct DetuneArgs {
    int64_t nfft, stride, pitch, k0, kspread, ntiles, nitems;
    int nfc;
    int32_t accumulate;
    double sign;
    uint64_t seed;
    const int64_t *keys;      // per-frame keys (null: the frame index)
    const int32_t *bins_in;   // [frame][nfc] injected offsets (null: k0 + the draw)
    cplx *ux, *uy;            // targets: u[(f nfc + c) pitch + j] *= exp(i sign theta[j stride])
    double *phi;              // [frame][nfc][nfft]: = theta, or += theta
    int32_t *bins_out;        // [frame][nfc]
};

// the offset of channel c of frame f in bins
__device__ __forceinline__ int64_t bin_of(const DetuneArgs &a, int64_t f, int c)
{
    if (a.bins_in) return (int64_t)a.bins_in[f * a.nfc + c];
    if (a.kspread == 0) return a.k0;
    const uint64_t key = a.keys ? (uint64_t)a.keys[f] : (uint64_t)f;
    uint32_t r[4];
    philox4x32(0u, 0u, (uint32_t)c, (uint32_t)PLX_PHILOX_LO_DETUNE, (uint32_t)(a.seed ^ key),
               (uint32_t)((a.seed >> 32) ^ (key * 0x9E3779B97F4A7C15ull >> 32)), r);
    const int64_t d = (int64_t)(((uint64_t)r[0] * (uint64_t)(2 * a.kspread + 1)) >> 32) - a.kspread;
    return a.k0 + d;
}

// theta of sample n (0-based) for the reduced offset bm in [0, nfft): m / nfft is exact, the product with 2 pi rounds once
__device__ __forceinline__ double theta_at(int64_t bm, int64_t n, int64_t mask, double inv)
{
    const int64_t m = (bm * (n + 1)) & mask;
    return 6.28318530717958647692 * ((double)m * inv);
}

__global__ __launch_bounds__(kThreads) void k_lo_detune(DetuneArgs a)
{
    const int tid = threadIdx.x;
    const int64_t mask = a.nfft - 1;
    const double inv = 1.0 / (double)a.nfft;
    for (int64_t item = blockIdx.x; item < a.nitems; item += gridDim.x) {
        const int64_t cf = item / a.ntiles, t0 = (item - cf * a.ntiles) * kTile;
        const int64_t b = bin_of(a, cf / a.nfc, (int)(cf % a.nfc));
        const int64_t bm = b & mask;                       // b mod nfft, in [0, nfft) for either sign (two's complement)
        if (a.bins_out && t0 == 0 && tid == 0) a.bins_out[cf] = (int32_t)b;
        if (a.phi) {
            double *row = a.phi + cf * a.nfft;
            for (int i = 2 * tid; i < kTile; i += 2 * kThreads) {
                const int64_t n = t0 + i;
                if (n >= a.nfft) break;                    // (nfft is even: a pair never straddles the end)
                double2 v = make_double2(theta_at(bm, n, mask, inv), theta_at(bm, n + 1, mask, inv));
                double2 *p = (double2 *)(row + n);
                if (a.accumulate) {
                    const double2 o = *p;
                    v.x += o.x; v.y += o.y;
                }
                *p = v;
            }
        }
        if (a.ux) {
            const int64_t end = a.phi ? a.nfft : a.nfft / a.stride;    // the tiles cover samples of theta, or target samples
            for (int i = tid; i < kTile; i += kThreads) {
                const int64_t q = t0 + i;
                if (q >= end) break;
                int64_t n, j;
                if (a.phi) {
                    if (q % a.stride) continue;
                    n = q; j = q / a.stride;
                } else {
                    j = q; n = q * a.stride;
                }
                const cplx r = cexpi(a.sign * theta_at(bm, n, mask, inv));
                const size_t o = (size_t)cf * a.pitch + j;
                a.ux[o] = cmul(a.ux[o], r);
                if (a.uy) a.uy[o] = cmul(a.uy[o], r);
            }
        }
    }
}

} // namespace

extern "C" int plx_lo_detune_dev(double *d_ux, double *d_uy, int64_t stride, int64_t pitch, double sign, int64_t nfft,
                                 int32_t nfc, int nframes, int64_t k0, int64_t kspread, uint64_t seed, const int64_t *d_keys,
                                 const int32_t *d_bins_in, double *d_phi, int32_t phi_accumulate, int32_t *d_bins_out,
                                 void *stream)
{
    if (nfft < 256 || nfft > (1 << 20) || (nfft & (nfft - 1)))
        PLX_FAIL(PLX_ERR_ARG, "plx_lo_detune_dev: nfft must be a power of two in [256, 2^20]");
    if (nfc < 1 || nfc > 64 || nframes < 1) PLX_FAIL(PLX_ERR_ARG, "plx_lo_detune_dev: nfc outside [1, 64] or no frames");
    if (!d_ux && !d_phi && !d_bins_out) PLX_FAIL(PLX_ERR_ARG, "plx_lo_detune_dev: nothing to write");
    if (d_uy && !d_ux) PLX_FAIL(PLX_ERR_ARG, "plx_lo_detune_dev: d_uy needs d_ux");
    if (d_ux && (stride < 1 || nfft % stride || pitch < nfft / stride))
        PLX_FAIL(PLX_ERR_ARG, "plx_lo_detune_dev: stride must divide nfft and pitch hold nfft / stride samples");
    if ((uintptr_t)d_phi & 15) PLX_FAIL(PLX_ERR_ARG, "plx_lo_detune_dev: d_phi must be 16-byte aligned");
    if (!d_bins_in) {
        if (kspread < 0 || 2 * kspread + 1 > nfft)
            PLX_FAIL(PLX_ERR_ARG, "plx_lo_detune_dev: kspread must be >= 0 and 2 kspread + 1 <= nfft");
        if (k0 < -(1ll << 30) || k0 > (1ll << 30)) PLX_FAIL(PLX_ERR_ARG, "plx_lo_detune_dev: |k0| must not exceed 2^30");
    }
    DetuneArgs a;
    a.nfft = nfft; a.nfc = nfc; a.stride = d_ux ? stride : 1; a.pitch = pitch; a.sign = sign;
    a.k0 = k0; a.kspread = d_bins_in ? 0 : kspread; a.seed = seed; a.keys = d_keys; a.bins_in = d_bins_in;
    a.ux = (cplx *)d_ux; a.uy = (cplx *)d_uy; a.phi = d_phi; a.accumulate = phi_accumulate; a.bins_out = d_bins_out;
    const int64_t span = d_phi ? nfft : (d_ux ? nfft / stride : 1);
    a.ntiles = (span + kTile - 1) / kTile;
    a.nitems = (int64_t)nframes * nfc * a.ntiles;
    const unsigned grid = (unsigned)(a.nitems < kMaxGrid ? a.nitems : kMaxGrid);
    PLX_LAUNCH(k_lo_detune, dim3(grid), dim3(kThreads), 0, stream, a);
    PLX_HIP(hipGetLastError());
    return PLX_OK;
}
