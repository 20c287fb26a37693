// plx_phase.hip -- laser phase noise on the device: the Wiener phase of lasersource.m:182-192 (transmitter) and
// receiver_cohmix.m:206-216 (local oscillator), per (frame key, channel, laser).
//
//   sigma = sqrt(2 pi linewidth / NT);  inc[0] = 0, inc[k] = sigma * n[k];  phi = cumsum(inc);
//   phi_b[k] = phi[k] - k / (N - 1) * phi[N - 1]        (Brownian bridge, N = nfft)
//
// n[k] is the cosine branch of Box-Muller on Philox-4x32-10 (plx_philox.h) with counter (k lo, k hi, channel, tag),
// tag 2 = transmitter, 3 = LO.  The cumulative sum runs across tiles of 2048 samples in two passes and keeps no
// [frame][nfft] buffer of normals: pass 1 writes each tile's sum of increments; pass 2 regenerates the tile's
// normals, adds the exclusive prefix of the tile sums to an in-tile scan, bridges with the total of ALL tile sums
// (the same value in every workgroup of a (frame, channel)) and applies the phase.  A 2^20-sample frame is 512
// workgroups per channel in each pass.
#include "plx_internal.h"
#include "plx_philox.h"

#include <cmath>

namespace {

constexpr int kThreads = 256, kPer = 8, kTile = kThreads * kPer;

struct PhaseArgs {
    int64_t nfft;
    int nfc, tag, ntiles;
    double sigma[64];         // per channel
    uint64_t seed;
    const int64_t *keys;      // per-frame keys (null: the frame index)
    const double *phi_in;     // injected phase [frame][nfc][nfft] (null: generated)
    cplx *ux, *uy;            // targets: u[(f nfc + c) pitch + j] *= exp(i sign phi[j stride])
    int64_t stride, pitch;
    double sign;
    double *phi_out;          // [frame][nfc][nfft] phi_b (generated route only)
    double *tile_sum;         // [frame][nfc][ntiles]
};

__device__ __forceinline__ double normal_at(const PhaseArgs &a, int64_t k, int c, uint64_t key)
{
    uint32_t r[4];
    philox4x32((uint32_t)k, (uint32_t)((uint64_t)k >> 32), (uint32_t)c, (uint32_t)a.tag,
               (uint32_t)(a.seed ^ key), (uint32_t)((a.seed >> 32) ^ (key * 0x9E3779B97F4A7C15ull >> 32)), r);
    const double u1 = ((double)(((uint64_t)r[0] << 21) ^ (r[1] >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
    const double u2 = ((double)(((uint64_t)r[2] << 21) ^ (r[3] >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
    return sqrt(-2.0 * log(u1)) * cos(6.28318530717958647692 * u2);
}

// the increments of this thread's kPer consecutive samples (zero past nfft, and at k = 0: freq_noise(1) = 0)
__device__ __forceinline__ void increments(const PhaseArgs &a, int64_t k0, int c, uint64_t key, double *inc)
{
    const double sg = a.sigma[c];
    for (int s = 0; s < kPer; s++) {
        const int64_t k = k0 + s;
        inc[s] = (k > 0 && k < a.nfft) ? sg * normal_at(a, k, c, key) : 0.0;
    }
}

// sum over the workgroup, the same order in every workgroup (red: 4 doubles of LDS)
__device__ __forceinline__ double block_sum(double v, double *red)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kThreads) void k_phase_tile_sums(PhaseArgs a)
{
    PLX_DYN_LDS(lds);
    double *red = (double *)lds;
    const int t = blockIdx.x, c = blockIdx.y, f = blockIdx.z;
    const uint64_t key = a.keys ? (uint64_t)a.keys[f] : (uint64_t)f;
    double inc[kPer];
    increments(a, (int64_t)t * kTile + (int64_t)threadIdx.x * kPer, c, key, inc);
    double s = 0;
    for (int i = 0; i < kPer; i++) s += inc[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) a.tile_sum[((size_t)f * a.nfc + c) * a.ntiles + t] = s;
}

// pass 2 (or the injected route): phi_b of the tile, staged in LDS, then written and applied with consecutive lanes on
// consecutive samples
__global__ __launch_bounds__(kThreads) void k_phase_apply(PhaseArgs a)
{
    PLX_DYN_LDS(lds);
    double *red = (double *)lds, *wsum = red + 4, *tile = red + 8;
    const int t = blockIdx.x, c = blockIdx.y, f = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t fc = (size_t)f * a.nfc + c;
    const int64_t t0 = (int64_t)t * kTile;
    if (!a.phi_in) {
        const uint64_t key = a.keys ? (uint64_t)a.keys[f] : (uint64_t)f;
        // exclusive prefix of the tile sums before tile t, and their total (pass 1)
        const double *ts = a.tile_sum + fc * a.ntiles;
        double pre = 0, tot = 0;
        for (int j = tid; j < a.ntiles; j += kThreads) {
            tot += ts[j];
            if (j < t) pre += ts[j];
        }
        pre = block_sum(pre, red);
        tot = block_sum(tot, red);
        // in-tile inclusive scan: thread-serial over kPer samples, then across the wave, then across the four waves
        double phi[kPer];
        const int64_t k0 = t0 + (int64_t)tid * kPer;
        increments(a, k0, c, key, phi);
        for (int s = 1; s < kPer; s++) phi[s] += phi[s - 1];
        const double own = phi[kPer - 1];
        double v = own;
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl(v, lane - d, 64);
            if (lane >= d) v += o;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        double off = pre + (v - own);
        for (int w = 0; w < wave; w++) off += wsum[w];
        const double slope = tot / (double)(a.nfft - 1);
        for (int s = 0; s < kPer; s++) tile[tid * kPer + s] = (off + phi[s]) - (double)(k0 + s) * slope;
        __syncthreads();
    }
    for (int s = 0; s < kPer; s++) {
        const int i = s * kThreads + tid;
        const int64_t k = t0 + i;
        if (k >= a.nfft) break;
        if (a.phi_out) a.phi_out[fc * a.nfft + k] = tile[i];
        if (!a.ux || k % a.stride) continue;
        const double p = a.phi_in ? a.phi_in[fc * a.nfft + k] : tile[i];
        const cplx r = cexpi(a.sign * p);
        const size_t o = fc * a.pitch + k / a.stride;
        a.ux[o] = cmul(a.ux[o], r);
        if (a.uy) a.uy[o] = cmul(a.uy[o], r);
    }
}

} // namespace

extern "C" int plx_phase_noise_dev(double *d_ux, double *d_uy, int64_t stride, int64_t pitch, double sign, int64_t nfft,
                                   int32_t nfc, int nframes, const double *sigma, uint64_t seed, const int64_t *d_keys,
                                   int32_t tag, const double *d_phi_in, double *d_phi_out, double *d_work, void *stream)
{
    if (nfft < 256 || nfft > (1 << 20) || (nfft & (nfft - 1)))
        PLX_FAIL(PLX_ERR_ARG, "plx_phase_noise_dev: nfft must be a power of two in [256, 2^20]");
    if (nfc < 1 || nfc > 64 || nframes < 1) PLX_FAIL(PLX_ERR_ARG, "plx_phase_noise_dev: nfc outside [1, 64] or no frames");
    if (!d_ux && !d_phi_out) PLX_FAIL(PLX_ERR_ARG, "plx_phase_noise_dev: nothing to write");
    if (d_ux && (stride < 1 || nfft % stride || pitch < nfft / stride))
        PLX_FAIL(PLX_ERR_ARG, "plx_phase_noise_dev: stride must divide nfft and pitch hold nfft / stride samples");
    if (!d_phi_in && (!sigma || !d_work)) PLX_FAIL(PLX_ERR_ARG, "plx_phase_noise_dev: the generator needs sigma and d_work");
    if (d_phi_in && d_phi_out) PLX_FAIL(PLX_ERR_ARG, "plx_phase_noise_dev: an injected phase is not written back");
    if (tag != PLX_PHASE_TX && tag != PLX_PHASE_LO) PLX_FAIL(PLX_ERR_ARG, "plx_phase_noise_dev: tag must be PLX_PHASE_TX or PLX_PHASE_LO");
    PhaseArgs a;
    a.nfft = nfft; a.nfc = nfc; a.tag = tag; a.ntiles = (int)((nfft + kTile - 1) / kTile);
    for (int c = 0; c < 64; c++) {
        a.sigma[c] = (sigma && c < nfc) ? sigma[c] : 0.0;
        if (!(a.sigma[c] >= 0) || !std::isfinite(a.sigma[c])) PLX_FAIL(PLX_ERR_ARG, "plx_phase_noise_dev: sigma must be finite and >= 0");
    }
    a.seed = seed; a.keys = d_keys; a.phi_in = d_phi_in; a.ux = (cplx *)d_ux; a.uy = (cplx *)d_uy;
    a.stride = stride; a.pitch = pitch; a.sign = sign; a.phi_out = d_phi_out; a.tile_sum = d_work;
    const dim3 grid((unsigned)a.ntiles, (unsigned)nfc, (unsigned)nframes);
    if (!d_phi_in) PLX_LAUNCH(k_phase_tile_sums, grid, dim3(kThreads), 4 * sizeof(double), stream, a);
    PLX_LAUNCH(k_phase_apply, grid, dim3(kThreads), (8 + kTile) * sizeof(double), stream, a);
    PLX_HIP(hipGetLastError());
    return PLX_OK;
}
