// plx_tx.hip -- a PDM-QPSK transmitter on the device: every realisation draws its own data.
//
// The waveform is the reference's Tx chain (electricsource 'cosroll' -> qi_modulator -> create_field(..., power
// 'average')) on random bits.  A cosroll pulse spans two symbol slots, so sample n = m nt + j of a stream's drive is
// sigma el[nt + j] + sigma' el[j] with the signs of symbols m and m + 1, and the modulator's sin(pi/2 .) is odd: a sample
// is +- one of TWO magnitudes per j,
//   drive[0][j] = sin(pi/2 (el[nt + j] + el[j]))   (b[m] == b[m + 1])      drive[1][j] = sin(pi/2 (el[nt + j] - el[j]))
// which the caller tabulates on the host.  The kernels evaluate no transcendental function:
//   k_tx_bits   one workgroup per channel-frame: the Philox words of its four bit streams, the pattern bytes beside the
//               field (d_pat, d_pat_dq), the number of transitions ntr (an integer, so the power below does not depend on a
//               reduction order) and from it the realisation's power after create_field's 'average' normalisation
//   k_tx_wave   a pure store stream: x[n] = ((a drive[t_0][j]) sigma_0) k + i ((a drive[t_1][j]) sigma_1) k, y from streams
//               2, 3; consecutive lanes on consecutive samples, 16-B stores, 32 B per dual-polarisation sample
// Bits: word group q = m >> 5 of channel c is ONE Philox-4x32-10 call, counter (lo32(q), hi32(q), c, PLX_PHILOX_TX_DATA),
// key as in plx_philox.h; b_s[m] = (r_s >> (m & 31)) & 1.
#include "../../include/polmux_hip.h"
#include "plx_philox.h"

#include <cmath>

namespace {

constexpr int kThreads = 256, kPer = 8, kTile = kThreads * kPer;   // samples of one polarisation per workgroup of k_tx_wave
constexpr int kMaxNt = 64;

struct TxArgs {
    cplx *ux, *uy;            // [frame][nfc][nsymb nt]
    uint8_t *pat, *pat_dq;    // [frame][nfc][4][nsymb] (pat_dq may be null)
    double *power;            // [frame][nfc]
    const int64_t *keys;      // per-frame keys (null: the frame index)
    uint64_t seed;
    int64_t nsymb;
    int nt, lognt, nfc;
    double a, pavg, e0, e1;   // a = sqrt(pavg) / sqrt(2); e_t = sum_j drive[t][j]^2
    double drive[2 * kMaxNt]; // [2][nt], packed
};

__device__ __forceinline__ void tx_words(const TxArgs &a, uint32_t q, int c, uint32_t k0, uint32_t k1, uint32_t *r)
{
    philox4x32(q, 0u, (uint32_t)c, (uint32_t)PLX_PHILOX_TX_DATA, k0, k1, r);
}

// bits 0 .. nb - 1 of w as nb bytes at dst (8-byte aligned; nb a multiple of 8)
__device__ __forceinline__ void put_bits(uint8_t *dst, uint32_t w, int nb)
{
    for (int k = 0; k < nb; k += 8) {
        uint64_t v = 0;
        for (int b = 0; b < 8; b++) v |= (uint64_t)((w >> (k + b)) & 1u) << (8 * b);
        *(uint64_t *)(dst + k) = v;
    }
}

__global__ __launch_bounds__(kThreads) void k_tx_bits(TxArgs a)
{
    PLX_DYN_LDS(lds);
    int *red = (int *)lds;
    const int c = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
    const size_t cf = (size_t)f * a.nfc + c;
    const uint64_t key = a.keys ? (uint64_t)a.keys[f] : (uint64_t)f;
    const uint32_t k0 = (uint32_t)(a.seed ^ key), k1 = (uint32_t)((a.seed >> 32) ^ (key * 0x9E3779B97F4A7C15ull >> 32));
    const int nb = a.nsymb >= 32 ? 32 : (int)a.nsymb;                 // symbols a word group holds (16 symbols: half a word)
    const int nwords = a.nsymb >= 32 ? (int)(a.nsymb >> 5) : 1;
    const uint32_t mask = nb == 32 ? 0xFFFFFFFFu : (1u << nb) - 1u;
    uint8_t *pat = a.pat + cf * 4 * (size_t)a.nsymb;
    uint8_t *pdq = a.pat_dq ? a.pat_dq + cf * 4 * (size_t)a.nsymb : nullptr;
    int ntr = 0;
    for (int q = tid; q < nwords; q += kThreads) {
        uint32_t r[4], rn[4], rp[4];
        tx_words(a, (uint32_t)q, c, k0, k1, r);
        for (int s = 0; s < 4; s++) rn[s] = rp[s] = r[s];             // one word group: the circular neighbours are inside it
        if (nwords > 1) tx_words(a, (uint32_t)(q + 1 == nwords ? 0 : q + 1), c, k0, k1, rn);
        uint32_t cur[4], prv[4];
        for (int s = 0; s < 4; s++) {
            cur[s] = r[s] & mask;
            const uint32_t nxt = (cur[s] >> 1) | ((rn[s] & 1u) << (nb - 1));   // bit i = b[m + 1]
            ntr += __builtin_popcount((cur[s] ^ nxt) & mask);
            put_bits(pat + (size_t)s * a.nsymb + (size_t)q * 32, cur[s], nb);
        }
        if (!pdq) continue;
        if (nwords > 1) tx_words(a, (uint32_t)(q == 0 ? nwords - 1 : q - 1), c, k0, k1, rp);
        for (int s = 0; s < 4; s++) prv[s] = ((cur[s] << 1) | ((rp[s] >> (nb - 1)) & 1u)) & mask;   // bit i = b[m - 1]
        for (int p = 0; p < 2; p++) {
            // pat_decoder(pat, 'dqpsk') on 32 symbols at once: quarter turns g = [0, 1, 3, 2][2 first + second] have the bits
            // (first, first ^ second); d = (g[m - 1] - g[m]) mod 4; (u, v) = (d >> 1, (d >> 1) ^ (d & 1)); rows 1 - u, 1 - v
            const uint32_t gh = cur[2 * p], gl = cur[2 * p] ^ cur[2 * p + 1];
            const uint32_t ph = prv[2 * p], pl = prv[2 * p] ^ prv[2 * p + 1];
            const uint32_t dl = pl ^ gl, dh = ph ^ gh ^ (~pl & gl);
            put_bits(pdq + (size_t)(2 * p) * a.nsymb + (size_t)q * 32, ~dh & mask, nb);
            put_bits(pdq + (size_t)(2 * p + 1) * a.nsymb + (size_t)q * 32, ~(dh ^ dl) & mask, nb);
        }
    }
    // ntr of the channel-frame: over the wave, then over the four waves
    for (int m = 32; m >= 1; m >>= 1) ntr += __shfl_xor(ntr, m, 64);
    if ((tid & 63) == 0) red[tid >> 6] = ntr;
    __syncthreads();
    if (tid == 0) {
        ntr = (red[0] + red[1]) + (red[2] + red[3]);
        // create_field.m:113-124: avge = mean(|x|^2 + |y|^2) of the unnormalised field, counted instead of summed
        const double avge = 0.5 * a.pavg * ((double)(4 * a.nsymb - ntr) * a.e0 + (double)ntr * a.e1) / ((double)a.nsymb * (double)a.nt);
        a.power[cf] = a.pavg * a.pavg / avge;
    }
}

__global__ __launch_bounds__(kThreads) void k_tx_wave(TxArgs a)
{
    PLX_DYN_LDS(lds);
    double *drv = (double *)lds;                           // [2][nt]
    uint8_t *code = (uint8_t *)(drv + 2 * kMaxNt);         // per symbol of the tile: bits 0-3 b_s[m], bits 4-7 b_s[m] ^ b_s[m + 1]
    const int c = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
    const size_t cf = (size_t)f * a.nfc + c;
    const int64_t nfft = a.nsymb << a.lognt, t0 = (int64_t)blockIdx.x * kTile;
    const int64_t left = nfft - t0;
    const int ns = (int)(left < kTile ? left : kTile);     // samples of this tile (a multiple of 256, so of nt)
    if (tid < 2 * a.nt) drv[tid] = a.drive[tid];
    const uint8_t *pat = a.pat + cf * 4 * (size_t)a.nsymb;
    const int64_t m0 = t0 >> a.lognt;
    for (int i = tid; i < (ns >> a.lognt); i += kThreads) {
        const int64_t m = m0 + i, m1 = (m + 1) & (a.nsymb - 1);
        unsigned cd = 0;
        for (int s = 0; s < 4; s++) {
            const unsigned b = pat[(size_t)s * a.nsymb + m], b1 = pat[(size_t)s * a.nsymb + m1];
            cd |= (b << s) | ((b ^ b1) << (4 + s));
        }
        code[i] = (uint8_t)cd;
    }
    __syncthreads();
    // the tile starts on a multiple of 256 and nt divides 256: j is the lane's own for the whole tile
    const double k = sqrt(a.power[cf] / a.pavg);           // sqrt(pavg / avge) of create_field, from the power k_tx_bits left
    const int j = tid & (a.nt - 1);
    const double v0 = (a.a * drv[j]) * k, v1 = (a.a * drv[a.nt + j]) * k;   // ((a drive) sigma) k: the sign is exact anywhere
    cplx *ux = a.ux + cf * (size_t)nfft + t0, *uy = a.uy + cf * (size_t)nfft + t0;
#pragma unroll
    for (int s = 0; s < kPer; s++) {
        const int i = s * kThreads + tid;
        if (i >= ns) break;
        const unsigned cd = code[i >> a.lognt];
        const double xr = (cd & 16u) ? v1 : v0, xi = (cd & 32u) ? v1 : v0;
        const double yr = (cd & 64u) ? v1 : v0, yi = (cd & 128u) ? v1 : v0;
        ux[i] = make_double2((cd & 1u) ? xr : -xr, (cd & 2u) ? xi : -xi);
        uy[i] = make_double2((cd & 4u) ? yr : -yr, (cd & 8u) ? yi : -yi);
    }
}

} // namespace

extern "C" int plx_tx_qpsk_dev(double *d_ux, double *d_uy, int64_t nsymb, int32_t nt, int32_t nfc, int nframes,
                               const double *drive, double pavg_mw, uint64_t seed, const int64_t *d_keys, uint8_t *d_pat,
                               uint8_t *d_pat_dq, double *d_power, void *stream)
{
    if (!d_ux || !d_uy || !drive || !d_pat || !d_power) PLX_FAIL(PLX_ERR_ARG, "plx_tx_qpsk_dev: null argument");
    if (nsymb < 16 || nsymb > ((int64_t)1 << 19) || (nsymb & (nsymb - 1)))
        PLX_FAIL(PLX_ERR_ARG, "plx_tx_qpsk_dev: nsymb must be a power of two in [16, 2^19]");
    if (nt < 2 || nt > kMaxNt || (nt & (nt - 1))) PLX_FAIL(PLX_ERR_ARG, "plx_tx_qpsk_dev: nt must be a power of two in [2, 64]");
    if (nsymb * nt < 256 || nsymb * nt > ((int64_t)1 << 20)) PLX_FAIL(PLX_ERR_ARG, "plx_tx_qpsk_dev: nsymb * nt must be in [256, 2^20]");
    if (nfc < 1 || nfc > 64) PLX_FAIL(PLX_ERR_ARG, "plx_tx_qpsk_dev: nfc must be in [1, 64]");
    if (nframes < 1 || nframes > 65535) PLX_FAIL(PLX_ERR_ARG, "plx_tx_qpsk_dev: nframes must be in [1, 65535]");
    if (!std::isfinite(pavg_mw) || !(pavg_mw > 0)) PLX_FAIL(PLX_ERR_ARG, "plx_tx_qpsk_dev: pavg_mw must be finite and > 0");
    if (((uintptr_t)d_pat | (uintptr_t)d_pat_dq) & 7) PLX_FAIL(PLX_ERR_ARG, "plx_tx_qpsk_dev: d_pat and d_pat_dq must be 8-byte aligned");
    TxArgs a;
    double e[2] = {0.0, 0.0};
    for (int t = 0; t < 2; t++)
        for (int j = 0; j < nt; j++) {
            const double d = drive[t * nt + j];
            if (!std::isfinite(d)) PLX_FAIL(PLX_ERR_ARG, "plx_tx_qpsk_dev: drive must be finite");
            a.drive[t * nt + j] = d;
            e[t] += d * d;
        }
    for (int i = 2 * nt; i < 2 * kMaxNt; i++) a.drive[i] = 0.0;
    if (!(e[0] > 0)) PLX_FAIL(PLX_ERR_ARG, "plx_tx_qpsk_dev: drive[0] is all zero (a frame of equal symbols would carry no power)");
    a.ux = (cplx *)d_ux; a.uy = (cplx *)d_uy; a.pat = d_pat; a.pat_dq = d_pat_dq; a.power = d_power; a.keys = d_keys;
    a.seed = seed; a.nsymb = nsymb; a.nt = nt; a.nfc = nfc;
    a.lognt = 0;
    while ((1 << a.lognt) < nt) a.lognt++;
    a.a = std::sqrt(pavg_mw) / std::sqrt(2.0); a.pavg = pavg_mw; a.e0 = e[0]; a.e1 = e[1];
    const int64_t nfft = nsymb * nt;
    PLX_LAUNCH(k_tx_bits, dim3(1, (unsigned)nfc, (unsigned)nframes), dim3(kThreads), 4 * sizeof(int), stream, a);
    PLX_LAUNCH(k_tx_wave, dim3((unsigned)((nfft + kTile - 1) / kTile), (unsigned)nfc, (unsigned)nframes), dim3(kThreads),
               2 * kMaxNt * sizeof(double) + kTile / 2, stream, a);
    PLX_HIP(hipGetLastError());
    return PLX_OK;
}
