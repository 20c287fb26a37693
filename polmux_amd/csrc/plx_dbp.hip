// plx_dbp.hip -- digital backpropagation: the receiver-side inverse of matrix_ssfm (fiber.m:459-555, :807-852).
//
// One forward step of length dz is NL(dz), then LIN(dz) = ifft(fft(u) .* exp(-i betat dz)), then the loss
// exp(-alphalin dz / 2).  Its inverse, in the opposite order: u *= exp(+alphalin dz / 2); u = ifft(fft(u) .*
// exp(+i betat dz)); the inverse Kerr step (both nonlinear forms are unitary and leave |ux|^2 + |uy|^2 and the Stokes
// component s3 unchanged, so the phases can be computed from the field they are applied to).  A span is its steps in
// reverse order behind u *= exp(-alphalin L / 2) (the amplifier after it).  No PMD.
//
// Two routes:
//   resident  (nfft <= 4096): k_dbp_resident, one workgroup per frame.  The dual-polarisation frame lives in LDS
//             (2 nfft x 16 B, 128 KiB at 4096) from its load to its store; every step of every span runs on chip: a
//             DIF forward transform (natural -> bit-reversed), the spectral multiplier exp(+i betat dz) with the step's
//             scalar factors and 1/nfft folded in (betat stored bit-reversed, in turns), a DIT inverse (bit-reversed ->
//             natural) and the Kerr step.  No bit-reversal pass.  The half twiddle table sits in LDS when it fits next
//             to the field (nfft <= 2048) and is read through the caches otherwise.  One HBM round trip per frame.
//   streamed  (larger nfft, or PLX_DBP_STREAMED): per step the SSFM plan's FFT engine as a spectral filter
//             (plx_ssfm_filter_dev) over the 2 nframes single-polarisation rows of [frame][X|Y][nfft] -- without PMD
//             the linear step does not couple the polarisations -- with one table exp(+i betat dz) per distinct step
//             length, then k_dbp_kerr, which pairs X and Y of each frame and applies the Kerr step and the scalar
//             factors that separate it from the next filter.
#include "../../include/polmux_hip.h"
#include "plx_fft.h"
#include "plx_gateway.h"
#include "plx_internal.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

const int64_t kResidentMax = 4096;     // 2 x 4096 x 16 B = 128 KiB of the 160 KiB LDS of a CU
const size_t kLdsMax = 160 * 1024;

// per-step constants of one span, in execution order (the forward list reversed)
struct DbpStep {
    double g;      // scalar factor applied before the linear step (loss undone, span amplifier undone, 1/nfft folded in on the resident route)
    double dz;     // step length [m] (spectral phase betat dz)
    double c;      // xi gam leff(dz) (times 8/9 for Manakov)
};

struct DbpArgs {
    const cplx *in;
    cplx *out;
    const double *scale;     // [nframes] or nullptr
    const cplx *tw;          // half table W_N^k, k < N/2
    const double *bt;        // resident: -betat / 2 pi at bit-reversed position; streamed: unused
    const DbpStep *steps;    // [nsteps]
    int logN, nsteps, nspans, manakov, tw_in_lds;
};

// inverse Kerr step on one sample pair (fiber.m:826-850 inverted)
__device__ __forceinline__ void kerr_inv(cplx &ux, cplx &uy, double c, int manakov)
{
    const double p = ux.x * ux.x + ux.y * ux.y + uy.x * uy.x + uy.y * uy.y;
    if (!manakov) {   // undo the rotation [cos phi, sin phi; -sin phi, cos phi], phi = c s3 / 3
        const double s3 = 2.0 * (ux.x * uy.y - ux.y * uy.x);
        double sn, cs;
        sincos(c * s3 * (1.0 / 3.0), &sn, &cs);
        const cplx nx = make_double2(cs * ux.x - sn * uy.x, cs * ux.y - sn * uy.y);
        const cplx ny = make_double2(sn * ux.x + cs * uy.x, sn * ux.y + cs * uy.y);
        ux = nx; uy = ny;
    }
    const cplx e = cexpi(c * p);
    ux = cmul(ux, e);
    uy = cmul(uy, e);
}

__global__ __launch_bounds__(1024) void k_dbp_resident(DbpArgs a)
{
    PLX_DYN_LDS(lds);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int N = 1 << a.logN;
    cplx *s = (cplx *)lds;                 // [2][N]: X then Y
    const size_t f = blockIdx.x;
    const cplx *tw = a.tw;
    if (a.tw_in_lds) {
        cplx *t = s + 2 * N;
        lds_load_twiddles(t, a.tw, N >> 1, tid, nthr);
        tw = t;
    }
    const double sc = a.scale ? a.scale[f] : 1.0;
    const cplx *x = a.in + f * 2 * (size_t)N;
    for (int e = tid; e < 2 * N; e += nthr) s[e] = cscale(x[e], sc);
    __syncthreads();
    for (int sp = 0; sp < a.nspans; sp++) {
        for (int k = 0; k < a.nsteps; k++) {
            const DbpStep st = a.steps[k];
            lds_fft_dif(s, a.logN, 1, N, 1, tw, tid, nthr, false);
            for (int i = tid; i < N; i += nthr) {      // position i holds bin bitrev(i) of both polarisations
                const cplx h = cscale(cexp_neg_turns(a.bt[i] * st.dz), st.g);
                s[i] = cmul(s[i], h);
                s[N + i] = cmul(s[N + i], h);
            }
            __syncthreads();
            lds_fft_dit(s, a.logN, 1, N, 1, tw, tid, nthr, false);
            for (int i = tid; i < N; i += nthr) {
                cplx ux = s[i], uy = s[N + i];
                kerr_inv(ux, uy, st.c, a.manakov);
                s[i] = ux; s[N + i] = uy;
            }
            __syncthreads();
        }
    }
    cplx *y = a.out + f * 2 * (size_t)N;
    const double inv = 1.0 / sc;
    for (int e = tid; e < 2 * N; e += nthr) y[e] = cscale(s[e], inv);
}

// streamed route, element-wise part: u = [frame][X|Y][N].  pre: multiply by g (times scale[f] if sc_mode == 1) only;
// otherwise the Kerr step with coefficient c, then the factor g (divided by scale[f] if sc_mode == 2).
struct KerrArgs {
    const cplx *in;
    cplx *out;
    const double *scale;
    int64_t N;
    double c, g;
    int manakov, kerr, sc_mode;
};

__global__ __launch_bounds__(256) void k_dbp_kerr(KerrArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.N) return;
    const size_t f = blockIdx.y;
    const size_t ox = f * 2 * (size_t)a.N + (size_t)i, oy = ox + (size_t)a.N;
    cplx ux = a.in[ox], uy = a.in[oy];
    if (a.kerr) kerr_inv(ux, uy, a.c, a.manakov);
    double g = a.g;
    if (a.scale && a.sc_mode == 1) g *= a.scale[f];
    if (a.scale && a.sc_mode == 2) g /= a.scale[f];
    a.out[ox] = cscale(ux, g);
    a.out[oy] = cscale(uy, g);
}

int ilog2i(int64_t v)
{
    int l = 0;
    while (((int64_t)1 << l) < v) l++;
    return l;
}

#ifndef PLX_EMU
template <class K> hipError_t allow_lds(K kern, size_t bytes)
{
    return hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
#else
template <class K> hipError_t allow_lds(K, size_t) { return hipSuccess; }
#endif

} // namespace

struct plx_dbp_plan {
    int64_t N = 0;
    int logN = 0, max_frames = 0, nspans = 0, nsteps = 0, manakov = 0, resident = 0;
    std::vector<DbpStep> steps;        // one span, execution order
    // resident route
    DbpStep *d_steps = nullptr;
    cplx *d_tw = nullptr;
    double *d_bt = nullptr;
    int nthr = 0, tw_in_lds = 0;
    size_t lds = 0;
    // streamed route
    plx_ssfm *fft = nullptr;
    std::vector<cplx *> d_h;           // one table per distinct step length
    std::vector<int> tab;              // table of each step (execution order)
};

extern "C" int plx_dbp_destroy(plx_dbp_plan *P)
{
    if (!P) return PLX_OK;
    if (P->d_steps) (void)hipFree(P->d_steps);
    if (P->d_tw) (void)hipFree(P->d_tw);
    if (P->d_bt) (void)hipFree(P->d_bt);
    for (cplx *h : P->d_h) (void)hipFree(h);
    if (P->fft) plx_ssfm_destroy(P->fft);
    delete P;
    return PLX_OK;
}

extern "C" int plx_dbp_create(plx_dbp_plan **out, const plx_dbp_desc *d, uint32_t flags)
{
    if (!out || !d || !d->betat) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: null argument");
    *out = nullptr;
    const int64_t N = d->nfft;
    const int logN = ilog2i(N > 0 ? N : 1);
    if (N < 256 || N > ((int64_t)1 << 20) || ((int64_t)1 << logN) != N)
        PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: nfft must be a power of two in [256, 2^20]");
    if (d->max_frames < 1) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: max_frames must be >= 1");
    if (d->nspans < 1) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: nspans must be >= 1");
    if (d->nsteps < 1) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: nsteps must be >= 1");
    if (!(d->span_length > 0.0) || !std::isfinite(d->span_length)) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: span_length must be > 0");
    if (!(d->alphalin >= 0.0) || !std::isfinite(d->alphalin)) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: alphalin must be >= 0");
    if (!std::isfinite(d->gam) || !std::isfinite(d->xi)) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: gam and xi must be finite");
    if (flags & ~PLX_DBP_STREAMED) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: unknown flag");
    const int ns = d->nsteps;
    std::vector<double> dz((size_t)ns, d->span_length / ns);
    if (d->dz) {
        double sum = 0.0;
        for (int k = 0; k < ns; k++) {
            if (!(d->dz[k] > 0.0) || !std::isfinite(d->dz[k])) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: every step dz must be > 0");
            dz[(size_t)k] = d->dz[k];
            sum += d->dz[k];
        }
        if (std::fabs(sum - d->span_length) > 1e-9 * d->span_length)
            PLX_FAIL(PLX_ERR_ARG, "plx_dbp_create: the steps dz must sum to span_length");
    }
    plx_dbp_plan *P = new plx_dbp_plan();
    P->N = N; P->logN = logN; P->max_frames = d->max_frames; P->nspans = d->nspans; P->nsteps = ns;
    P->manakov = d->manakov ? 1 : 0;
    P->resident = (N <= kResidentMax && !(flags & PLX_DBP_STREAMED)) ? 1 : 0;
    const double a = d->alphalin, gnl = d->xi * d->gam * (P->manakov ? 8.0 / 9.0 : 1.0);
    // execution order: the span's forward steps reversed; the first one also undoes the span's amplifier
    for (int k = 0; k < ns; k++) {
        const double h = dz[(size_t)(ns - 1 - k)];
        const double leff = a == 0.0 ? h : -std::expm1(-a * h) / a;          // fiber.m:821-825
        DbpStep s;
        s.g = std::exp(0.5 * a * h) * (k == 0 ? std::exp(-0.5 * a * d->span_length) : 1.0);
        s.dz = h;
        s.c = gnl * leff;
        P->steps.push_back(s);
    }
    int rc = PLX_OK;
    if (P->resident) {
        std::vector<cplx> tw((size_t)(N / 2));
        std::vector<double> bt((size_t)N);
        for (int64_t k = 0; k < N / 2; k++) {
            long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)N;
            tw[(size_t)k] = make_double2((double)cosl(ang), (double)sinl(ang));
        }
        // cexp_neg_turns(t dz) = exp(-2 pi i t dz) = exp(+i betat dz) for t = -betat / 2 pi
        for (int64_t i = 0; i < N; i++) bt[(size_t)i] = -d->betat[plx_bitrev((unsigned)i, logN)] / 6.28318530717958647692;
        std::vector<DbpStep> st = P->steps;
        for (DbpStep &s : st) s.g /= (double)N;                              // ifft's 1/N
        P->tw_in_lds = (2 * N + N / 2) * (int64_t)sizeof(cplx) <= (int64_t)kLdsMax - 32 * 1024 ? 1 : 0;
        P->lds = (size_t)(2 * N + (P->tw_in_lds ? N / 2 : 0)) * sizeof(cplx);
        P->nthr = (int)(N / 2 < 1024 ? N / 2 : 1024);
        if (hipMalloc((void **)&P->d_tw, tw.size() * sizeof(cplx)) != hipSuccess ||
            hipMalloc((void **)&P->d_bt, bt.size() * sizeof(double)) != hipSuccess ||
            hipMalloc((void **)&P->d_steps, st.size() * sizeof(DbpStep)) != hipSuccess ||
            hipMemcpy(P->d_tw, tw.data(), tw.size() * sizeof(cplx), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(P->d_bt, bt.data(), bt.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(P->d_steps, st.data(), st.size() * sizeof(DbpStep), hipMemcpyHostToDevice) != hipSuccess) {
            plx_dbp_destroy(P);
            PLX_FAIL(PLX_ERR_HIP, "plx_dbp_create: device allocation/upload failed");
        }
        if (allow_lds(k_dbp_resident, P->lds) != hipSuccess) { plx_dbp_destroy(P); PLX_FAIL(PLX_ERR_HIP, "plx_dbp_create: cannot reserve LDS"); }
    } else {
        // the FFT engine of a single-field, single-polarisation plan over 2 max_frames rows
        std::vector<double> zeros((size_t)N, 0.0);
        double gam0 = 0.0;
        plx_ssfm_desc sd;
        std::memset(&sd, 0, sizeof(sd));
        sd.nfft = N; sd.nfc = 1; sd.dual_pol = 0; sd.max_frames = 2 * d->max_frames;
        sd.dzmaxt = 1; sd.dphimaxt = 1; sd.length = 1; sd.nplates = 1; sd.gam = &gam0; sd.betat = zeros.data();
        rc = plx_ssfm_create(&P->fft, &sd);
        std::vector<double> hr((size_t)N), hi((size_t)N), seen;
        for (int k = 0; k < ns && rc == PLX_OK; k++) {
            const double h = P->steps[(size_t)k].dz;
            size_t t = 0;
            while (t < seen.size() && seen[t] != h) t++;
            if (t == seen.size()) {
                for (int64_t j = 0; j < N; j++) {
                    hr[(size_t)j] = std::cos(d->betat[j] * h);
                    hi[(size_t)j] = std::sin(d->betat[j] * h);
                }
                cplx *tab = nullptr;
                rc = plx_ssfm_filter_table(P->fft, hr.data(), hi.data(), &tab);
                if (rc == PLX_OK) { P->d_h.push_back(tab); seen.push_back(h); }
            }
            P->tab.push_back((int)t);
        }
        if (rc != PLX_OK) { plx_dbp_destroy(P); return rc; }
    }
    *out = P;
    return PLX_OK;
}

extern "C" int plx_dbp_apply_dev(plx_dbp_plan *P, const double *d_in, double *d_out, int nframes, const double *d_scale, void *stream)
{
    if (!P || !d_in || !d_out) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_apply_dev: null argument");
    if (nframes < 1 || nframes > P->max_frames) PLX_FAIL(PLX_ERR_ARG, "plx_dbp_apply_dev: nframes outside [1, max_frames]");
    if (P->resident) {
        DbpArgs a;
        a.in = (const cplx *)d_in; a.out = (cplx *)d_out; a.scale = d_scale; a.tw = P->d_tw; a.bt = P->d_bt; a.steps = P->d_steps;
        a.logN = P->logN; a.nsteps = P->nsteps; a.nspans = P->nspans; a.manakov = P->manakov; a.tw_in_lds = P->tw_in_lds;
        PLX_LAUNCH(k_dbp_resident, dim3((unsigned)nframes), dim3((unsigned)P->nthr), P->lds, stream, a);
        PLX_HIP(hipGetLastError());
        return PLX_OK;
    }
    const int64_t N = P->N;
    const dim3 grid((unsigned)((N + 255) / 256), (unsigned)nframes);
    cplx *u = (cplx *)d_out;
    KerrArgs k;
    k.out = u; k.scale = d_scale; k.N = N; k.manakov = P->manakov;
    // u = scale * in, times the first step's factor
    k.in = (const cplx *)d_in; k.c = 0.0; k.g = P->steps[0].g; k.kerr = 0; k.sc_mode = 1;
    PLX_LAUNCH(k_dbp_kerr, grid, dim3(256), 0, stream, k);
    PLX_HIP(hipGetLastError());
    k.in = u;
    const int total = P->nspans * P->nsteps;
    for (int j = 0; j < total; j++) {
        const int s = j % P->nsteps;
        int rc = plx_ssfm_filter_dev(P->fft, u, nullptr, P->d_h[(size_t)P->tab[(size_t)s]], 2 * nframes, stream);
        if (rc != PLX_OK) return rc;
        const bool last = j + 1 == total;
        k.c = P->steps[(size_t)s].c; k.kerr = 1;
        k.g = last ? 1.0 : P->steps[(size_t)((s + 1) % P->nsteps)].g;
        k.sc_mode = last ? 2 : 0;
        PLX_LAUNCH(k_dbp_kerr, grid, dim3(256), 0, stream, k);
        PLX_HIP(hipGetLastError());
    }
    return PLX_OK;
}

// gateway tier: one frame on host arrays with MATLAB's separate planes
extern "C" int plx_dbp(const double *xr, const double *xi, const double *yr, const double *yi, int64_t nx, const plx_dbp_desc *desc,
                       double scale, double *oxr, double *oxi, double *oyr, double *oyi)
{
    if (!xr || !yr || !desc || !oxr || !oxi || !oyr || !oyi) PLX_FAIL(PLX_ERR_ARG, "plx_dbp: null argument");
    if (nx != desc->nfft) PLX_FAIL(PLX_ERR_ARG, "plx_dbp: the signal length must equal desc->nfft");
    if (!(scale != 0.0) || !std::isfinite(scale)) PLX_FAIL(PLX_ERR_ARG, "plx_dbp: scale must be finite and nonzero");
    plx_dbp_desc d = *desc;
    d.max_frames = 1;
    plx_dbp_plan *P = nullptr;
    int rc = plx_dbp_create(&P, &d, 0);
    if (rc != PLX_OK) return rc;
    std::lock_guard<std::mutex> lk(plxgw::mutex());
    plxgw::count_call();
    // staging: [X | Y | scale] (the scale travels with the field)
    const size_t n = (size_t)nx, bytes = 2 * n * sizeof(cplx);
    cplx *h = (cplx *)plxgw::pinned(plxgw::S_IN, bytes + sizeof(cplx));
    cplx *du = (cplx *)plxgw::dev(plxgw::S_IN, bytes + sizeof(cplx));
    if (!h || !du) { plx_dbp_destroy(P); return PLX_ERR_HIP; }
    for (size_t i = 0; i < n; i++) {
        h[i] = make_double2(xr[i], xi ? xi[i] : 0.0);
        h[n + i] = make_double2(yr[i], yi ? yi[i] : 0.0);
    }
    h[2 * n] = make_double2(scale, 0.0);
    if (hipMemcpyAsync(du, h, bytes + sizeof(cplx), hipMemcpyHostToDevice, nullptr) != hipSuccess) {
        plx_dbp_destroy(P);
        PLX_FAIL(PLX_ERR_HIP, "plx_dbp: upload failed");
    }
    rc = plx_dbp_apply_dev(P, (const double *)du, (double *)du, 1, (const double *)(du + 2 * n), nullptr);
    if (rc == PLX_OK && (hipMemcpyAsync(h, du, bytes, hipMemcpyDeviceToHost, nullptr) != hipSuccess ||
                         hipStreamSynchronize(nullptr) != hipSuccess)) {
        plx_set_error("plx_dbp: download failed");
        rc = PLX_ERR_HIP;
    }
    plx_dbp_destroy(P);
    if (rc != PLX_OK) return rc;
    for (size_t i = 0; i < n; i++) {
        oxr[i] = h[i].x; oxi[i] = h[i].y;
        oyr[i] = h[n + i].x; oyi[i] = h[n + i].y;
    }
    return PLX_OK;
}
