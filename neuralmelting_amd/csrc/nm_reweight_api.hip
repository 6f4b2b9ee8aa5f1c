// nm_reweight_api.hip — the multistate reweighting of the replica grid (include/nm_reweight.h, nm_reweight_hist.h; kernels:
// nm_reweight.h) and its block-bootstrap replicates (include/nm_reweight_boot.h; kernels: nm_reweight_boot.h), which work on the
// same problem as the device sees it (RwProblem).
#include "../../include/nm_reweight.h"
#include "../../include/nm_reweight_boot.h"
#include "nm_reweight.h"
#include "nm_reweight_boot.h"
#include "nm_host.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace nm;

namespace {
thread_local std::string g_rw_error;
std::string &stage_error() { return g_rw_error; }

// what both entry points ask of the states and the samples
int rw_check(const char *fn, int nstates, const double *b, const double *c, const int64_t *count, const double *f, int64_t nsamples,
             const double *e, const double *v)
{
    if (nstates < 1 || nstates > RW_MAXSTATES) return refuse(fn, "nstates must lie in 1..4096");
    if (nsamples < 1) return refuse(fn, "nsamples must be at least 1");
    if (!b || !c || !count || !f || !e || !v) return refuse(fn, "a needed pointer is null");
    int64_t sum = 0;
    for (int k = 0; k < nstates; ++k) {
        if (count[k] < 0) return refuse(fn, "a count is negative");
        if (count[k] > nsamples - sum) return refuse(fn, "the counts do not sum to nsamples");
        sum += count[k];
    }
    if (sum != nsamples) return refuse(fn, "the counts do not sum to nsamples");
    if (first_not_finite(b, nstates) >= 0 || first_not_finite(c, nstates) >= 0) return refuse(fn, "a state's b or c is not finite");
    if (first_not_finite(f, nstates) >= 0) return refuse(fn, "an f is not finite");
    if (first_not_finite(e, nsamples) >= 0 || first_not_finite(v, nsamples) >= 0) return refuse(fn, "a sample's e or v is not finite");
    return NM_OK;
}

// what nm_reweight_expect and nm_reweight_boot_expect ask of the targets and the observables; `rest`: the entry point's other
// needed pointers are all there.  nm_reweight_histogram checks its nq and nbins between the range of ntargets and the pointers,
// and the first refusal wins, so it keeps its own lines.
int rw_targets_check(const char *fn, int ntargets, const double *tb, const double *tc, int nobs, const double *obs, const double *omean,
                     bool rest)
{
    if (ntargets < 1 || ntargets > 65536) return refuse(fn, "ntargets must lie in 1..65536");
    if (nobs < 0 || nobs > RW_MAXOBS) return refuse(fn, "nobs must lie in 0..8");
    if (!tb || !tc || !rest || (nobs > 0 && (!obs || !omean))) return refuse(fn, "a needed pointer is null");
    if (first_not_finite(tb, ntargets) >= 0 || first_not_finite(tc, ntargets) >= 0) return refuse(fn, "a target's tb or tc is not finite");
    return NM_OK;
}

// s = b e0 + c v0 as an unevaluated sum: the two rounded products and what their roundings lost (exactly, by fma).  With e0 or v0
// at 1e6 a long double product is good to 1e-13 only, and the weights would carry that; the differences below cancel the large
// parts first (sums of doubles of one magnitude are exact in a long double) and add the small parts last.
struct RwOffset {
    double p1 = 0.0, p2 = 0.0, lo = 0.0;
    RwOffset() = default;
    RwOffset(double b, double c, double e0, double v0)
    {
#pragma clang fp contract(off)
        p1 = b * e0;
        p2 = c * v0;
        lo = std::fma(b, e0, -p1) + std::fma(c, v0, -p2);
    }
    // x + (this - o)
    long double add_to(long double x, const RwOffset &o) const { return ((((x + p1) + p2) - o.p1) - o.p2) + ((long double)lo - o.lo); }
    // (x - y) - (this - o): x and y first, then the large parts pair by pair, so that every partial sum is exact
    long double take_from(double x, double y, const RwOffset &o) const
    {
        return ((((((long double)x - y) - p1) + o.p1) - p2) + o.p2) - ((long double)lo - o.lo);
    }
    long double value() const { return ((long double)p1 + p2) + lo; }
};

// The problem as the device sees it: samples centred on their means, the sampled states as a list, f in the centred gauge
// (f_centred[k] = (f[k] - f[0]) - (s_k - s_0), s_k = b[k] e0 + c[k] v0: of the size of the centred u whatever f[0], e0 and v0
// are), and the scratch of the moments kernels.  With logd' and F' what the kernels make of it: logd = logd' + f[0] - s_0 and
// F[i] = F'[i] + (s_i - s_0) + f[0].
struct RwProblem {
    int K = 0, ka = 0;
    int64_t N = 0, nchunks = 0;
    double e0 = 0.0, v0 = 0.0;
    std::vector<RwOffset> s; // s_k
    RwOffset s0;
    double f0 = 0.0; // f[0] as it came in
    DevBuf<double> e, v, logd, b, c, f, ab, ac, alc, part, F;
    DevBuf<int> aidx;
    DevBuf<RwStatus> st;

    // x + (s_t - s_0) + f[0] for a target
    double shifted(double x, double tb, double tc) const { return (double)(RwOffset(tb, tc, e0, v0).add_to(x, s0) + f0); }

    int setup(const char *fn, int nstates, const double *hb, const double *hc, const int64_t *count, const double *hf, int64_t nsamples,
              const double *he, const double *hv)
    {
        K = nstates;
        N = nsamples;
        nchunks = (N + RW_CH - 1) / RW_CH;
        long double se = 0.0L, sv = 0.0L;
        for (int64_t i = 0; i < N; ++i) { se += he[i]; sv += hv[i]; }
        e0 = (double)(se / N);
        v0 = (double)(sv / N);
        if (!std::isfinite(e0) || !std::isfinite(v0)) return refuse(fn, "the mean of e or v is not finite");
        std::vector<double> ce((size_t)N), cv((size_t)N);
        for (int64_t i = 0; i < N; ++i) { ce[i] = he[i] - e0; cv[i] = hv[i] - v0; }
        s0 = RwOffset(hb[0], hc[0], e0, v0);
        f0 = hf[0];
        s.resize(K);
        std::vector<double> cf(K), hab, hac, halc;
        std::vector<int> hidx;
        for (int k = 0; k < K; ++k) {
            s[k] = RwOffset(hb[k], hc[k], e0, v0);
            cf[k] = (double)s[k].take_from(hf[k], hf[0], s0);
            if (count[k] > 0) {
                hab.push_back(hb[k]);
                hac.push_back(hc[k]);
                halc.push_back(std::log((double)count[k]));
                hidx.push_back(k);
            }
        }
        ka = (int)hidx.size(); // >= 1: the counts sum to N >= 1
        STAGE_CHK(fn, e.upload(ce.data(), N));
        STAGE_CHK(fn, v.upload(cv.data(), N));
        STAGE_CHK(fn, logd.alloc(N));
        STAGE_CHK(fn, b.upload(hb, K));
        STAGE_CHK(fn, c.upload(hc, K));
        STAGE_CHK(fn, f.upload(cf.data(), K));
        STAGE_CHK(fn, F.alloc(K));
        STAGE_CHK(fn, ab.upload(hab.data(), ka));
        STAGE_CHK(fn, ac.upload(hac.data(), ka));
        STAGE_CHK(fn, alc.upload(halc.data(), ka));
        STAGE_CHK(fn, aidx.upload(hidx.data(), ka));
        STAGE_CHK(fn, st.alloc(1));
        STAGE_CHK(fn, st.zero(1));
        return NM_OK;
    }

    // how many targets a launch of the moments kernel takes: its partials stay within 128 MiB (but TB targets at least)
    int batch(int nf, int tb, int most) const
    {
        int64_t n = ((int64_t)1 << 24) / (nchunks * nf);
        n = n / tb * tb;
        if (n < tb) n = tb;
        return n < most ? (int)n : most;
    }

    int scratch(const char *fn, int nf, int nbatch)
    {
        STAGE_CHK(fn, part.alloc((size_t)((int64_t)nbatch * nchunks * nf)));
        return NM_OK;
    }

    void denominators()
    {
        hipLaunchKernelGGL(nm_rw_denom_kernel, dim3((unsigned)((N + RW_BLOCK - 1) / RW_BLOCK)), dim3(RW_BLOCK), 0, 0, st, N, e, v, ka, ab, ac, alc,
                           aidx, f, logd);
    }

    // the targets t0 .. t0 + nb - 1 of (tb, tc): partials, then F[t] (and sums[t][RW_NF] with MOM); nb is at most the batch
    template <int TB, bool MOM>
    void moments(int t0, int nb, const double *tb, const double *tc, int nobs, const double *obs, double *Fout, double *sums)
    {
        hipLaunchKernelGGL((nm_rw_moments_kernel<TB, MOM>), dim3((unsigned)nchunks, (unsigned)((nb + TB - 1) / TB)), dim3(RW_BLOCK), 0, 0, st, N, e, v,
                           logd, t0, t0 + nb, tb, tc, nobs, obs, part);
        hipLaunchKernelGGL((nm_rw_combine_kernel<MOM>), dim3((unsigned)((nb + RW_WAVES - 1) / RW_WAVES)), dim3(RW_BLOCK), 0, 0, st, nb, nchunks, nobs,
                           part, Fout + t0, MOM ? sums + (size_t)t0 * RW_NF : nullptr);
    }

    // the base free energy F'[t] of all n targets (tb, tc), with the scratch it needs: the scale that keeps a target's weights
    // at or below 1 in the kernels that follow
    int base_F(const char *fn, int n, const double *tb, const double *tc, double *Fout)
    {
        const int nbatch = batch(2, RW_TB, (n + RW_TB - 1) / RW_TB * RW_TB);
        if (const int rc = scratch(fn, 2, nbatch)) return rc;
        denominators();
        for (int t0 = 0; t0 < n; t0 += nbatch) moments<RW_TB, false>(t0, batch_rest(n, t0, nbatch), tb, tc, 0, nullptr, Fout, nullptr);
        STAGE_CHK(fn, hipGetLastError());
        return NM_OK;
    }

    // A row q of weighted sums (sum w, sum w^2, sums of w e, w v, w ee, w ev, w vv, w obs; centred e, v) to the results of slot o:
    // the Kish sample size clamped to 1..N, the means with e0 and v0 added back, the covariance and the observables' means
    void results(const double *q, int nobs, size_t o, double *ess, double *mean, double *cov, double *omean) const
    {
        const long double s0 = q[0];
        const long double me = q[2] / s0, mv = q[3] / s0;
        const long double n_eff = s0 * s0 / q[1];
        ess[o] = (double)(n_eff < 1.0L ? 1.0L : (n_eff > (long double)N ? (long double)N : n_eff));
        mean[2 * o] = (double)((long double)e0 + me);
        mean[2 * o + 1] = (double)((long double)v0 + mv);
        cov[3 * o] = (double)(q[4] / s0 - me * me);
        cov[3 * o + 1] = (double)(q[5] / s0 - me * mv);
        cov[3 * o + 2] = (double)(q[6] / s0 - mv * mv);
        for (int j = 0; j < nobs; ++j) omean[o * nobs + j] = (double)(q[7 + j] / s0);
    }
};

// the targets of a call on the device: tb, tc and the free energies F' the kernels leave per target
struct RwTargets {
    DevBuf<double> tb, tc, F;
    int upload(const char *fn, int ntargets, const double *htb, const double *htc)
    {
        STAGE_CHK(fn, tb.upload(htb, ntargets));
        STAGE_CHK(fn, tc.upload(htc, ntargets));
        STAGE_CHK(fn, F.alloc(ntargets));
        return NM_OK;
    }
};
} // namespace

extern "C" {
const char *nm_reweight_last_error(void) { return g_rw_error.c_str(); }

int nm_reweight_solve(int device, int nstates, const double *b, const double *c, const int64_t *count, int64_t nsamples, const double *e,
                      const double *v, double tol, int max_iter, double *f, double *logd, int *iters, double *delta)
{
    static const char *const fn = "nm_reweight_solve";
    if (const int rc = rw_check(fn, nstates, b, c, count, f, nsamples, e, v)) return rc;
    if (!iters || !delta) return refuse(fn, "a needed pointer is null");
    if (!(tol >= 0.0)) return refuse(fn, "tol must not be negative");
    if (max_iter < 1) return refuse(fn, "max_iter must be at least 1");
    if (const int rc = stage_device(fn, device)) return rc;
    RwProblem p;
    if (const int rc = p.setup(fn, nstates, b, c, count, f, nsamples, e, v)) return rc;
    const int nbatch = p.batch(2, RW_TB, (nstates + RW_TB - 1) / RW_TB * RW_TB);
    if (const int rc = p.scratch(fn, 2, nbatch)) return rc;
    RwStatus st = {0, 0, 0.0};
    for (int it = 0; it < max_iter && !st.done; ++it) {
        p.denominators();
        for (int t0 = 0; t0 < nstates; t0 += nbatch)
            p.moments<RW_TB, false>(t0, batch_rest(nstates, t0, nbatch), p.b, p.c, 0, nullptr, p.F, nullptr);
        hipLaunchKernelGGL(nm_rw_update_kernel, dim3(1), dim3(RW_BLOCK), 0, 0, p.st, nstates, p.F, p.f, it == 0 ? p.f0 : 0.0, tol);
        STAGE_CHK(fn, hipGetLastError());
        if ((it + 1) % RW_POLL == 0 || it + 1 == max_iter) STAGE_CHK(fn, hipMemcpy(&st, p.st, sizeof(st), hipMemcpyDeviceToHost));
    }
    STAGE_CHK(fn, hipDeviceSynchronize());
    std::vector<double> cf(nstates);
    STAGE_CHK(fn, p.f.download(cf.data(), nstates));
    if (logd) {
        std::vector<double> cl((size_t)nsamples);
        STAGE_CHK(fn, p.logd.download(cl.data(), nsamples));
        const long double g = (st.iters == 1 ? (long double)p.f0 : 0.0L) - p.s0.value(); // behind the first application f[0] = 0
        for (int64_t i = 0; i < nsamples; ++i) logd[i] = (double)((long double)cl[i] + g);
    }
    for (int k = 0; k < nstates; ++k) f[k] = (double)p.s[k].add_to(cf[k], p.s0);
    *iters = st.iters;
    *delta = st.delta;
    return NM_OK;
}

int nm_reweight_expect(int device, int nstates, const double *b, const double *c, const int64_t *count, const double *f, int64_t nsamples,
                       const double *e, const double *v, int ntargets, const double *tb, const double *tc, int nobs, const double *obs,
                       double *tf, double *ess, double *mean, double *cov, double *omean)
{
    static const char *const fn = "nm_reweight_expect";
    if (const int rc = rw_check(fn, nstates, b, c, count, f, nsamples, e, v)) return rc;
    if (const int rc = rw_targets_check(fn, ntargets, tb, tc, nobs, obs, omean, tf && ess && mean && cov)) return rc;
    if (const int rc = stage_device(fn, device)) return rc;
    RwProblem p;
    if (const int rc = p.setup(fn, nstates, b, c, count, f, nsamples, e, v)) return rc;
    const int nbatch = p.batch(RW_NF, 1, RW_TGB);
    if (const int rc = p.scratch(fn, RW_NF, nbatch)) return rc;
    RwTargets tg;
    DevBuf<double> d_obs, d_sums;
    if (const int rc = tg.upload(fn, ntargets, tb, tc)) return rc;
    STAGE_CHK(fn, d_sums.alloc((size_t)ntargets * RW_NF));
    if (nobs > 0) STAGE_CHK(fn, d_obs.upload(obs, (size_t)nobs * nsamples));
    p.denominators();
    for (int t0 = 0; t0 < ntargets; t0 += nbatch)
        p.moments<1, true>(t0, batch_rest(ntargets, t0, nbatch), tg.tb, tg.tc, nobs, d_obs, tg.F, d_sums);
    STAGE_CHK(fn, hipGetLastError());
    STAGE_CHK(fn, hipDeviceSynchronize());
    std::vector<double> hF(ntargets), hs((size_t)ntargets * RW_NF);
    STAGE_CHK(fn, tg.F.download(hF.data(), ntargets));
    STAGE_CHK(fn, d_sums.download(hs.data(), hs.size()));
    for (int t = 0; t < ntargets; ++t) {
        tf[t] = p.shifted(hF[t], tb[t], tc[t]);
        p.results(hs.data() + (size_t)t * RW_NF + 1, nobs, t, ess, mean, cov, omean); // (the row's first double is the largest log weight)
    }
    return NM_OK;
}

int nm_reweight_histogram(int device, int nstates, const double *b, const double *c, const int64_t *count, const double *f, int64_t nsamples,
                          const double *e, const double *v, int ntargets, const double *tb, const double *tc, int nq, const double *x,
                          int nbins, const double *edges, double *hist, double *outside)
{
    static const char *const fn = "nm_reweight_histogram";
    if (nsamples > RW_HIST_MAXN) return refuse(fn, "nsamples must not exceed 2^28");
    if (const int rc = rw_check(fn, nstates, b, c, count, f, nsamples, e, v)) return rc;
    if (ntargets < 1 || ntargets > 65536) return refuse(fn, "ntargets must lie in 1..65536");
    if (nq < 1 || nq > RW_MAXQ) return refuse(fn, "nq must lie in 1..8");
    if (nbins < 1 || nbins > RW_MAXBINS) return refuse(fn, "nbins must lie in 1..1024");
    if (!tb || !tc || !x || !edges || !hist) return refuse(fn, "a needed pointer is null");
    if (first_not_finite(tb, ntargets) >= 0 || first_not_finite(tc, ntargets) >= 0) return refuse(fn, "a target's tb or tc is not finite");
    if (first_not_finite(edges, (int64_t)nq * (nbins + 1)) >= 0) return refuse(fn, "an edge is not finite");
    for (int q = 0; q < nq; ++q)
        for (int j = 0; j < nbins; ++j)
            if (!(edges[(size_t)q * (nbins + 1) + j] < edges[(size_t)q * (nbins + 1) + j + 1])) return refuse(fn, "the edges are not strictly increasing");
    if (first_not_finite(x, (int64_t)nq * nsamples) >= 0) return refuse(fn, "an x is not finite");
    if (const int rc = stage_device(fn, device)) return rc;
    RwProblem p;
    if (const int rc = p.setup(fn, nstates, b, c, count, f, nsamples, e, v)) return rc;
    const int nb2 = nbins + 2, per = nq * nb2;                    // a target's counters: per quantity the bins, below, above
    const int nlaunch = ntargets < RW_TGB ? ntargets : RW_TGB;
    const size_t ncount = (size_t)nlaunch * per;
    RwTargets tg;
    DevBuf<double> d_edges, d_out;
    DevBuf<uint16_t> d_code;
    DevBuf<unsigned long long> d_hi, d_lo;
    if (const int rc = tg.upload(fn, ntargets, tb, tc)) return rc;
    STAGE_CHK(fn, d_edges.upload(edges, (size_t)nq * (nbins + 1)));
    STAGE_CHK(fn, d_code.alloc((size_t)nq * nsamples));
    STAGE_CHK(fn, d_hi.alloc(ncount));
    STAGE_CHK(fn, d_lo.alloc(ncount));
    STAGE_CHK(fn, d_out.alloc(ncount));
    STAGE_CHK(fn, d_hi.zero(ncount));
    STAGE_CHK(fn, d_lo.zero(ncount));
    {   // the bin codes, a quantity at a time: the quantities themselves do not stay on the device
        DevBuf<double> d_x;
        STAGE_CHK(fn, d_x.alloc((size_t)nsamples));
        for (int q = 0; q < nq; ++q) {
            STAGE_CHK(fn, hipMemcpy(d_x, x + (size_t)q * nsamples, (size_t)nsamples * sizeof(double), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(nm_rw_bins_kernel, dim3((unsigned)((nsamples + RW_BLOCK - 1) / RW_BLOCK)), dim3(RW_BLOCK), 0, 0, nsamples, d_x, nbins,
                               d_edges + (size_t)q * (nbins + 1), d_code + (size_t)q * nsamples);
        }
        STAGE_CHK(fn, hipGetLastError());
        STAGE_CHK(fn, hipDeviceSynchronize());
    }
    if (const int rc = p.base_F(fn, ntargets, tg.tb, tg.tc, tg.F)) return rc;
    // the tile of targets: four where their counters stay within RW_HIST_LDS, else two, else one (131,328 B at nq = 8, nbins = 1024)
    const size_t one = (size_t)per * 2 * sizeof(unsigned long long);
    const int tt = 4 * one <= (size_t)RW_HIST_LDS ? 4 : 2 * one <= (size_t)RW_HIST_LDS ? 2 : 1;
    const size_t lds = tt * one;
    const void *kern = tt == 4 ? (const void *)nm_rw_hist_kernel<4> : tt == 2 ? (const void *)nm_rw_hist_kernel<2> : (const void *)nm_rw_hist_kernel<1>;
    STAGE_CHK(fn, hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned gx = (unsigned)((p.nchunks + RW_HG - 1) / RW_HG);
    std::vector<double> out(ncount);
    for (int t0 = 0; t0 < ntargets; t0 += RW_TGB) {
        const int nb = batch_rest(ntargets, t0, RW_TGB);
        const dim3 grid(gx, (unsigned)((nb + tt - 1) / tt));
#define RW_HIST_LAUNCH(TT)                                                                                                                   \
        hipLaunchKernelGGL(nm_rw_hist_kernel<TT>, grid, dim3(RW_BLOCK), lds, 0, p.N, p.e, p.v, p.logd, t0, t0 + nb, tg.tb, tg.tc, tg.F, nq, nb2, d_code, \
                           d_hi, d_lo)
        if (tt == 4) RW_HIST_LAUNCH(4);
        else if (tt == 2) RW_HIST_LAUNCH(2);
        else RW_HIST_LAUNCH(1);
#undef RW_HIST_LAUNCH
        const int64_t cnt = (int64_t)nb * per;
        hipLaunchKernelGGL(nm_rw_hist_out_kernel, dim3((unsigned)((cnt + RW_BLOCK - 1) / RW_BLOCK)), dim3(RW_BLOCK), 0, 0, cnt, d_hi, d_lo, d_out);
        STAGE_CHK(fn, hipGetLastError());
        STAGE_CHK(fn, d_out.download(out.data(), (size_t)cnt));
        for (int t = 0; t < nb; ++t)
            for (int q = 0; q < nq; ++q) {
                const double *src = out.data() + ((size_t)t * nq + q) * nb2;
                std::copy(src, src + nbins, hist + ((size_t)(t0 + t) * nq + q) * nbins);
                if (outside) {
                    outside[((size_t)(t0 + t) * nq + q) * 2] = src[nbins];
                    outside[((size_t)(t0 + t) * nq + q) * 2 + 1] = src[nbins + 1];
                }
            }
    }
    return NM_OK;
}
} // extern "C"

// ------------------------------------------------------------------------------------------------------------------
// block-bootstrap replicates of the reweighting (include/nm_reweight_boot.h; kernels: nm_reweight_boot.h)
// ------------------------------------------------------------------------------------------------------------------
namespace {
// what both entry points ask of the replicates
int rb_check(const char *fn, int nrep, const uint16_t *mult, int64_t nsamples)
{
    if (nrep < 1 || nrep > RB_MAXREP) return refuse(fn, "nrep must lie in 1..1024");
    if (!mult) return refuse(fn, "a needed pointer is null");
    for (int r = 0; r < nrep; ++r) {
        const uint16_t *m = mult + (size_t)r * nsamples;
        int64_t sum = 0;
        for (int64_t i = 0; i < nsamples; ++i) sum += m[i];
        if (sum != nsamples) return refuse(fn, "a replicate's multiplicities do not sum to nsamples");
    }
    return NM_OK;
}

// the replicates on the device: the multiplicities, the perturbations d [nrep][K], the tile's weights g [RB_RT][N], and the
// words that freeze a finished replicate
struct RbWork {
    int nrep = 0;
    DevBuf<uint16_t> mult;
    DevBuf<double> d, g;
    DevBuf<int> done;
    DevBuf<RbControl> ctl;
    std::vector<double> cf; // the centred base solution as the device holds it

    int setup(const char *fn, const RwProblem &p, int nrep_, const uint16_t *hmult, const std::vector<double> &hd)
    {
        nrep = nrep_;
        const RbControl hc = {0, nrep};
        STAGE_CHK(fn, mult.upload(hmult, (size_t)nrep * p.N));
        STAGE_CHK(fn, d.upload(hd.data(), (size_t)nrep * p.K));
        STAGE_CHK(fn, g.alloc((size_t)RB_RT * p.N));
        STAGE_CHK(fn, done.alloc(nrep));
        STAGE_CHK(fn, done.zero(nrep));
        STAGE_CHK(fn, ctl.upload(&hc, 1));
        return NM_OK;
    }

    template <bool INV>
    void weights(const RwProblem &p, int r0, int rt)
    {
        hipLaunchKernelGGL((nm_rb_weights_kernel<INV>), dim3((unsigned)((p.N + RW_BLOCK - 1) / RW_BLOCK)), dim3(RW_BLOCK), 0, 0, ctl, done, p.N, p.e,
                           p.v, p.logd, p.ka, p.ab, p.ac, p.alc, p.aidx, p.f, p.K, d, r0, rt, mult, g);
    }
};
} // namespace

extern "C" {
int nm_reweight_boot_solve(int device, int nstates, const double *b, const double *c, const int64_t *count, int64_t nsamples,
                           const double *e, const double *v, const double *f, int nrep, const uint16_t *mult, double tol, int max_iter,
                           double *fr, int *iters, double *delta, int *status)
{
    static const char *const fn = "nm_reweight_boot_solve";
    if (const int rc = rw_check(fn, nstates, b, c, count, f, nsamples, e, v)) return rc;
    if (!fr || !iters || !delta || !status) return refuse(fn, "a needed pointer is null");
    if (!(tol >= 0.0)) return refuse(fn, "tol must not be negative");
    if (max_iter < 1) return refuse(fn, "max_iter must be at least 1");
    if (const int rc = rb_check(fn, nrep, mult, nsamples)) return rc;
    if (const int rc = stage_device(fn, device)) return rc;
    RwProblem p;
    if (const int rc = p.setup(fn, nstates, b, c, count, f, nsamples, e, v)) return rc;
    RbWork w;
    if (const int rc = w.setup(fn, p, nrep, mult, std::vector<double>((size_t)nrep * nstates, 0.0))) return rc;
    DevBuf<double> d_S, d_part, d_delta;
    DevBuf<int> d_iters, d_status;
    std::vector<int> hstatus(nrep, 1), hiters(nrep, 0);
    std::vector<double> hdelta(nrep, 0.0);
    STAGE_CHK(fn, d_S.alloc((size_t)nrep * nstates));
    STAGE_CHK(fn, d_part.alloc((size_t)RB_RT * nstates * p.nchunks));
    STAGE_CHK(fn, d_delta.alloc(nrep));
    STAGE_CHK(fn, d_iters.alloc(nrep));
    STAGE_CHK(fn, d_status.upload(hstatus.data(), nrep));
    STAGE_CHK(fn, d_iters.zero(nrep));
    STAGE_CHK(fn, d_delta.zero(nrep));
    p.denominators(); // of the base solution, once
    RbControl hc = {0, nrep};
    const dim3 sgrid((unsigned)(p.nchunks * ((nstates + RB_SB - 1) / RB_SB))); // chunk-major: nm_rb_sums_kernel
    for (int it = 0; it < max_iter && hc.ndone < nrep; ++it) {
        for (int r0 = 0; r0 < nrep; r0 += RB_RT) {
            const int rt = batch_rest(nrep, r0, RB_RT);
            const int64_t rows = (int64_t)rt * nstates;
            w.weights<false>(p, r0, rt);
            hipLaunchKernelGGL(nm_rb_sums_kernel, sgrid, dim3(RW_BLOCK), 0, 0, w.ctl, w.done, p.N, p.e, p.v, p.logd, nstates, p.b, p.c, p.f, r0, rt,
                               w.g, d_part);
            hipLaunchKernelGGL(nm_rb_combine_kernel<1>, dim3((unsigned)((rows + RW_WAVES - 1) / RW_WAVES)), dim3(RW_BLOCK), 0, 0, w.ctl, w.done, r0,
                               rt, rows, p.nchunks, d_part, d_S + (size_t)r0 * nstates);
        }
        hipLaunchKernelGGL(nm_rb_update_kernel, dim3((unsigned)nrep), dim3(RW_BLOCK), 0, 0, w.ctl, w.done, nstates, d_S, w.d, it == 0 ? p.f0 : 0.0,
                           tol, d_iters, d_delta, d_status);
        STAGE_CHK(fn, hipGetLastError());
        if ((it + 1) % RB_POLL == 0 || it + 1 == max_iter) STAGE_CHK(fn, hipMemcpy(&hc, w.ctl, sizeof(hc), hipMemcpyDeviceToHost));
    }
    STAGE_CHK(fn, hipDeviceSynchronize());
    std::vector<double> cf(nstates), hd((size_t)nrep * nstates);
    STAGE_CHK(fn, p.f.download(cf.data(), nstates));
    STAGE_CHK(fn, w.d.download(hd.data(), hd.size()));
    STAGE_CHK(fn, d_iters.download(hiters.data(), nrep));
    STAGE_CHK(fn, d_delta.download(hdelta.data(), nrep));
    STAGE_CHK(fn, d_status.download(hstatus.data(), nrep));
    for (int r = 0; r < nrep; ++r) {
        for (int k = 0; k < nstates; ++k)
            fr[(size_t)r * nstates + k] =
                hstatus[r] == 2 ? NAN : (double)p.s[k].add_to((long double)cf[k] + hd[(size_t)r * nstates + k], p.s0);
        iters[r] = hiters[r];
        delta[r] = hdelta[r];
        status[r] = hstatus[r];
    }
    return NM_OK;
}

int nm_reweight_boot_expect(int device, int nstates, const double *b, const double *c, const int64_t *count, const double *f,
                            int64_t nsamples, const double *e, const double *v, int nrep, const uint16_t *mult, const double *fr,
                            int ntargets, const double *tb, const double *tc, int nobs, const double *obs, double *tf, double *ess,
                            double *mean, double *cov, double *omean)
{
    static const char *const fn = "nm_reweight_boot_expect";
    if (const int rc = rw_check(fn, nstates, b, c, count, f, nsamples, e, v)) return rc;
    if (const int rc = rw_targets_check(fn, ntargets, tb, tc, nobs, obs, omean, tf && ess && mean && cov && fr)) return rc;
    if (const int rc = rb_check(fn, nrep, mult, nsamples)) return rc;
    std::vector<char> skip(nrep, 0); // a replicate without a solution: NaN in, NaN out
    for (int r = 0; r < nrep; ++r)
        for (int k = 0; k < nstates; ++k) {
            const double x = fr[(size_t)r * nstates + k];
            if (std::isinf(x)) return refuse(fn, "an fr is neither finite nor NaN");
            if (std::isnan(x)) skip[r] = 1;
        }
    if (const int rc = stage_device(fn, device)) return rc;
    RwProblem p;
    if (const int rc = p.setup(fn, nstates, b, c, count, f, nsamples, e, v)) return rc;
    std::vector<double> cf(nstates), hd((size_t)nrep * nstates, 0.0);
    STAGE_CHK(fn, p.f.download(cf.data(), nstates));
    for (int r = 0; r < nrep; ++r) {
        if (skip[r]) continue;
        const double *x = fr + (size_t)r * nstates;
        for (int k = 0; k < nstates; ++k) hd[(size_t)r * nstates + k] = (double)(p.s[k].take_from(x[k], x[0], p.s0) - (long double)cf[k]);
    }
    RbWork w;
    if (const int rc = w.setup(fn, p, nrep, mult, hd)) return rc;
    RwTargets tg;
    DevBuf<double> d_obs, d_part, d_sums;
    if (const int rc = tg.upload(fn, ntargets, tb, tc)) return rc;
    if (nobs > 0) STAGE_CHK(fn, d_obs.upload(obs, (size_t)nobs * nsamples));
    if (const int rc = p.base_F(fn, ntargets, tg.tb, tg.tc, tg.F)) return rc; // the scale that keeps q_t(n) <= 1
    std::vector<double> hF(ntargets);
    STAGE_CHK(fn, tg.F.download(hF.data(), ntargets));
    const int64_t nech = (p.N + RB_ECH - 1) / RB_ECH; // the expectation kernel's own chunks
    int64_t nbatch = ((int64_t)1 << 24) / ((int64_t)RB_RT * nech * RB_NS); // the partials stay within 128 MiB (one target at least)
    nbatch = nbatch < 1 ? 1 : nbatch > RW_TGB ? RW_TGB : nbatch;
    STAGE_CHK(fn, d_part.alloc((size_t)nbatch * RB_RT * nech * RB_NS));
    STAGE_CHK(fn, d_sums.alloc((size_t)nbatch * RB_RT * RB_NS));
    std::vector<double> hs((size_t)nbatch * RB_RT * RB_NS);
    for (int r0 = 0; r0 < nrep; r0 += RB_RT) {
        const int rt = batch_rest(nrep, r0, RB_RT);
        w.weights<true>(p, r0, rt);
        for (int t0 = 0; t0 < ntargets; t0 += (int)nbatch) {
            const int nb = batch_rest(ntargets, t0, nbatch);
            const int64_t rows = (int64_t)nb * rt;
            const int tt = nobs > 0 ? RB_ETO : RB_ET;
            const dim3 egrid((unsigned)(nech * ((nb + tt - 1) / tt) * ((rt + RB_RE - 1) / RB_RE)));
            if (nobs > 0)
                hipLaunchKernelGGL((nm_rb_expect_kernel<RB_ETO, RB_NS>), egrid, dim3(RW_BLOCK), 0, 0, p.N, p.e, p.v, p.logd, t0, nb, tg.tb, tg.tc, tg.F, nobs,
                                   d_obs, r0, rt, w.mult, w.g, d_part);
            else
                hipLaunchKernelGGL((nm_rb_expect_kernel<RB_ET, 7>), egrid, dim3(RW_BLOCK), 0, 0, p.N, p.e, p.v, p.logd, t0, nb, tg.tb, tg.tc, tg.F, nobs,
                                   d_obs, r0, rt, w.mult, w.g, d_part);
            hipLaunchKernelGGL(nm_rb_combine_kernel<RB_NS>, dim3((unsigned)((rows + RW_WAVES - 1) / RW_WAVES)), dim3(RW_BLOCK), 0, 0, w.ctl, nullptr, r0,
                               rt, rows, nech, d_part, d_sums);
            STAGE_CHK(fn, hipGetLastError());
            STAGE_CHK(fn, d_sums.download(hs.data(), (size_t)rows * RB_NS));
            for (int t = 0; t < nb; ++t) {
                const RwOffset st(tb[t0 + t], tc[t0 + t], p.e0, p.v0);
                for (int j = 0; j < rt; ++j) {
                    const size_t o = (size_t)(r0 + j) * ntargets + t0 + t;
                    if (skip[r0 + j]) {
                        tf[o] = ess[o] = mean[2 * o] = mean[2 * o + 1] = cov[3 * o] = cov[3 * o + 1] = cov[3 * o + 2] = NAN;
                        for (int q = 0; q < nobs; ++q) omean[o * nobs + q] = NAN;
                        continue;
                    }
                    const double *q = hs.data() + ((size_t)t * rt + j) * RB_NS; // sums of x = m w, x w, x e, x v, x ee, x ev, x vv, x obs
                    tf[o] = (double)(st.add_to((long double)hF[t0 + t] - logl((long double)q[0]), p.s0) + fr[(size_t)(r0 + j) * nstates]);
                    p.results(q, nobs, o, ess, mean, cov, omean);
                }
            }
        }
    }
    return NM_OK;
}
} // extern "C"
