// nm_tsne_api.hip — the manifold stage (include/nm_tsne.h; kernels: nm_tsne.h): the affinities (screen, radix select, gather, the
// row kernel), the symmetric lists on the host, and the steps of the gradient and the descent queued without a wait between them.
#include "../../include/nm_tsne.h"
#include "nm_tsne.h"
#include "nm_host.h"

#include <cmath>
#include <new>
#include <vector>

using namespace nm;

namespace {
thread_local std::string g_tsne_error;
std::string &stage_error() { return g_tsne_error; }

// the slots of nm_tsne_last_timing
enum { TS_T_SETUP, TS_T_A, TS_T_B, TS_T_C, TS_T_ALL, TS_T_COUNT };
thread_local double g_tsne_ms[TS_T_COUNT];

// the scans over x for one ndim
struct Scans {
    void (*count)(int, const double *, const unsigned long long *, int *);
    void (*gather)(int, int, const double *, const unsigned long long *, const int *, int *);
};
const auto SCANS = scan_table<TS_MAXDIM>([](auto nd) {
    constexpr int ND = decltype(nd)::value;
    return Scans{nm_tsne_count_kernel<ND>, nm_tsne_gather_kernel<ND>};
});
// and those over y for one ncomp
struct Steps {
    void (*attract)(int, const long long *, const int *, const double *, const double *, double *);
    void (*pairs)(int, const double *, double *);
};
const auto STEPS = scan_table<TS_MAXCOMP>([](auto nc) {
    constexpr int NC = decltype(nc)::value;
    return Steps{nm_tsne_attract_kernel<NC>, nm_tsne_pairs_kernel<NC>};
});

const char *check_lists(int64_t npoints, int k, int ncomp)
{
    if (npoints < 2 || npoints > TS_MAXN) return "npoints must lie in 2..2^20";
    if (k < 1 || k > TS_MAXK || k > npoints - 1) return "k must lie in 1..min(npoints - 1, 4096)";
    if (ncomp < 1 || ncomp > TS_MAXCOMP) return "ncomp must lie in 1..3";
    return nullptr;
}

// The symmetric lists of the header: row i holds (j, (p_{j|i} + p_{i|j}) / (2 N)) for every j that has i in its list or is in i's,
// in ascending j.  Two counting sorts and a merge: the transposed lists (row j: the rows i that hold j, ascending), those
// transposed again (row i: its own entries in ascending j), and the two merged row by row.  Returns the first point whose list
// holds an entry that is no other point or a p that is not finite or negative, or -1.
int64_t symmetric_lists(int n, int k, const int32_t *nbr, const double *p, std::vector<long long> &rowptr, std::vector<int> &col,
                        std::vector<double> &val)
{
    const size_t edges = (size_t)n * k;
    std::vector<long long> tptr((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i)
        for (int m = 0; m < k; ++m) {
            const int32_t j = nbr[(size_t)i * k + m];
            const double v = p[(size_t)i * k + m];
            if (j < 0 || j >= n || j == i || !std::isfinite(v) || v < 0.0) return i;
            ++tptr[(size_t)j + 1];
        }
    for (int j = 0; j < n; ++j) tptr[(size_t)j + 1] += tptr[j];
    std::vector<int> tsrc(edges), acol(edges);
    std::vector<double> tval(edges), aval(edges);
    std::vector<long long> fill(tptr.begin(), tptr.end() - 1);
    for (int i = 0; i < n; ++i)
        for (int m = 0; m < k; ++m) {
            const long long at = fill[nbr[(size_t)i * k + m]]++;
            tsrc[at] = i;
            tval[at] = p[(size_t)i * k + m];
        }
    for (int i = 0; i < n; ++i) fill[i] = (long long)i * k;
    for (int j = 0; j < n; ++j)
        for (long long e = tptr[j]; e < tptr[(size_t)j + 1]; ++e) {
            const long long at = fill[tsrc[e]]++;
            acol[at] = j;
            aval[at] = tval[e];
        }
    rowptr.assign((size_t)n + 1, 0);
    col.clear();
    val.clear();
    col.reserve(edges + edges / 2);
    val.reserve(edges + edges / 2);
    const double twon = 2.0 * n;
    for (int i = 0; i < n; ++i) {
        long long a = (long long)i * k, t = tptr[i];
        const long long aend = a + k, tend = tptr[(size_t)i + 1];
        while (a < aend || t < tend) {
            const int ja = a < aend ? acol[a] : n, jt = t < tend ? tsrc[t] : n;
            const int j = ja < jt ? ja : jt;
            double out = 0.0, in = 0.0;
            if (ja == j) out = aval[a++];
            if (jt == j) in = tval[t++];
            col.push_back(j);
            val.push_back((out + in) / twon);
        }
        rowptr[(size_t)i + 1] = (long long)col.size();
    }
    return -1;
}

// nm_tsne_gradient (niter == 0: one evaluation, grad, kl and z are written) and nm_tsne_descend behind their checks
int run_steps(const char *fn, int device, int n, int k, const int32_t *nbr, const double *p, int ncomp, double *y, double *update,
              double *gains, int niter, double exaggeration, double momentum, double rate, double *grad, double *kl, double *z, double *trace)
{
    const bool descend = niter > 0;
    const int steps = descend ? niter : 1;
    const size_t ne = (size_t)n * ncomp;
    int64_t bad = first_not_finite(y, ne);
    if (bad >= 0) return fail(NM_ERR_ARG, std::string(fn) + ": y is not finite in point " + std::to_string(bad / ncomp));
    if (descend && (bad = first_not_finite(update, ne)) >= 0)
        return fail(NM_ERR_ARG, std::string(fn) + ": update is not finite in point " + std::to_string(bad / ncomp));
    if (descend && (bad = first_not_finite(gains, ne)) >= 0)
        return fail(NM_ERR_ARG, std::string(fn) + ": gains is not finite in point " + std::to_string(bad / ncomp));
    std::vector<long long> rowptr;
    std::vector<int> col;
    std::vector<double> val;
    try {
        bad = symmetric_lists(n, k, nbr, p, rowptr, col, val);
    } catch (const std::bad_alloc &) {
        return fail(NM_ERR_HIP, std::string(fn) + ": no host memory for the symmetric lists");
    }
    if (bad >= 0) return fail(NM_ERR_ARG, std::string(fn) + ": the list of point " + std::to_string(bad) +
                                              " holds an entry that is no other point, or a p that is not finite or negative");
    if (const int rc = stage_device(fn, device)) return rc;
    const Steps &kern = STEPS[ncomp - 1];
    const dim3 grid = scan_grid<TsScan>(n, n), block(TS_BLOCK);
    const int slices = (int)grid.y, rblocks = (n + TS_BLOCK - 1) / TS_BLOCK, eblocks = (n * ncomp + TS_BLOCK - 1) / TS_BLOCK;
    const dim3 waves((unsigned)((n + TS_BLOCK / 64 - 1) / (TS_BLOCK / 64)));
    Laps<TS_T_COUNT> laps;
    DevBuf<long long> d_rowptr;
    DevBuf<int> d_col;
    DevBuf<double> d_val, d_y, d_update, d_gains, d_grad, d_pconst, d_att, d_part, d_rep, d_bsum, d_tot, d_bnorm, d_trace;
    laps.lap(TS_T_SETUP);
    STAGE_CHK(fn, d_rowptr.upload(rowptr.data(), rowptr.size()));
    STAGE_CHK(fn, d_col.upload(col.data(), col.size()));
    STAGE_CHK(fn, d_val.upload(val.data(), val.size()));
    STAGE_CHK(fn, d_y.upload(y, ne));
    if (descend) {
        STAGE_CHK(fn, d_update.upload(update, ne));
        STAGE_CHK(fn, d_gains.upload(gains, ne));
    }
    STAGE_CHK(fn, d_grad.alloc(ne));
    STAGE_CHK(fn, d_pconst.alloc(2 * (size_t)n));
    STAGE_CHK(fn, d_att.alloc((size_t)n * TS_ATT));
    STAGE_CHK(fn, d_part.alloc((size_t)slices * n * TS_PART));
    STAGE_CHK(fn, d_rep.alloc((size_t)n * TS_MAXCOMP));
    STAGE_CHK(fn, d_bsum.alloc((size_t)rblocks * 4));
    STAGE_CHK(fn, d_tot.alloc(2));
    STAGE_CHK(fn, d_bnorm.alloc(eblocks));
    STAGE_CHK(fn, d_trace.alloc((size_t)steps * 3));
    hipLaunchKernelGGL(nm_tsne_plogp_kernel, waves, block, 0, 0, n, d_rowptr, d_val, d_pconst);
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(TS_T_SETUP);
    for (int s = 0; s < steps; ++s) {                           // queued one behind the other: nothing returns to the host
        hipLaunchKernelGGL(kern.attract, waves, block, 0, 0, n, d_rowptr, d_col, d_val, d_y, d_att);
        if (s == 0) laps.lap(TS_T_A);
        hipLaunchKernelGGL(kern.pairs, grid, block, 0, 0, n, d_y, d_part);
        if (s == 0) laps.lap(TS_T_B);
        hipLaunchKernelGGL(nm_tsne_rows_kernel, dim3((unsigned)rblocks), block, 0, 0, n, ncomp, slices, d_part, d_att, d_pconst, d_rep, d_bsum);
        hipLaunchKernelGGL(nm_tsne_total_kernel, dim3(1), block, 0, 0, rblocks, d_bsum, d_tot);
        hipLaunchKernelGGL(nm_tsne_step_kernel, dim3((unsigned)eblocks), block, 0, 0, n, ncomp, exaggeration, d_att, d_rep, d_tot, d_grad,
                           descend ? 1 : 0, momentum, rate, d_y, d_update, d_gains, d_bnorm);
        hipLaunchKernelGGL(nm_tsne_norm_kernel, dim3(1), block, 0, 0, eblocks, d_bnorm, d_tot, d_trace + (size_t)s * 3);
        if (s == 0) laps.lap(TS_T_C);
        STAGE_CHK(fn, hipGetLastError());
    }
    laps.lap(TS_T_ALL);
    STAGE_CHK(fn, hipDeviceSynchronize());
    laps.book(g_tsne_ms);
    g_tsne_ms[TS_T_ALL] += g_tsne_ms[TS_T_A] + g_tsne_ms[TS_T_B] + g_tsne_ms[TS_T_C];
    if (descend) {
        std::vector<double> ny(ne), nu(ne), ng(ne);             // all of them arrive before one is written
        STAGE_CHK(fn, d_y.download(ny.data(), ne));
        STAGE_CHK(fn, d_update.download(nu.data(), ne));
        STAGE_CHK(fn, d_gains.download(ng.data(), ne));
        STAGE_CHK(fn, d_trace.download(trace, (size_t)steps * 3));
        for (size_t e = 0; e < ne; ++e) { y[e] = ny[e]; update[e] = nu[e]; gains[e] = ng[e]; }
    } else {
        double tot[2];
        std::vector<double> g(ne);
        STAGE_CHK(fn, d_tot.download(tot, 2));
        STAGE_CHK(fn, d_grad.download(g.data(), ne));
        for (size_t e = 0; e < ne; ++e) grad[e] = g[e];
        *z = tot[0];
        *kl = tot[1];
    }
    return NM_OK;
}
} // namespace

extern "C" {
const char *nm_tsne_last_error(void) { return g_tsne_error.c_str(); }

int nm_tsne_last_timing(double *ms) { return last_timing("nm_tsne_last_timing", g_tsne_ms, ms); }

int nm_tsne_affinities(int device, int64_t npoints, int ndim, const double *x, double perplexity, int k, int32_t *nbr, double *p,
                       double *beta)
{
    static const char *const fn = "nm_tsne_affinities";
    if (npoints < 2 || npoints > TS_MAXN) return refuse(fn, "npoints must lie in 2..2^20");
    if (ndim < 1 || ndim > TS_MAXDIM) return refuse(fn, "ndim must lie in 1..16");
    if (k < 1 || k > TS_MAXK || k > npoints - 1) return refuse(fn, "k must lie in 1..min(npoints - 1, 4096)");
    if (!std::isfinite(perplexity) || !(perplexity > 1.0) || !(perplexity < (double)k)) return refuse(fn, "perplexity must be finite and lie in (1, k)");
    if (!x || !nbr || !p || !beta) return refuse(fn, "a needed pointer is null");
    if (const int rc = stage_device(fn, device)) return rc;
    const int n = (int)npoints;
    const Scans &kern = SCANS[ndim - 1];
    const dim3 grid = scan_grid<TsScan>(n, n), block(TS_BLOCK), flat((unsigned)((n + TS_BLOCK - 1) / TS_BLOCK));
    const size_t nk = (size_t)n * k;
    Laps<TS_T_COUNT> laps;
    DevBuf<double> d_x, d_p, d_beta;
    DevBuf<unsigned long long> d_key, d_thr;
    DevBuf<int> d_count, d_nbr;
    laps.lap(TS_T_SETUP);
    STAGE_CHK(fn, d_x.upload(x, (size_t)n * ndim));
    STAGE_CHK(fn, d_key.alloc(n));
    STAGE_CHK(fn, d_thr.alloc(n));
    STAGE_CHK(fn, d_count.alloc(n));
    STAGE_CHK(fn, d_nbr.alloc_zeroed(nk));
    STAGE_CHK(fn, d_p.alloc(nk));
    STAGE_CHK(fn, d_beta.alloc(n));
    int first = -1;
    STAGE_CHK(fn, scan_screen<TsScan>(n, ndim, d_x, first));
    if (first >= 0) return fail(NM_ERR_ARG, std::string(fn) + ": x is not finite in point " + std::to_string(first));
    laps.lap(TS_T_SETUP);
    // bits 62 .. 0 of the k-th smallest d2 of every row (the sign is 0), then the count strictly below it
    for (int b = 62; b >= -1; --b) {
        hipLaunchKernelGGL(nm_tsne_bit_kernel, flat, block, 0, 0, n, k, b == 62 ? -1 : b + 1, b, d_key, d_thr, d_count);
        hipLaunchKernelGGL(kern.count, grid, block, 0, 0, n, d_x, d_thr, d_count);
        STAGE_CHK(fn, hipGetLastError());
    }
    laps.lap(TS_T_A);
    hipLaunchKernelGGL(kern.gather, dim3(grid.x), block, 0, 0, n, k, d_x, d_key, d_count, d_nbr);
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(TS_T_B);
    hipLaunchKernelGGL(nm_tsne_row_kernel, dim3((unsigned)n), block, 0, 0, n, ndim, k, d_x, std::log(perplexity), d_nbr, d_p, d_beta);
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(TS_T_C);
    STAGE_CHK(fn, hipDeviceSynchronize());
    laps.book(g_tsne_ms);
    // into buffers of the library first: a failure on the way leaves the caller's untouched
    std::vector<int> hn(nk);
    std::vector<double> hp(nk);
    STAGE_CHK(fn, d_nbr.download(hn.data(), nk));
    STAGE_CHK(fn, d_p.download(hp.data(), nk));
    STAGE_CHK(fn, d_beta.download(beta, n));
    for (size_t e = 0; e < nk; ++e) { nbr[e] = hn[e]; p[e] = hp[e]; }
    return NM_OK;
}

int nm_tsne_gradient(int device, int64_t npoints, int k, const int32_t *nbr, const double *p, int ncomp, const double *y,
                     double exaggeration, double *grad, double *kl, double *z)
{
    static const char *const fn = "nm_tsne_gradient";
    if (const char *why = check_lists(npoints, k, ncomp)) return refuse(fn, why);
    if (!std::isfinite(exaggeration) || !(exaggeration > 0.0)) return refuse(fn, "exaggeration must be finite and positive");
    if (!nbr || !p || !y || !grad || !kl || !z) return refuse(fn, "a needed pointer is null");
    if (device < 0) return refuse(fn, "device ordinal out of range");
    return run_steps(fn, device, (int)npoints, k, nbr, p, ncomp, const_cast<double *>(y), nullptr, nullptr, 0, exaggeration, 0.0, 0.0, grad,
                     kl, z, nullptr);
}

int nm_tsne_descend(int device, int64_t npoints, int k, const int32_t *nbr, const double *p, int ncomp, double *y, double *update,
                    double *gains, int niter, double exaggeration, double momentum, double learning_rate, double *trace)
{
    static const char *const fn = "nm_tsne_descend";
    if (const char *why = check_lists(npoints, k, ncomp)) return refuse(fn, why);
    if (niter < 1 || niter > (1 << 20)) return refuse(fn, "niter must lie in 1..2^20");
    if (!std::isfinite(exaggeration) || !(exaggeration > 0.0)) return refuse(fn, "exaggeration must be finite and positive");
    if (!std::isfinite(momentum) || !(momentum >= 0.0) || !(momentum < 1.0)) return refuse(fn, "momentum must be finite and lie in [0, 1)");
    if (!std::isfinite(learning_rate) || !(learning_rate > 0.0)) return refuse(fn, "learning_rate must be finite and positive");
    if (!y || !update || !gains || !nbr || !p || !trace) return refuse(fn, "a needed pointer is null");
    if (device < 0) return refuse(fn, "device ordinal out of range");
    return run_steps(fn, device, (int)npoints, k, nbr, p, ncomp, y, update, gains, niter, exaggeration, momentum, learning_rate, nullptr,
                     nullptr, nullptr, trace);
}
} // extern "C"
