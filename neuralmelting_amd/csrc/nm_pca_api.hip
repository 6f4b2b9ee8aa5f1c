// nm_pca_api.hip — the principal component stage (include/nm_pca.h; kernels: nm_pca.h): the batches of x, the two passes of the
// moments and the projection.
#include "../../include/nm_pca.h"
#include "nm_pca.h"
#include "nm_host.h"

#include <cmath>
#include <cstdlib>
#include <vector>

using namespace nm;

namespace {
thread_local std::string g_pca_error;
std::string &stage_error() { return g_pca_error; }

// what both entry points ask of the samples
int pca_check(const char *fn, int64_t nsamples, int nfeat)
{
    if (nfeat < 1 || nfeat > PCA_MAXFEAT) return refuse(fn, "nfeat must lie in 1..4096");
    if (nsamples < 2) return refuse(fn, "nsamples must be at least 2");
    if (nsamples > ((int64_t)1 << 40) / nfeat) return refuse(fn, "nsamples * nfeat must not exceed 2^40");
    return NM_OK;
}

// the slots of nm_pca_last_timing
enum { PCA_T_UPLOAD, PCA_T_COLSUM, PCA_T_GRAM, PCA_T_PROJECT, PCA_T_COUNT };
thread_local double g_pca_ms[PCA_T_COUNT];

// x on the device, a batch of PCA_BATCH samples at a time: all of it where it fits half of the free memory (then a second pass
// uploads nothing), else one batch's buffer that every pass fills again.  The batches, and so the arithmetic, are the same in
// both cases.  NM_PCA_STREAM=1 in the environment takes the second way whatever the size (for tests of it).
struct PcaSamples {
    const float *host = nullptr;
    int64_t n = 0;
    int d = 0;
    bool resident = false, filled = false;
    DevBuf<float> buf;
    DevBuf<unsigned long long> bad;
    Laps<PCA_T_COUNT> laps;

    int64_t batches() const { return (n + PCA_BATCH - 1) / PCA_BATCH; }
    int rest(int64_t b) const { return (int)((n - b * PCA_BATCH) < PCA_BATCH ? (n - b * PCA_BATCH) : PCA_BATCH); }

    int setup(const char *fn, int64_t nsamples, int nfeat, const float *x)
    {
        host = x;
        n = nsamples;
        d = nfeat;
        size_t free_b = 0, total_b = 0;
        STAGE_CHK(fn, hipMemGetInfo(&free_b, &total_b));
        const char *env = std::getenv("NM_PCA_STREAM");
        const size_t all = (size_t)n * d * sizeof(float);
        resident = all <= free_b / 2 && !(env && env[0] == '1');
        STAGE_CHK(fn, buf.alloc(resident ? (size_t)n * d : (size_t)(n < PCA_BATCH ? n : PCA_BATCH) * d));
        const unsigned long long none = PCA_NOBAD;
        STAGE_CHK(fn, bad.upload(&none, 1));
        laps.lap(PCA_T_UPLOAD);
        return NM_OK;
    }

    // batch b on the device; the last batch of a pass marks a resident x as filled
    int batch(const char *fn, int64_t b, const float *&p)
    {
        const size_t off = (size_t)b * PCA_BATCH * d;
        p = resident ? buf.p + off : buf.p;
        if (!filled) STAGE_CHK(fn, hipMemcpy((void *)p, host + off, (size_t)rest(b) * d * sizeof(float), hipMemcpyHostToDevice));
        if (resident && b + 1 == batches()) filled = true;
        laps.lap(PCA_T_UPLOAD);
        return NM_OK;
    }

    // NM_ERR_ARG if a kernel met a value that is not finite
    int screen(const char *fn)
    {
        unsigned long long first = PCA_NOBAD;
        STAGE_CHK(fn, hipMemcpy(&first, bad.p, sizeof(first), hipMemcpyDeviceToHost));
        if (first != PCA_NOBAD) return fail(NM_ERR_ARG, std::string(fn) + ": x is not finite in sample " + std::to_string(first));
        return NM_OK;
    }
};
} // namespace

extern "C" {
const char *nm_pca_last_error(void) { return g_pca_error.c_str(); }

int nm_pca_last_timing(double *ms) { return last_timing("nm_pca_last_timing", g_pca_ms, ms); }

int nm_pca_moments(int device, int64_t nsamples, int nfeat, const float *x, double *mean, double *lo, double *hi, double *gram)
{
    static const char *const fn = "nm_pca_moments";
    if (const int rc = pca_check(fn, nsamples, nfeat)) return rc;
    if (!x || !mean || !lo || !hi || !gram) return refuse(fn, "a needed pointer is null");
    if (const int rc = stage_device(fn, device)) return rc;
    PcaSamples xs;
    if (const int rc = xs.setup(fn, nsamples, nfeat, x)) return rc;
    const int D = nfeat, cgroups = (D + 63) / 64, tiles = (D + PCA_TILE - 1) / PCA_TILE, ntri = tiles * (tiles + 1) / 2;
    const size_t npart = (size_t)PCA_SLICES * ntri * PCA_TILE * PCA_TILE;
    constexpr int chunks = PCA_BATCH / PCA_MCH;
    DevBuf<double> d_csum, d_sum, d_lo, d_hi, d_mean, d_part, d_gram;
    DevBuf<float> d_clo, d_chi;
    STAGE_CHK(fn, d_csum.alloc((size_t)chunks * D));
    STAGE_CHK(fn, d_clo.alloc((size_t)chunks * D));
    STAGE_CHK(fn, d_chi.alloc((size_t)chunks * D));
    STAGE_CHK(fn, d_sum.alloc(D));
    STAGE_CHK(fn, d_sum.zero(D));
    STAGE_CHK(fn, d_mean.alloc(D));
    {
        std::vector<double> inf((size_t)D, INFINITY), ninf((size_t)D, -INFINITY);
        STAGE_CHK(fn, d_lo.upload(inf.data(), D));
        STAGE_CHK(fn, d_hi.upload(ninf.data(), D));
    }
    const int64_t nbatches = xs.batches();
    for (int64_t b = 0; b < nbatches; ++b) {                    // the first pass: column sums, extremes, the screen for values that are not finite
        const float *xb = nullptr;
        if (const int rc = xs.batch(fn, b, xb)) return rc;
        const int nb = xs.rest(b), nch = (nb + PCA_MCH - 1) / PCA_MCH;
        hipLaunchKernelGGL(nm_pca_colsum_kernel, dim3((unsigned)cgroups, (unsigned)nch), dim3(PCA_BLOCK), 0, 0, xb, nb, D, b * PCA_BATCH, d_csum,
                           d_clo, d_chi, xs.bad);
        hipLaunchKernelGGL(nm_pca_coljoin_kernel, dim3((unsigned)((D + PCA_BLOCK - 1) / PCA_BLOCK)), dim3(PCA_BLOCK), 0, 0, nch, D, d_csum, d_clo,
                           d_chi, d_sum, d_lo, d_hi, b + 1 == nbatches ? nsamples : (int64_t)0, d_mean);
        STAGE_CHK(fn, hipGetLastError());
        xs.laps.lap(PCA_T_COLSUM);
    }
    if (const int rc = xs.screen(fn)) return rc;
    STAGE_CHK(fn, d_part.alloc(npart));
    STAGE_CHK(fn, d_part.zero(npart));
    STAGE_CHK(fn, d_gram.alloc((size_t)D * D));
    xs.laps.lap(PCA_T_UPLOAD);
    for (int64_t b = 0; b < nbatches; ++b) {                    // the second pass: every slice's partial, batch after batch
        const float *xb = nullptr;
        if (const int rc = xs.batch(fn, b, xb)) return rc;
        hipLaunchKernelGGL(nm_pca_gram_kernel, dim3((unsigned)(ntri * PCA_SLICES)), dim3(PCA_BLOCK), 0, 0, xb, xs.rest(b), D, d_mean, d_part);
        STAGE_CHK(fn, hipGetLastError());
        xs.laps.lap(PCA_T_GRAM);
    }
    hipLaunchKernelGGL(nm_pca_gramsum_kernel, dim3((unsigned)ntri), dim3(PCA_BLOCK), 0, 0, D, d_part, d_gram);
    STAGE_CHK(fn, hipGetLastError());
    xs.laps.lap(PCA_T_GRAM);
    STAGE_CHK(fn, hipDeviceSynchronize());
    xs.laps.book(g_pca_ms);
    STAGE_CHK(fn, d_mean.download(mean, D));
    STAGE_CHK(fn, d_lo.download(lo, D));
    STAGE_CHK(fn, d_hi.download(hi, D));
    STAGE_CHK(fn, d_gram.download(gram, (size_t)D * D));
    return NM_OK;
}

int nm_pca_project(int device, int64_t nsamples, int nfeat, const float *x, const double *mean, const double *inv_scale, int ncomp,
                   const double *comp, double *z, double *norm2)
{
    static const char *const fn = "nm_pca_project";
    if (const int rc = pca_check(fn, nsamples, nfeat)) return rc;
    if (ncomp < 1 || ncomp > PCA_MAXCOMP || ncomp > nfeat) return refuse(fn, "ncomp must lie in 1..64 and not exceed nfeat");
    if (!x || !mean || !inv_scale || !comp || !z) return refuse(fn, "a needed pointer is null");
    if (first_not_finite(mean, nfeat) >= 0 || first_not_finite(inv_scale, nfeat) >= 0 || first_not_finite(comp, (int64_t)ncomp * nfeat) >= 0)
        return refuse(fn, "a value of mean, inv_scale or comp is not finite");
    if (const int rc = stage_device(fn, device)) return rc;
    PcaSamples xs;
    if (const int rc = xs.setup(fn, nsamples, nfeat, x)) return rc;
    DevBuf<double> d_mean, d_inv, d_comp, d_z, d_norm;
    STAGE_CHK(fn, d_mean.upload(mean, nfeat));
    STAGE_CHK(fn, d_inv.upload(inv_scale, nfeat));
    STAGE_CHK(fn, d_comp.upload(comp, (size_t)ncomp * nfeat));
    STAGE_CHK(fn, d_z.alloc((size_t)nsamples * ncomp));         // the results stay on the device until x has been screened to its end
    if (norm2) STAGE_CHK(fn, d_norm.alloc((size_t)nsamples));
    constexpr int per = PCA_BLOCK / 64 * PCA_PS;                // samples of a workgroup
    for (int64_t b = 0; b < xs.batches(); ++b) {
        const float *xb = nullptr;
        if (const int rc = xs.batch(fn, b, xb)) return rc;
        const int nb = xs.rest(b);
        hipLaunchKernelGGL(nm_pca_project_kernel, dim3((unsigned)((nb + per - 1) / per)), dim3(PCA_BLOCK), 0, 0, xb, nb, nfeat, b * PCA_BATCH, d_mean,
                           d_inv, ncomp, d_comp, d_z.p + (size_t)b * PCA_BATCH * ncomp, norm2 ? d_norm.p + (size_t)b * PCA_BATCH : nullptr, xs.bad);
        STAGE_CHK(fn, hipGetLastError());
        xs.laps.lap(PCA_T_PROJECT);
    }
    if (const int rc = xs.screen(fn)) return rc;
    xs.laps.book(g_pca_ms);
    STAGE_CHK(fn, d_z.download(z, (size_t)nsamples * ncomp));
    if (norm2) STAGE_CHK(fn, d_norm.download(norm2, (size_t)nsamples));
    return NM_OK;
}
} // extern "C"
