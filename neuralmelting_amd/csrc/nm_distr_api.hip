// nm_distr_api.hip — the structural histograms and order parameters of include/nm_distr.h over the kernels of nm_distr.h
// (lammps_distr.py:123-171).  Every entry point takes a device ordinal, owns what it allocates for the length of the call and
// walks the samples in chunks.  The last one, nm_distr_lof, is the outlier stage's (kernels: nm_lof.h): float64 points in sets, one
// upload, the screen of nm_scan.h, the neighbour pass and two gathers.  nm_cluster_kmeans, the cluster stage's k-means (kernels:
// nm_kmeans.h), stands here too, with this file's error channel: the screen, the chain of steps of all restarts with a look at their
// states every KM_LOOK steps, and the choice of the best restart.  nm_cluster_spectral, the cluster stage's spectral embedding (kernels:
// nm_spectral.h), likewise: the degree pass, then rounds of a Rayleigh-Ritz pass and a Chebyshev filter, the small matrices on the host.
#include "../../include/nm_distr.h"
#include "nm_distr.h"
#include "nm_distr_w.h"
#include "nm_lof.h"
#include "nm_kmeans.h"
#include "nm_spectral.h"
#include "nm_host.h"

#include <cmath>
#include <type_traits>
#include <vector>

using namespace nm;

namespace {
thread_local std::string g_distr_error;
std::string &stage_error() { return g_distr_error; }

constexpr int DISTR_CHUNK = 4096; // most samples per launch: bounds device memory (pos 12 N B + results) for long trajectories

// The chunk loop of an entry point: the device copies of `cs` samples' positions and boxes, filled for one chunk after the
// other; body(s0, n) computes the samples s0 .. s0 + n - 1 from them (launch, synchronise, copy back) and returns NM_OK or
// what it failed with.
struct DistrChunks {
    DevBuf<float> pos, box;
    template <class Body>
    int run(const char *fn, int ns, int cs, int natoms, const float *h_pos, const float *h_box, Body &&body)
    {
        STAGE_CHK(fn, pos.alloc((size_t)cs * natoms * 3));
        STAGE_CHK(fn, box.alloc((size_t)cs));
        for (int s0 = 0; s0 < ns; s0 += cs) {
            const int n = batch_rest(ns, s0, cs);
            STAGE_CHK(fn, hipMemcpy(pos, h_pos + (size_t)s0 * natoms * 3, (size_t)n * natoms * 3 * sizeof(float), hipMemcpyHostToDevice));
            STAGE_CHK(fn, hipMemcpy(box, h_box + s0, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
            const int rc = body(s0, n);
            if (rc != NM_OK) return rc;
        }
        return NM_OK;
    }
};

int distr_boxes_check(const char *fn, int ns, const float *box)
{
    for (int s = 0; s < ns; ++s)
        if (!(box[s] > 0.0f) || !std::isfinite(box[s])) return refuse(fn, "a box is not finite and positive");
    return NM_OK;
}

// the neighbour shell of nm_distr_angles and nm_distr_bondorder
int shell_check(const char *fn, double r_lo, double r_hi)
{
    if (!(r_lo >= 0.0) || !(r_lo < r_hi)) return refuse(fn, "the shell needs 0 <= r_lo < r_hi");
    return NM_OK;
}

// beyond half the smallest box an atom could neighbour its own image (a zero angle that is no bond angle)
int half_box_check(const char *fn, int ns, const float *box, double r_hi)
{
    for (int s = 0; s < ns; ++s)
        if (!(r_hi <= 0.5 * (double)box[s])) return refuse(fn, "r_hi exceeds half the smallest box");
    return NM_OK;
}

// the image pre-test of the scan compares float components with a float at or above r_hi; it is switched off for shells
// so small that the squares of such components could underflow
float shell_cube(double r_hi) { return r_hi < 1.0e-15 ? INFINITY : nextafterf((float)r_hi, INFINITY); }

// what the bond-order kernels need to know of the requested l (nm_distr.h, BoSet); ls increases strictly within 1..12
BoSet bo_set(int nl, const int *ls)
{
    BoSet set = {nl, 0, ls[nl - 1], 0u, 0ull, 0u};
    for (int i = 0; i < nl; ++i) {
        const int l = ls[i];
        set.lmask |= 1u << l;
        if (l <= 8) set.off_lo |= (unsigned long long)set.nc << (8 * (l - 1));
        else set.off_hi |= (unsigned int)set.nc << (8 * (l - 9));
        set.nc += l + 1;
    }
    return set;
}

// the constants of the harmonics' recurrence (nm_distr.h): long double, rounded once
std::vector<double> bo_table()
{
    const int W = BO_LMAX + 1;
    std::vector<double> tab((size_t)BO_TAB, 0.0);
    long double c = sqrtl(1.0L / (4.0L * 3.14159265358979323846264338327950288L));
    for (int m = 0; m <= BO_LMAX; ++m) {
        if (m > 0) c = -c * sqrtl((long double)(2 * m + 1) / (long double)(2 * m));
        tab[m] = (double)c;
        for (int l = m + 1; l <= BO_LMAX; ++l) {
            tab[W + l * W + m] = (double)sqrtl((long double)(4 * l * l - 1) / (long double)(l * l - m * m));
            tab[W + W * W + l * W + m] = (double)sqrtl((long double)((l - 1) * (l - 1) - m * m) / (long double)(4 * (l - 1) * (l - 1) - 1));
        }
    }
    return tab;
}

// The table of nm_distr_w.h: for l = 2, 4, .., 12 the terms (m1, m2) in that header's order, a symbol whose S is 0 left out, each the position triple and the
// coefficient (4 pi / (2l+1))^(3/2) (l l l; m1 m2 m3).  Racah's formula with the alternating sum in integers: for j1 = j2 = j3 = l
//   (l l l; m1 m2 m3) = (-1)^m3 S sqrt(prod_i (l + m_i)! (l - m_i)! / ((3l+1)! l!^3)),   S = sum_k (-1)^k C(l, k) C(l, l - m1 - k) C(l, l + m2 - k),
// S exact (each binomial is at most C(12, 6) = 924, at most 13 terms), the root's argument a product and quotient of factorials up to
// 37! in long double, the whole rounded to double once.
void bo_w_table(std::vector<double> &coef, std::vector<int> &idx)
{
    long double fact[3 * BO_LMAX + 2];
    fact[0] = 1.0L;
    for (int k = 1; k <= 3 * BO_LMAX + 1; ++k) fact[k] = fact[k - 1] * (long double)k;
    auto binom = [](int n, int k) -> long long {
        if (k < 0 || k > n) return 0;
        long long b = 1;
        for (int i = 1; i <= k; ++i) b = b * (n - k + i) / i;
        return b;
    };
    coef.clear();
    idx.clear();
    for (int l = 2; l <= BO_LMAX; l += 2) {
        const long double pre = powl(4.0L * 3.14159265358979323846264338327950288L / (long double)(2 * l + 1), 1.5L);
        const long double den = fact[3 * l + 1] * fact[l] * fact[l] * fact[l];
        for (int m1 = -l; m1 <= l; ++m1)
            for (int m2 = -l; m2 <= l; ++m2) {
                const int m3 = -m1 - m2;
                if (m3 < -l || m3 > l) continue;
                long long S = 0;
                for (int k = 0; k <= l; ++k) S += ((k & 1) ? -1 : 1) * binom(l, k) * binom(l, l - m1 - k) * binom(l, l + m2 - k);
                if (S == 0) continue;
                const long double num = fact[l + m1] * fact[l - m1] * fact[l + m2] * fact[l - m2] * fact[l + m3] * fact[l - m3];
                const long double t = pre * (long double)S * sqrtl(num / den);
                coef.push_back((double)((m3 & 1) ? -t : t));
                idx.push_back((m1 + l) | ((m2 + l) << 8) | ((m3 + l) << 16));
            }
    }
}

// samples per launch of the entry points that keep the moments q_lm in a device scratch of `per` bytes per sample: at most
// DISTR_CHUNK as the other entry points, fewer where the scratch would pass 256 MiB
int bo_chunk(int ns, size_t per)
{
    size_t fit = ((size_t)256 << 20) / per;
    if (fit < 1) fit = 1;
    int cs = ns < DISTR_CHUNK ? ns : DISTR_CHUNK;
    if ((size_t)cs > fit) cs = (int)fit;
    return cs;
}

// An optional per-sample output: the caller's array (null: not wanted), its `per` values per sample, and the chunk's device
// copy.  The device pointer stays null with the caller's, and the kernels branch on that.  `always`: a later kernel reads the
// device copy whether or not the caller wants it, so it is allocated (and passed) either way and only the copy-back is optional.
template <class T> struct DistrOut {
    T *const host;
    const size_t per;
    const bool always;
    DevBuf<T> d;
    DistrOut(T *host_, size_t per_, bool always_ = false) : host(host_), per(per_), always(always_) {}
    hipError_t alloc(int cs) { return host || always ? d.alloc((size_t)cs * per) : hipSuccess; }
    hipError_t zero(int n) { return host ? d.zero((size_t)n * per) : hipSuccess; }
    hipError_t fetch(int s0, int n) const { return host ? d.download(host + (size_t)s0 * per, (size_t)n * per) : hipSuccess; }
    operator T *() const { return d; }
};

// The first pass of nm_distr_bondorder and nm_distr_solid: the moments q_lm of every atom for the requested l, with what it
// needs on the device (the recurrence's table, the moments, the per-group partial sums and counts) and the chunk that keeps
// the moments within bo_chunk's cap.
struct BoMoments {
    BoSet set;
    int nc2, groups, cs;
    float cube;
    size_t lds;
    DevBuf<double> tab, qlm, part;
    DevBuf<int> cnt;

    int setup(const char *fn, int ns, int natoms, int nl, const int *ls, double r_hi)
    {
        set = bo_set(nl, ls);
        nc2 = 2 * set.nc;
        const std::vector<double> htab = bo_table();
        cube = shell_cube(r_hi);
        groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
        cs = bo_chunk(ns, (size_t)natoms * nc2 * sizeof(double));
        lds = bo_lds_bytes(natoms, set.nc, true); // at most 98,932 B (4095 atoms, six l from 7 to 12)
        STAGE_CHK(fn, hipFuncSetAttribute((const void *)nm_bo_moments_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        STAGE_CHK(fn, tab.upload(htab.data(), htab.size()));
        STAGE_CHK(fn, qlm.alloc((size_t)cs * natoms * nc2));
        STAGE_CHK(fn, part.alloc((size_t)cs * groups * nc2));
        STAGE_CHK(fn, cnt.alloc((size_t)cs * groups));
        return NM_OK;
    }

    // the moments of the chunk's n samples; q2 and nnb: null, or where the kernel leaves q_l^2 and the neighbour counts
    void launch(int n, int natoms, const float *pos, const float *box, double r_lo, double r_hi, double *q2, int *nnb)
    {
        hipLaunchKernelGGL(nm_bo_moments_kernel, dim3(n * groups), dim3(SHELL_BLOCK), lds, 0, natoms, pos, box, r_lo, r_hi, cube, set, tab,
                           qlm, q2, nnb, part, cnt);
    }
};

// nm_distr_lof: its slots of nm_distr_last_timing and its neighbour pass for one ndim
enum { LOF_T_UPLOAD, LOF_T_NEIGHBOURS, LOF_T_LRD, LOF_T_LOF, LOF_T_COUNT };
thread_local double g_distr_ms[LOF_T_COUNT];
using LofNeighbours = void (*)(int, int, int, const double *, int *, double *, double *);
const auto LOF_NEIGHBOURS = scan_table<LOF_MAXDIM>([](auto nd) -> LofNeighbours { return nm_lof_neighbours_kernel<decltype(nd)::value>; });

// the slots of nm_cluster_kmeans_last_timing
enum { KM_T_UPLOAD, KM_T_ASSIGN, KM_T_UPDATE, KM_T_COUNT };
thread_local double g_kmeans_ms[KM_T_COUNT];

// the kernels of k-means for one ndim
struct Lloyd {
    void (*assign)(int, const double *, int, int, const double *, const int *, size_t, uint8_t *, int *);
    void (*sums)(int, const double *, int, int, int, const int *, const int *, size_t, const uint8_t *, double *, int *);
    void (*inertia)(int, const double *, int, int, const double *, size_t, const uint8_t *, double *);
};
const auto LLOYD = scan_table<KM_MAXDIM>([](auto nd) {
    constexpr int ND = decltype(nd)::value;
    return Lloyd{nm_kmeans_assign_kernel<ND>, nm_kmeans_sums_kernel<ND>, nm_kmeans_inertia_kernel<ND>};
});

// the slots of nm_cluster_spectral_last_timing
enum { SP_T_UPLOAD, SP_T_DEGREE, SP_T_PASS, SP_T_BLOCK, SP_T_HOST, SP_T_COUNT };
thread_local double g_spectral_ms[SP_T_COUNT];

// the kernels of the spectral embedding that depend on ndim or on the padded width: [ndim - 1], then [0, 1, 2] for the widths 1, 8, 16
using SpPass = void (*)(int, const double *, double, const double *, double *);
using SpGram = void (*)(int, const double *, const double *, double *);
using SpApply = void (*)(int, const double *, const double *, const double *, double *, double *);
const auto SP_PASS = scan_table<SP_MAXDIM>([](auto nd) {
    constexpr int ND = decltype(nd)::value;
    return std::array<SpPass, 3>{nm_spectral_pass_kernel<ND, 1>, nm_spectral_pass_kernel<ND, 8>, nm_spectral_pass_kernel<ND, 16>};
});
const SpGram SP_GRAM[3] = {nm_spectral_gram_kernel<1>, nm_spectral_gram_kernel<8>, nm_spectral_gram_kernel<16>};
const SpApply SP_APPLY[3] = {nm_spectral_apply_kernel<1>, nm_spectral_apply_kernel<8>, nm_spectral_apply_kernel<16>};

// The host's small matrices are m x m in the corner of w x w (w the padded width), row-major, the rest zero.

// c = L^-T for g = L L^T, so that the columns of Y c are orthonormal where g = Y^T Y; false where a pivot is not above 256 u of its
// diagonal element: the columns are dependent to working precision
bool sp_cholesky(int m, int w, const double *g, double *c)
{
    double l[SP_MAXBLOCK][SP_MAXBLOCK] = {}, li[SP_MAXBLOCK][SP_MAXBLOCK] = {};
    for (int j = 0; j < m; ++j) {
        double d = g[j * w + j];
        for (int k = 0; k < j; ++k) d -= l[j][k] * l[j][k];
        if (!(d > 256.0 * 0x1p-53 * g[j * w + j])) return false;
        l[j][j] = std::sqrt(d);
        for (int i = j + 1; i < m; ++i) {
            double v = 0.5 * (g[i * w + j] + g[j * w + i]);
            for (int k = 0; k < j; ++k) v -= l[i][k] * l[j][k];
            l[i][j] = v / l[j][j];
        }
    }
    for (int j = 0; j < m; ++j) {                               // column j of L^-1 by forward substitution
        li[j][j] = 1.0 / l[j][j];
        for (int i = j + 1; i < m; ++i) {
            double v = 0.0;
            for (int k = j; k < i; ++k) v -= l[i][k] * li[k][j];
            li[i][j] = v / l[i][i];
        }
    }
    for (int e = 0; e < w * w; ++e) c[e] = 0.0;
    for (int i = 0; i < m; ++i)
        for (int j = 0; j <= i; ++j) c[j * w + i] = li[i][j];
    return true;
}

// cyclic Jacobi of the symmetric part of h: theta[0 .. m-1] descending (the lower index first on equal values) and q, whose column
// c is the eigenvector of theta[c].  A rotation is skipped where the element cannot change the diagonal's bits; the sweeps end
// where one skipped them all (64 at most: a 16 x 16 matrix takes about 8).
void sp_jacobi(int m, int w, const double *h, double *q, double *theta)
{
    double a[SP_MAXBLOCK][SP_MAXBLOCK], v[SP_MAXBLOCK][SP_MAXBLOCK];
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            a[i][j] = 0.5 * (h[i * w + j] + h[j * w + i]);
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 64; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < m - 1; ++p)
            for (int r = p + 1; r < m; ++r) {
                const double apr = a[p][r];
                if (std::fabs(apr) <= 0x1p-60 * (std::fabs(a[p][p]) + std::fabs(a[r][r])) || apr == 0.0) continue;
                rotated = true;
                const double tau = (a[r][r] - a[p][p]) / (2.0 * apr);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = t * cs;
                for (int k = 0; k < m; ++k) {                   // columns p and r
                    const double akp = a[k][p], akr = a[k][r];
                    a[k][p] = cs * akp - sn * akr;
                    a[k][r] = sn * akp + cs * akr;
                }
                for (int k = 0; k < m; ++k) {                   // rows p and r
                    const double apk = a[p][k], ark = a[r][k];
                    a[p][k] = cs * apk - sn * ark;
                    a[r][k] = sn * apk + cs * ark;
                }
                a[p][r] = a[r][p] = 0.0;
                for (int k = 0; k < m; ++k) {
                    const double vkp = v[k][p], vkr = v[k][r];
                    v[k][p] = cs * vkp - sn * vkr;
                    v[k][r] = sn * vkp + cs * vkr;
                }
            }
        if (!rotated) break;
    }
    int order[SP_MAXBLOCK];
    for (int c = 0; c < m; ++c) order[c] = c;
    for (int c = 1; c < m; ++c)                                 // a stable insertion sort, descending
        for (int k = c; k > 0 && a[order[k]][order[k]] > a[order[k - 1]][order[k - 1]]; --k) std::swap(order[k], order[k - 1]);
    for (int e = 0; e < w * w; ++e) q[e] = 0.0;
    for (int c = 0; c < m; ++c) {
        theta[c] = a[order[c]][order[c]];
        for (int k = 0; k < m; ++k) q[k * w + c] = v[k][order[c]];
    }
}

// What one call of nm_cluster_spectral holds on the device and the launches it is made of.  a, b and u are npoints x w.
struct Spectral {
    int n, ndim, m, w, wi, ne, nchunks;
    double gamma;
    dim3 grid, flat, rows;
    DevBuf<double> x, deg, rs, a, b, u, part, gpart, small, theta;
    DevBuf<int> bad;
    Laps<SP_T_COUNT> laps;

    void pass(const double *in, int width_index, int slot)
    {
        hipLaunchKernelGGL(SP_PASS[ndim - 1][width_index], grid, dim3(SP_BLOCK), 0, 0, n, x, gamma, in, part);
        laps.lap(slot);
    }
    // dst = alpha M cur + beta cur + gam dst behind a pass over u; the next pass's u where `next`
    void join(double alpha, double beta, double gam, const double *cur, double *dst, bool next)
    {
        hipLaunchKernelGGL(nm_spectral_rows_kernel, flat, dim3(SP_BLOCK), 0, 0, ne, w, (int)grid.y, part, rs, alpha, beta, gam, cur, dst,
                           next ? u.p : nullptr);
        laps.lap(SP_T_PASS);
    }
    // g (w x w, on the host) = p^T q
    hipError_t gram(const double *p, const double *q, double *g)
    {
        hipLaunchKernelGGL(SP_GRAM[wi], dim3((unsigned)nchunks), dim3(SP_BLOCK), 0, 0, n, p, q, gpart);
        hipLaunchKernelGGL(nm_spectral_gram_join_kernel, dim3(1), dim3(SP_BLOCK), 0, 0, nchunks, w * w, gpart, small);
        hipError_t e = hipGetLastError();
        laps.lap(SP_T_BLOCK);
        if (e == hipSuccess) e = small.download(g, (size_t)w * w);
        laps.lap(SP_T_HOST);
        return e;
    }
    // dst = src c, c (w x w) from the host; u = rs dst where `next`
    hipError_t apply(const double *src, const double *c, double *dst, bool next)
    {
        hipError_t e = hipMemcpy(small, c, (size_t)w * w * sizeof(double), hipMemcpyHostToDevice);
        laps.lap(SP_T_HOST);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(SP_APPLY[wi], rows, dim3(SP_BLOCK), 0, 0, n, src, small, rs, dst, next ? u.p : nullptr);
        e = hipGetLastError();
        laps.lap(SP_T_BLOCK);
        return e;
    }
    // the columns of src made orthonormal into a (Cholesky QR, twice), u = rs a; *rank = false where the first factor fails
    hipError_t orthonormalise(const double *src, bool *rank)
    {
        double g[SP_MAXBLOCK * SP_MAXBLOCK], c[SP_MAXBLOCK * SP_MAXBLOCK];
        *rank = true;
        for (int round = 0; round < 2; ++round) {
            hipError_t e = gram(src, src, g);
            if (e != hipSuccess) return e;
            if (!sp_cholesky(m, w, g, c)) { *rank = false; return hipSuccess; }
            if ((e = apply(src, c, a, round == 1)) != hipSuccess) return e;
            src = a;
        }
        return hipSuccess;
    }
};
} // namespace

extern "C" {

const char *nm_distr_last_error(void) { return g_distr_error.c_str(); }

int nm_distr_last_timing(double *ms) { return last_timing("nm_distr_last_timing", g_distr_ms, ms); }

int nm_distr_histograms(int device, int ns, int natoms, const float *pos, const float *box, int sbins, const double *r_edges,
                        int cbins, const double *rv_edges, float *rdf, float *cdf)
{
    static const char *const fn = "nm_distr_histograms";
    if (ns < 0 || natoms < 1 || !pos || !box) return refuse(fn, "bad argument");
    if (rdf && (!r_edges || sbins < 2 || sbins > DISTR_MAXS)) return refuse(fn, "bad spherical bins");
    if (cdf && (!rv_edges || cbins < 1 || cbins > DISTR_MAXC)) return refuse(fn, "bad cartesian bins");
    if (const int rc = stage_device(fn, device)) return rc;
    if (ns == 0) return NM_OK;
    const int sb = rdf ? sbins : 0, cb = cdf ? cbins : 0;
    const size_t nc = (size_t)cb * cb * cb;
    const size_t lds = distr_lds_bytes(natoms, sb, cb);
    if (lds > 160 * 1024) return refuse(fn, "working set exceeds LDS");
    // one image block's count of a bin is at most natoms^2, exact as a float below 2^24; the sum of the 27 blocks can exceed
    // natoms^2 (a displacement on +-l/2 lies in the closed cube in two images per axis) and is checked after the copy-back
    if (natoms >= 4096) return refuse(fn, "natoms^2 must stay below 2^24 (float32 counts of one periodic image)");
    STAGE_CHK(fn, hipFuncSetAttribute((const void *)nm_distr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int cs = ns < DISTR_CHUNK ? ns : DISTR_CHUNK;
    DevBuf<double> d_re, d_ve;
    DistrOut<float> d_r(rdf, sbins), d_c(cdf, nc);
    if (rdf) STAGE_CHK(fn, d_re.upload(r_edges, sbins));
    STAGE_CHK(fn, d_r.alloc(cs));
    if (cdf) STAGE_CHK(fn, d_ve.upload(rv_edges, cbins + 1));
    STAGE_CHK(fn, d_c.alloc(cs));
    DistrChunks ch;
    return ch.run(fn, ns, cs, natoms, pos, box, [&](int s0, int n) -> int {
        STAGE_CHK(fn, d_r.zero(n));
        STAGE_CHK(fn, d_c.zero(n));
        hipLaunchKernelGGL(nm_distr_kernel, dim3(n * 27), dim3(DISTR_BLOCK), lds, 0, natoms, ch.pos, ch.box, sb, d_re, cb, d_ve, d_r, d_c);
        STAGE_CHK(fn, hipGetLastError());
        STAGE_CHK(fn, hipDeviceSynchronize());
        STAGE_CHK(fn, d_r.fetch(s0, n));
        STAGE_CHK(fn, d_c.fetch(s0, n));
        // every partial sum below 2^24 is exact, so a total reaches 2^24 exactly when the returned float does; from there on
        // the float atomics round in the order they land, and the counts are no longer the reference's
        bool big = false;
        if (rdf) for (size_t i = 0; i < (size_t)n * sbins; ++i) big |= rdf[(size_t)s0 * sbins + i] >= 16777216.0f;
        if (cdf) for (size_t i = 0; i < (size_t)n * nc; ++i) big |= cdf[(size_t)s0 * nc + i] >= 16777216.0f;
        if (big) return refuse(fn, "a bin holds 2^24 counts or more, beyond what float32 counts hold exactly");
        return NM_OK;
    });
}

int nm_distr_angles(int device, int ns, int natoms, const float *pos, const float *box, double r_lo, double r_hi, int abins,
                    const double *cos_edges, uint64_t *adf)
{
    static const char *const fn = "nm_distr_angles";
    if (ns < 0 || !pos || !box || !cos_edges || !adf) return refuse(fn, "bad argument");
    if (natoms < 1 || natoms > 4095) return refuse(fn, "natoms must lie in 1..4095");
    if (abins < 2 || abins > ADF_MAXB) return refuse(fn, "abins must lie in 2..256");
    for (int k = 0; k + 1 < abins; ++k)
        if (!(cos_edges[k] > cos_edges[k + 1])) return refuse(fn, "cos_edges must decrease strictly");
    if (const int rc = shell_check(fn, r_lo, r_hi)) return rc;
    if (const int rc = half_box_check(fn, ns, box, r_hi)) return rc;
    if (const int rc = stage_device(fn, device)) return rc;
    if (ns == 0) return NM_OK;
    const float cube = shell_cube(r_hi);
    const int cs = ns < DISTR_CHUNK ? ns : DISTR_CHUNK;
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const size_t lds = adf_lds_bytes(natoms, abins); // at most 109,652 B (natoms 4095, abins 256)
    STAGE_CHK(fn, hipFuncSetAttribute((const void *)nm_adf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    DevBuf<double> d_e;
    DevBuf<unsigned long long> d_a;
    STAGE_CHK(fn, d_e.upload(cos_edges, abins));
    STAGE_CHK(fn, d_a.alloc((size_t)cs * abins));
    DistrChunks ch;
    return ch.run(fn, ns, cs, natoms, pos, box, [&](int s0, int n) -> int {
        STAGE_CHK(fn, d_a.zero((size_t)n * abins));
        hipLaunchKernelGGL(nm_adf_kernel, dim3(n * groups), dim3(SHELL_BLOCK), lds, 0, natoms, ch.pos, ch.box, r_lo, r_hi, cube, abins, d_e, d_a);
        STAGE_CHK(fn, hipGetLastError());
        STAGE_CHK(fn, hipDeviceSynchronize());
        STAGE_CHK(fn, hipMemcpy(adf + (size_t)s0 * abins, d_a, (size_t)n * abins * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return NM_OK;
    });
}

int nm_distr_sfactor(int device, int ns, int natoms, const float *pos, const float *box, int qmax, double *sf_sum, double *sf_max)
{
    static const char *const fn = "nm_distr_sfactor";
    if (ns < 0 || !pos || !box) return refuse(fn, "bad argument");
    if (!sf_sum && !sf_max) return refuse(fn, "sf_sum and sf_max are both null");
    if (natoms < 1 || natoms > 4095) return refuse(fn, "natoms must lie in 1..4095");
    if (qmax < 1 || qmax > SF_QMAX) return refuse(fn, "qmax must lie in 1..32");
    if (const int rc = distr_boxes_check(fn, ns, box)) return rc;
    if (const int rc = stage_device(fn, device)) return rc;
    if (ns == 0) return NM_OK;
    // the work items (nm_distr.h): every (h >= 0, k >= 0, l0) whose chunk l0 .. l0 + SF_LB - 1 reaches into the sphere, l0 slowest
    std::vector<unsigned int> items;
    for (int l0 = 0; l0 <= qmax; l0 += SF_LB)
        for (int h = 0; h <= qmax; ++h)
            for (int k = 0; k <= qmax; ++k)
                if (h * h + k * k + l0 * l0 <= qmax * qmax) items.push_back(sf_item(h, k, l0));
    const int nitems = (int)items.size();
    const size_t nsh = (size_t)qmax * qmax + 1;
    const int cs = ns < DISTR_CHUNK ? ns : DISTR_CHUNK;
    const size_t lds = sf_lds_bytes(qmax); // below the 64 KiB a kernel gets without asking
    DevBuf<unsigned int> d_it;
    DistrOut<double> d_sum(sf_sum, nsh), d_max(sf_max, nsh);
    STAGE_CHK(fn, d_it.upload(items.data(), nitems));
    STAGE_CHK(fn, d_sum.alloc(cs));
    STAGE_CHK(fn, d_max.alloc(cs));
    DistrChunks ch;
    return ch.run(fn, ns, cs, natoms, pos, box, [&](int s0, int n) -> int {
        hipLaunchKernelGGL(nm_sfac_kernel, dim3(n), dim3(SF_BLOCK), lds, 0, natoms, ch.pos, ch.box, qmax, nitems, d_it, d_sum, d_max);
        STAGE_CHK(fn, hipGetLastError());
        STAGE_CHK(fn, hipDeviceSynchronize());
        STAGE_CHK(fn, d_sum.fetch(s0, n));
        STAGE_CHK(fn, d_max.fetch(s0, n));
        return NM_OK;
    });
}

int nm_distr_bondorder(int device, int ns, int natoms, const float *pos, const float *box, double r_lo, double r_hi, int nl,
                       const int *ls, double *q2, double *qbar2, double *Q2, int32_t *nnb)
{
    static const char *const fn = "nm_distr_bondorder";
    if (ns < 0 || !pos || !box || !ls) return refuse(fn, "bad argument");
    if (!q2 && !qbar2 && !Q2 && !nnb) return refuse(fn, "all four outputs are null");
    if (natoms < 1 || natoms > 4095) return refuse(fn, "natoms must lie in 1..4095");
    if (nl < 1 || nl > BO_MAXL) return refuse(fn, "nl must lie in 1..6");
    for (int i = 0; i < nl; ++i)
        if (ls[i] < 1 || ls[i] > BO_LMAX || (i > 0 && ls[i] <= ls[i - 1]))
            return refuse(fn, "ls must increase strictly within 1..12");
    if (const int rc = shell_check(fn, r_lo, r_hi)) return rc;
    if (const int rc = distr_boxes_check(fn, ns, box)) return rc;
    if (const int rc = half_box_check(fn, ns, box, r_hi)) return rc;
    if (const int rc = stage_device(fn, device)) return rc;
    if (ns == 0) return NM_OK;
    BoMoments m;
    if (const int rc = m.setup(fn, ns, natoms, nl, ls, r_hi)) return rc;
    const size_t lds2 = bo_lds_bytes(natoms, m.set.nc, false); // below the moments kernel's
    STAGE_CHK(fn, hipFuncSetAttribute((const void *)nm_bo_average_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    const size_t pa = (size_t)natoms * nl;
    DistrOut<double> d_q2(q2, pa), d_qb(qbar2, pa), d_Q(Q2, nl);
    DistrOut<int> d_nnb(nnb, natoms);
    STAGE_CHK(fn, d_q2.alloc(m.cs));
    STAGE_CHK(fn, d_qb.alloc(m.cs));
    STAGE_CHK(fn, d_Q.alloc(m.cs));
    STAGE_CHK(fn, d_nnb.alloc(m.cs));
    DistrChunks ch;
    return ch.run(fn, ns, m.cs, natoms, pos, box, [&](int s0, int n) -> int {
        m.launch(n, natoms, ch.pos, ch.box, r_lo, r_hi, d_q2, d_nnb);
        STAGE_CHK(fn, hipGetLastError());
        if (qbar2) {
            hipLaunchKernelGGL(nm_bo_average_kernel, dim3(n * m.groups), dim3(SHELL_BLOCK), lds2, 0, natoms, ch.pos, ch.box, r_lo, r_hi, m.cube,
                               m.set, m.qlm, d_qb);
            STAGE_CHK(fn, hipGetLastError());
        }
        if (Q2) {
            hipLaunchKernelGGL(nm_bo_global_kernel, dim3(n), dim3(128), 0, 0, m.groups, m.set, m.part, m.cnt, d_Q);
            STAGE_CHK(fn, hipGetLastError());
        }
        STAGE_CHK(fn, hipDeviceSynchronize());
        STAGE_CHK(fn, d_q2.fetch(s0, n));
        STAGE_CHK(fn, d_qb.fetch(s0, n));
        STAGE_CHK(fn, d_Q.fetch(s0, n));
        STAGE_CHK(fn, d_nnb.fetch(s0, n));
        return NM_OK;
    });
}

int nm_distr_bondorder_w(int device, int ns, int natoms, const float *pos, const float *box, double r_lo, double r_hi, int nl,
                         const int *ls, double *w3, double *wbar3, double *W3, double *q2, double *qbar2, double *Q2, int32_t *nnb)
{
    static const char *const fn = "nm_distr_bondorder_w";
    if (ns < 0 || !pos || !box || !ls) return refuse(fn, "bad argument");
    if (!w3 && !wbar3 && !W3 && !q2 && !qbar2 && !Q2 && !nnb) return refuse(fn, "all seven outputs are null");
    if (natoms < 1 || natoms > 4095) return refuse(fn, "natoms must lie in 1..4095");
    if (nl < 1 || nl > BO_MAXL) return refuse(fn, "nl must lie in 1..6");
    for (int i = 0; i < nl; ++i)
        if (ls[i] < 1 || ls[i] > BO_LMAX || (i > 0 && ls[i] <= ls[i - 1]))
            return refuse(fn, "ls must increase strictly within 1..12");
    for (int i = 0; i < nl; ++i)
        if (ls[i] & 1)
            return refuse(fn, "an odd l: the 3j symbol (l l l; m1 m2 m3) is antisymmetric under the exchange of two columns for odd 3l, "
                              "so the third-order invariant vanishes identically; ls takes even values only");
    if (const int rc = shell_check(fn, r_lo, r_hi)) return rc;
    if (const int rc = distr_boxes_check(fn, ns, box)) return rc;
    if (const int rc = half_box_check(fn, ns, box, r_hi)) return rc;
    if (const int rc = stage_device(fn, device)) return rc;
    if (ns == 0) return NM_OK;
    BoMoments m;
    if (const int rc = m.setup(fn, ns, natoms, nl, ls, r_hi)) return rc;
    std::vector<double> hcoef;
    std::vector<int> hidx;
    bo_w_table(hcoef, hidx);
    DevBuf<double> d_coef;
    DevBuf<int> d_idx;
    STAGE_CHK(fn, d_coef.upload(hcoef.data(), hcoef.size()));
    STAGE_CHK(fn, d_idx.upload(hidx.data(), hidx.size()));
    const BoW w = {d_coef, d_idx};
    const size_t lds2 = bo_lds_bytes(natoms, m.set.nc, false), lds2w = bo_w_lds_bytes(natoms, m.set.nc); // below the moments kernel's
    STAGE_CHK(fn, hipFuncSetAttribute((const void *)nm_bo_average_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    STAGE_CHK(fn, hipFuncSetAttribute((const void *)nm_bo_w_average_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2w));
    const size_t pa = (size_t)natoms * nl;
    DistrOut<double> d_w3(w3, pa), d_wb(wbar3, pa), d_W(W3, nl), d_q2(q2, pa), d_qb(qbar2, pa), d_Q(Q2, nl);
    DistrOut<int> d_nnb(nnb, natoms);
    STAGE_CHK(fn, d_w3.alloc(m.cs));
    STAGE_CHK(fn, d_wb.alloc(m.cs));
    STAGE_CHK(fn, d_W.alloc(m.cs));
    STAGE_CHK(fn, d_q2.alloc(m.cs));
    STAGE_CHK(fn, d_qb.alloc(m.cs));
    STAGE_CHK(fn, d_Q.alloc(m.cs));
    STAGE_CHK(fn, d_nnb.alloc(m.cs));
    DistrChunks ch;
    return ch.run(fn, ns, m.cs, natoms, pos, box, [&](int s0, int n) -> int {
        m.launch(n, natoms, ch.pos, ch.box, r_lo, r_hi, d_q2, d_nnb);
        STAGE_CHK(fn, hipGetLastError());
        if (w3) {
            const int nvec = n * natoms; // at most 4096 * 4095
            hipLaunchKernelGGL(nm_bo_w_kernel, dim3((nvec + SHELL_WAVES - 1) / SHELL_WAVES), dim3(SHELL_BLOCK), 0, 0, nvec, m.set, m.qlm, w, d_w3);
            STAGE_CHK(fn, hipGetLastError());
        }
        if (wbar3) {
            hipLaunchKernelGGL(nm_bo_w_average_kernel, dim3(n * m.groups), dim3(SHELL_BLOCK), lds2w, 0, natoms, ch.pos, ch.box, r_lo, r_hi,
                               m.cube, m.set, m.qlm, w, d_qb, d_wb);
            STAGE_CHK(fn, hipGetLastError());
        } else if (qbar2) {
            hipLaunchKernelGGL(nm_bo_average_kernel, dim3(n * m.groups), dim3(SHELL_BLOCK), lds2, 0, natoms, ch.pos, ch.box, r_lo, r_hi, m.cube,
                               m.set, m.qlm, d_qb);
            STAGE_CHK(fn, hipGetLastError());
        }
        if (W3) {
            hipLaunchKernelGGL(nm_bo_w_global_kernel, dim3(n), dim3(128), 0, 0, m.groups, m.set, m.part, m.cnt, w, d_Q, d_W);
            STAGE_CHK(fn, hipGetLastError());
        } else if (Q2) {
            hipLaunchKernelGGL(nm_bo_global_kernel, dim3(n), dim3(128), 0, 0, m.groups, m.set, m.part, m.cnt, d_Q);
            STAGE_CHK(fn, hipGetLastError());
        }
        STAGE_CHK(fn, hipDeviceSynchronize());
        STAGE_CHK(fn, d_w3.fetch(s0, n));
        STAGE_CHK(fn, d_wb.fetch(s0, n));
        STAGE_CHK(fn, d_W.fetch(s0, n));
        STAGE_CHK(fn, d_q2.fetch(s0, n));
        STAGE_CHK(fn, d_qb.fetch(s0, n));
        STAGE_CHK(fn, d_Q.fetch(s0, n));
        STAGE_CHK(fn, d_nnb.fetch(s0, n));
        return NM_OK;
    });
}

int nm_distr_solid(int device, int ns, int natoms, const float *pos, const float *box, double r_lo, double r_hi, int l, double s_min,
                   int n_min, int32_t *nconn, int32_t *label, int32_t *nsolid, int32_t *nclus, int32_t *largest)
{
    static const char *const fn = "nm_distr_solid";
    if (ns < 0 || !pos || !box) return refuse(fn, "bad argument");
    if (!nconn && !label && !nsolid && !nclus && !largest) return refuse(fn, "all five outputs are null");
    if (natoms < 1 || natoms > 4095) return refuse(fn, "natoms must lie in 1..4095");
    if (l < 1 || l > BO_LMAX) return refuse(fn, "l must lie in 1..12");
    if (!(s_min >= -1.0) || !(s_min < 1.0)) return refuse(fn, "s_min must lie in [-1, 1)");
    if (n_min < 1) return refuse(fn, "n_min must be at least 1");
    if (const int rc = shell_check(fn, r_lo, r_hi)) return rc;
    if (const int rc = distr_boxes_check(fn, ns, box)) return rc;
    if (const int rc = half_box_check(fn, ns, box, r_hi)) return rc;
    if (const int rc = stage_device(fn, device)) return rc;
    if (ns == 0) return NM_OK;
    BoMoments m;
    if (const int rc = m.setup(fn, ns, natoms, 1, &l, r_hi)) return rc;
    const int cs = m.cs, groups = m.groups;
    const float cube = m.cube;
    const size_t lds2 = solid_lds_bytes(natoms); // at most 51,284 B (4095 atoms)
    // the kernels pass all five on to one another, so the device holds them whatever the caller asks for
    DistrOut<int> d_conn(nconn, natoms, true), d_lab(label, natoms, true), d_ns(nsolid, 1, true), d_nc(nclus, 1, true), d_big(largest, 1, true);
    DevBuf<int> d_par;
    STAGE_CHK(fn, d_conn.alloc(cs));
    STAGE_CHK(fn, d_par.alloc((size_t)cs * natoms));
    STAGE_CHK(fn, d_lab.alloc(cs));
    STAGE_CHK(fn, d_ns.alloc(cs));
    STAGE_CHK(fn, d_nc.alloc(cs));
    STAGE_CHK(fn, d_big.alloc(cs));
    DistrChunks ch;
    return ch.run(fn, ns, cs, natoms, pos, box, [&](int s0, int n) -> int {
        // each kernel reads what the one before it wrote for the whole chunk: the launches of one stream run in order
        m.launch(n, natoms, ch.pos, ch.box, r_lo, r_hi, nullptr, nullptr);
        STAGE_CHK(fn, hipGetLastError());
        hipLaunchKernelGGL(nm_solid_connect_kernel, dim3(n * groups), dim3(SHELL_BLOCK), lds2, 0, natoms, ch.pos, ch.box, r_lo, r_hi, cube, l,
                           s_min, m.qlm, d_conn, d_par);
        STAGE_CHK(fn, hipGetLastError());
        hipLaunchKernelGGL(nm_solid_union_kernel, dim3(n * groups), dim3(SHELL_BLOCK), lds2, 0, natoms, ch.pos, ch.box, r_lo, r_hi, cube, n_min,
                           d_conn, d_par);
        STAGE_CHK(fn, hipGetLastError());
        hipLaunchKernelGGL(nm_solid_label_kernel, dim3(n), dim3(SOLID_BLOCK), 0, 0, natoms, n_min, d_conn, d_par, d_lab, d_ns, d_nc, d_big);
        STAGE_CHK(fn, hipGetLastError());
        STAGE_CHK(fn, hipDeviceSynchronize());
        STAGE_CHK(fn, d_conn.fetch(s0, n));
        STAGE_CHK(fn, d_lab.fetch(s0, n));
        STAGE_CHK(fn, d_ns.fetch(s0, n));
        STAGE_CHK(fn, d_nc.fetch(s0, n));
        STAGE_CHK(fn, d_big.fetch(s0, n));
        return NM_OK;
    });
}

int nm_distr_cna(int device, int ns, int natoms, const float *pos, const float *box, double r_lo, double r_hi, int mode,
                 int32_t *type, int32_t *sig, int32_t *ntype, int32_t *nsig)
{
    static const char *const fn = "nm_distr_cna";
    if (ns < 0 || !pos || !box) return refuse(fn, "bad argument");
    if (!type && !sig && !ntype && !nsig) return refuse(fn, "all four outputs are null");
    if (natoms < 1 || natoms > 4095) return refuse(fn, "natoms must lie in 1..4095");
    if (mode != NM_CNA_FIXED && mode != NM_CNA_ADAPTIVE) return refuse(fn, "mode must be NM_CNA_FIXED or NM_CNA_ADAPTIVE");
    if (const int rc = shell_check(fn, r_lo, r_hi)) return rc;
    if (const int rc = distr_boxes_check(fn, ns, box)) return rc;
    if (const int rc = half_box_check(fn, ns, box, r_hi)) return rc;
    const size_t lds = cna_lds_bytes(natoms); // at most 51,604 B (4095 atoms)
    if (lds > 160 * 1024) return refuse(fn, "working set exceeds LDS");
    if (const int rc = stage_device(fn, device)) return rc;
    if (ns == 0) return NM_OK;
    const float cube = shell_cube(r_hi);
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const size_t pa = (size_t)natoms, ps = pa * CNA_NSIG;
    const int cs = bo_chunk(ns, ps * sizeof(int)); // the per-atom columns are the largest device array
    DistrOut<int> d_type(type, pa), d_sig(sig, ps), d_ntype(ntype, CNA_NTYPE), d_nsig(nsig, CNA_NSIG);
    STAGE_CHK(fn, d_type.alloc(cs));
    STAGE_CHK(fn, d_sig.alloc(cs));
    STAGE_CHK(fn, d_ntype.alloc(cs));
    STAGE_CHK(fn, d_nsig.alloc(cs));
    DistrChunks ch;
    return ch.run(fn, ns, cs, natoms, pos, box, [&](int s0, int n) -> int {
        // the per-sample sums are added to by every workgroup of the sample
        STAGE_CHK(fn, d_ntype.zero(n));
        STAGE_CHK(fn, d_nsig.zero(n));
        hipLaunchKernelGGL(nm_cna_kernel, dim3(n * groups), dim3(SHELL_BLOCK), lds, 0, natoms, ch.pos, ch.box, r_lo, r_hi, cube,
                           mode == NM_CNA_ADAPTIVE, d_type, d_sig, d_ntype, d_nsig);
        STAGE_CHK(fn, hipGetLastError());
        STAGE_CHK(fn, hipDeviceSynchronize());
        STAGE_CHK(fn, d_type.fetch(s0, n));
        STAGE_CHK(fn, d_sig.fetch(s0, n));
        STAGE_CHK(fn, d_ntype.fetch(s0, n));
        STAGE_CHK(fn, d_nsig.fetch(s0, n));
        return NM_OK;
    });
}

int nm_distr_entropy(int device, int ns, int natoms, const float *pos, const float *box, double r_m, double sigma, int nbins, double r_avg,
                     double s_cut, double *s, double *sbar, int32_t *nnb, double *smean, double *sbarmean, int32_t *nlow)
{
    static const char *const fn = "nm_distr_entropy";
    if (ns < 0 || !pos || !box) return refuse(fn, "bad argument");
    if (!s && !sbar && !nnb && !smean && !sbarmean && !nlow) return refuse(fn, "all six outputs are null");
    if (natoms < 1 || natoms > 4095) return refuse(fn, "natoms must lie in 1..4095");
    if (nbins < 1 || nbins > ENT_MAXBINS) return refuse(fn, "nbins must lie in 1..1024");
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return refuse(fn, "sigma must be positive and finite");
    if (!(r_m > 0.0) || !std::isfinite(r_m)) return refuse(fn, "r_m must be positive and finite");
    if (!(r_avg > 0.0)) return refuse(fn, "r_avg must be positive");
    if (s_cut != s_cut) return refuse(fn, "s_cut is not a number");
    if (const int rc = distr_boxes_check(fn, ns, box)) return rc;
    for (int i = 0; i < ns; ++i)
        if (!(r_m <= 0.5 * (double)box[i]) || !(r_avg <= 0.5 * (double)box[i])) return refuse(fn, "r_m or r_avg exceeds half the smallest box");
    if (const int rc = stage_device(fn, device)) return rc;
    if (ns == 0) return NM_OK;
    const bool average = sbar || sbarmean || nlow, means = smean || sbarmean || nlow;
    const float cube_m = shell_cube(r_m), cube_a = shell_cube(r_avg);
    const double D = r_m / (double)nbins, inv2s2 = 1.0 / (2.0 * (sigma * sigma));
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const int cs = ns < DISTR_CHUNK ? ns : DISTR_CHUNK;
    const size_t lds1 = ent_lds_bytes(natoms, false), lds2 = ent_lds_bytes(natoms, true); // at most 49,284 B and 51,332 B (4095 atoms)
    DistrOut<double> d_s(s, natoms, true), d_b(sbar, natoms), d_sm(smean, 1), d_bm(sbarmean, 1); // s: pass 2 reads it, whether or not the caller asks for it
    DistrOut<int> d_nnb(nnb, natoms), d_low(nlow, 1);
    DevBuf<double> d_ps, d_pb;
    DevBuf<int> d_pl;
    STAGE_CHK(fn, d_s.alloc(cs));
    STAGE_CHK(fn, d_ps.alloc((size_t)cs * groups));
    STAGE_CHK(fn, d_nnb.alloc(cs));
    STAGE_CHK(fn, d_b.alloc(cs));
    if (average) {
        STAGE_CHK(fn, d_pb.alloc((size_t)cs * groups));
        STAGE_CHK(fn, d_pl.alloc((size_t)cs * groups));
    }
    STAGE_CHK(fn, d_sm.alloc(cs));
    STAGE_CHK(fn, d_bm.alloc(cs));
    STAGE_CHK(fn, d_low.alloc(cs));
    const int points = nbins + 1; // a lane owns ceil(points / 64) grid points: the next instantiation that holds them
    DistrChunks ch;
    return ch.run(fn, ns, cs, natoms, pos, box, [&](int s0, int n) -> int {
        auto local = [&](auto na) {
            hipLaunchKernelGGL(nm_ent_local_kernel<decltype(na)::value>, dim3(n * groups), dim3(SHELL_BLOCK), lds1, 0, natoms, ch.pos, ch.box, r_m,
                               cube_m, sigma, inv2s2, nbins, D, d_s, d_nnb, d_ps);
        };
        if (points <= 64) local(std::integral_constant<int, 1>());
        else if (points <= 128) local(std::integral_constant<int, 2>());
        else if (points <= 256) local(std::integral_constant<int, 4>());
        else if (points <= 512) local(std::integral_constant<int, 8>());
        else local(std::integral_constant<int, ENT_MAXACC>());
        STAGE_CHK(fn, hipGetLastError());
        if (average) {
            hipLaunchKernelGGL(nm_ent_average_kernel, dim3(n * groups), dim3(SHELL_BLOCK), lds2, 0, natoms, ch.pos, ch.box, r_avg, cube_a, s_cut,
                               d_s, d_b, d_pb, d_pl);
            STAGE_CHK(fn, hipGetLastError());
        }
        if (means) {
            hipLaunchKernelGGL(nm_ent_mean_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, n, natoms, groups, d_ps, d_pb, d_pl, d_sm, d_bm, d_low);
            STAGE_CHK(fn, hipGetLastError());
        }
        STAGE_CHK(fn, hipDeviceSynchronize());
        STAGE_CHK(fn, d_s.fetch(s0, n));
        STAGE_CHK(fn, d_b.fetch(s0, n));
        STAGE_CHK(fn, d_nnb.fetch(s0, n));
        STAGE_CHK(fn, d_sm.fetch(s0, n));
        STAGE_CHK(fn, d_bm.fetch(s0, n));
        STAGE_CHK(fn, d_low.fetch(s0, n));
        return NM_OK;
    });
}

int nm_cluster_spectral_last_timing(double *ms) { return last_timing("nm_cluster_spectral_last_timing", g_spectral_ms, ms); }

int nm_cluster_spectral(int device, int64_t npoints, int ndim, const double *x, double gamma, int ncomp, int nblock, const double *init,
                        int degree, int max_pass, double tol, double *embed, double *eigval, double *resid, double *deg, int32_t *info)
{
    static const char *const fn = "nm_cluster_spectral";
    if (npoints < 2 || npoints > SP_MAXN) return refuse(fn, "npoints must lie in 2..2^20");
    if (ndim < 1 || ndim > SP_MAXDIM) return refuse(fn, "ndim must lie in 1..16");
    if (!std::isfinite(gamma) || !(gamma > 0.0)) return refuse(fn, "gamma must be finite and positive");
    if (ncomp < 1 || ncomp > SP_MAXCOMP || ncomp > npoints) return refuse(fn, "ncomp must lie in 1..8 and be at most npoints");
    if (nblock < ncomp || nblock > SP_MAXBLOCK || nblock > npoints) return refuse(fn, "nblock must lie in ncomp..16 and be at most npoints");
    if (degree < 1 || degree > 64) return refuse(fn, "degree must lie in 1..64");
    if (max_pass < 1 || max_pass > 100000) return refuse(fn, "max_pass must lie in 1..100000");
    if (!std::isfinite(tol) || tol < 0.0) return refuse(fn, "tol must be finite and not negative");
    if (!x || !init || !embed || !eigval || !resid || !deg || !info) return refuse(fn, "a needed pointer is null");
    const int64_t bad = first_not_finite(init, npoints * nblock);
    if (bad >= 0)
        return fail(NM_ERR_ARG, std::string(fn) + ": init is not finite in row " + std::to_string(bad / nblock) + ", column " + std::to_string(bad % nblock));
    if (const int rc = stage_device(fn, device)) return rc;

    Spectral sp;
    const int n = sp.n = (int)npoints, m = sp.m = nblock, w = sp.w = sp_width(nblock);
    sp.ndim = ndim;
    sp.gamma = gamma;
    sp.wi = w == 1 ? 0 : w == 8 ? 1 : 2;
    sp.ne = n * w;
    sp.nchunks = (n + SP_CHUNK - 1) / SP_CHUNK;
    sp.grid = scan_grid<SpScan>(n, n);
    sp.flat = dim3((unsigned)((sp.ne + SP_BLOCK - 1) / SP_BLOCK));
    sp.rows = dim3((unsigned)((n + SP_BLOCK - 1) / SP_BLOCK));
    std::vector<double> block((size_t)n * w, 0.0);             // the start block at the padded width
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < m; ++c) block[(size_t)i * w + c] = init[(size_t)i * m + c];

    sp.laps.lap(SP_T_UPLOAD);
    STAGE_CHK(fn, sp.x.upload(x, (size_t)n * ndim));
    STAGE_CHK(fn, sp.a.upload(block.data(), block.size()));
    STAGE_CHK(fn, sp.b.alloc((size_t)sp.ne));
    STAGE_CHK(fn, sp.u.alloc((size_t)sp.ne));
    STAGE_CHK(fn, sp.deg.alloc(n));
    STAGE_CHK(fn, sp.rs.alloc(n));
    STAGE_CHK(fn, sp.part.alloc((size_t)sp.grid.y * sp.ne));
    STAGE_CHK(fn, sp.gpart.alloc((size_t)sp.nchunks * w * w));
    STAGE_CHK(fn, sp.small.alloc((size_t)w * w));
    STAGE_CHK(fn, sp.theta.alloc(w));
    int first = -1;
    STAGE_CHK(fn, scan_screen<SpScan>(n, ndim, sp.x, first));
    if (first >= 0) return fail(NM_ERR_ARG, std::string(fn) + ": x is not finite in point " + std::to_string(first));
    sp.laps.lap(SP_T_UPLOAD);

    // the degree: the pass at width 1 over u = 1, and the screen for a point that no other point reaches
    const int none = 0x7fffffff;
    STAGE_CHK(fn, sp.bad.upload(&none, 1));
    sp.pass(nullptr, 0, SP_T_DEGREE);
    hipLaunchKernelGGL(nm_spectral_degree_kernel, sp.rows, dim3(SP_BLOCK), 0, 0, n, (int)sp.grid.y, sp.part, sp.deg, sp.rs, sp.bad);
    STAGE_CHK(fn, hipGetLastError());
    STAGE_CHK(fn, sp.bad.download(&first, 1));
    sp.laps.lap(SP_T_DEGREE);
    if (first != none)
        return fail(NM_ERR_ARG, std::string(fn) + ": the degree of point " + std::to_string(first) +
                                    " is 0: gamma is too large for it, no other point lies within its reach");

    bool rank = true;
    STAGE_CHK(fn, sp.orthonormalise(sp.a, &rank));
    if (!rank) return refuse(fn, "the columns of init are linearly dependent to working precision");

    double h[SP_MAXBLOCK * SP_MAXBLOCK], q[SP_MAXBLOCK * SP_MAXBLOCK], theta[SP_MAXBLOCK] = {}, res[SP_MAXBLOCK] = {};
    double low = 0.0;                                           // the upper end of the damped interval
    int passes = 0, status = 0;
    for (int round = 0;; ++round) {
        // the Rayleigh-Ritz pass: b = M a, the Ritz pairs of a^T b, both rotated onto them, and the residuals b - a theta
        sp.pass(sp.u, sp.wi, SP_T_PASS);
        sp.join(1.0, 0.0, 0.0, nullptr, sp.b, false);
        ++passes;
        STAGE_CHK(fn, sp.gram(sp.a, sp.b, h));
        sp_jacobi(m, w, h, q, theta);
        STAGE_CHK(fn, sp.apply(sp.a, q, sp.a, false));
        STAGE_CHK(fn, sp.apply(sp.b, q, sp.b, false));
        STAGE_CHK(fn, hipMemcpy(sp.theta, theta, (size_t)w * sizeof(double), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(nm_spectral_resid_kernel, sp.flat, dim3(SP_BLOCK), 0, 0, sp.ne, w, sp.theta, sp.a, sp.b, sp.u);
        STAGE_CHK(fn, sp.gram(sp.u, sp.u, h));
        double worst = 0.0;
        for (int c = 0; c < m; ++c) {
            res[c] = std::sqrt(h[c * w + c]);
            if (c < ncomp && !(res[c] <= worst)) worst = res[c];
        }
        if (worst <= tol) { status = 0; break; }
        if (passes + degree > max_pass) { status = 2; break; } // the next round is degree - 1 filter passes and its Rayleigh-Ritz pass
        // The filter: Zhou and Saad's scaled Chebyshev recurrence that damps [-1, low] and is 1 at 1.  low is the smallest Ritz
        // value of the block; a block no wider than ncomp keeps that of its first round, since its last column is wanted and
        // must stay outside.  Its first term needs M a, which is b.
        if (round == 0 || m > ncomp) low = theta[m - 1] > -1.0 + 0x1p-10 ? theta[m - 1] : -1.0 + 0x1p-10;
        const double e = 0.5 * (low + 1.0), c0 = 0.5 * (low - 1.0);
        double sigma = e / (1.0 - c0);
        const double sigma1 = sigma;
        hipLaunchKernelGGL(nm_spectral_axpby_kernel, sp.flat, dim3(SP_BLOCK), 0, 0, sp.ne, w, sp.rs, sigma1 / e, -c0 * (sigma1 / e), sp.a, sp.b,
                           sp.u);
        sp.laps.lap(SP_T_BLOCK);
        double *cur = sp.b, *prev = sp.a;
        for (int k = 2; k <= degree; ++k) {
            const double sigma2 = 1.0 / (2.0 / sigma1 - sigma);
            sp.pass(sp.u, sp.wi, SP_T_PASS);
            sp.join(2.0 * (sigma2 / e), -2.0 * c0 * (sigma2 / e), -(sigma * sigma2), cur, prev, true);
            ++passes;
            std::swap(cur, prev);
            sigma = sigma2;
        }
        STAGE_CHK(fn, hipGetLastError());
        STAGE_CHK(fn, sp.orthonormalise(cur, &rank));
        if (!rank) return fail(NM_ERR_STATE, std::string(fn) + ": the filtered block lost its rank in pass " + std::to_string(passes));
    }
    STAGE_CHK(fn, hipDeviceSynchronize());
    sp.laps.lap(SP_T_HOST);
    sp.laps.book(g_spectral_ms);

    std::vector<double> d((size_t)n);
    STAGE_CHK(fn, sp.a.download(block.data(), block.size()));
    STAGE_CHK(fn, sp.deg.download(d.data(), d.size()));
    for (int c = 0; c < ncomp; ++c) {                           // embed = v / sqrt(deg), the entry of largest magnitude positive
        double top = -1.0, sign = 1.0;
        for (int i = 0; i < n; ++i) {
            const double v = block[(size_t)i * w + c] / std::sqrt(d[i]);
            embed[(size_t)i * ncomp + c] = v;
            if (std::fabs(v) > top) { top = std::fabs(v); sign = v < 0.0 ? -1.0 : 1.0; }
        }
        if (sign < 0.0)
            for (int i = 0; i < n; ++i) embed[(size_t)i * ncomp + c] = -embed[(size_t)i * ncomp + c];
    }
    for (int i = 0; i < n; ++i) deg[i] = d[i];
    for (int c = 0; c < m; ++c) { eigval[c] = theta[c]; resid[c] = res[c]; }
    info[0] = passes;
    info[1] = status;
    return NM_OK;
}

int nm_distr_lof(int device, int64_t nsets, int npts, int ndim, const double *x, int k, double *lof, double *lrd, double *kdist,
                 int32_t *nbr)
{
    static const char *const fn = "nm_distr_lof";
    if (nsets < 1 || nsets > LOF_MAXSETS) return refuse(fn, "nsets must lie in 1..2^20");
    if (npts < 2 || npts > LOF_MAXPTS) return refuse(fn, "npts must lie in 2..4096");
    if (nsets * npts > LOF_MAXN) return refuse(fn, "nsets * npts must not exceed 2^21 points");
    if (ndim < 1 || ndim > LOF_MAXDIM) return refuse(fn, "ndim must lie in 1..16");
    if (k < 1 || k > npts - 1 || k > LOF_MAXK) return refuse(fn, "k must lie in 1..min(npts - 1, 64)");
    if (!x || !lof || !lrd || !kdist) return refuse(fn, "a needed pointer is null");
    if (const int rc = stage_device(fn, device)) return rc;
    const int n = (int)(nsets * npts), rows = lof_rows(k), blocks = (npts + rows - 1) / rows;
    const dim3 flat((unsigned)((n + LOF_BLOCK - 1) / LOF_BLOCK));
    Laps<LOF_T_COUNT> laps;
    DevBuf<double> d_x, d_dist, d_kdist, d_lrd, d_lof;
    DevBuf<int> d_nbr;
    laps.lap(LOF_T_UPLOAD);
    STAGE_CHK(fn, d_x.upload(x, (size_t)n * ndim));
    STAGE_CHK(fn, d_nbr.alloc((size_t)n * k));
    STAGE_CHK(fn, d_dist.alloc((size_t)n * k));
    STAGE_CHK(fn, d_kdist.alloc(n));
    STAGE_CHK(fn, d_lrd.alloc(n));
    STAGE_CHK(fn, d_lof.alloc(n));
    int first = -1;
    STAGE_CHK(fn, scan_screen<LofScreen>(n, ndim, d_x, first));
    if (first >= 0)
        return fail(NM_ERR_ARG, std::string(fn) + ": x is not finite in set " + std::to_string(first / npts) + ", point " + std::to_string(first % npts));
    laps.lap(LOF_T_UPLOAD);
    hipLaunchKernelGGL(LOF_NEIGHBOURS[ndim - 1], dim3((unsigned)(nsets * blocks)), dim3((unsigned)rows), lof_list_bytes(k), 0, npts, k, blocks,
                       d_x, d_nbr, d_dist, d_kdist);
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(LOF_T_NEIGHBOURS);
    hipLaunchKernelGGL(nm_lof_lrd_kernel, flat, dim3(LOF_BLOCK), 0, 0, n, npts, k, d_nbr, d_dist, d_kdist, d_lrd);
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(LOF_T_LRD);
    hipLaunchKernelGGL(nm_lof_lof_kernel, flat, dim3(LOF_BLOCK), 0, 0, n, npts, k, d_nbr, d_lrd, d_lof);
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(LOF_T_LOF);
    STAGE_CHK(fn, hipDeviceSynchronize());
    laps.book(g_distr_ms);
    STAGE_CHK(fn, d_lof.download(lof, n));
    STAGE_CHK(fn, d_lrd.download(lrd, n));
    STAGE_CHK(fn, d_kdist.download(kdist, n));
    if (nbr) STAGE_CHK(fn, d_nbr.download(nbr, (size_t)n * k));
    return NM_OK;
}

int nm_cluster_kmeans_last_timing(double *ms) { return last_timing("nm_cluster_kmeans_last_timing", g_kmeans_ms, ms); }

int nm_cluster_kmeans(int device, int64_t npoints, int ndim, const double *x, int k, int nrestarts, const double *init, int max_iter,
                      double tol, int32_t *label, double *centre, int32_t *count, double *inertia, int32_t *iters, int32_t *status,
                      int32_t *best)
{
    static const char *const fn = "nm_cluster_kmeans";
    if (npoints < 1 || npoints > KM_MAXN) return refuse(fn, "npoints must lie in 1..2^21");
    if (ndim < 1 || ndim > KM_MAXDIM) return refuse(fn, "ndim must lie in 1..16");
    if (k < 1 || k > KM_MAXK || k > npoints) return refuse(fn, "k must lie in 1..256 and be at most npoints");
    if (nrestarts < 1 || nrestarts > KM_MAXR || k * nrestarts > KM_MAXCOLS)
        return refuse(fn, "nrestarts must lie in 1..64 and k * nrestarts be at most 4096");
    if (max_iter < 1 || max_iter > 10000) return refuse(fn, "max_iter must lie in 1..10000");
    if (!std::isfinite(tol) || tol < 0.0) return refuse(fn, "tol must be finite and not negative");
    if (!x || !init || !label || !centre || !count || !inertia || !iters || !status || !best) return refuse(fn, "a needed pointer is null");
    const int64_t bad = first_not_finite(init, (int64_t)nrestarts * k * ndim);
    if (bad >= 0)
        return fail(NM_ERR_ARG, std::string(fn) + ": init is not finite in restart " + std::to_string(bad / ((int64_t)k * ndim)) + ", centre " +
                                    std::to_string(bad / ndim % k));
    if (const int rc = stage_device(fn, device)) return rc;
    const int n = (int)npoints, nr = nrestarts, nchunks = (n + KM_CHUNK - 1) / KM_CHUNK;
    const size_t stride = (size_t)nchunks * KM_CHUNK;           // of a restart's labels
    const Lloyd &kn = LLOYD[ndim - 1];
    const dim3 rows((unsigned)((n + KM_ROWS - 1) / KM_ROWS)), chunks((unsigned)nchunks, (unsigned)nr);
    Laps<KM_T_COUNT> laps;
    DevBuf<double> d_x, d_centre, d_part, d_ipart;
    DevBuf<uint8_t> d_lab;
    DevBuf<int> d_cntp, d_ctl;                                  // d_ctl: state, status, iters, changed, nr ints each
    laps.lap(KM_T_UPLOAD);
    STAGE_CHK(fn, d_x.upload(x, (size_t)n * ndim));
    STAGE_CHK(fn, d_centre.upload(init, (size_t)nr * k * ndim));
    STAGE_CHK(fn, d_part.alloc((size_t)nchunks * nr * k * ndim));
    STAGE_CHK(fn, d_cntp.alloc((size_t)nchunks * nr * k));
    STAGE_CHK(fn, d_ipart.alloc((size_t)nchunks * nr));
    STAGE_CHK(fn, d_lab.alloc(stride * nr));
    STAGE_CHK(fn, d_ctl.alloc_zeroed((size_t)4 * nr));          // KM_RUN
    int *const d_state = d_ctl, *const d_status = d_state + nr, *const d_iters = d_status + nr, *const d_changed = d_iters + nr;
    int first = -1;
    STAGE_CHK(fn, scan_screen<KmScan>(n, ndim, d_x, first));
    if (first >= 0) return fail(NM_ERR_ARG, std::string(fn) + ": x is not finite in point " + std::to_string(first));
    laps.lap(KM_T_UPLOAD);
    // step max_iter + 1 holds nothing but the last assignment of a restart that stopped at max_iter
    std::vector<int> ctl((size_t)4 * nr);
    for (int step = 1, live = nr; live && step <= max_iter + 1; ++step) {
        hipLaunchKernelGGL(kn.assign, rows, dim3(KM_BLOCK), 0, 0, n, d_x, k, nr, d_centre, d_state, stride, d_lab, d_changed);
        laps.lap(KM_T_ASSIGN);
        hipLaunchKernelGGL(kn.sums, chunks, dim3(KM_BLOCK), 0, 0, n, d_x, k, nr, step, d_state, d_changed, stride, d_lab, d_part, d_cntp);
        hipLaunchKernelGGL(nm_kmeans_finish_kernel, dim3((unsigned)nr), dim3(KM_BLOCK), 0, 0, ndim, k, nr, nchunks, step, max_iter, tol, d_part,
                           d_cntp, d_centre, d_state, d_status, d_iters, d_changed);
        STAGE_CHK(fn, hipGetLastError());
        laps.lap(KM_T_UPDATE);
        if (step % KM_LOOK && step != max_iter + 1) continue;
        STAGE_CHK(fn, d_ctl.download(ctl.data(), (size_t)4 * nr));
        live = 0;
        for (int r = 0; r < nr; ++r) live += ctl[r] != KM_DONE;
        laps.lap(KM_T_UPDATE);
    }
    hipLaunchKernelGGL(kn.inertia, chunks, dim3(64), 0, 0, n, d_x, k, nr, d_centre, stride, d_lab, d_ipart);
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(KM_T_ASSIGN);
    STAGE_CHK(fn, hipDeviceSynchronize());
    laps.book(g_kmeans_ms);
    std::vector<double> ipart((size_t)nchunks * nr), sum((size_t)nr, 0.0), cen((size_t)k * ndim);
    std::vector<uint8_t> lab((size_t)n);
    STAGE_CHK(fn, d_ipart.download(ipart.data(), ipart.size()));
    int b = 0;
    for (int r = 0; r < nr; ++r) {
        for (int c = 0; c < nchunks; ++c) sum[r] += ipart[(size_t)c * nr + r];      // the chunks ascending
        if (sum[r] < sum[b]) b = r;                             // the lowest index on equal bits
    }
    STAGE_CHK(fn, hipMemcpy(lab.data(), d_lab.p + stride * b, (size_t)n, hipMemcpyDeviceToHost));
    STAGE_CHK(fn, hipMemcpy(cen.data(), d_centre.p + (size_t)b * k * ndim, cen.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int j = 0; j < k; ++j) count[j] = 0;
    for (int i = 0; i < n; ++i) { label[i] = lab[i]; ++count[lab[i]]; }
    for (size_t e = 0; e < cen.size(); ++e) centre[e] = cen[e];
    for (int r = 0; r < nr; ++r) { inertia[r] = sum[r]; status[r] = ctl[nr + r]; iters[r] = ctl[2 * nr + r]; }
    *best = b;
    return NM_OK;
}

} // extern "C"
