// nm_reweight.h — the streaming kernels of the multistate reweighting (include/nm_reweight.h: the definitions of the map, the
// iteration and the targets).  The K x N matrix of reduced potentials is never stored: both kernels form u_k(n) from the two
// numbers of a state and the two numbers of a sample where they need it, so an application of the map is 2 K N float64
// exponentials on 3 N doubles of input.
//
//   nm_rw_denom_kernel     one thread per sample; the sampled states' (b, c, ln count + f) in LDS, RW_KT at a time.
//   nm_rw_moments_kernel   one workgroup per (TB states or targets, chunk of RW_CH samples): a thread strides over the chunk
//                          with a running (max, sums) per target; workgroup maximum, one rescale, wave64 butterfly, LDS across
//                          the four waves, one partial per (target, chunk).  <RW_TB, false> is the iteration (max and sum),
//                          <1, true> the expectation (the weights' squares, five centred moments, up to eight observables).
//   nm_rw_combine_kernel   one wave per target: the chunks' partials in a fixed order.
//   nm_rw_update_kernel    one workgroup: f <- F - F[0], delta, the iteration count, and the `done` word.
// An iteration is these four plain launches on the null stream.  Convergence is decided on the device: nm_rw_update_kernel
// sets RwStatus::done when delta <= tol and every kernel queued behind it returns at once, so the host reads the 16-byte
// status every RW_POLL iterations only and still returns the first iterate that met the tolerance.
//
// Error bound (u = 2^-53 = one rounding; exp and log of the device library: 1 ulp = 2 u; centred data; U = max |b e + c v|,
// A = max |ln count + f|, K' = the sampled states):
//   t_k = a_k - (b e + c v)          a_k one rounding, the product, the fma, the difference: |dt| <= 2 u A + 3 u U.
//   a tile's sum of exp(t_k - M)     M is exact.  Rounding the argument x = M - t_k costs the term u x e^-x, which matters only
//                                    for the terms that carry the sum, x <= ln K: (1 + ln K) u of the sum; the exp 2 u; four
//                                    interleaved accumulators of at most RW_KT/4 terms and their three additions: (K'/4 + 2) u.
//   tiles                            joined as running (max, sum): one exp, one product, one addition each: 4 u per further tile.
//   logd = M + log(sum)              2 u ln K for the log, u |logd| for the addition.
//   => |d logd| <= (K'/4 + 4 (tiles - 1) + 3 ln K + 5) u + 2 u A + 3 u U + u |logd|.
//   moments, t = -(b e + c v + logd) two fmas: 2 u (U + |logd|), and the argument's rounding (1 + ln N) u as above.
//   a thread's running sums          at most RW_CH/RW_BLOCK = 16 samples, each step one exp (2 u) and one fma (u): 3 min(16,
//                                    ceil(N/256)) u; no rescale happens where a thread holds one sample (N <= 256).
//   the workgroup                    exact maximum; one rescale 3 u; butterfly 6 u; four waves 3 u.
//   the combination                  exact maximum; one rescale 3 u; ceil(chunks/64) additions per lane; butterfly 6 u.
//   F = -(M + log(sum))              2 u ln N, u |F|.
//   => |dF| <= |d logd| + (3 min(16, ceil(N/256)) + ceil(N/2^18) + 22 + 3 ln N) u + 2 u (U + |logd|) + u |F|,
//   against (N + K + 64) u + 16 u U for any sequential summation: the sample count enters as N/2^18, not as N.
// A ratio of two such sums (a mean, a second moment) carries twice the relative bound of one sum, times the largest summand.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nm {

constexpr int RW_BLOCK = 256;
constexpr int RW_WAVES = RW_BLOCK / 64;
constexpr int RW_KT = 512;       // states per LDS tile of the denominator kernel: 12 KiB.  Registers, not LDS, set the occupancy: 96 / 68 /
                                 // 101 VGPRs = 5 / 7 / 4 waves per SIMD for the denominators / the iteration / the expectation
constexpr int RW_CH = 4096;      // samples per chunk: 2^20 samples are 256 chunks, one per CU even with two states
constexpr int RW_TB = 4;         // states per workgroup in the iteration: a sample is read once for four exponentials
constexpr int RW_TGB = 256;      // most targets per launch of the expectation
constexpr int RW_MAXOBS = 8;
constexpr int RW_NF = 8 + RW_MAXOBS; // a partial of the expectation: max, sum w, sum w^2, sums of w e, w v, w ee, w ev, w vv, w obs[0..7]
constexpr int RW_POLL = 8;       // iterations between two looks at the status word
constexpr int RW_MAXSTATES = 4096;

struct RwStatus {
    int done;      // delta <= tol was reached: every later kernel of the call returns at once
    int iters;     // applications of the map so far
    double delta;  // of the last one
};

// One step of a running log-sum-exp: the sums so far are to be multiplied by `scale`, the new term enters with weight `w`,
// one of the two is 1.  m = -inf at the start: exp(-inf) = 0 scales the empty sums, no NaN arises for finite t.
__device__ __forceinline__ void rw_step(double &m, double t, double &scale, double &w)
{
    const double d = t - m;
    const double x = exp(-fabs(d));
    const bool up = d > 0.0;
    scale = up ? x : 1.0;
    w = up ? 1.0 : x;
    m = up ? t : m;
}

// the same value in every lane, in a fixed order
__device__ __forceinline__ double rw_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__device__ __forceinline__ double rw_wave_max(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

// logd[n] = LSE over the ka sampled states of (alc[k] + f[aidx[k]] - (ab[k] e[n] + ac[k] v[n])); alc = ln count
__global__ void __launch_bounds__(RW_BLOCK)
nm_rw_denom_kernel(const RwStatus *__restrict__ st, int64_t n, const double *__restrict__ e, const double *__restrict__ v, int ka,
                   const double *__restrict__ ab, const double *__restrict__ ac, const double *__restrict__ alc,
                   const int *__restrict__ aidx, const double *__restrict__ f, double *__restrict__ logd)
{
    if (st->done) return;
    __shared__ double sb[RW_KT], sc[RW_KT], sa[RW_KT];
    const int64_t i = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    const bool live = i < n;
    const double ei = live ? e[i] : 0.0, vi = live ? v[i] : 0.0;
    double m = -INFINITY, s = 0.0;
    for (int k0 = 0; k0 < ka; k0 += RW_KT) {
        const int kt = (ka - k0) < RW_KT ? (ka - k0) : RW_KT;
        __syncthreads(); // the tile before this one has been read
        for (int k = threadIdx.x; k < kt; k += RW_BLOCK) {
            sb[k] = ab[k0 + k];
            sc[k] = ac[k0 + k];
            sa[k] = alc[k0 + k] + f[aidx[k0 + k]];
        }
        __syncthreads();
        double mt = -INFINITY;
        for (int k = 0; k < kt; ++k) mt = fmax(mt, sa[k] - fma(sb[k], ei, sc[k] * vi));
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        int k = 0;
        for (; k + 4 <= kt; k += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s4[j] += exp((sa[k + j] - fma(sb[k + j], ei, sc[k + j] * vi)) - mt);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (k + j < kt) s4[j] += exp((sa[k + j] - fma(sb[k + j], ei, sc[k + j] * vi)) - mt);
        const double stile = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        double scale, w;
        rw_step(m, mt, scale, w);
        s = fma(s, scale, w * stile);
    }
    if (live) logd[i] = m + log(s);
}

// part[(target - t0) * nchunks + chunk][NF] for the targets t0 + blockIdx.y * TB + (0..TB-1) below nt and the chunk blockIdx.x,
// with t = -(tb e[n] + tc v[n] + logd[n]).  NF = 2 (max, sum of exp(t - max)) without MOM, RW_NF with it.
template <int TB, bool MOM>
__global__ void __launch_bounds__(RW_BLOCK)
nm_rw_moments_kernel(const RwStatus *__restrict__ st, int64_t n, const double *__restrict__ e, const double *__restrict__ v,
                     const double *__restrict__ logd, int t0, int nt, const double *__restrict__ tb, const double *__restrict__ tc,
                     int nobs, const double *__restrict__ obs, double *__restrict__ part)
{
    static_assert(!MOM || TB == 1, "the expectation takes one target per workgroup");
    if (st->done) return;
    constexpr int NF = MOM ? RW_NF : 2;
    constexpr int NS = NF - 1; // sums
    __shared__ double red[RW_WAVES][TB * NS];
    __shared__ double redm[RW_WAVES][TB];
    __shared__ double bmax[TB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * RW_CH;
    const int64_t c1 = (n - c0) < RW_CH ? n : c0 + RW_CH;
    const int tfirst = t0 + (int)blockIdx.y * TB;
    double b[TB], c[TB], m[TB], s[TB][NS];
#pragma unroll
    for (int j = 0; j < TB; ++j) {
        const int t = (tfirst + j) < nt ? (tfirst + j) : nt - 1; // a group past the end repeats the last target and does not write it
        b[j] = tb[t];
        c[j] = tc[t];
        m[j] = -INFINITY;
#pragma unroll
        for (int q = 0; q < NS; ++q) s[j][q] = 0.0;
    }
    const int ns = MOM ? 7 + nobs : 1; // sums in use
    for (int64_t i = c0 + tid; i < c1; i += RW_BLOCK) {
        const double ei = e[i], vi = v[i], li = logd[i];
        double val[MOM ? NS : 1];
        if constexpr (MOM) {
            val[2] = ei;
            val[3] = vi;
            val[4] = ei * ei;
            val[5] = ei * vi;
            val[6] = vi * vi;
#pragma unroll
            for (int q = 0; q < RW_MAXOBS; ++q) val[7 + q] = q < nobs ? obs[(int64_t)q * n + i] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            const double t = -fma(b[j], ei, fma(c[j], vi, li));
            double scale, w;
            rw_step(m[j], t, scale, w);
            s[j][0] = fma(s[j][0], scale, w);
            if constexpr (MOM) {
                s[j][1] = fma(s[j][1], scale * scale, w * w);
#pragma unroll
                for (int q = 2; q < NS; ++q) s[j][q] = fma(s[j][q], scale, w * val[q]);
            }
        }
    }
    // the workgroup's maximum, exactly; a thread without a sample holds -inf and sums of 0, and exp(-inf) = 0
#pragma unroll
    for (int j = 0; j < TB; ++j) {
        const double wm = rw_wave_max(m[j]);
        if (lane == 0) redm[wave][j] = wm;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TB; ++j) {
        double mm = redm[0][j];
#pragma unroll
        for (int w = 1; w < RW_WAVES; ++w) mm = fmax(mm, redm[w][j]);
        const double r = exp(m[j] - mm); // the chunk holds a sample, so mm is finite
        if (tid == 0) bmax[j] = mm;
        s[j][0] *= r;
        if constexpr (MOM) {
            s[j][1] *= r * r;
#pragma unroll
            for (int q = 2; q < NS; ++q) s[j][q] *= r;
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            if (q < ns) { // uniform
                const double ws = rw_wave_sum(s[j][q]);
                if (lane == 0) red[wave][j * NS + q] = ws;
            }
        }
    }
    __syncthreads();
    if (tid < TB * NF) {
        const int j = tid / NF, q = tid % NF;
        if (tfirst + j < nt) {
            double x = 0.0;
            if (q == 0) x = bmax[j];
            else if (q - 1 < ns) x = ((red[0][j * NS + q - 1] + red[1][j * NS + q - 1]) + red[2][j * NS + q - 1]) + red[3][j * NS + q - 1];
            part[((int64_t)(tfirst + j - t0) * gridDim.x + blockIdx.x) * NF + q] = x;
        }
    }
}

// F[t] = -LSE over the chunks, and with MOM sums[t][RW_NF] = (max, the sums relative to it), for the nt targets of a launch
template <bool MOM>
__global__ void __launch_bounds__(RW_BLOCK)
nm_rw_combine_kernel(const RwStatus *__restrict__ st, int nt, int64_t nchunks, int nobs, const double *__restrict__ part,
                     double *__restrict__ F, double *__restrict__ sums)
{
    if (st->done) return;
    constexpr int NF = MOM ? RW_NF : 2;
    constexpr int NS = NF - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = (int)blockIdx.x * RW_WAVES + wave;
    if (t >= nt) return; // a whole wave; no barrier follows
    const double *p = part + (int64_t)t * nchunks * NF;
    double mm = -INFINITY;
    for (int64_t ch = lane; ch < nchunks; ch += 64) mm = fmax(mm, p[ch * NF]);
    mm = rw_wave_max(mm);
    double s[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0.0;
    for (int64_t ch = lane; ch < nchunks; ch += 64) {
        const double r = exp(p[ch * NF] - mm);
        s[0] = fma(r, p[ch * NF + 1], s[0]);
        if constexpr (MOM) {
            s[1] = fma(r * r, p[ch * NF + 2], s[1]);
#pragma unroll
            for (int q = 2; q < NS; ++q) s[q] = fma(r, p[ch * NF + 1 + q], s[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = rw_wave_sum(s[q]);
    if (lane == 0) {
        F[t] = -(mm + log(s[0]));
        if constexpr (MOM) {
            sums[(int64_t)t * RW_NF] = mm;
#pragma unroll
            for (int q = 0; q < NS; ++q) sums[(int64_t)t * RW_NF + 1 + q] = (q < 7 + nobs) ? s[q] : 0.0;
        }
    }
}

// f <- F - F[0], delta = max |f_new - (f_old + gauge)|; one workgroup.  gauge: the caller's f[0] in the first application (the
// centred f holds the start without it), 0 afterwards
__global__ void __launch_bounds__(RW_BLOCK)
nm_rw_update_kernel(RwStatus *__restrict__ st, int k, const double *__restrict__ F, double *__restrict__ f, double gauge, double tol)
{
    if (st->done) return;
    __shared__ double red[RW_WAVES];
    const double f0 = F[0];
    double d = 0.0;
    for (int i = threadIdx.x; i < k; i += RW_BLOCK) {
        const double fn = F[i] - f0;
        d = fmax(d, fabs((fn - f[i]) - gauge));
        f[i] = fn;
    }
    d = rw_wave_max(d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
    __syncthreads(); // also: every thread has read st->done
    if (threadIdx.x == 0) {
        d = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        st->iters += 1;
        st->delta = d;
        if (d <= tol) st->done = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Reweighted histograms (include/nm_reweight_hist.h, nm_reweight_histogram): hist[t][q][j] = the sum of the weights w_n =
// exp(-u_t(n) - logd[n] + tf) over the samples whose x[q][n] lies in bin j, and the weight below and above the edges.
//
//   nm_rw_bins_kernel      once per call and quantity: one thread per sample, the quantity's edges in LDS, a bisection that
//                          compares x with the edges themselves.  It writes a 16-bit code per sample: the bin 0 .. nbins - 1,
//                          nbins for "below", nbins + 1 for "above" - the index of the sample's counter, so that the histogram
//                          kernel does not branch on it.
//   tf                     nm_rw_denom_kernel, nm_rw_moments_kernel<RW_TB, false>, nm_rw_combine_kernel<false> as they are.
//   nm_rw_hist_kernel<TT>  one workgroup per (TT targets, RW_HG chunks of RW_CH samples).  A thread reads a sample and its nq
//                          codes once, forms the TT exponentials, and adds each weight to the nq counters it belongs to.
//   nm_rw_hist_out_kernel  the launch's integer counters to float64 with ordinary stores; it leaves the counters at zero.
//
// Fixed point.  A weight lies in [0, 1 + 1e-9]: tf = -(M + log S) with S >= 1 the sum of exp(t_n - M), so exp(t_n + tf) <= 1 up to
// the roundings of tf and of the exponential.  w 2^RW_HS = hi + fr with hi the integer part (hi <= 2^48 + 2^19, exact as a double,
// and x - hi is exact); lo = the integer part of fr 2^RW_LS < 2^48: a power of two times a double is exact, so the only loss is
// what lies below 2^-(RW_HS + RW_LS) = 2^-96 of the weight, less than 2^-96 per term, N 2^-96 per counter.  hi and lo go to two
// 64-bit LDS counters by integer atomics: integer addition is associative, so a counter holds the same bits in whatever order
// the lanes arrive.
// Overflow.  Low word in LDS: between two normalisations it takes at most RW_CH = 2^12 terms below 2^48 on top of a rest below
//   2^48: < 2^61.  A normalisation moves lo >> 48 into the high word and keeps lo < 2^48.
//   High word in LDS: a workgroup adds at most RW_HG RW_CH = 2^14 terms of at most 2^48 (1 + 1e-9) and RW_HG carries of at most
//   2^12: < 2^63, whatever the weights sum to.
//   Global low word: every workgroup adds a normalised rest below 2^48, one per RW_HG chunks: with nsamples <= 2^28 =
//   RW_HIST_MAXN at most 2^14 of them, < 2^62.  (2^16 single chunks would still fit: the limit does not depend on RW_HG.)
//   Global high word: with the last carry it is the integer part of 2^48 times a sum of weights of one target, and all weights of
//   a target sum to 1 up to the error bound of tf (< 1e-9 for every admitted problem): < 2^49.
//   nm_rw_hist_out_kernel normalises once more: hi < 2^49 and lo < 2^48 convert exactly, hi 2^-48 + lo 2^-96 rounds once.
// LDS.  2 words of 8 B per (target of the tile, quantity, nbins + 2 counters).  The host takes TT = 4 targets where that stays
// within RW_HIST_LDS = 40 KiB (four workgroups per CU), else 2, else 1; one target at nq = 8, nbins = 1024 is 131,328 B of the
// CU's 163,840 B, one workgroup per CU.
constexpr int RW_MAXQ = 8;
constexpr int RW_MAXBINS = 1024;
constexpr int RW_HS = 48, RW_LS = 48;           // the weight's fixed-point split: truncation unit 2^-(RW_HS + RW_LS)
constexpr int RW_HG = 4;                        // chunks per workgroup of the histogram kernel: a quarter of the global atomics
constexpr int RW_HIST_LDS = 40 * 1024;          // what a tile of more than one target may take
constexpr int64_t RW_HIST_MAXN = (int64_t)1 << 28;
constexpr unsigned long long RW_LMASK = (1ull << RW_LS) - 1ull;
static_assert(RW_LS + 12 + 1 <= 64 && (1 << 12) == RW_CH, "the LDS low word takes a chunk of terms on top of a rest");
static_assert(RW_HS + 14 + 1 <= 63 && RW_HG * RW_CH == (1 << 14), "the LDS high word takes a workgroup's terms and carries");

__global__ void __launch_bounds__(RW_BLOCK)
nm_rw_bins_kernel(int64_t n, const double *__restrict__ x, int nbins, const double *__restrict__ edges, uint16_t *__restrict__ code)
{
    __shared__ double se[RW_MAXBINS + 1];
    for (int k = threadIdx.x; k <= nbins; k += RW_BLOCK) se[k] = edges[k];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double xi = x[i];
    int lo = 0, hi = nbins; // se[lo] <= xi, and xi < se[hi] or hi = nbins: the last bin is closed on the right
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (se[mid] <= xi) lo = mid;
        else hi = mid;
    }
    code[i] = (uint16_t)(xi < se[0] ? nbins : xi > se[nbins] ? nbins + 1 : lo);
}

// ghi, glo [(target - t0)][nq][nb2 = nbins + 2] += the fixed-point weights of the targets t0 + blockIdx.y * TT + (0..TT-1) below
// nt over the chunks blockIdx.x * RW_HG + (0..RW_HG-1); F [nt] is tf in the centred gauge, code [nq][n].  Dynamic LDS: 16 TT nq nb2 B.
template <int TT>
__global__ void __launch_bounds__(RW_BLOCK)
nm_rw_hist_kernel(int64_t n, const double *__restrict__ e, const double *__restrict__ v, const double *__restrict__ logd, int t0, int nt,
                  const double *__restrict__ tb, const double *__restrict__ tc, const double *__restrict__ F, int nq, int nb2,
                  const uint16_t *__restrict__ code, unsigned long long *__restrict__ ghi, unsigned long long *__restrict__ glo)
{
    extern __shared__ __align__(16) unsigned char rw_smem[];
    const int tid = threadIdx.x;
    const int per = nq * nb2, nc = TT * per;
    unsigned long long *shi = (unsigned long long *)rw_smem, *slo = shi + nc;
    for (int k = tid; k < 2 * nc; k += RW_BLOCK) shi[k] = 0ull;
    const int tfirst = t0 + (int)blockIdx.y * TT;
    double b[TT], c[TT], f[TT];
#pragma unroll
    for (int j = 0; j < TT; ++j) {
        const int t = (tfirst + j) < nt ? (tfirst + j) : nt - 1; // a tile past the end repeats the last target and does not write it
        b[j] = tb[t];
        c[j] = tc[t];
        f[j] = F[t];
    }
    __syncthreads();
    for (int g = 0; g < RW_HG; ++g) {
        const int64_t c0 = ((int64_t)blockIdx.x * RW_HG + g) * RW_CH;
        if (c0 >= n) break; // uniform
        const int64_t c1 = (n - c0) < RW_CH ? n : c0 + RW_CH;
        for (int64_t i = c0 + tid; i < c1; i += RW_BLOCK) {
            const double ei = e[i], vi = v[i], li = logd[i];
            int cd[RW_MAXQ];
#pragma unroll
            for (int q = 0; q < RW_MAXQ; ++q) cd[q] = q < nq ? (int)code[(int64_t)q * n + i] : 0;
#pragma unroll
            for (int j = 0; j < TT; ++j) {
                const double x = exp(f[j] - fma(b[j], ei, fma(c[j], vi, li))) * 0x1p48;
                const unsigned long long hi = (unsigned long long)x;
                const unsigned long long lo = (unsigned long long)((x - (double)hi) * 0x1p48); // x - hi is exact
#pragma unroll
                for (int q = 0; q < RW_MAXQ; ++q) {
                    if (q < nq) { // uniform
                        const int k = j * per + q * nb2 + cd[q];
                        if (hi) atomicAdd(&shi[k], hi);
                        if (lo) atomicAdd(&slo[k], lo);
                    }
                }
            }
        }
        __syncthreads();
        for (int k = tid; k < nc; k += RW_BLOCK) { // the carries of this chunk
            const unsigned long long l = slo[k];
            shi[k] += l >> RW_LS;
            slo[k] = l & RW_LMASK;
        }
        __syncthreads();
    }
    for (int k = tid; k < nc; k += RW_BLOCK) {
        const int j = k / per;
        if (tfirst + j >= nt) break; // j does not decrease with k
        const size_t dst = (size_t)(tfirst - t0) * per + k;
        if (shi[k]) atomicAdd(&ghi[dst], shi[k]);
        if (slo[k]) atomicAdd(&glo[dst], slo[k]);
    }
}

// out[k] = the counter k as a float64, k < count; the counters are left at zero for the next launch
__global__ void __launch_bounds__(RW_BLOCK)
nm_rw_hist_out_kernel(int64_t count, unsigned long long *__restrict__ ghi, unsigned long long *__restrict__ glo, double *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    if (k >= count) return;
    const unsigned long long l = glo[k], h = ghi[k] + (l >> RW_LS);
    out[k] = (double)h * 0x1p-48 + (double)(l & RW_LMASK) * 0x1p-96;
    ghi[k] = 0ull;
    glo[k] = 0ull;
}

} // namespace nm
