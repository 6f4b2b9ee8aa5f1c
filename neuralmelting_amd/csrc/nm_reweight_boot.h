// nm_reweight_boot.h — the kernels of the batched weighted MBAR (include/nm_reweight_boot.h: the definition).  A bootstrap
// replicate r is the sample set of the base problem with integer multiplicities m_r[n]; its solution f_r = f + d_r is sought as
// the perturbation d_r of the base solution f.  With logd[n] the base denominators (nm_rw_denom_kernel as it is) and
//   p_k(n) = exp(ln count[k] + f[k] - u_k(n) - logd[n])      (sampled states; sum_k p_k(n) = 1)
//   q_i(n) = exp(f[i] - u_i(n) - logd[n])                    (every state; sum_n q_i(n) = 1 at the fixed point)
// which depend on the base solution only, one application of replicate r's map is
//   ratio_r(n) = sum_k p_k(n) exp(d_r[k]),  g_r[n] = m_r[n] / ratio_r(n),  S_r[i] = sum_n q_i(n) g_r[n],
//   d_r[i] <- log S_r[0] - log S_r[i]
// (logd_r = logd + log ratio_r, exp(-F_r[i]) = exp(-f[i]) S_r[i]).  The exponentials p and q are formed once per (state,
// sample) and tile of RB_RT replicates; per replicate there is one fused multiply-add.  All terms are non-negative and of order
// one: nothing is rescaled in the inner loops, a sample of multiplicity 0 contributes an exact 0.
//
//   nm_rb_weights_kernel<INV>  one thread per sample; the sampled states' (b, c, ln count + f) and exp(d_r[k]) of the tile's
//                              replicates in LDS, RB_KT states at a time.  Writes g_r[n] (INV: 1 / ratio_r(n), the expectation
//                              multiplies by m itself, because it needs m w^2 as well) for the tile, g[j][n].
//   nm_rb_sums_kernel          one workgroup per (RB_SB states, chunk of RW_CH samples): one exponential per (state, sample),
//                              RB_SB x RB_RT accumulators per thread, wave64 butterfly, LDS across the four waves.
//   nm_rb_combine_kernel<NS>   one wave per (replicate of the tile, state or target): the chunks' partials in a fixed order.
//   nm_rb_update_kernel        one workgroup per replicate: d_r, delta_r, iters_r, and the replicate's `done` word; a replicate
//                              that is done is not touched again.  RbControl::ndone counts them (an integer atomic: the count
//                              does not depend on the order); once it reaches nrep every kernel queued behind returns at once.
//                              A tile whose replicates are all done returns at once too.
//   nm_rb_expect_kernel        one workgroup per (4 or 2 targets, chunk of RB_ECH samples, RB_RE replicates of the tile): q_t(n) =
//                              exp(tf_t - u_t(n) - logd[n]) with the base tf (the existing kernels), a = q / ratio_r, x = m a; sums
//                              of x, x a (= m w^2), x times the five centred moments and the observables.
//
// Error bound of one application (u = 2^-53; U, A as in nm_reweight.h; K' sampled states; an error of logd[n] itself cancels
// between p, q and ratio: logd is only the common scale of sample n):
//   p_k(n), q_i(n)   the argument a_k - (b e + c v) - logd: 2 u A + 3 u U + u |logd| absolute, i.e. relative in p; the exp 2 u.
//   ratio            K' products with exp(d) (2 u + u) and K' fmas into one accumulator: (K' + 3) u relative, all terms >= 0.
//   g                one conversion (exact, m < 2^16), one division: u.
//   S                a thread at most RW_CH / RW_BLOCK = 16 fmas, butterfly 6 u, four waves 3 u, the chunks ceil(chunks/64) + 6:
//                    (31 + ceil(N / 2^18)) u relative.
//   d                two logs (2 u each, of values near 1: absolute), one difference.
//   => |d d_r| <= (K' + 45 + ceil(N / 2^18)) u + 2 (2 u A + 3 u U + u max |logd|), against the 3 ((N + K + 64) u + 16 u U) of
//   three sequential sums that the tests allow.
// Compiler report (gfx950, -O3): see DESIGN.md §9 f-5.
#pragma once
#include "nm_reweight.h"

namespace nm {

constexpr int RB_KT = 128;       // states per LDS tile of the weights kernel: 3 KiB of (b, c, a) and 16 KiB of exp(d)
constexpr int RB_RT = 16;        // replicates per tile: the workspace is RB_RT x N doubles, never nrep x N
constexpr int RB_SB = 2;         // states per workgroup of the sums kernel: 32 accumulators per thread
constexpr int RB_RE = 4;         // replicates per workgroup of the expectation kernel
constexpr int RB_ET = 4, RB_ETO = 2; // targets per workgroup of the expectation kernel without and with observables: 112 and 120 accumulators
constexpr int RB_ECH = 4 * RW_CH; // samples per chunk of the expectation kernel
constexpr int RB_NS = 7 + RW_MAXOBS; // sums of the expectation: x, x a, x e, x v, x ee, x ev, x vv, x obs[0..7]
constexpr int RB_MAXREP = 1024;
constexpr int RB_POLL = 4;       // applications between two looks at RbControl
static_assert(RB_RT % RB_RE == 0, "the expectation splits a tile into whole groups");
static_assert(RB_SB * RB_RT <= RW_BLOCK, "one thread per partial of a workgroup");

struct RbControl {
    int ndone; // replicates whose `done` word is set
    int nrep;
};

// true where every replicate of the tile r0 .. r0 + rt - 1 is done (uniform)
__device__ __forceinline__ bool rb_tile_done(const int *__restrict__ done, int r0, int rt)
{
    int live = 0;
    for (int j = 0; j < rt; ++j) live |= !done[r0 + j];
    return !live;
}

// g[j][n] = m_{r0+j}[n] / ratio_{r0+j}(n) (INV: 1 / ratio), j < rt <= RB_RT.  f [K] the centred base solution, d [nrep][K].
template <bool INV>
__global__ void __launch_bounds__(RW_BLOCK)
nm_rb_weights_kernel(const RbControl *__restrict__ ctl, const int *__restrict__ done, int64_t n, const double *__restrict__ e,
                     const double *__restrict__ v, const double *__restrict__ logd, int ka, const double *__restrict__ ab,
                     const double *__restrict__ ac, const double *__restrict__ alc, const int *__restrict__ aidx,
                     const double *__restrict__ f, int K, const double *__restrict__ d, int r0, int rt,
                     const uint16_t *__restrict__ mult, double *__restrict__ g)
{
    if (ctl->ndone >= ctl->nrep || rb_tile_done(done, r0, rt)) return;
    __shared__ double sb[RB_KT], sc[RB_KT], sa[RB_KT];
    __shared__ double sx[RB_KT][RB_RT];
    const int64_t i = (int64_t)blockIdx.x * RW_BLOCK + threadIdx.x;
    const bool live = i < n;
    const double ei = live ? e[i] : 0.0, vi = live ? v[i] : 0.0, li = live ? logd[i] : INFINITY; // past the end: p = 0
    double acc[RB_RT];
#pragma unroll
    for (int j = 0; j < RB_RT; ++j) acc[j] = 0.0;
    for (int k0 = 0; k0 < ka; k0 += RB_KT) {
        const int kt = (ka - k0) < RB_KT ? (ka - k0) : RB_KT;
        __syncthreads(); // the tile before this one has been read
        for (int k = threadIdx.x; k < kt; k += RW_BLOCK) {
            sb[k] = ab[k0 + k];
            sc[k] = ac[k0 + k];
            sa[k] = alc[k0 + k] + f[aidx[k0 + k]];
        }
        for (int q = threadIdx.x; q < kt * RB_RT; q += RW_BLOCK) {
            const int k = q / RB_RT, j = q % RB_RT;
            sx[k][j] = j < rt ? exp(d[(int64_t)(r0 + j) * K + aidx[k0 + k]]) : 0.0; // a replicate past the end: 0, never written
        }
        __syncthreads();
        for (int k = 0; k < kt; ++k) {
            const double p = exp((sa[k] - fma(sb[k], ei, sc[k] * vi)) - li);
#pragma unroll
            for (int j = 0; j < RB_RT; ++j) acc[j] = fma(p, sx[k][j], acc[j]);
        }
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < RB_RT; ++j) {
        if (j < rt) { // uniform
            const double m = INV ? 1.0 : (double)mult[(int64_t)(r0 + j) * n + i];
            g[(int64_t)j * n + i] = m / acc[j];
        }
    }
}

// part[(j * K + state) * nchunks + chunk] = the chunk's sum of q_state(n) g[j][n], for the states group * RB_SB + (0..RB_SB-1)
// below K and j < rt.  A linear grid of nchunks x ceil(K / RB_SB) workgroups with the group as the fast index: the workgroups that
// run at one time share a few chunks, whose samples and RB_RT weights (about 0.6 MiB a chunk) then come from the L2, not from memory
__global__ void __launch_bounds__(RW_BLOCK)
nm_rb_sums_kernel(const RbControl *__restrict__ ctl, const int *__restrict__ done, int64_t n, const double *__restrict__ e,
                  const double *__restrict__ v, const double *__restrict__ logd, int K, const double *__restrict__ b,
                  const double *__restrict__ c, const double *__restrict__ f, int r0, int rt, const double *__restrict__ g,
                  double *__restrict__ part)
{
    if (ctl->ndone >= ctl->nrep || rb_tile_done(done, r0, rt)) return;
    __shared__ double red[RW_WAVES][RB_SB * RB_RT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ngroups = (K + RB_SB - 1) / RB_SB;
    const int64_t chunk = blockIdx.x / ngroups, nchunks = gridDim.x / ngroups;
    const int64_t c0 = chunk * RW_CH;
    const int64_t c1 = (n - c0) < RW_CH ? n : c0 + RW_CH;
    const int sfirst = (int)(blockIdx.x % ngroups) * RB_SB;
    double bs[RB_SB], cs[RB_SB], fs[RB_SB], acc[RB_SB][RB_RT];
#pragma unroll
    for (int s = 0; s < RB_SB; ++s) {
        const int k = (sfirst + s) < K ? (sfirst + s) : K - 1; // a group past the end repeats the last state and does not write it
        bs[s] = b[k];
        cs[s] = c[k];
        fs[s] = f[k];
#pragma unroll
        for (int j = 0; j < RB_RT; ++j) acc[s][j] = 0.0;
    }
    for (int64_t i = c0 + tid; i < c1; i += RW_BLOCK) {
        const double ei = e[i], vi = v[i], li = logd[i];
        double q[RB_SB];
#pragma unroll
        for (int s = 0; s < RB_SB; ++s) q[s] = exp(fs[s] - fma(bs[s], ei, fma(cs[s], vi, li)));
#pragma unroll
        for (int j = 0; j < RB_RT; ++j) {
            const double gj = j < rt ? g[(int64_t)j * n + i] : 0.0;
#pragma unroll
            for (int s = 0; s < RB_SB; ++s) acc[s][j] = fma(q[s], gj, acc[s][j]);
        }
    }
#pragma unroll
    for (int s = 0; s < RB_SB; ++s) {
#pragma unroll
        for (int j = 0; j < RB_RT; ++j) {
            const double ws = rw_wave_sum(acc[s][j]);
            if (lane == 0) red[wave][s * RB_RT + j] = ws;
        }
    }
    __syncthreads();
    if (tid < RB_SB * RB_RT) {
        const int s = tid / RB_RT, j = tid % RB_RT;
        if (sfirst + s < K && j < rt)
            part[((int64_t)j * K + sfirst + s) * nchunks + chunk] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

// out[row][NS] = the sums over the chunks of part[row][chunk][NS], one wave per row; a row is (replicate of the tile, state)
// with NS = 1 and (target of the launch, replicate of the tile) with NS = RB_NS.  done = nullptr: every row.
template <int NS>
__global__ void __launch_bounds__(RW_BLOCK)
nm_rb_combine_kernel(const RbControl *__restrict__ ctl, const int *__restrict__ done, int r0, int rt, int64_t rows, int64_t nchunks,
                     const double *__restrict__ part, double *__restrict__ out)
{
    if (done && (ctl->ndone >= ctl->nrep || rb_tile_done(done, r0, rt))) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * RW_WAVES + wave;
    if (row >= rows) return; // a whole wave; no barrier follows
    const double *p = part + row * nchunks * NS;
    double s[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0.0;
    for (int64_t ch = lane; ch < nchunks; ch += 64) {
#pragma unroll
        for (int q = 0; q < NS; ++q) s[q] += p[ch * NS + q];
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = rw_wave_sum(s[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) out[row * NS + q] = s[q];
    }
}

// replicate r = blockIdx.x: d_r[i] <- log S_r[0] - log S_r[i], delta_r = max |d_new - d_old - gauge| (gauge: the caller's f[0]
// in the first application, 0 afterwards), iters_r; status 0 and done where delta_r <= tol; status 2 and done where an S_r[i]
// is zero, subnormal or not finite (d_r is then not to be used).  S [nrep][K].
__global__ void __launch_bounds__(RW_BLOCK)
nm_rb_update_kernel(RbControl *__restrict__ ctl, int *__restrict__ done, int K, const double *__restrict__ S, double *__restrict__ d,
                    double gauge, double tol, int *__restrict__ iters, double *__restrict__ delta, int *__restrict__ status)
{
    const int r = blockIdx.x;
    if (done[r]) return; // set by this workgroup only, in an earlier launch
    __shared__ double red[RW_WAVES];
    __shared__ int redbad[RW_WAVES];
    const double *s = S + (int64_t)r * K;
    double *dr = d + (int64_t)r * K;
    const double l0 = log(s[0]);
    double dm = 0.0;
    int bad = 0;
    for (int i = threadIdx.x; i < K; i += RW_BLOCK) {
        const double si = s[i];
        bad |= !(si >= 0x1p-1022 && si <= 0x1.fffffffffffffp1023);
        const double dn = l0 - log(si);
        dm = fmax(dm, fabs((dn - dr[i]) - gauge));
        dr[i] = dn;
    }
    dm = rw_wave_max(dm);
    bad = __any(bad);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = dm;
        redbad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        dm = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        bad = redbad[0] | redbad[1] | redbad[2] | redbad[3];
        iters[r] += 1;
        delta[r] = dm;
        if (bad || dm <= tol) {
            status[r] = bad ? 2 : 0;
            done[r] = 1;
            atomicAdd(&ctl->ndone, 1);
        }
    }
}

// part[(((t - t0) * rt + j) * nech + chunk) * RB_NS + q] for the targets t0 .. t0 + nb - 1, the nech = ceil(n / RB_ECH) chunks of
// RB_ECH samples and the replicates j < rt of the tile that starts at r0.  A workgroup takes TT targets, RB_RE replicates and one
// chunk: a sample's e, v, logd, RB_RE weights and multiplicities are read once for TT x RB_RE sets of sums (the kernel is bound
// by that traffic, not by the exponentials: with one target and 4096 samples per workgroup it moved 68 GB per launch of 256 targets and took three times as long),
// and the workgroup's reduction is spread over 64 samples per thread.  A linear grid of nech x ceil(nb / TT) x ceil(rt / RB_RE)
// workgroups, the chunk the slow index (as in nm_rb_sums_kernel).  NSUM = 7 without observables (the other columns are written as
// 0), RB_NS with them.  F [nt]: the base tf in the centred gauge, so that q_t(n) = exp(F[t] - u_t(n) - logd[n]) <= 1; g [rt][n] =
// 1 / ratio (nm_rb_weights_kernel<true>).
template <int TT, int NSUM>
__global__ void __launch_bounds__(RW_BLOCK)
nm_rb_expect_kernel(int64_t n, const double *__restrict__ e, const double *__restrict__ v, const double *__restrict__ logd, int t0, int nb,
                    const double *__restrict__ tb, const double *__restrict__ tc, const double *__restrict__ F, int nobs,
                    const double *__restrict__ obs, int r0, int rt, const uint16_t *__restrict__ mult, const double *__restrict__ g,
                    double *__restrict__ part)
{
    static_assert(NSUM == 7 || NSUM == RB_NS, "without or with the observables");
    static_assert(TT * RB_RE * RB_NS <= RW_BLOCK, "one thread per partial of a workgroup");
    constexpr int NP = TT * RB_RE * NSUM;
    __shared__ double red[RW_WAVES][NP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ngroups = (rt + RB_RE - 1) / RB_RE, inner = (nb + TT - 1) / TT * ngroups;
    const int64_t chunk = blockIdx.x / inner, nech = gridDim.x / inner;
    const int64_t c0 = chunk * RB_ECH;
    const int64_t c1 = (n - c0) < RB_ECH ? n : c0 + RB_ECH;
    const int tl = (int)(blockIdx.x % inner) / ngroups * TT; // the first target, counted from t0
    const int jfirst = (int)(blockIdx.x % inner) % ngroups * RB_RE;
    const int ns = 7 + nobs; // sums in use
    double bt[TT], ct[TT], ft[TT], acc[TT][RB_RE][NSUM];
#pragma unroll
    for (int s = 0; s < TT; ++s) {
        const int t = t0 + ((tl + s) < nb ? (tl + s) : nb - 1); // a group past the end repeats the last target and does not write it
        bt[s] = tb[t];
        ct[s] = tc[t];
        ft[s] = F[t];
#pragma unroll
        for (int j = 0; j < RB_RE; ++j) {
#pragma unroll
            for (int q = 0; q < NSUM; ++q) acc[s][j][q] = 0.0;
        }
    }
    for (int64_t i = c0 + tid; i < c1; i += RW_BLOCK) {
        const double ei = e[i], vi = v[i], li = logd[i];
        double val[NSUM], gj[RB_RE], mj[RB_RE];
        val[2] = ei;
        val[3] = vi;
        val[4] = ei * ei;
        val[5] = ei * vi;
        val[6] = vi * vi;
#pragma unroll
        for (int q = 7; q < NSUM; ++q) val[q] = q < ns ? obs[(int64_t)(q - 7) * n + i] : 0.0;
#pragma unroll
        for (int j = 0; j < RB_RE; ++j) {
            const bool in = jfirst + j < rt; // uniform
            gj[j] = in ? g[(int64_t)(jfirst + j) * n + i] : 0.0;
            mj[j] = in ? (double)mult[(int64_t)(r0 + jfirst + j) * n + i] : 0.0;
        }
#pragma unroll
        for (int s = 0; s < TT; ++s) {
            const double qt = exp(ft[s] - fma(bt[s], ei, fma(ct[s], vi, li)));
#pragma unroll
            for (int j = 0; j < RB_RE; ++j) {
                const double a = qt * gj[j], x = a * mj[j];
                acc[s][j][0] += x;
                acc[s][j][1] = fma(x, a, acc[s][j][1]);
#pragma unroll
                for (int q = 2; q < NSUM; ++q) {
                    if (q < 7 || q < ns) acc[s][j][q] = fma(x, val[q], acc[s][j][q]); // uniform
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < TT; ++s) {
#pragma unroll
        for (int j = 0; j < RB_RE; ++j) {
#pragma unroll
            for (int q = 0; q < NSUM; ++q) {
                const double ws = rw_wave_sum(acc[s][j][q]);
                if (lane == 0) red[wave][(s * RB_RE + j) * NSUM + q] = ws;
            }
        }
    }
    __syncthreads();
    if (tid < TT * RB_RE * RB_NS) {
        const int s = tid / (RB_RE * RB_NS), j = tid / RB_NS % RB_RE, q = tid % RB_NS;
        if (tl + s < nb && jfirst + j < rt) {
            const int k = (s * RB_RE + j) * NSUM + q;
            const double x = q < NSUM ? ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k] : 0.0;
            part[((((int64_t)(tl + s) * rt + jfirst + j) * nech) + chunk) * RB_NS + q] = x;
        }
    }
}

} // namespace nm
