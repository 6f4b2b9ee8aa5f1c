// nm_vae.h — the kernels of the VAE stage (include/nm_vae.h; host side: nm_vae_api.hip).  float32 storage and arithmetic, tensors
// channels-last (n, z, y, x, c).  Every sum runs in an order that the shapes alone fix; no floating-point atomics.
//
// Three shapes of work cover the nine 3 x 3 x 3 layers and their gradients:
//   gather   out[n, o, co] = act(bias[co] + sum_{k, cr} src'[n, s(o, k), cr] W(k, cr, co)), src' = src, or src * act'(dy) (the backward
//            prologue).  direct:  s = stride o + k - p, W at (k, cr, co);  adjoint: s = (o + p - k) / stride where that divides,
//            W at (k, co, cr);  p = 1 at stride 1, 0 at stride 2 (TensorFlow's SAME), a source outside 0..si-1 counts as 0.
//            A convolution forward and a transposed convolution's data gradient are direct; a transposed convolution forward and
//            a convolution's data gradient are adjoint, and the Keras kernel layouts are exactly the two W layouts above.
//   wgrad    part[chunk][k][cb][cs] = sum_{(n, o) in chunk} big'[n, stride o + k - p, cb] small'[n, o, cs]: the weight gradient in
//            the layer's own layout (convolution: big = x, small = gy'; transposed: big = gy', small = x); dy, the layer's
//            output y, is never null here.  The n so^3 positions of the smaller grid are split into chunks of L consecutive ones
//            (L from the shapes: vae_split), nm_vae_sum_kernel adds the chunks in two levels.
//   bgrad    the bias gradient by the same split of the rows.
// gather and wgrad have two forms.  Where the reduced channel count is 32 or 64 and the produced one a multiple of 32 (the 32 <-> 64
// layers; wgrad: both multiples of 32) they are implicit GEMMs on v_mfma_f32_32x32x2_f32, one 32 x 32 tile per wave: operands
// A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31], result register r of a lane = entry (row (r & 3) + 8 (r >> 2) +
// 4 (lane >> 5), col lane & 31).
// In gather the rows are 32 positions and a lane reads 4 consecutive channels of its position per tap as one float4, used by 4
// instructions (the k order inside a tap is 0..3, 8..11, .. on the low half-wave and 4..7, 12..15, .. on the high one: fixed);
// in wgrad the rows are 32 channels of big, the columns 32 of small, k runs over positions and both operands are coalesced reads.
// The 1-channel ends (conv0: K = 27; the output layer: cout = 1) have nothing for the matrix unit and take the plain forms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nm {

constexpr int VAE_BLOCK = 256;
constexpr int VAE_TAPS = 27;
constexpr int VAE_WG_CHUNKS_MFMA = 32, VAE_WG_CHUNKS_PLAIN = 256, VAE_BG_CHUNKS = 256; // the most chunks of a split
constexpr int VAE_DENSE_WIDE = 1024;                       // from this dout on a workgroup, not a thread, adds a dense layer's data gradient
constexpr unsigned long long VAE_NOBAD = ~0ull;
enum { VAE_ACT_NONE = 0, VAE_ACT_RELU = 1, VAE_ACT_TANH = 2 };

typedef float vae_f32x16 __attribute__((ext_vector_type(16)));

struct VaeGather { int n, so, si, cr, co, stride, adj; };
struct VaeWgrad { int n, ss, sb, cb, cs, stride; long long L; };

// tanh in float64, rounded once: within 1 ulp of float32 of the tanh of the float32 argument
__device__ inline float vae_act(float v, int act)
{
    if (act == VAE_ACT_RELU) return v > 0.0f ? v : 0.0f;
    if (act == VAE_ACT_TANH) return (float)tanh((double)v);
    return v;
}
// the activation's derivative from its value
__device__ inline float vae_dact(float y, int act)
{
    const float relu = y > 0.0f ? 1.0f : 0.0f, th = 1.0f - y * y;
    return act == VAE_ACT_RELU ? relu : act == VAE_ACT_TANH ? th : 1.0f;
}
// the source coordinate of output coordinate o under tap k; false where it is padding (or, adjoint, no source maps there)
__device__ inline bool vae_tap(int o, int k, int stride, int adj, int si, int &s)
{
    const int p = stride == 1;
    if (!adj) s = stride * o + k - p;
    else {
        const int t = o + p - k;
        if (t < 0 || (t & (stride - 1))) return false;
        s = t >> (stride - 1);
    }
    return s >= 0 && s < si;
}
__device__ inline void vae_decode(long long m, int side, int &n, int &z, int &y, int &x)
{
    x = (int)(m % side); m /= side;
    y = (int)(m % side); m /= side;
    z = (int)(m % side);
    n = (int)(m / side);
}
// (n, z, y, x) moved `by` positions on
__device__ inline void vae_advance(int by, int side, int &n, int &z, int &y, int &x)
{
    x += by;
    while (x >= side) { x -= side; ++y; }
    while (y >= side) { y -= side; ++z; }
    while (z >= side) { z -= side; ++n; }
}

// ---- gather, plain: one thread per (position, co)
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_gather_kernel(VaeGather g, const float *__restrict__ src, const float *__restrict__ dy, int pact,
                                                                  const float *__restrict__ W, const float *__restrict__ bias, int act,
                                                                  float *__restrict__ out)
{
    const long long total = (long long)g.n * g.so * g.so * g.so * g.co;
    const long long e = (long long)blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % g.co);
    int nn, oz, oy, ox;
    vae_decode(e / g.co, g.so, nn, oz, oy, ox);
    float acc = 0.0f;
    for (int kz = 0; kz < 3; ++kz) {
        int sz, sy, sx;
        if (!vae_tap(oz, kz, g.stride, g.adj, g.si, sz)) continue;
        for (int ky = 0; ky < 3; ++ky) {
            if (!vae_tap(oy, ky, g.stride, g.adj, g.si, sy)) continue;
            for (int kx = 0; kx < 3; ++kx) {
                if (!vae_tap(ox, kx, g.stride, g.adj, g.si, sx)) continue;
                const int k = (kz * 3 + ky) * 3 + kx;
                const size_t sp = ((((size_t)nn * g.si + sz) * g.si + sy) * g.si + sx) * g.cr;
                const float *wp = g.adj ? W + ((size_t)k * g.co + c) * g.cr : W + (size_t)k * g.cr * g.co + c;
                const int ws = g.adj ? 1 : g.co;
                if (g.cr % 4 == 0) {                             // (the same sum, read four channels at a time)
                    for (int r = 0; r < g.cr; r += 4) {
                        float4 v = *reinterpret_cast<const float4 *>(src + sp + r);
                        if (dy) {
                            const float4 d = *reinterpret_cast<const float4 *>(dy + sp + r);
                            v.x *= vae_dact(d.x, pact); v.y *= vae_dact(d.y, pact); v.z *= vae_dact(d.z, pact); v.w *= vae_dact(d.w, pact);
                        }
                        acc = fmaf(v.x, wp[(size_t)r * ws], acc);
                        acc = fmaf(v.y, wp[(size_t)(r + 1) * ws], acc);
                        acc = fmaf(v.z, wp[(size_t)(r + 2) * ws], acc);
                        acc = fmaf(v.w, wp[(size_t)(r + 3) * ws], acc);
                    }
                    continue;
                }
                for (int r = 0; r < g.cr; ++r) {
                    float v = src[sp + r];
                    if (dy) v *= vae_dact(dy[sp + r], pact);
                    acc = fmaf(v, wp[(size_t)r * ws], acc);
                }
            }
        }
    }
    out[e] = vae_act(acc + (bias ? bias[c] : 0.0f), act);
}

// ---- gather on the matrix unit: cr = CR (32 or 64), co a multiple of 32; a wave per (32 positions, 32 co), 4 waves a workgroup.
// The 32 positions of a wave are consecutive ones, except in the adjoint map at stride 2: there only the taps of an output
// coordinate's own parity have a source, so the positions are taken class by class of the 8 parities (pz, py, px), consecutive
// within the class's (n, so/2, so/2, so/2) grid, and a wave skips the taps of the other parities as a whole: 27 / 8 taps on average.
// (The sum of an output runs over its taps in ascending k either way.)
template <int CR, int ADJ, int STRIDE>
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_gather_mfma_kernel(VaeGather g, const float *__restrict__ src, const float *__restrict__ dy, int pact,
                                                                       const float *__restrict__ W, const float *__restrict__ bias, int act,
                                                                       float *__restrict__ out)
{
    constexpr bool CLASSES = ADJ && STRIDE == 2;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int side = CLASSES ? g.so / 2 : g.so;                  // of the grid that a wave's positions are consecutive in
    const long long P = (long long)g.n * side * side * side;     // positions (of a class)
    const long long tiles = (P + 31) / 32;
    const long long tile = (long long)blockIdx.x * (VAE_BLOCK / 64) + (threadIdx.x >> 6);
    if (tile >= (CLASSES ? 8 * tiles : tiles)) return;           // (the whole wave; no barrier follows)
    const int cls = CLASSES ? (int)(tile / tiles) : 0;           // wave-uniform
    const int pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1;
    const long long m0 = (CLASSES ? tile % tiles : tile) * 32;
    const int c0 = blockIdx.y * 32;
    const bool live = m0 + r < P;
    int nn = 0, oz = 0, oy = 0, ox = 0;
    if (live) vae_decode(m0 + r, side, nn, oz, oy, ox);
    if (CLASSES) { oz = 2 * oz + pz; oy = 2 * oy + py; ox = 2 * ox + px; }
    const int mine = live ? (int)((((long long)nn * g.so + oz) * g.so + oy) * g.so + ox) : -1;   // the output position of row r
    vae_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int kz = CLASSES ? pz : 0; kz < 3; kz += CLASSES ? 2 : 1)
        for (int ky = CLASSES ? py : 0; ky < 3; ky += CLASSES ? 2 : 1)
            for (int kx = CLASSES ? px : 0; kx < 3; kx += CLASSES ? 2 : 1) {
                const int k = (kz * 3 + ky) * 3 + kx;
                int sz = 0, sy = 0, sx = 0;
                const bool ok = live && vae_tap(oz, kz, STRIDE, ADJ, g.si, sz) && vae_tap(oy, ky, STRIDE, ADJ, g.si, sy) && vae_tap(ox, kx, STRIDE, ADJ, g.si, sx);
                const size_t sp = ok ? ((((size_t)nn * g.si + sz) * g.si + sy) * g.si + sx) * CR + 4 * h : 0;
                float4 a[CR / 8], b[CR / 8];                      // this lane's four reduced channels of every eight
#pragma unroll
                for (int j = 0; j < CR / 8; ++j) {
                    a[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (ok) {
                        a[j] = *reinterpret_cast<const float4 *>(src + sp + 8 * j);
                        if (dy) {
                            const float4 d = *reinterpret_cast<const float4 *>(dy + sp + 8 * j);
                            a[j].x *= vae_dact(d.x, pact); a[j].y *= vae_dact(d.y, pact); a[j].z *= vae_dact(d.z, pact); a[j].w *= vae_dact(d.w, pact);
                        }
                    }
                    if (ADJ) b[j] = *reinterpret_cast<const float4 *>(W + ((size_t)k * g.co + c0 + r) * CR + 8 * j + 4 * h);
                    else {
                        const float *wp = W + ((size_t)k * CR + 8 * j + 4 * h) * g.co + c0 + r;
                        b[j] = make_float4(wp[0], wp[g.co], wp[2 * (size_t)g.co], wp[3 * (size_t)g.co]);
                    }
                }
#pragma unroll
                for (int j = 0; j < CR / 8; ++j) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].x, b[j].x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].y, b[j].y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].z, b[j].z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].w, b[j].w, acc, 0, 0, 0);
                }
            }
    const float bc = bias ? bias[c0 + r] : 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = __shfl(mine, (i & 3) + 8 * (i >> 2) + 4 * h);      // the output position of this register's row
        if (m >= 0) out[(size_t)m * g.co + c0 + r] = vae_act(acc[i] + bc, act);
    }
}

// ---- wgrad, plain: one thread per (k, cb, cs) of a chunk
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_wgrad_kernel(VaeWgrad g, const float *__restrict__ big, const float *__restrict__ small,
                                                                 const float *__restrict__ dy, int dy_on_big, int pact, float *__restrict__ part)
{
    const int count = VAE_TAPS * g.cb * g.cs;
    const int e = blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (e >= count) return;
    const int k = e / (g.cb * g.cs), b = (e / g.cs) % g.cb, s = e % g.cs;
    const int kz = k / 9, ky = (k / 3) % 3, kx = k % 3, p = g.stride == 1;
    const long long Q = (long long)g.n * g.ss * g.ss * g.ss, q0 = (long long)blockIdx.y * g.L, q1 = q0 + g.L < Q ? q0 + g.L : Q;
    int nn, oz, oy, ox;
    vae_decode(q0, g.ss, nn, oz, oy, ox);
    float acc = 0.0f;
    for (long long q = q0; q < q1; ++q) {
        const int sz = g.stride * oz + kz - p, sy = g.stride * oy + ky - p, sx = g.stride * ox + kx - p;
        if (sz >= 0 && sz < g.sb && sy >= 0 && sy < g.sb && sx >= 0 && sx < g.sb) {
            const size_t ib = ((((size_t)nn * g.sb + sz) * g.sb + sy) * g.sb + sx) * g.cb + b, is = (size_t)q * g.cs + s;
            float vb = big[ib], vs = small[is];
            if (dy_on_big) vb *= vae_dact(dy[ib], pact);
            else vs *= vae_dact(dy[is], pact);
            acc = fmaf(vb, vs, acc);
        }
        vae_advance(1, g.ss, nn, oz, oy, ox);
    }
    part[(size_t)blockIdx.y * count + e] = acc;
}

// ---- wgrad on the matrix unit: cb and cs multiples of 32; a wave per (k, 32 cb, 32 cs, chunk); L is even
__global__ __launch_bounds__(64) void nm_vae_wgrad_mfma_kernel(VaeWgrad g, const float *__restrict__ big, const float *__restrict__ small,
                                                               const float *__restrict__ dy, int dy_on_big, int pact, float *__restrict__ part)
{
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int tb = g.cb / 32, ts = g.cs / 32;
    const int k = blockIdx.x / (tb * ts), rem = blockIdx.x % (tb * ts), b0 = (rem / ts) * 32, s0 = (rem % ts) * 32;
    const int kz = k / 9, ky = (k / 3) % 3, kx = k % 3, p = g.stride == 1;
    const long long Q = (long long)g.n * g.ss * g.ss * g.ss, q0 = (long long)blockIdx.y * g.L, q1 = q0 + g.L < Q ? q0 + g.L : Q;
    int nn, oz, oy, ox;
    vae_decode(q0 + h, g.ss, nn, oz, oy, ox);
    vae_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (long long t = q0; t < q1; t += 2) {
        const long long q = t + h;
        float a = 0.0f, b = 0.0f;
        const int sz = g.stride * oz + kz - p, sy = g.stride * oy + ky - p, sx = g.stride * ox + kx - p;
        if (q < q1 && sz >= 0 && sz < g.sb && sy >= 0 && sy < g.sb && sx >= 0 && sx < g.sb) {
            const size_t ib = ((((size_t)nn * g.sb + sz) * g.sb + sy) * g.sb + sx) * g.cb + b0 + r, is = (size_t)q * g.cs + s0 + r;
            a = big[ib];
            b = small[is];
            if (dy_on_big) a *= vae_dact(dy[ib], pact);
            else b *= vae_dact(dy[is], pact);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        vae_advance(2, g.ss, nn, oz, oy, ox);
    }
    float *o = part + ((size_t)blockIdx.y * VAE_TAPS + k) * g.cb * g.cs;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[(size_t)(b0 + (i & 3) + 8 * (i >> 2) + 4 * h) * g.cs + s0 + r] = acc[i];
}

// out[e] = the chunks' partials added in two levels: every 16 consecutive chunks in chunk order, then those sums in order (the
// rounding error grows with 16 + chunks / 16 additions, not with their number)
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_sum_kernel(const float *__restrict__ part, int nchunks, int count, float *__restrict__ out)
{
    const int e = blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (e >= count) return;
    float acc = 0.0f;
    for (int c0 = 0; c0 < nchunks; c0 += 16) {
        float v[16], sub = 0.0f;                                // (sixteen reads under way together; a chunk past the end counts as 0)
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = c0 + u < nchunks ? part[(size_t)(c0 + u) * count + e] : 0.0f;
#pragma unroll
        for (int u = 0; u < 16; ++u) sub += v[u];
        acc += sub;
    }
    out[e] = acc;
}

// ---- bgrad: part[chunk][c] = sum over the chunk's rows of g * act'(y); C <= 64.  A thread adds every (256 / C)-th row of its
// channel, the threads of a channel are added as a binary tree (the sums 2 j and 2 j + 1 of a level make sum j of the next)
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_bgrad_kernel(const float *__restrict__ gy, const float *__restrict__ y, int act, long long rows, int C,
                                                                 long long L, float *__restrict__ part)
{
    __shared__ float s[VAE_BLOCK];
    const int tid = threadIdx.x, rl = VAE_BLOCK / C, c = tid % C, j = tid / C;
    const long long r0 = (long long)blockIdx.x * L, r1 = r0 + L < rows ? r0 + L : rows;
    float acc = 0.0f;
    if (j < rl)
        for (long long rr = r0 + j; rr < r1; rr += rl) acc += gy[(size_t)rr * C + c] * vae_dact(y[(size_t)rr * C + c], act);
    s[tid] = acc;
    __syncthreads();
    for (int live = rl; live > 1; live = (live + 1) / 2) {      // (uniform: every thread meets every barrier)
        const int half = live / 2;
        float t = 0.0f;
        if (j < half) t = s[(2 * j) * C + c] + s[(2 * j + 1) * C + c];
        else if (j == half && (live & 1)) t = s[(2 * j) * C + c];
        __syncthreads();
        if (j < (live + 1) / 2) s[j * C + c] = t;
        __syncthreads();
    }
    if (tid < C) part[(size_t)blockIdx.x * C + tid] = s[tid];
}

// ---- dense.  y[n][j] = act(b[j] + sum_i x[n][i] w[i][j]): a workgroup per (64 j, n), wave s adds i = s, s + 4, .., the four are added in order
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_dense_kernel(int din, int dout, const float *__restrict__ x, const float *__restrict__ w,
                                                                 const float *__restrict__ b, int act, float *__restrict__ y)
{
    __shared__ float s[VAE_BLOCK];
    const int tid = threadIdx.x, j = blockIdx.x * 64 + (tid & 63), sl = tid >> 6, n = blockIdx.y;
    float acc = 0.0f;
    if (j < dout)
        for (int i = sl; i < din; i += 4) acc = fmaf(x[(size_t)n * din + i], w[(size_t)i * dout + j], acc);
    s[tid] = acc;
    __syncthreads();
    if (sl == 0 && j < dout) y[(size_t)n * dout + j] = vae_act(((s[tid] + s[tid + 64]) + s[tid + 128]) + s[tid + 192] + b[j], act);
}
// gw[i][j] = sum_n x[n][i] g'[n][j], g' = gy act'(y), in n order
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_dense_gw_kernel(int n, int din, int dout, const float *__restrict__ x, const float *__restrict__ y,
                                                                    const float *__restrict__ gy, int act, float *__restrict__ gw)
{
    const long long e = (long long)blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (e >= (long long)din * dout) return;
    const int i = (int)(e / dout), j = (int)(e % dout);
    float acc = 0.0f;
    for (int m = 0; m < n; ++m) acc = fmaf(x[(size_t)m * din + i], gy[(size_t)m * dout + j] * vae_dact(y[(size_t)m * dout + j], act), acc);
    gw[e] = acc;
}
// gb[j] = sum_n g'[n][j], in n order
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_dense_gb_kernel(int n, int dout, const float *__restrict__ y, const float *__restrict__ gy, int act,
                                                                    float *__restrict__ gb)
{
    const int j = blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (j >= dout) return;
    float acc = 0.0f;
    for (int m = 0; m < n; ++m) acc += gy[(size_t)m * dout + j] * vae_dact(y[(size_t)m * dout + j], act);
    gb[j] = acc;
}
// gx[n][i] (+)= sum_j g'[n][j] w[i][j], in j order
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_dense_gx_kernel(int n, int din, int dout, const float *__restrict__ w, const float *__restrict__ y,
                                                                    const float *__restrict__ gy, int act, int add, float *__restrict__ gx)
{
    const long long e = (long long)blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (e >= (long long)n * din) return;
    const int m = (int)(e / din), i = (int)(e % din);
    float acc = 0.0f;
    for (int j = 0; j < dout; ++j) acc = fmaf(gy[(size_t)m * dout + j] * vae_dact(y[(size_t)m * dout + j], act), w[(size_t)i * dout + j], acc);
    gx[e] = add ? gx[e] + acc : acc;
}

// the same for a long sum (dout >= VAE_DENSE_WIDE): a workgroup per (n, i), thread t adds j = t, t + 256, .., then a tree over the threads
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_dense_gx_wide_kernel(int n, int din, int dout, const float *__restrict__ w, const float *__restrict__ y,
                                                                         const float *__restrict__ gy, int act, int add, float *__restrict__ gx)
{
    __shared__ float s[VAE_BLOCK];
    const int tid = threadIdx.x, m = blockIdx.x / din, i = blockIdx.x % din;
    float acc = 0.0f;
    for (int j = tid; j < dout; j += VAE_BLOCK) acc = fmaf(gy[(size_t)m * dout + j] * vae_dact(y[(size_t)m * dout + j], act), w[(size_t)i * dout + j], acc);
    s[tid] = acc;
    __syncthreads();
    for (int wd = VAE_BLOCK / 2; wd > 0; wd >>= 1) {
        if (tid < wd) s[tid] += s[tid + wd];
        __syncthreads();
    }
    if (tid == 0) gx[blockIdx.x] = add ? gx[blockIdx.x] + s[0] : s[0];
}

// ---- the model's own pieces
// bad = the first sample (atomicMin of an integer) that holds a value that is not finite
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_screen_kernel(const float *__restrict__ x, long long count, long long per, unsigned long long *bad)
{
    const long long e = (long long)blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (e < count && !isfinite(x[e])) atomicMin(bad, (unsigned long long)(e / per));
}
// xb[b] = data[idx[b]]
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_take_kernel(const float *__restrict__ data, const long long *__restrict__ idx, int nb, long long per,
                                                                float *__restrict__ xb)
{
    const long long e = (long long)blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (e >= nb * per) return;
    xb[e] = data[(size_t)idx[e / per] * per + e % per];
}
// z = mu + exp(lv / 2) eps (eps null: z = mu); kl[n] = sum_d (exp(lv) + mu^2 - lv - 1) / 2 in d order
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_latent_kernel(int nb, int ld, const float *__restrict__ mu, const float *__restrict__ lv,
                                                                  const float *__restrict__ eps, float *__restrict__ z, float *__restrict__ kl)
{
    const int n = blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (n >= nb) return;
    float acc = 0.0f;
    for (int d = 0; d < ld; ++d) {
        const float m = mu[n * ld + d], l = lv[n * ld + d];
        z[n * ld + d] = eps ? fmaf(expf(0.5f * l), eps[n * ld + d], m) : m;
        acc += expf(l) + m * m - l - 1.0f;
    }
    kl[n] = 0.5f * acc;
}
// rec[n] = sum_voxels (x - y)^2: a workgroup per sample, thread t adds the voxels t, t + 256, .., then a tree over the threads;
// gy = 2 (y - x) / nb where asked for: the gradient of the batch mean
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_rec_kernel(int nb, long long per, const float *__restrict__ x, const float *__restrict__ y,
                                                               float *__restrict__ rec, float *__restrict__ gy)
{
    __shared__ float s[VAE_BLOCK];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float scale = 2.0f / (float)nb;
    float acc = 0.0f;
    for (long long e = tid; e < per; e += VAE_BLOCK) {
        const float d = y[(size_t)n * per + e] - x[(size_t)n * per + e];
        acc = fmaf(d, d, acc);
        if (gy) gy[(size_t)n * per + e] = scale * d;
    }
    s[tid] = acc;
    __syncthreads();
    for (int w = VAE_BLOCK / 2; w > 0; w >>= 1) {
        if (tid < w) s[tid] += s[tid + w];
        __syncthreads();
    }
    if (tid == 0) rec[n] = s[0];
}
// from gz, the decoder's gradient of the batch mean with respect to z (in place): gmu = gz + mu / nb and
// glv = gz eps exp(lv / 2) / 2 + (exp(lv) - 1) / (2 nb)
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_latent_grad_kernel(int nb, int ld, const float *__restrict__ mu, const float *__restrict__ lv,
                                                                       const float *__restrict__ eps, float *__restrict__ gz_gmu, float *__restrict__ glv)
{
    const int e = blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (e >= nb * ld) return;
    const float inv = 1.0f / (float)nb, g = gz_gmu[e], l = lv[e];
    gz_gmu[e] = fmaf(mu[e], inv, g);
    glv[e] = (eps ? 0.5f * g * eps[e] * expf(0.5f * l) : 0.0f) + 0.5f * (expf(l) - 1.0f) * inv;
}
// loss[0], loss[1] = the means of rec and kl over the batch, in sample order
__global__ void nm_vae_mean_kernel(int nb, const float *__restrict__ rec, const float *__restrict__ kl, float *__restrict__ loss)
{
    if (threadIdx.x > 1 || blockIdx.x) return;
    const float *v = threadIdx.x ? kl : rec;
    float acc = 0.0f;
    for (int n = 0; n < nb; ++n) acc += v[n];
    loss[threadIdx.x] = acc / (float)nb;
}
// Keras 2's Nadam on the flat vector; cg = (1 - mc_t) / (1 - M), cm = mc_t1 / (1 - M'), cv = 1 / (1 - beta2^t): the host's float64, rounded
__global__ __launch_bounds__(VAE_BLOCK) void nm_vae_nadam_kernel(long long count, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                                                                 float *__restrict__ theta, float lr, float cg, float cm, float cv)
{
    const long long e = (long long)blockIdx.x * VAE_BLOCK + threadIdx.x;
    if (e >= count) return;
    const float ge = g[e];
    const float me = 0.9f * m[e] + 0.1f * ge;
    const float ve = 0.999f * v[e] + 0.001f * (ge * ge);
    m[e] = me;
    v[e] = ve;
    theta[e] -= lr * (cg * ge + cm * me) / (sqrtf(ve * cv) + 1e-7f);
}

} // namespace nm
