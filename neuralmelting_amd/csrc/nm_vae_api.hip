// nm_vae_api.hip — the VAE stage (include/nm_vae.h; kernels: nm_vae.h): the layer launchers that the primitives and the model share,
// the network's table of layers and parameter offsets, forward, backward and the Nadam steps of an epoch.
#include "../../include/nm_vae.h"
#include "nm_vae.h"
#include "nm_host.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

using namespace nm;

namespace {
thread_local std::string g_vae_error;
std::string &stage_error() { return g_vae_error; }

enum { VAE_T_UPLOAD, VAE_T_FORWARD, VAE_T_BACKWARD, VAE_T_OPTIMISER, VAE_T_COUNT };
thread_local double g_vae_ms[VAE_T_COUNT];

constexpr int64_t VAE_MAX_ELEMS = (int64_t)1 << 30;
constexpr int VAE_MAX_BATCH = 4096, VAE_EVAL_BATCH = 64;
constexpr int VAE_LAYERS = 13;

struct Conv {
    int side_in, cin, cout, stride, transposed, act;
    int side_out() const { return transposed ? side_in * stride : side_in / stride; }
    int64_t in_per() const { return (int64_t)side_in * side_in * side_in * cin; }
    int64_t out_per() const { return (int64_t)side_out() * side_out() * side_out() * cout; }
    int64_t wcount() const { return (int64_t)VAE_TAPS * cin * cout; }
};

unsigned blocks(int64_t count) { return (unsigned)((count + VAE_BLOCK - 1) / VAE_BLOCK); }

// how the weight gradient's n ss^3 positions and the bias gradient's rows are split: from the shapes alone
struct Split { int64_t L; int chunks; };
Split vae_split(int64_t count, int most, bool even)
{
    int64_t L = (count + most - 1) / most;
    if (even) L = std::max<int64_t>(2, L + (L & 1));
    if (L < 1) L = 1;
    return Split{L, (int)((count + L - 1) / L)};
}
bool wgrad_mfma(const Conv &c) { return c.cin % 32 == 0 && c.cout % 32 == 0; }
Split wgrad_split(const Conv &c, int n)
{
    const int ss = c.transposed ? c.side_in : c.side_out();
    const bool mf = wgrad_mfma(c);
    return vae_split((int64_t)n * ss * ss * ss, mf ? VAE_WG_CHUNKS_MFMA : VAE_WG_CHUNKS_PLAIN, mf);
}
Split bgrad_split(const Conv &c, int n) { return vae_split((int64_t)n * c.out_per() / c.cout, VAE_BG_CHUNKS, false); }
// the partial sums that conv_backward needs room for at any n: the most chunks of either split (a smaller n can split into more
// chunks than a larger one)
size_t part_count(const Conv &c)
{
    return std::max((size_t)(wgrad_mfma(c) ? VAE_WG_CHUNKS_MFMA : VAE_WG_CHUNKS_PLAIN) * (size_t)c.wcount(), (size_t)VAE_BG_CHUNKS * (size_t)c.cout);
}

template <int CR> void launch_gather_mfma(const VaeGather &g, dim3 grid, const float *src, const float *dy, int pact, const float *W, const float *bias,
                                           int act, float *out)
{
#define VAE_GATHER(ADJ, STRIDE) \
    hipLaunchKernelGGL((nm_vae_gather_mfma_kernel<CR, ADJ, STRIDE>), grid, dim3(VAE_BLOCK), 0, 0, g, src, dy, pact, W, bias, act, out)
    if (g.adj) {
        if (g.stride == 2) VAE_GATHER(1, 2);
        else VAE_GATHER(1, 1);
    } else {
        if (g.stride == 2) VAE_GATHER(0, 2);
        else VAE_GATHER(0, 1);
    }
#undef VAE_GATHER
}

void launch_gather(const VaeGather &g, const float *src, const float *dy, int pact, const float *W, const float *bias, int act, float *out)
{
    const int64_t P = (int64_t)g.n * g.so * g.so * g.so;
    if ((g.cr == 32 || g.cr == 64) && g.co % 32 == 0) {
        // the adjoint map at stride 2 takes the positions class by class of the 8 parities, each class's tiles on their own
        const int64_t tiles = g.adj && g.stride == 2 ? 8 * ((P / 8 + 31) / 32) : (P + 31) / 32;
        const dim3 grid((unsigned)((tiles + 3) / 4), (unsigned)(g.co / 32));
        if (g.cr == 32) launch_gather_mfma<32>(g, grid, src, dy, pact, W, bias, act, out);
        else launch_gather_mfma<64>(g, grid, src, dy, pact, W, bias, act, out);
    } else
        hipLaunchKernelGGL(nm_vae_gather_kernel, dim3(blocks(P * g.co)), dim3(VAE_BLOCK), 0, 0, g, src, dy, pact, W, bias, act, out);
}

void conv_forward(const Conv &c, int n, const float *x, const float *w, const float *b, float *y)
{
    launch_gather(VaeGather{n, c.side_out(), c.side_in, c.cin, c.cout, c.stride, c.transposed}, x, nullptr, 0, w, b, c.act, y);
}

// gx may be null; part holds part_count(c) floats
void conv_backward(const Conv &c, int n, const float *x, const float *w, const float *y, const float *gy, float *gx, float *gw, float *gb, float *part)
{
    if (gx) launch_gather(VaeGather{n, c.side_in, c.side_out(), c.cout, c.cin, c.stride, !c.transposed}, gy, y, c.act, w, nullptr, VAE_ACT_NONE, gx);
    const Split sw = wgrad_split(c, n);
    const VaeWgrad g = c.transposed ? VaeWgrad{n, c.side_in, c.side_out(), c.cout, c.cin, c.stride, sw.L}
                                    : VaeWgrad{n, c.side_out(), c.side_in, c.cin, c.cout, c.stride, sw.L};
    const float *big = c.transposed ? gy : x, *small = c.transposed ? x : gy;
    const int count = (int)c.wcount();
    if (wgrad_mfma(c))
        hipLaunchKernelGGL(nm_vae_wgrad_mfma_kernel, dim3((unsigned)(VAE_TAPS * (g.cb / 32) * (g.cs / 32)), (unsigned)sw.chunks), dim3(64), 0, 0, g, big,
                           small, y, c.transposed, c.act, part);
    else
        hipLaunchKernelGGL(nm_vae_wgrad_kernel, dim3(blocks(count), (unsigned)sw.chunks), dim3(VAE_BLOCK), 0, 0, g, big, small, y, c.transposed, c.act,
                           part);
    hipLaunchKernelGGL(nm_vae_sum_kernel, dim3(blocks(count)), dim3(VAE_BLOCK), 0, 0, part, sw.chunks, count, gw);
    const Split sb = bgrad_split(c, n);
    hipLaunchKernelGGL(nm_vae_bgrad_kernel, dim3((unsigned)sb.chunks), dim3(VAE_BLOCK), 0, 0, gy, y, c.act, (long long)((int64_t)n * c.out_per() / c.cout),
                       c.cout, (long long)sb.L, part);
    hipLaunchKernelGGL(nm_vae_sum_kernel, dim3(blocks(c.cout)), dim3(VAE_BLOCK), 0, 0, part, sb.chunks, c.cout, gb);
}

void dense_forward(int n, int din, int dout, int act, const float *x, const float *w, const float *b, float *y)
{
    hipLaunchKernelGGL(nm_vae_dense_kernel, dim3((unsigned)((dout + 63) / 64), (unsigned)n), dim3(VAE_BLOCK), 0, 0, din, dout, x, w, b, act, y);
}
// gx may be null; add: gx += instead of =
void dense_backward(int n, int din, int dout, int act, const float *x, const float *w, const float *y, const float *gy, float *gx, int add, float *gw,
                    float *gb)
{
    hipLaunchKernelGGL(nm_vae_dense_gw_kernel, dim3(blocks((int64_t)din * dout)), dim3(VAE_BLOCK), 0, 0, n, din, dout, x, y, gy, act, gw);
    hipLaunchKernelGGL(nm_vae_dense_gb_kernel, dim3(blocks(dout)), dim3(VAE_BLOCK), 0, 0, n, dout, y, gy, act, gb);
    if (!gx) return;
    if (dout >= VAE_DENSE_WIDE)
        hipLaunchKernelGGL(nm_vae_dense_gx_wide_kernel, dim3((unsigned)((int64_t)n * din)), dim3(VAE_BLOCK), 0, 0, n, din, dout, w, y, gy, act, add, gx);
    else
        hipLaunchKernelGGL(nm_vae_dense_gx_kernel, dim3(blocks((int64_t)n * din)), dim3(VAE_BLOCK), 0, 0, n, din, dout, w, y, gy, act, add, gx);
}

int conv_check(const char *fn, int n, const Conv &c)
{
    if (n < 1) return refuse(fn, "n must be at least 1");
    if (c.stride != 1 && c.stride != 2) return refuse(fn, "stride must be 1 or 2");
    if (c.transposed != 0 && c.transposed != 1) return refuse(fn, "transposed must be 0 or 1");
    if (c.act < VAE_ACT_NONE || c.act > VAE_ACT_TANH) return refuse(fn, "act must be 0 (none), 1 (relu) or 2 (tanh)");
    if (c.cin < 1 || c.cin > 64 || c.cout < 1 || c.cout > 64) return refuse(fn, "cin and cout must lie in 1..64");
    if (c.side_in < 1 || c.side_in > 64) return refuse(fn, "side_in must lie in 1..64");
    if (!c.transposed && c.side_in % c.stride) return refuse(fn, "the stride must divide side_in");
    if (c.side_out() > 64) return refuse(fn, "the output's side must not exceed 64");
    if (n > VAE_MAX_ELEMS / std::max(c.in_per(), c.out_per())) return refuse(fn, "a tensor must not exceed 2^30 elements");
    return NM_OK;
}
int dense_check(const char *fn, int n, int din, int dout, int act)
{
    if (n < 1 || n > 65535) return refuse(fn, "n must lie in 1..65535");
    if (act < VAE_ACT_NONE || act > VAE_ACT_TANH) return refuse(fn, "act must be 0 (none), 1 (relu) or 2 (tanh)");
    if (din < 1 || dout < 1 || (int64_t)din * dout > ((int64_t)1 << 28)) return refuse(fn, "din and dout must be at least 1 and din * dout at most 2^28");
    if (n > VAE_MAX_ELEMS / std::max(din, dout)) return refuse(fn, "a tensor must not exceed 2^30 elements");
    return NM_OK;
}

// ---- the network: its activations by name, and one row per layer that net_make fills; the parameters' offsets, the activations'
// sizes, forward and backward are all walks of these rows
enum { X, A0, A1, A2, A3, E0, MU, LV, Z, F1, T0, T1, T2, T3, Y, VAE_ACTS, NO_GRAD = -1 };

struct Layer {
    bool dense;
    Conv c;                 // a convolution's shape, or
    int din, dout, act;     // a dense layer's
    int in, out;            // the activation it reads and the one it writes
    int gin, add;           // whose gradient buffer takes its data gradient (NO_GRAD: none is taken), and whether it is added there
};
Layer conv_layer(const Conv &c, int in, int out, int gin) { return Layer{false, c, 0, 0, 0, in, out, gin, 0}; }
Layer dense_layer(int din, int dout, int act, int in, int out, int gin, int add = 0) { return Layer{true, Conv{}, din, dout, act, in, out, gin, add}; }
// backward walks the rows from the last to the first, but the two heads as they came: dm writes E0's gradient, dv adds to it
constexpr int VAE_BACKWARD[VAE_LAYERS] = {12, 11, 10, 9, 8, 7, 5, 6, 4, 3, 2, 1, 0};

struct Net {
    int LD = 0;
    Layer layer[VAE_LAYERS];
    int64_t off[NM_VAE_NTENSORS + 1];   // of layer l the kernel at off[2 l], the bias at off[2 l + 1]
    int64_t size[VAE_ACTS];             // of an activation, per sample
    int64_t per() const { return size[X]; }
    int64_t nparams() const { return off[NM_VAE_NTENSORS]; }
};
int net_make(const char *fn, int side, int latent, Net &net)
{
    if (side < 4 || side > 32 || side % 4)
        return refuse(fn, "side must be a multiple of 4 in 4..32: the decoder doubles a quarter of the side twice and cannot rebuild another one "
                          "(-cb 11 gives 11 -> 6 -> 3 -> 6 -> 12)");
    if (latent < 1 || latent > 64) return refuse(fn, "latent must lie in 1..64");
    const int S = side, h = S / 2, q = S / 4, LD = latent, F = 64 * q * q * q, R = VAE_ACT_RELU, TANH = VAE_ACT_TANH, NONE = VAE_ACT_NONE;
    const Layer rows[VAE_LAYERS] = {
        //          the shape                   reads writes  its data gradient goes to
        conv_layer({S, 1, 32, 1, 0, R},         X,    A0,     NO_GRAD),     // c0: the samples take no gradient
        conv_layer({S, 32, 64, 2, 0, R},        A0,   A1,     A0),          // c1
        conv_layer({h, 64, 32, 1, 0, R},        A1,   A2,     A1),          // c2
        conv_layer({h, 32, 64, 2, 0, R},        A2,   A3,     A2),          // c3
        dense_layer(F, 8 * LD, R,               A3,   E0,     A3),          // d0
        dense_layer(8 * LD, LD, NONE,           E0,   MU,     E0),          // dm
        dense_layer(8 * LD, LD, NONE,           E0,   LV,     E0, 1),       // dv: added to what dm wrote
        // d1's data gradient gz goes to MU's gradient buffer (Z has none): nm_vae_latent_grad_kernel turns it into mu's and lv's in place
        dense_layer(LD, F, R,                   Z,    F1,     MU),          // d1
        conv_layer({q, 64, 64, 1, 1, R},        F1,   T0,     F1),          // t0
        conv_layer({q, 64, 32, 2, 1, R},        T0,   T1,     T0),          // t1
        conv_layer({h, 32, 64, 1, 1, R},        T1,   T2,     T1),          // t2
        conv_layer({h, 64, 32, 2, 1, R},        T2,   T3,     T2),          // t3
        conv_layer({S, 32, 1, 1, 1, TANH},      T3,   Y,      T3)};         // t4
    net.LD = LD;
    net.size[X] = (int64_t)S * S * S;
    net.size[Z] = LD;                   // (nm_vae_latent_kernel writes it, no layer does)
    int64_t at = 0;
    for (int l = 0; l < VAE_LAYERS; ++l) {
        const Layer &L = net.layer[l] = rows[l];
        net.size[L.out] = L.dense ? L.dout : L.c.out_per();
        net.off[2 * l] = at; at += L.dense ? (int64_t)L.din * L.dout : L.c.wcount();
        net.off[2 * l + 1] = at; at += L.dense ? L.dout : L.c.cout;
    }
    net.off[NM_VAE_NTENSORS] = at;
    return NM_OK;
}

// the activations of a batch (and, for training, the gradients of every layer's output), sized for `cap` samples
struct Acts {
    int cap = 0;
    bool grads = false;
    DevBuf<float> v[VAE_ACTS], g[VAE_ACTS], eps, rec, kl, part;
    DevBuf<long long> idx;
};
} // namespace

struct nm_vae_ctx {
    int device = 0;
    Net net;
    bool have_params = false;
    DevBuf<float> theta, m, v, grad, data, lossb;
    int64_t ndata = 0;
    double msched = 1.0;
    int64_t step = 0;
    Acts acts;
    Laps<VAE_T_COUNT> laps;
};

namespace {
#define ACT_ALLOC(buf, count) STAGE_CHK(fn, (buf).alloc((size_t)(count)))
int acts_reserve(const char *fn, nm_vae_ctx *ctx, int nb, bool grads)
{
    Acts &A = ctx->acts;
    if (nb <= A.cap && (!grads || A.grads)) return NM_OK;
    const Net &N = ctx->net;
    const int64_t cap = std::max(nb, A.cap);
    Acts B;
    for (int a = 0; a < VAE_ACTS; ++a) ACT_ALLOC(B.v[a], cap * N.size[a]);
    ACT_ALLOC(B.eps, cap * N.LD); ACT_ALLOC(B.rec, cap); ACT_ALLOC(B.kl, cap); ACT_ALLOC(B.idx, cap);
    if (grads || A.grads) {
        // backward reads the gradient of every layer's output; X and Z are no layer's output and have none
        size_t part = 1;
        for (const Layer &L : N.layer) {
            ACT_ALLOC(B.g[L.out], cap * N.size[L.out]);
            if (!L.dense) part = std::max(part, part_count(L.c));
        }
        ACT_ALLOC(B.part, part);
        B.grads = true;
    }
    B.cap = (int)cap;
    A = std::move(B);
    return NM_OK;
}

// the batch idx (device) with its noise eps (device, or null) through the network; A.rec and A.kl hold the loss terms
void forward(nm_vae_ctx *ctx, int nb, const long long *idx, const float *eps, bool want_gy)
{
    Acts &A = ctx->acts;
    const Net &N = ctx->net;
    hipLaunchKernelGGL(nm_vae_take_kernel, dim3(blocks(nb * N.per())), dim3(VAE_BLOCK), 0, 0, ctx->data.p, idx, nb, (long long)N.per(), A.v[X].p);
    ctx->laps.lap(VAE_T_UPLOAD);
    for (int l = 0; l < VAE_LAYERS; ++l) {
        const Layer &L = N.layer[l];
        const float *w = ctx->theta.p + N.off[2 * l], *b = ctx->theta.p + N.off[2 * l + 1];
        if (L.in == Z) hipLaunchKernelGGL(nm_vae_latent_kernel, dim3(blocks(nb)), dim3(VAE_BLOCK), 0, 0, nb, N.LD, A.v[MU].p, A.v[LV].p, eps, A.v[Z].p, A.kl.p);
        if (L.dense) dense_forward(nb, L.din, L.dout, L.act, A.v[L.in], w, b, A.v[L.out]);
        else conv_forward(L.c, nb, A.v[L.in], w, b, A.v[L.out]);
    }
    hipLaunchKernelGGL(nm_vae_rec_kernel, dim3((unsigned)nb), dim3(VAE_BLOCK), 0, 0, nb, (long long)N.per(), A.v[X].p, A.v[Y].p, A.rec.p,
                       want_gy ? A.g[Y].p : nullptr);
    ctx->laps.lap(VAE_T_FORWARD);
}

// behind forward(.., true): ctx->grad = the gradient of the batch's mean loss
void backward(nm_vae_ctx *ctx, int nb, const float *eps)
{
    Acts &A = ctx->acts;
    const Net &N = ctx->net;
    for (const int l : VAE_BACKWARD) {
        const Layer &L = N.layer[l];
        const float *w = ctx->theta.p + N.off[2 * l];
        float *gw = ctx->grad.p + N.off[2 * l], *gb = ctx->grad.p + N.off[2 * l + 1], *gx = L.gin == NO_GRAD ? nullptr : A.g[L.gin].p;
        if (L.dense) dense_backward(nb, L.din, L.dout, L.act, A.v[L.in], w, A.v[L.out], A.g[L.out], gx, L.add, gw, gb);
        else conv_backward(L.c, nb, A.v[L.in], w, A.v[L.out], A.g[L.out], gx, gw, gb, A.part);
        if (L.in == Z)
            hipLaunchKernelGGL(nm_vae_latent_grad_kernel, dim3(blocks((int64_t)nb * N.LD)), dim3(VAE_BLOCK), 0, 0, nb, N.LD, A.v[MU].p, A.v[LV].p, eps,
                               A.g[MU].p, A.g[LV].p);
    }
    ctx->laps.lap(VAE_T_BACKWARD);
}

// forward, the batch's mean rec and kl into the two floats at `loss` (device), backward: what nm_vae_grad and a step of nm_vae_epoch share
void batch_gradient(nm_vae_ctx *ctx, int nb, const long long *idx, const float *eps, float *loss)
{
    forward(ctx, nb, idx, eps, true);
    hipLaunchKernelGGL(nm_vae_mean_kernel, dim3(1), dim3(64), 0, 0, nb, ctx->acts.rec.p, ctx->acts.kl.p, loss);
    backward(ctx, nb, eps);
}

// what every model call asks first
int ctx_enter(const char *fn, nm_vae_ctx *ctx, bool need_params, bool need_data)
{
    if (!ctx) return refuse(fn, "ctx is null");
    if (need_params && !ctx->have_params) return fail(NM_ERR_STATE, std::string(fn) + ": the parameters were not set (nm_vae_set_params)");
    if (need_data && ctx->ndata < 1) return fail(NM_ERR_STATE, std::string(fn) + ": no samples are resident (nm_vae_data)");
    return NM_OK;
}
int idx_check(const char *fn, const nm_vae_ctx *ctx, int64_t nidx, const int64_t *idx)
{
    for (int64_t i = 0; i < nidx; ++i)
        if (idx[i] < 0 || idx[i] >= ctx->ndata) return fail(NM_ERR_ARG, std::string(fn) + ": idx[" + std::to_string(i) + "] is outside the resident samples");
    return NM_OK;
}
// behind a layer primitive's launches: their error, their lap into `slot`, the device's end and the booking of the laps
int primitive_done(const char *fn, Laps<VAE_T_COUNT> &laps, int slot)
{
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(slot);
    STAGE_CHK(fn, hipDeviceSynchronize());
    laps.book(g_vae_ms);
    return NM_OK;
}
} // namespace

extern "C" {
const char *nm_vae_last_error(void) { return g_vae_error.c_str(); }

int nm_vae_last_timing(double *ms) { return last_timing("nm_vae_last_timing", g_vae_ms, ms); }

int64_t nm_vae_nparams(int side, int latent)
{
    Net net;
    if (const int rc = net_make("nm_vae_nparams", side, latent, net)) return rc;
    return net.nparams();
}

int nm_vae_layout(int side, int latent, int64_t *off)
{
    static const char *const fn = "nm_vae_layout";
    Net net;
    if (const int rc = net_make(fn, side, latent, net)) return rc;
    if (!off) return refuse(fn, "a needed pointer is null");
    std::copy(net.off, net.off + NM_VAE_NTENSORS + 1, off);
    return NM_OK;
}

int nm_vae_conv(int device, int n, int side_in, int cin, int cout, int stride, int transposed, int act, const float *x, const float *w, const float *b,
                float *y)
{
    static const char *const fn = "nm_vae_conv";
    const Conv c{side_in, cin, cout, stride, transposed, act};
    if (const int rc = conv_check(fn, n, c)) return rc;
    if (!x || !w || !b || !y) return refuse(fn, "a needed pointer is null");
    if (const int rc = stage_device(fn, device)) return rc;
    Laps<VAE_T_COUNT> laps;
    laps.lap(VAE_T_UPLOAD);
    DevBuf<float> dx, dw, db, dy;
    STAGE_CHK(fn, dx.upload(x, (size_t)(n * c.in_per())));
    STAGE_CHK(fn, dw.upload(w, (size_t)c.wcount()));
    STAGE_CHK(fn, db.upload(b, (size_t)cout));
    STAGE_CHK(fn, dy.alloc((size_t)(n * c.out_per())));
    laps.lap(VAE_T_UPLOAD);
    conv_forward(c, n, dx, dw, db, dy);
    if (const int rc = primitive_done(fn, laps, VAE_T_FORWARD)) return rc;
    STAGE_CHK(fn, dy.download(y, (size_t)(n * c.out_per())));
    return NM_OK;
}

int nm_vae_conv_grad(int device, int n, int side_in, int cin, int cout, int stride, int transposed, int act, const float *x, const float *w,
                     const float *y, const float *gy, float *gx, float *gw, float *gb)
{
    static const char *const fn = "nm_vae_conv_grad";
    const Conv c{side_in, cin, cout, stride, transposed, act};
    if (const int rc = conv_check(fn, n, c)) return rc;
    if (!x || !w || !y || !gy || !gw || !gb) return refuse(fn, "a needed pointer is null");
    if (const int rc = stage_device(fn, device)) return rc;
    Laps<VAE_T_COUNT> laps;
    laps.lap(VAE_T_UPLOAD);
    DevBuf<float> dx, dw, dy, dgy, dgx, dgw, dgb, part;
    STAGE_CHK(fn, dx.upload(x, (size_t)(n * c.in_per())));
    STAGE_CHK(fn, dw.upload(w, (size_t)c.wcount()));
    STAGE_CHK(fn, dy.upload(y, (size_t)(n * c.out_per())));
    STAGE_CHK(fn, dgy.upload(gy, (size_t)(n * c.out_per())));
    if (gx) STAGE_CHK(fn, dgx.alloc((size_t)(n * c.in_per())));
    STAGE_CHK(fn, dgw.alloc((size_t)c.wcount()));
    STAGE_CHK(fn, dgb.alloc((size_t)cout));
    STAGE_CHK(fn, part.alloc(part_count(c)));
    laps.lap(VAE_T_UPLOAD);
    conv_backward(c, n, dx, dw, dy, dgy, gx ? dgx.p : nullptr, dgw, dgb, part);
    if (const int rc = primitive_done(fn, laps, VAE_T_BACKWARD)) return rc;
    if (gx) STAGE_CHK(fn, dgx.download(gx, (size_t)(n * c.in_per())));
    STAGE_CHK(fn, dgw.download(gw, (size_t)c.wcount()));
    STAGE_CHK(fn, dgb.download(gb, (size_t)cout));
    return NM_OK;
}

int nm_vae_dense(int device, int n, int din, int dout, int act, const float *x, const float *w, const float *b, float *y)
{
    static const char *const fn = "nm_vae_dense";
    if (const int rc = dense_check(fn, n, din, dout, act)) return rc;
    if (!x || !w || !b || !y) return refuse(fn, "a needed pointer is null");
    if (const int rc = stage_device(fn, device)) return rc;
    Laps<VAE_T_COUNT> laps;
    laps.lap(VAE_T_UPLOAD);
    DevBuf<float> dx, dw, db, dy;
    STAGE_CHK(fn, dx.upload(x, (size_t)n * din));
    STAGE_CHK(fn, dw.upload(w, (size_t)din * dout));
    STAGE_CHK(fn, db.upload(b, (size_t)dout));
    STAGE_CHK(fn, dy.alloc((size_t)n * dout));
    laps.lap(VAE_T_UPLOAD);
    dense_forward(n, din, dout, act, dx, dw, db, dy);
    if (const int rc = primitive_done(fn, laps, VAE_T_FORWARD)) return rc;
    STAGE_CHK(fn, dy.download(y, (size_t)n * dout));
    return NM_OK;
}

int nm_vae_dense_grad(int device, int n, int din, int dout, int act, const float *x, const float *w, const float *y, const float *gy, float *gx,
                      float *gw, float *gb)
{
    static const char *const fn = "nm_vae_dense_grad";
    if (const int rc = dense_check(fn, n, din, dout, act)) return rc;
    if (!x || !w || !y || !gy || !gw || !gb) return refuse(fn, "a needed pointer is null");
    if (const int rc = stage_device(fn, device)) return rc;
    Laps<VAE_T_COUNT> laps;
    laps.lap(VAE_T_UPLOAD);
    DevBuf<float> dx, dw, dy, dgy, dgx, dgw, dgb;
    STAGE_CHK(fn, dx.upload(x, (size_t)n * din));
    STAGE_CHK(fn, dw.upload(w, (size_t)din * dout));
    STAGE_CHK(fn, dy.upload(y, (size_t)n * dout));
    STAGE_CHK(fn, dgy.upload(gy, (size_t)n * dout));
    if (gx) STAGE_CHK(fn, dgx.alloc((size_t)n * din));
    STAGE_CHK(fn, dgw.alloc((size_t)din * dout));
    STAGE_CHK(fn, dgb.alloc((size_t)dout));
    laps.lap(VAE_T_UPLOAD);
    dense_backward(n, din, dout, act, dx, dw, dy, dgy, gx ? dgx.p : nullptr, 0, dgw, dgb);
    if (const int rc = primitive_done(fn, laps, VAE_T_BACKWARD)) return rc;
    if (gx) STAGE_CHK(fn, dgx.download(gx, (size_t)n * din));
    STAGE_CHK(fn, dgw.download(gw, (size_t)din * dout));
    STAGE_CHK(fn, dgb.download(gb, (size_t)dout));
    return NM_OK;
}

int nm_vae_create(int device, int side, int latent, nm_vae_ctx **out)
{
    static const char *const fn = "nm_vae_create";
    Net net;
    if (const int rc = net_make(fn, side, latent, net)) return rc;
    if (!out) return refuse(fn, "a needed pointer is null");
    if (const int rc = stage_device(fn, device)) return rc;
    nm_vae_ctx *ctx = new (std::nothrow) nm_vae_ctx;
    if (!ctx) return fail(NM_ERR_HIP, std::string(fn) + ": out of host memory");
    ctx->device = device;
    ctx->net = net;
    const size_t np = (size_t)net.nparams();
    hipError_t e = ctx->theta.alloc_zeroed(np);
    if (e == hipSuccess) e = ctx->m.alloc_zeroed(np);
    if (e == hipSuccess) e = ctx->v.alloc_zeroed(np);
    if (e == hipSuccess) e = ctx->grad.alloc_zeroed(np);
    if (e != hipSuccess) {
        delete ctx;
        return fail(NM_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
    }
    *out = ctx;
    return NM_OK;
}

int nm_vae_destroy(nm_vae_ctx *ctx)
{
    if (!ctx) return refuse("nm_vae_destroy", "ctx is null");
    hipSetDevice(ctx->device);
    delete ctx;
    return NM_OK;
}

int nm_vae_set_params(nm_vae_ctx *ctx, const float *theta)
{
    static const char *const fn = "nm_vae_set_params";
    if (const int rc = ctx_enter(fn, ctx, false, false)) return rc;
    if (!theta) return refuse(fn, "a needed pointer is null");
    const size_t np = (size_t)ctx->net.nparams();
    if (first_not_finite(theta, (int64_t)np) >= 0) return refuse(fn, "a parameter is not finite");
    STAGE_CHK(fn, hipSetDevice(ctx->device));
    STAGE_CHK(fn, hipMemcpy(ctx->theta.p, theta, np * sizeof(float), hipMemcpyHostToDevice));
    STAGE_CHK(fn, ctx->m.zero(np));
    STAGE_CHK(fn, ctx->v.zero(np));
    ctx->msched = 1.0;
    ctx->step = 0;
    ctx->have_params = true;
    return NM_OK;
}

int nm_vae_get_params(nm_vae_ctx *ctx, float *theta)
{
    static const char *const fn = "nm_vae_get_params";
    if (const int rc = ctx_enter(fn, ctx, true, false)) return rc;
    if (!theta) return refuse(fn, "a needed pointer is null");
    STAGE_CHK(fn, hipSetDevice(ctx->device));
    STAGE_CHK(fn, ctx->theta.download(theta, (size_t)ctx->net.nparams()));
    return NM_OK;
}

int nm_vae_data(nm_vae_ctx *ctx, int64_t n, const float *x)
{
    static const char *const fn = "nm_vae_data";
    if (const int rc = ctx_enter(fn, ctx, false, false)) return rc;
    const int64_t per = ctx->net.per();
    if (n < 1 || n > ((int64_t)1 << 40) / per) return refuse(fn, "n must be at least 1 and n * side^3 at most 2^40");
    if (!x) return refuse(fn, "a needed pointer is null");
    STAGE_CHK(fn, hipSetDevice(ctx->device));
    size_t free_b = 0, total_b = 0;
    STAGE_CHK(fn, hipMemGetInfo(&free_b, &total_b));
    const size_t held = ctx->data.n * sizeof(float), want = (size_t)(n * per) * sizeof(float);
    if (want > (free_b + held) / 2)
        return fail(NM_ERR_HIP, std::string(fn) + ": " + std::to_string(want) + " bytes of samples do not fit half of the device's free memory");
    ctx->ndata = 0;
    DevBuf<float> d;
    DevBuf<unsigned long long> bad;
    const unsigned long long none = VAE_NOBAD;
    STAGE_CHK(fn, d.upload(x, (size_t)(n * per)));
    STAGE_CHK(fn, bad.upload(&none, 1));
    hipLaunchKernelGGL(nm_vae_screen_kernel, dim3(blocks(n * per)), dim3(VAE_BLOCK), 0, 0, d.p, (long long)(n * per), (long long)per, bad.p);
    STAGE_CHK(fn, hipGetLastError());
    unsigned long long first = VAE_NOBAD;
    STAGE_CHK(fn, bad.download(&first, 1));
    ctx->data = Buf<float, DeviceMem>();
    if (first != VAE_NOBAD) return fail(NM_ERR_ARG, std::string(fn) + ": x is not finite in sample " + std::to_string(first));
    ctx->data = std::move(d);
    ctx->ndata = n;
    return NM_OK;
}

int nm_vae_eval(nm_vae_ctx *ctx, int64_t nidx, const int64_t *idx, const float *eps, float *z_mean, float *z_log_var, float *recon, float *rec, float *kl)
{
    static const char *const fn = "nm_vae_eval";
    if (const int rc = ctx_enter(fn, ctx, true, true)) return rc;
    if (nidx < 1) return refuse(fn, "nidx must be at least 1");
    if (!idx || !z_mean || !z_log_var || !rec || !kl) return refuse(fn, "a needed pointer is null");
    if (const int rc = idx_check(fn, ctx, nidx, idx)) return rc;
    STAGE_CHK(fn, hipSetDevice(ctx->device));
    const Net &N = ctx->net;
    const int LD = N.LD;
    const int64_t per = N.per();
    if (const int rc = acts_reserve(fn, ctx, (int)std::min<int64_t>(nidx, VAE_EVAL_BATCH), false)) return rc;
    Acts &A = ctx->acts;
    ctx->laps = Laps<VAE_T_COUNT>();
    ctx->laps.lap(VAE_T_UPLOAD);
    // the results gather in host vectors, so that a failure half way leaves the outputs untouched
    std::vector<float> hmu((size_t)nidx * LD), hlv((size_t)nidx * LD), hrec((size_t)nidx), hkl((size_t)nidx), hy(recon ? (size_t)(nidx * per) : 0);
    for (int64_t b0 = 0; b0 < nidx; b0 += VAE_EVAL_BATCH) {
        const int nb = (int)std::min<int64_t>(VAE_EVAL_BATCH, nidx - b0);
        STAGE_CHK(fn, hipMemcpy(A.idx.p, idx + b0, (size_t)nb * sizeof(int64_t), hipMemcpyHostToDevice));
        if (eps) STAGE_CHK(fn, hipMemcpy(A.eps.p, eps + b0 * LD, (size_t)nb * LD * sizeof(float), hipMemcpyHostToDevice));
        forward(ctx, nb, A.idx, eps ? A.eps.p : nullptr, false);
        STAGE_CHK(fn, hipGetLastError());
        STAGE_CHK(fn, A.v[MU].download(hmu.data() + b0 * LD, (size_t)nb * LD));
        STAGE_CHK(fn, A.v[LV].download(hlv.data() + b0 * LD, (size_t)nb * LD));
        STAGE_CHK(fn, A.rec.download(hrec.data() + b0, (size_t)nb));
        STAGE_CHK(fn, A.kl.download(hkl.data() + b0, (size_t)nb));
        if (recon) STAGE_CHK(fn, A.v[Y].download(hy.data() + b0 * per, (size_t)(nb * per)));
        ctx->laps.lap(VAE_T_UPLOAD);
    }
    ctx->laps.book(g_vae_ms);
    std::copy(hmu.begin(), hmu.end(), z_mean);
    std::copy(hlv.begin(), hlv.end(), z_log_var);
    std::copy(hrec.begin(), hrec.end(), rec);
    std::copy(hkl.begin(), hkl.end(), kl);
    if (recon) std::copy(hy.begin(), hy.end(), recon);
    return NM_OK;
}

int nm_vae_grad(nm_vae_ctx *ctx, int64_t nidx, const int64_t *idx, const float *eps, float *grad, double *loss)
{
    static const char *const fn = "nm_vae_grad";
    if (const int rc = ctx_enter(fn, ctx, true, true)) return rc;
    if (nidx < 1 || nidx > VAE_MAX_BATCH) return refuse(fn, "nidx must lie in 1..4096");
    if (!idx || !grad || !loss) return refuse(fn, "a needed pointer is null");
    if (const int rc = idx_check(fn, ctx, nidx, idx)) return rc;
    STAGE_CHK(fn, hipSetDevice(ctx->device));
    const Net &N = ctx->net;
    const int nb = (int)nidx;
    if (const int rc = acts_reserve(fn, ctx, nb, true)) return rc;
    Acts &A = ctx->acts;
    STAGE_CHK(fn, ctx->lossb.reserve(2));
    ctx->laps = Laps<VAE_T_COUNT>();
    ctx->laps.lap(VAE_T_UPLOAD);
    STAGE_CHK(fn, hipMemcpy(A.idx.p, idx, (size_t)nb * sizeof(int64_t), hipMemcpyHostToDevice));
    if (eps) STAGE_CHK(fn, hipMemcpy(A.eps.p, eps, (size_t)nb * N.LD * sizeof(float), hipMemcpyHostToDevice));
    batch_gradient(ctx, nb, A.idx, eps ? A.eps.p : nullptr, ctx->lossb.p);
    STAGE_CHK(fn, hipGetLastError());
    STAGE_CHK(fn, hipDeviceSynchronize());
    ctx->laps.book(g_vae_ms);
    float l2[2];
    STAGE_CHK(fn, ctx->lossb.download(l2, 2));
    STAGE_CHK(fn, ctx->grad.download(grad, (size_t)N.nparams()));
    loss[0] = l2[0];
    loss[1] = l2[1];
    return NM_OK;
}

int nm_vae_epoch(nm_vae_ctx *ctx, int64_t nidx, const int64_t *idx, const float *eps, int batch, double lr, double *loss)
{
    static const char *const fn = "nm_vae_epoch";
    if (const int rc = ctx_enter(fn, ctx, true, true)) return rc;
    if (nidx < 1) return refuse(fn, "nidx must be at least 1");
    if (batch < 1 || batch > VAE_MAX_BATCH) return refuse(fn, "batch must lie in 1..4096");
    if (!(lr > 0.0) || !std::isfinite(lr)) return refuse(fn, "lr must be finite and positive");
    if (!idx || !loss) return refuse(fn, "a needed pointer is null");
    if (const int rc = idx_check(fn, ctx, nidx, idx)) return rc;
    STAGE_CHK(fn, hipSetDevice(ctx->device));
    const Net &N = ctx->net;
    const int64_t steps = (nidx + batch - 1) / batch, np = N.nparams();
    if (const int rc = acts_reserve(fn, ctx, (int)std::min<int64_t>(batch, nidx), true)) return rc;
    STAGE_CHK(fn, ctx->lossb.reserve((size_t)(2 * steps)));
    ctx->laps = Laps<VAE_T_COUNT>();
    ctx->laps.lap(VAE_T_UPLOAD);
    DevBuf<long long> didx;
    DevBuf<float> deps;
    static_assert(sizeof(long long) == sizeof(int64_t), "idx is uploaded as it is");
    STAGE_CHK(fn, didx.upload((const long long *)idx, (size_t)nidx));
    if (eps) STAGE_CHK(fn, deps.upload(eps, (size_t)nidx * N.LD));
    ctx->laps.lap(VAE_T_UPLOAD);
    for (int64_t s = 0; s < steps; ++s) {
        const int64_t b0 = s * batch;
        const int nb = (int)std::min<int64_t>(batch, nidx - b0);
        batch_gradient(ctx, nb, didx.p + b0, eps ? deps.p + b0 * N.LD : nullptr, ctx->lossb.p + 2 * s);
        // Keras 2's Nadam: the schedule in float64 on the host
        const double t = (double)(ctx->step + 1);
        const double mc_t = 0.9 * (1.0 - 0.5 * std::pow(0.96, 0.004 * t)), mc_t1 = 0.9 * (1.0 - 0.5 * std::pow(0.96, 0.004 * (t + 1.0)));
        const double M = ctx->msched * mc_t, M1 = M * mc_t1;
        hipLaunchKernelGGL(nm_vae_nadam_kernel, dim3(blocks(np)), dim3(VAE_BLOCK), 0, 0, (long long)np, ctx->grad.p, ctx->m.p, ctx->v.p, ctx->theta.p, (float)lr,
                           (float)((1.0 - mc_t) / (1.0 - M)), (float)(mc_t1 / (1.0 - M1)), (float)(1.0 / (1.0 - std::pow(0.999, t))));
        ctx->msched = M;
        ctx->step += 1;
        ctx->laps.lap(VAE_T_OPTIMISER);
        STAGE_CHK(fn, hipGetLastError());
    }
    STAGE_CHK(fn, hipDeviceSynchronize());
    ctx->laps.book(g_vae_ms);
    std::vector<float> lb((size_t)(2 * steps));
    STAGE_CHK(fn, ctx->lossb.download(lb.data(), lb.size()));
    double rec = 0.0, kl = 0.0;
    for (int64_t s = 0; s < steps; ++s) {
        const double nb = (double)std::min<int64_t>(batch, nidx - s * batch);
        rec += nb * lb[(size_t)(2 * s)];
        kl += nb * lb[(size_t)(2 * s + 1)];
    }
    loss[0] = rec / (double)nidx;
    loss[1] = kl / (double)nidx;
    return NM_OK;
}
} // extern "C"
