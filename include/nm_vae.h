/*
 * nm_vae.h — C-ABI of the VAE stage: the 3-D convolutional variational autoencoder of the reference's
 * lammps_vae.py (build_variational_autoencoder), its loss, its gradient and Keras 2's Nadam, in float32 on the device.
 *
 * Tensors.  float32, channels last: a batch of n cubes of side S with c channels is [n][z][y][x][c], in host memory for the layer
 *   primitives.  Activations (act): NM_VAE_ACT_NONE 0, NM_VAE_ACT_RELU 1, NM_VAE_ACT_TANH 2.
 * Layers.  All kernels are 3 x 3 x 3, taps k = (kz, ky, kx); padding is TensorFlow's SAME, p = 1 at stride 1 and 0 at stride 2:
 *   convolution            y[n][o][co] = act(b[co] + sum_{k, ci} x[n][stride o + k - p][ci] w[k][ci][co]),  x taken as 0 outside 0..S-1;
 *                          the output side is S / stride (S a multiple of the stride), w is [kz][ky][kx][cin][cout] (Keras).
 *   transposed convolution y[n][i][co] = act(b[co] + sum_{stride o + k - p = i, ci} x[n][o][ci] w[k][co][ci]) for i in 0..stride S - 1
 *                          (the adjoint of the convolution's linear map; at stride 2 the full result with its last plane dropped),
 *                          w is [kz][ky][kx][cout][cin] (Keras).
 *   dense                  y[n][j] = act(b[j] + sum_i x[n][i] w[i][j]),  w is [din][dout].
 *   The gradients take gy, the gradient with respect to the ACTIVATED output, and y; the activation's derivative is taken from y
 *   (relu: y > 0; tanh: 1 - y^2).  gx, gw, gb are the gradients with respect to x, w and b, in their layouts.
 * Network, for a cube side S (a multiple of 4 in 4..32) and a latent size LD in 1..64, h = S / 2, q = S / 4, F = 64 q^3:
 *   encoder  c0 conv 1->32 s1 relu | c1 conv 32->64 s2 relu | c2 conv 64->32 s1 relu | c3 conv 32->64 s2 relu | flatten (z, y, x, c)
 *            | d0 dense F->8 LD relu | dm dense 8 LD->LD (z_mean) | dv dense 8 LD->LD (z_log_var)
 *   latent   z = z_mean + exp(z_log_var / 2) eps
 *   decoder  d1 dense LD->F relu | reshape (q, q, q, 64) | t0 convT 64->64 s1 relu | t1 convT 64->32 s2 relu | t2 convT 32->64 s1 relu
 *            | t3 convT 64->32 s2 relu | t4 convT 32->1 s1 tanh
 *   Another side cannot be rebuilt by the reference's own decoder (-cb 11 gives 11 -> 6 -> 3 -> 6 -> 12): NM_ERR_ARG.
 * Parameters.  One flat float32 vector, the layers in the order c0 c1 c2 c3 d0 dm dv d1 t0 t1 t2 t3 t4, of each the kernel, then the
 *   bias.  nm_vae_layout writes the 27 offsets: off[2 l] the kernel of layer l, off[2 l + 1] its bias, off[26] = nm_vae_nparams:
 *   kernels 27*1*32, 27*32*64, 27*64*32, 27*32*64, F*8LD, 8LD*LD, 8LD*LD, LD*F, 27*64*64, 27*32*64, 27*64*32, 27*32*64, 27*1*32
 *   elements, biases 32, 64, 32, 64, 8LD, LD, LD, F, 64, 32, 64, 32, 1.
 * Loss of a sample: rec + kl, rec = sum_voxels (x - y)^2, kl = sum_d (exp(lv_d) + mu_d^2 - lv_d - 1) / 2; of a batch: the mean.
 * Optimiser.  Keras 2's Nadam, beta1 0.9, beta2 0.999, epsilon 1e-7, schedule decay 0.004; at step t = 1, 2, .. (M starts at 1):
 *   mc_t = beta1 (1 - 0.5 0.96^(0.004 t)), mc_t1 the same of t + 1, M <- M mc_t, M' = M mc_t1, g' = g / (1 - M),
 *   m <- beta1 m + (1 - beta1) g, m' = m / (1 - M'), v <- beta2 v + (1 - beta2) g^2, v' = v / (1 - beta2^t),
 *   theta <- theta - lr ((1 - mc_t) g' + mc_t1 m') / (sqrt(v') + epsilon).  The schedule's scalars are the host's, in float64.
 * Arithmetic.  float32 storage and arithmetic; the 32 <-> 64 channel layers and their gradients run on v_mfma_f32_32x32x2_f32, whose
 *   result is a chain of float32 fused multiply-adds.  No random number is drawn here: the caller gives the order and the noise.
 *   Every sum runs in a fixed order that depends on the shapes alone, there are no floating-point atomics: the same call twice gives
 *   the same bits.  A layer's result lies within gamma_(K+1) sum |terms| of the exact one (u = 2^-24, K the number of terms of the
 *   sum, the bias included), whatever the order.  tanh is evaluated in float64 and rounded once, so the tanh layer's output is
 *   within 2 ulp (2^-22 |y|) of the tanh of the float32 pre-activation; tanh's slope is at most 1, so the pre-activation's error
 *   adds at most itself.
 *
 * Every function returns 0 or a negative NM_ERR_* code (include/nm.h), nm_vae_nparams the count or such a code; message via
 * nm_vae_last_error(), the calling thread's own, starting with the function's name.  NM_ERR_ARG, checked before a device is looked
 * for and with every output left untouched, for: a side, latent size, channel count (1..64), stride (1, 2), act, transposed flag
 * (0, 1) or count out of range, a side that the stride does not divide, a tensor of more than 2^30 elements, a needed pointer
 * that is null, an index outside the resident samples, a learning rate that is not finite and positive, a negative device.
 * NM_ERR_STATE for a model call before the parameters or the data were set.  NM_ERR_HIP without a device or when a HIP call fails
 * (what does not fit the device fails so).
 */
#ifndef NM_VAE_H
#define NM_VAE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define NM_VAE_ACT_NONE 0
#define NM_VAE_ACT_RELU 1
#define NM_VAE_ACT_TANH 2
#define NM_VAE_NTENSORS 26

typedef struct nm_vae_ctx nm_vae_ctx;

/* The number of parameters, or NM_ERR_ARG. */
int64_t nm_vae_nparams(int side, int latent);
/* off [NM_VAE_NTENSORS + 1]. */
int nm_vae_layout(int side, int latent, int64_t *off);

/* ---- the layer primitives: stateless, host arrays.  side_in is x's side; sides 1..64, channels 1..64. */
/* x [n][side_in^3][cin]; y [n][side_out^3][cout], side_out = side_in / stride, transposed: side_in * stride. */
int nm_vae_conv(int device, int n, int side_in, int cin, int cout, int stride, int transposed, int act, const float *x, const float *w,
                const float *b, float *y);
/* gy like y; gx like x, or NULL; gw like w; gb [cout]. */
int nm_vae_conv_grad(int device, int n, int side_in, int cin, int cout, int stride, int transposed, int act, const float *x, const float *w,
                     const float *y, const float *gy, float *gx, float *gw, float *gb);
/* x [n][din]; w [din][dout]; b [dout]; y [n][dout]; din, dout >= 1, din * dout <= 2^28. */
int nm_vae_dense(int device, int n, int din, int dout, int act, const float *x, const float *w, const float *b, float *y);
int nm_vae_dense_grad(int device, int n, int din, int dout, int act, const float *x, const float *w, const float *y, const float *gy, float *gx,
                      float *gw, float *gb);

/* ---- the model: an opaque context that owns its device memory. */
int nm_vae_create(int device, int side, int latent, nm_vae_ctx **ctx);
int nm_vae_destroy(nm_vae_ctx *ctx);
/* theta [nm_vae_nparams]; set also resets the optimiser (m = v = 0, M = 1, t = 0); a value that is not finite is refused. */
int nm_vae_set_params(nm_vae_ctx *ctx, const float *theta);
int nm_vae_get_params(nm_vae_ctx *ctx, float *theta);
/* x [n][side^3]: the samples, resident from here on (they replace the ones before).  A value that is not finite is NM_ERR_ARG, the
 * message names the first such sample, and the context then holds no data. */
int nm_vae_data(nm_vae_ctx *ctx, int64_t n, const float *x);
/* Forward for the resident samples idx[0 .. nidx - 1]: eps [nidx][latent] or NULL (z = z_mean); z_mean, z_log_var [nidx][latent];
 * recon [nidx][side^3] or NULL; rec, kl [nidx]. */
int nm_vae_eval(nm_vae_ctx *ctx, int64_t nidx, const int64_t *idx, const float *eps, float *z_mean, float *z_log_var, float *recon, float *rec,
                float *kl);
/* The gradient of the mean loss of the batch idx[0 .. nidx - 1] (nidx <= 4096) with respect to every parameter, no update:
 * grad [nm_vae_nparams]; loss [2] the mean rec and the mean kl. */
int nm_vae_grad(nm_vae_ctx *ctx, int64_t nidx, const int64_t *idx, const float *eps, float *grad, double *loss);
/* Nadam steps over the consecutive batches of `batch` (1..4096) indices of idx, the last one ragged: eps [nidx][latent] or NULL;
 * loss [2] the sample-weighted means of the batches' mean rec and kl, each batch's taken before its step. */
int nm_vae_epoch(nm_vae_ctx *ctx, int64_t nidx, const int64_t *idx, const float *eps, int batch, double lr, double *loss);

/* Where the device time of the calling thread's last successful model call or layer primitive went, in milliseconds between device
 * events: ms[0] uploads and the taking of the batch, ms[1] forward (loss included), ms[2] backward, ms[3] the optimiser. */
int nm_vae_last_timing(double *ms);

const char *nm_vae_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
