"""The VAE stage restated in torch on the CPU (include/nm_vae.h), float64 unless asked otherwise: the layers from the two padding
expressions of TensorFlow's SAME rule, the network, its loss, its gradient (autograd) and Keras 2's Nadam.  Arrays are numpy,
channels last, kernels in Keras's layouts; on integer data within 2^53 every result is exact."""
import numpy as np
import torch
import torch.nn.functional as F

NONE, RELU, TANH = 0, 1, 2
NAMES = ('c0', 'c1', 'c2', 'c3', 'd0', 'dm', 'dv', 'd1', 't0', 't1', 't2', 't3', 't4')
B1, B2, EPSILON, DECAY = 0.9, 0.999, 1e-7, 0.004


def _act(v, act):
    return torch.relu(v) if act == RELU else torch.tanh(v) if act == TANH else v


def conv_t(x, w, stride, transposed):
    """the linear map of a layer on torch tensors: x (n, cin, z, y, x), w in Keras's layout"""
    if not transposed:                                          # w (kz, ky, kx, cin, cout) -> (cout, cin, kz, ky, kx)
        wt = w.permute(4, 3, 0, 1, 2)
        return F.conv3d(F.pad(x, (1, 1, 1, 1, 1, 1)), wt) if stride == 1 else F.conv3d(F.pad(x, (0, 1, 0, 1, 0, 1)), wt, stride=2)
    wt = w.permute(4, 3, 0, 1, 2)                               # w (kz, ky, kx, cout, cin) -> (cin, cout, kz, ky, kx)
    if stride == 1:
        return F.conv_transpose3d(x, wt, padding=1)
    s = 2 * x.shape[-1]
    return F.conv_transpose3d(x, wt, stride=2)[..., :s, :s, :s]


def _cl(t):                                                     # (n, c, z, y, x) -> channels last
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _cf(a, dtype=torch.float64):                                # channels last numpy -> (n, c, z, y, x)
    return torch.as_tensor(np.asarray(a), dtype=dtype).permute(0, 4, 1, 2, 3)


def conv(x, w, b, stride, transposed, act, dtype=torch.float64):
    """y (n, side_out, side_out, side_out, cout) of x (n, side, side, side, cin)"""
    y = conv_t(_cf(x, dtype), torch.as_tensor(w, dtype=dtype), stride, transposed) + torch.as_tensor(b, dtype=dtype).view(1, -1, 1, 1, 1)
    return _cl(_act(y, act)).numpy()


def conv_abs(x, w, b, stride, transposed):
    """the sum of the absolute terms of every output of the layer's pre-activation, the bias included"""
    return conv(np.abs(x), np.abs(w), np.abs(b), stride, transposed, NONE)


def dact(y, act):
    y = np.asarray(y, dtype=np.float64)
    return (y > 0).astype(np.float64) if act == RELU else 1.0 - y * y if act == TANH else np.ones_like(y)


def conv_grad(x, w, y, gy, stride, transposed, act):
    """(gx, gw, gb) from gy, the gradient with respect to the activated output y, the activation's derivative taken from y"""
    xt = _cf(x).requires_grad_(True)
    wt = torch.as_tensor(w, dtype=torch.float64).requires_grad_(True)
    gpre = _cf(np.asarray(gy, dtype=np.float64) * dact(y, act))
    out = conv_t(xt, wt, stride, transposed)
    gx, gw = torch.autograd.grad(out, (xt, wt), gpre)
    return _cl(gx).numpy(), gw.numpy(), gpre.sum(dim=(0, 2, 3, 4)).numpy()


def conv_grad_abs(x, w, y, gy, stride, transposed, act):
    """the sums of the absolute terms of gx, gw and gb"""
    g = np.abs(np.asarray(gy, dtype=np.float64) * dact(y, act))
    return conv_grad(np.abs(x), np.abs(w), np.ones_like(g), g, stride, transposed, NONE)


def dense(x, w, b, act):
    return _act(torch.as_tensor(x, dtype=torch.float64) @ torch.as_tensor(w, dtype=torch.float64) + torch.as_tensor(b, dtype=torch.float64), act).numpy()


def dense_grad(x, w, y, gy, act):
    x, w, g = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64), np.asarray(gy, dtype=np.float64) * dact(y, act)
    return g @ w.T, x.T @ g, g.sum(axis=0)


# ---- the network
def shapes(S, LD):
    """the 26 parameter tensors' shapes: of every layer the kernel, then the bias"""
    q = S // 4
    f = 64 * q ** 3
    k = {'c0': (3, 3, 3, 1, 32), 'c1': (3, 3, 3, 32, 64), 'c2': (3, 3, 3, 64, 32), 'c3': (3, 3, 3, 32, 64), 'd0': (f, 8 * LD), 'dm': (8 * LD, LD),
         'dv': (8 * LD, LD), 'd1': (LD, f), 't0': (3, 3, 3, 64, 64), 't1': (3, 3, 3, 32, 64), 't2': (3, 3, 3, 64, 32), 't3': (3, 3, 3, 32, 64),
         't4': (3, 3, 3, 1, 32)}
    nb = {'c0': 32, 'c1': 64, 'c2': 32, 'c3': 64, 'd0': 8 * LD, 'dm': LD, 'dv': LD, 'd1': f, 't0': 64, 't1': 32, 't2': 64, 't3': 32, 't4': 1}
    out = []
    for name in NAMES:
        out += [k[name], (nb[name],)]
    return out


def offsets(S, LD):
    return np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes(S, LD)])]).astype(np.int64)


def nparams(S, LD):
    return int(offsets(S, LD)[-1])


def split(theta, S, LD):
    off = offsets(S, LD)
    return [theta[off[i]:off[i + 1]].reshape(s) for i, s in enumerate(shapes(S, LD))]


def forward(theta, S, LD, x, eps):
    """theta a flat torch vector, x (n, S, S, S) and eps (n, LD) or None torch tensors of its dtype:
    (z_mean, z_log_var, recon (n, S^3), rec (n,), kl (n,))"""
    p = split(theta, S, LD)
    n, q = x.shape[0], S // 4
    a = x.reshape(n, 1, S, S, S)
    for l, stride in enumerate((1, 2, 1, 2)):
        a = torch.relu(conv_t(a, p[2 * l], stride, False) + p[2 * l + 1].view(1, -1, 1, 1, 1))
    e0 = torch.relu(_cl(a).reshape(n, -1) @ p[8] + p[9])
    mu, lv = e0 @ p[10] + p[11], e0 @ p[12] + p[13]
    z = mu if eps is None else mu + torch.exp(0.5 * lv) * eps
    a = torch.relu(z @ p[14] + p[15]).reshape(n, q, q, q, 64).permute(0, 4, 1, 2, 3)
    for l, (stride, act) in enumerate(((1, RELU), (2, RELU), (1, RELU), (2, RELU), (1, TANH))):
        a = _act(conv_t(a, p[16 + 2 * l], stride, True) + p[17 + 2 * l].view(1, -1, 1, 1, 1), act)
    y = a.reshape(n, -1)
    rec = ((x.reshape(n, -1) - y) ** 2).sum(dim=1)
    kl = 0.5 * (torch.exp(lv) + mu * mu - lv - 1.0).sum(dim=1)
    return mu, lv, y, rec, kl


def evaluate(theta, S, LD, x, eps, dtype=torch.float64):
    with torch.no_grad():
        out = forward(torch.as_tensor(theta, dtype=dtype), S, LD, torch.as_tensor(x, dtype=dtype), None if eps is None else torch.as_tensor(eps, dtype=dtype))
    return [o.numpy() for o in out]


def gradient(theta, S, LD, x, eps, dtype=torch.float64):
    """(the gradient of the batch's mean loss, (mean rec, mean kl))"""
    t = torch.as_tensor(theta, dtype=dtype).clone().requires_grad_(True)
    _, _, _, rec, kl = forward(t, S, LD, torch.as_tensor(x, dtype=dtype), None if eps is None else torch.as_tensor(eps, dtype=dtype))
    (g,) = torch.autograd.grad((rec + kl).mean(), t)
    return g.numpy(), (float(rec.detach().mean()), float(kl.detach().mean()))


class Nadam:
    """Keras 2's Nadam on a flat vector, in theta's dtype; the schedule's scalars in float64"""

    def __init__(self, theta):
        self.theta = np.array(theta)
        self.m, self.v, self.sched, self.t = np.zeros_like(self.theta), np.zeros_like(self.theta), 1.0, 0

    def step(self, g, lr):
        ty = self.theta.dtype.type
        self.t += 1
        t = self.t
        mc_t, mc_t1 = B1 * (1.0 - 0.5 * 0.96 ** (DECAY * t)), B1 * (1.0 - 0.5 * 0.96 ** (DECAY * (t + 1)))
        self.sched *= mc_t
        nxt = self.sched * mc_t1
        g = np.asarray(g, dtype=self.theta.dtype)
        self.m = ty(B1) * self.m + ty(1.0 - B1) * g
        self.v = ty(B2) * self.v + ty(1.0 - B2) * (g * g)
        num = ty((1.0 - mc_t) / (1.0 - self.sched)) * g + ty(mc_t1 / (1.0 - nxt)) * self.m
        self.theta = self.theta - ty(lr) * num / (np.sqrt(self.v * ty(1.0 / (1.0 - B2 ** t))) + ty(EPSILON))
        return self.theta


def epoch(opt, S, LD, x, idx, eps, batch, lr, dtype=torch.float64):
    """Nadam steps over the consecutive batches of idx; (mean rec, mean kl), sample-weighted"""
    tot = np.zeros(2)
    for b0 in range(0, len(idx), batch):
        sel = idx[b0:b0 + batch]
        g, loss = gradient(opt.theta, S, LD, x[sel], None if eps is None else eps[b0:b0 + batch], dtype)
        tot += len(sel) * np.array(loss)
        opt.step(g, lr)
    return tot / len(idx)
