"""What a training step of the VAE stage costs: one nm_vae_epoch over --nsamples random cubes of side --side at
batch --batch, split by nm_vae_last_timing's device events into the taking of the batch, forward, backward and the optimiser, the
rate against the 157 TFLOP/s peak of the float32 matrix instruction, and every convolution layer on its own through the layer
primitives.  Beside it, in the same process and on the same device, torch's own conv3d / conv_transpose3d training step of the
same network (NAdam, channels first, float32) and the same layers on their own: the yardstick.

    python scripts/probe_vae.py [--side 16] [--latent 8] [--nsamples 4096] [--batch 64] [--repeats 3] [--no-torch] [--no-layers]

One JSON line per measurement.  FLOPs are counted from the shapes: 2 * 27 * cin * cout per output position of a convolution
(of the SMALLER grid for a stride-2 layer: the taps that meet padding or no source are not counted at stride 1 either), 2 * din *
dout per dense sample; backward counts the data and the weight gradient, each as much as forward (conv0 has no data gradient).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmelting_amd import _lib as B  # noqa: E402
from neuralmelting_amd import vae  # noqa: E402

PEAK_TFLOPS = 157.0
NAMES = ('c0', 'c1', 'c2', 'c3', 't0', 't1', 't2', 't3', 't4')


def layers(S):
    """(name, side_in, cin, cout, stride, transposed, act) of the nine convolution layers"""
    h, q = S // 2, S // 4
    return (('c0', S, 1, 32, 1, 0, 1), ('c1', S, 32, 64, 2, 0, 1), ('c2', h, 64, 32, 1, 0, 1), ('c3', h, 32, 64, 2, 0, 1), ('t0', q, 64, 64, 1, 1, 1),
            ('t1', q, 64, 32, 2, 1, 1), ('t2', h, 32, 64, 1, 1, 1), ('t3', h, 64, 32, 2, 1, 1), ('t4', S, 32, 1, 1, 1, 2))


def conv_flops(side, cin, cout, stride, transposed):
    """of one sample, forward"""
    small = side if transposed or stride == 1 else side // stride
    return 2.0 * 27 * cin * cout * small ** 3


def step_flops(S, LD):
    """(forward, backward) of one sample"""
    f = 64 * (S // 4) ** 3
    fwd = bwd = 0.0
    for name, side, cin, cout, stride, tr, _ in layers(S):
        c = conv_flops(side, cin, cout, stride, tr)
        fwd += c
        bwd += c if name == 'c0' else 2 * c
    dense = 2.0 * (f * 8 * LD + 2 * 8 * LD * LD + LD * f)
    return fwd + dense, bwd + 2 * dense


def emit(**res):
    print(json.dumps({k: (float('%.5g' % v) if isinstance(v, float) else v) for k, v in res.items()}))
    sys.stdout.flush()


def _fp(a):
    return a.ctypes.data_as(B.c_float_p)


def probe_layers(S, batch, repeats, rng):
    L = B.load()
    ms = np.zeros(4)
    out = {}
    for name, side, cin, cout, stride, tr, act in layers(S):
        so = side * stride if tr else side // stride
        x = rng.standard_normal((batch, side, side, side, cin), dtype=np.float32)
        w = 0.1 * rng.standard_normal((27, cin, cout), dtype=np.float32)
        b, y = np.zeros(cout, dtype=np.float32), np.empty((batch, so, so, so, cout), dtype=np.float32)
        gy, gx, gw, gb = rng.standard_normal(y.shape, dtype=np.float32), np.empty_like(x), np.empty_like(w), np.empty(cout, dtype=np.float32)
        fwd, bwd = [], []
        for rep in range(repeats + 1):              # the first call is the warm-up and is not counted
            assert L.nm_vae_conv(0, batch, side, cin, cout, stride, tr, act, _fp(x), _fp(w), _fp(b), _fp(y)) == 0, L.nm_vae_last_error()
            L.nm_vae_last_timing(ms.ctypes.data_as(B.c_double_p))
            f = ms[1]
            assert L.nm_vae_conv_grad(0, batch, side, cin, cout, stride, tr, act, _fp(x), _fp(w), _fp(y), _fp(gy), None if name == 'c0' else _fp(gx),
                                      _fp(gw), _fp(gb)) == 0, L.nm_vae_last_error()
            L.nm_vae_last_timing(ms.ctypes.data_as(B.c_double_p))
            if rep:
                fwd.append(f)
                bwd.append(ms[2])
        c = conv_flops(side, cin, cout, stride, tr) * batch
        out[name] = (float(np.median(fwd)), float(np.median(bwd)))
        emit(what='layer', layer=name, batch=batch, forward_ms=out[name][0], backward_ms=out[name][1], forward_Tflops=c / out[name][0] / 1e9,
             backward_Tflops=(c if name == 'c0' else 2 * c) / out[name][1] / 1e9)
    return out


def torch_yardstick(S, LD, batch, steps, repeats, do_layers, ours):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    dev = torch.device('cuda:0')
    q = S // 4

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.c = nn.ModuleList([nn.Conv3d(1, 32, 3), nn.Conv3d(32, 64, 3, stride=2), nn.Conv3d(64, 32, 3), nn.Conv3d(32, 64, 3, stride=2)])
            self.d0, self.dm, self.dv, self.d1 = nn.Linear(64 * q ** 3, 8 * LD), nn.Linear(8 * LD, LD), nn.Linear(8 * LD, LD), nn.Linear(LD, 64 * q ** 3)
            self.t = nn.ModuleList([nn.ConvTranspose3d(64, 64, 3, padding=1), nn.ConvTranspose3d(64, 32, 3, stride=2),
                                    nn.ConvTranspose3d(32, 64, 3, padding=1), nn.ConvTranspose3d(64, 32, 3, stride=2), nn.ConvTranspose3d(32, 1, 3, padding=1)])

        def forward(self, x, eps):
            a = x
            for l, c in enumerate(self.c):
                a = torch.relu(c(F.pad(a, (0, 1, 0, 1, 0, 1) if l % 2 else (1, 1, 1, 1, 1, 1))))
            e0 = torch.relu(self.d0(a.flatten(1)))
            mu, lv = self.dm(e0), self.dv(e0)
            a = torch.relu(self.d1(mu + torch.exp(0.5 * lv) * eps)).reshape(-1, 64, q, q, q)
            for l, t in enumerate(self.t):
                a = t(a)
                if l in (1, 3):
                    s = 2 * (q if l == 1 else 2 * q)
                    a = a[..., :s, :s, :s]
                a = torch.tanh(a) if l == 4 else torch.relu(a)
            rec = ((x - a) ** 2).flatten(1).sum(1)
            kl = 0.5 * (torch.exp(lv) + mu * mu - lv - 1.0).sum(1)
            return (rec + kl).mean()

    net = Net().to(dev)
    opt = torch.optim.NAdam(net.parameters(), lr=1e-4)
    x = torch.rand(batch, 1, S, S, S, device=dev)
    eps = torch.randn(batch, LD, device=dev)

    def run(k):
        for _ in range(k):
            opt.zero_grad(set_to_none=True)
            net(x, eps).backward()
            opt.step()
    run(5)                                          # warm-up: the library picks its algorithms
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(steps)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / steps)
    fwd, bwd = step_flops(S, LD)
    emit(what='torch step', side=S, latent=LD, batch=batch, steps=steps, ms_per_step=float(np.median(times)), spread_ms=float(np.ptp(times)),
         Tflops=(fwd + bwd) * batch / float(np.median(times)) / 1e9, torch=torch.__version__)
    if not do_layers:
        return
    for name, side, cin, cout, stride, tr, act in layers(S):
        mod = (nn.ConvTranspose3d(cin, cout, 3, stride=stride, padding=1 if stride == 1 else 0) if tr else nn.Conv3d(cin, cout, 3, stride=stride)).to(dev)
        xin = torch.randn(batch, cin, side, side, side, device=dev, requires_grad=name != 'c0')

        def fwd_only():
            a = mod(xin) if tr else mod(F.pad(xin, (0, 1, 0, 1, 0, 1) if stride == 2 else (1, 1, 1, 1, 1, 1)))
            if tr and stride == 2:
                a = a[..., :2 * side, :2 * side, :2 * side]
            return torch.tanh(a) if act == 2 else torch.relu(a)
        y = fwd_only()
        gy = torch.randn_like(y)
        y.backward(gy)
        torch.cuda.synchronize()
        tf, tb = [], []
        for _ in range(repeats):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            y = fwd_only()
            e[1].record()
            y.backward(gy)
            e[2].record()
            torch.cuda.synchronize()
            tf.append(e[0].elapsed_time(e[1]))
            tb.append(e[1].elapsed_time(e[2]))
        emit(what='torch layer', layer=name, batch=batch, forward_ms=float(np.median(tf)), backward_ms=float(np.median(tb)),
             ours_forward_ms=ours.get(name, (None, None))[0], ours_backward_ms=ours.get(name, (None, None))[1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--side', type=int, default=16)
    p.add_argument('--latent', type=int, default=8)
    p.add_argument('--nsamples', type=int, default=4096)
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--no-torch', action='store_true')
    p.add_argument('--no-layers', action='store_true')
    a = p.parse_args()
    S, LD, n = a.side, a.latent, a.nsamples
    rng = np.random.default_rng(256)
    steps = -(-n // a.batch)
    fwd, bwd = step_flops(S, LD)
    if not a.no_torch:                              # torch finds the device only if it looks before the library has opened it
        import torch
        torch.cuda.init()
        torch.zeros(1, device='cuda:0')
    with vae.Model(S, LD) as m:
        m.set_params(vae.initial_params(S, LD, rng))
        m.data(rng.random((n, S ** 3), dtype=np.float32))
        idx, eps = np.arange(n, dtype=np.int64), rng.standard_normal((n, LD), dtype=np.float32)
        m.epoch(idx[:4 * a.batch], eps[:4 * a.batch], a.batch, 1e-4)             # warm-up: every kernel at the timed shapes
        rows = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            loss = m.epoch(idx, eps, a.batch, 1e-4)
            wall = (time.perf_counter() - t0) * 1e3
            rows.append(np.concatenate([m.timing(), [wall]]))
        rows = np.array(rows) / steps
        take, f, b, o, wall = np.median(rows, axis=0)
        emit(what='nm_vae_epoch', side=S, latent=LD, nsamples=n, batch=a.batch, steps=steps, repeats=a.repeats, nparams=m.nparams,
             ms_per_step=wall, take_ms=take, forward_ms=f, backward_ms=b, optimiser_ms=o, spread_ms=float(np.ptp(rows[:, 4])),
             gflop_per_sample_forward=fwd / 1e9, Tflops=(fwd + bwd) * a.batch / wall / 1e9, share_of_peak=(fwd + bwd) * a.batch / wall / 1e9 / PEAK_TFLOPS,
             forward_Tflops=fwd * a.batch / f / 1e9, backward_Tflops=bwd * a.batch / b / 1e9, loss=float(loss.sum()))
    ours = {} if a.no_layers else probe_layers(S, a.batch, a.repeats, rng)
    if not a.no_torch:
        torch_yardstick(S, LD, a.batch, min(steps, 16), a.repeats, not a.no_layers, ours)
    return 0


if __name__ == '__main__':
    sys.exit(main())
