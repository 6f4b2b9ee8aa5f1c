"""dev probe (experiment build `make expda`): the exchange that completes an energy evaluation and the draws of the move behind it, slot 0's
workgroups x 8 waves on the 100 MHz clock.  NM_DRAW_AHEAD=0: the draws are made behind the exchange, so the exchange span is the bare
hop and the draw span is what stands on the serial path; as built: the draws lie inside the exchange span.

    span (a): entry of the exchange, in front of its first put_granule -> return of its get_granules (slots 3 -> 4), per wave
    span (b): entry of draw_ahead -> end of its loop over the atoms (slots 5 -> 6), per wave
both by the phase the evaluation belongs to (a) and by the kind of move that was drawn (b: told apart by what the next evaluation belongs to)."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ['NM_HIP_LIB'] = os.environ.get('NM_EXP_LIB', os.path.join(ROOT, 'build', 'variants', 'libnm_hip_expda.so'))
import numpy as np
import neuralmelting_amd as nm
from neuralmelting_amd import lattice, _lib

ROWS = int(os.environ.get('NM_TL_ROWS', '8'))   # 8 rows x 8 = 64 replicas (Q = 4)
EQ = int(os.environ.get('NM_TL_EQUIL', '30'))   # cycles of 128 moves with the bench's mix and the exchange in front of the block that is read
P = np.linspace(1, 8, 8, dtype=np.float32); T = np.linspace(.25, 2.5, 8, dtype=np.float32)
if os.environ.get('NM_TL_TREV'):   # slot 0 is then the hottest replica of the first pressure row
    T = T[::-1].copy()
x, v, box, d = lattice.init_states(4, P, T, 0.03125, 0.03125, row0=0, nrows=ROWS)
e = nm.Engine(256, P, T, row0=0, nrows=ROWS)
e.set_state(x, v, box, d)
for s in range(EQ):
    e.set_step(s); e.run_block(128); e.adapt(); e.exchange(count=False)
e.synchronize()
L = _lib.load()
L.nm_tline_get.argtypes = [C.c_void_p, C.c_void_p]
buf = np.zeros((8, 8, 512, 8), dtype=np.uint64)   # [q][wave][eval][point]
L.nm_tline_get(e.h, buf.ctypes.data)
Q = e.cus_per_replica
st = e.stats()
print('Q %d, NM_DRAW_AHEAD=%s, moves drawn ahead (slot 0) %d of %d' % (Q, os.environ.get('NM_DRAW_AHEAD', '1'), st[0, 11], 128 * EQ))
e.close()
t = buf[:Q].astype(np.int64)
t0 = t[0, 0, :, 0]
n = 1 + int(np.argmax(np.append(np.diff(t0) <= 0, True)))   # the rows of the LAST block: entries in rising order (later rows are older blocks')
PH = {1: 'block start', 2: 'position move', 3: 'volume move', 4: 'trajectory start (run 0)', 5: 'trajectory end'}
# an energy evaluation's row: its exchange stamps are younger than its entry (a force-only evaluation's row keeps whatever an older block left)
fresh = np.array([(t[:, :, k, 4] > t[:, :, k, 3]).all() and (t[:, :, k, 3] > t[:, :, k, 0]).all() and int(t[0, 0, k, 7]) in PH for k in range(n)])
kind = np.where(fresh, t[0, 0, :n, 7], 0)
ks = [k for k in range(2, n - 1) if fresh[k]]


def next_kind(k):
    """the phase of the next energy evaluation behind row k: what the move drawn with row k turned out to be"""
    for j in range(k + 1, n):
        if fresh[j]:
            return int(kind[j])
    return 0
print('energy evaluations of the last block with an exchange on record: %d of %d evaluations' % (len(ks), n))


def stats(a):
    a = np.asarray(a, dtype=float) * 10.0   # ns
    return 'n %5d  median %6.0f  mean %6.0f  p10 %6.0f  p90 %6.0f' % (a.size, np.median(a), a.mean(), np.percentile(a, 10), np.percentile(a, 90))


print('span (a), ns per wave: exchange entry -> granules read')
for ph, name in PH.items():
    sel = [k for k in ks if kind[k] == ph]
    if sel:
        print('  %-26s %s' % (name, stats((t[:, :, sel, 4] - t[:, :, sel, 3]).ravel())))
print('span (a), ns per cluster: first entry -> last wave has its granules')
for ph, name in PH.items():
    sel = [k for k in ks if kind[k] == ph]
    if sel:
        print('  %-26s %s' % (name, stats([t[:, :, k, 4].max() - t[:, :, k, 3].min() for k in sel])))
# the draws that evaluation k's row holds were made for the move behind it; which kind that was shows in the next evaluation's phase
print('span (b), ns per wave: draw_ahead entry -> end of its loop, by the move drawn')
DR = {2: 'position move (3N uniforms)', 3: 'volume move (1 uniform)', 4: 'trajectory (2N gaussians)', 5: 'trajectory (2N gaussians)'}
for name in sorted(set(DR.values())):
    sel = [k for k in ks if DR.get(next_kind(k)) == name and kind[k] != 4 and (t[:, :, k, 6] > t[:, :, k, 5]).all() and (t[:, :, k, 5] >= t[:, :, k, 3]).all()]
    if sel:
        print('  %-28s %s' % (name, stats((t[:, :, sel, 6] - t[:, :, sel, 5]).ravel())))
        print('  %-28s %s' % ('  ... slowest wave', stats([(t[:, :, k, 6] - t[:, :, k, 5]).max() for k in sel])))
