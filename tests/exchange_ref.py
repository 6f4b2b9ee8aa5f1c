"""A plain restatement of the replica-exchange sweep (the reference's replica_exchange, remcmc:776-803) for the tests: its own
Philox4x32-10 on Python integers, the criterion in numpy.longdouble, nothing imported from the package under test.

Conventions (those of the device sweep and of the oracle's): all arrays are per LOCAL slot k = r * nt + t of the rows row0 .. row0 +
nrows - 1; etot[k], vol[k] belong to whatever state sits in slot k when the sweep starts; perm[k] is the buffer (state) in slot k, the
identity unless given.  Pairs are visited per row in the order v = nt-1 .. 0, w = 0 .. v-1 (i = slot v, j = slot w); pair q of local row
r draws Philox counter ((row0 + r) * ppr + q, 7, 0, step) under key (seed, 0xFFFFFFFF), or reads tape[r * ppr + q]."""
import functools
from collections import namedtuple

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57           # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85           # Weyl increments of the key
MASK = 0xFFFFFFFF
S_EXCH = 7                                # the exchange sweep's stream number (counter word 1)
ULP = 2.0 ** -53                          # float64 unit round-off

Sweep = namedtuple('Sweep', 'perm swaps dh u margin bound')


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011; Random123) on Python integers"""
    c0, c1, c2, c3 = (int(v) & MASK for v in ctr)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def u01(hi, lo):
    """53 bits of (hi, lo) as a uniform in [0, 1)"""
    return (((int(hi) << 32) | int(lo)) >> 11) * 2.0 ** -53


def uniform(row, ppr, q, seed, step):
    o = philox4x32_10((row * ppr + q, S_EXCH, 0, step), (seed, MASK))
    return u01(o[0], o[1])


def constants_lj(P, T, row0=0, nrows=None):
    """(et, pf) per local slot in lj units: float64 arithmetic on the float32 grid values (init_constant, remcmc:128-131)"""
    P, T = np.asarray(P, dtype=np.float32), np.asarray(T, dtype=np.float32)
    nrows = len(P) - row0 if nrows is None else nrows
    et = np.array([float(T[t]) for r in range(nrows) for t in range(len(T))])
    pf = np.array([float(P[row0 + r]) / float(T[t]) for r in range(nrows) for t in range(len(T))])
    return et, pf


def grids(npn, nt, pr=(1.0, 8.0), tr=(0.25, 2.5)):
    """the float32 P and T grids of the driver (remcmc:895-897)"""
    return np.linspace(pr[0], pr[1], npn, dtype=np.float32), np.linspace(tr[0], tr[1], nt, dtype=np.float32)


def synthetic(ns, seed, natoms=256):
    """thermo rows [ns][5] = temp, pe, ke, virial, vol of a 4^3 LJ crystal's size: pe uniform in [-1900, -1897] and ke in [100, 101], both
    scaled by natoms / 256, vol in [225, 226]"""
    rng = np.random.default_rng(seed)
    th = np.zeros((ns, 5))
    s = natoms / 256.0
    th[:, 0] = 1.0
    th[:, 1] = s * (-1900.0 + 3.0 * rng.random(ns))
    th[:, 2] = s * (100.0 + rng.random(ns))
    th[:, 4] = 225.0 + rng.random(ns)
    return th


def sweep(npn, nt, row0, nrows, seed, step, etot, vol, et, pf, tape=None, perm=None):
    """One sweep over local rows 0 .. nrows-1 (global rows row0 ..).  Returns Sweep(perm, swaps, dh, u, margin, bound); dh, u, margin and
    bound are per pair in local sweep order [r * ppr + q]:
      dh      the criterion in longdouble from the float64 inputs,
      u       the uniform the pair was decided on,
      margin  |u - min(1, exp(dh))|: how far the decision is from flipping,
      bound   8 ulp (|Ei| + |Ej|) (1/et_i + 1/et_j) + 8 ulp (|pf_i| + |pf_j|) (|Vi| + |Vj|): what a float64 evaluation of dh (two
              differences, two products, one sum, the reciprocals rounded) can be off by, with room to spare.
    The decision is u <= min(1, exp(dh)); a NaN criterion compares false, so it never swaps."""
    assert 0 <= row0 and row0 + nrows <= npn
    ld = np.longdouble
    ns = nrows * nt
    E = [ld(v) for v in np.asarray(etot, dtype=np.float64).reshape(ns)]
    V = [ld(v) for v in np.asarray(vol, dtype=np.float64).reshape(ns)]
    B = [ld(v) for v in np.asarray(et, dtype=np.float64).reshape(ns)]
    F = [ld(v) for v in np.asarray(pf, dtype=np.float64).reshape(ns)]
    perm = list(range(ns)) if perm is None else [int(b) for b in perm]
    assert len(perm) == ns
    ppr = nt * (nt - 1) // 2
    npairs = nrows * ppr
    if tape is not None:
        assert len(tape) == npairs
    dh_out, u_out = np.zeros(npairs, dtype=ld), np.zeros(npairs)
    margin, bound = np.zeros(npairs), np.zeros(npairs)
    swaps = 0
    one = ld(1)
    with np.errstate(all='ignore'):
        for r in range(nrows):
            q = 0
            for v in range(nt - 1, -1, -1):
                for w in range(v):
                    i, j = r * nt + v, r * nt + w
                    dh = (E[i] - E[j]) * (one / B[i] - one / B[j]) + (F[i] - F[j]) * (V[i] - V[j])
                    u = float(tape[r * ppr + q]) if tape is not None else uniform(row0 + r, ppr, q, seed, step)
                    e = np.exp(dh)
                    m = e if e != e else min(e, one)
                    t = r * ppr + q
                    dh_out[t], u_out[t] = dh, u
                    margin[t] = abs(ld(u) - m)
                    bound[t] = float(8 * ULP * ((abs(E[i]) + abs(E[j])) * (one / B[i] + one / B[j])
                                                + (abs(F[i]) + abs(F[j])) * (abs(V[i]) + abs(V[j]))))
                    if ld(u) <= m:
                        swaps += 1
                        E[i], E[j] = E[j], E[i]
                        V[i], V[j] = V[j], V[i]
                        perm[i], perm[j] = perm[j], perm[i]
                    q += 1
    return Sweep(np.array(perm, dtype=np.int64), swaps, dh_out, u_out, margin, bound)


def pair_slots(nt):
    """(v, w) of a row's pairs in sweep order"""
    return [(v, w) for v in range(nt - 1, -1, -1) for w in range(v)]


# ---- the cases both test files use -------------------------------------------------------------------------------------------------------

# np x nt: no pairs (nt = 1) under and over one wave of rows; one pair per row (nt = 2) likewise, 130 rows giving three rows to lanes 0
# and 1; odd shapes; 33, 64, 127, 128 temperatures, the row widths at which the fused launch changes its workgroups per replica and its
# scratch crosses the reduction area
SHAPES = [(1, 1), (130, 1), (1, 2), (65, 2), (130, 2), (3, 5), (5, 6), (2, 33), (1, 64), (2, 64), (1, 127), (1, 128)]
SEED = 256                                 # the engine's default Philox key word
NSWEEPS = 3
MARGIN_MIN = 1e-9                          # far above what `bound` (at most 6e-11 on these inputs) and a 1-ulp exp can move a criterion


def case_step(npn, nt):
    """first step number of a shape's three sweeps"""
    return 11 + 3 * npn + nt


def case_thermo(npn, nt, s, row0=0, nrows=None):
    """thermo rows of sweep s (0-based) of a shape, for local rows row0 .. (slices of one full-grid draw, so that a shard sees its rows of it)"""
    nrows = npn - row0 if nrows is None else nrows
    return synthetic(npn * nt, 100000 * npn + 100 * nt + s)[row0 * nt:(row0 + nrows) * nt]


def check_margins(res, what):
    """the precondition of every decision test: no pair of the REFERENCE sits within MARGIN_MIN of flipping"""
    fin = np.isfinite(res.margin)
    worst = res.margin[fin].min() if fin.any() else np.inf
    assert worst > MARGIN_MIN, '%s: a pair decides within %.3g of its uniform; choose another seed' % (what, worst)


@functools.lru_cache(maxsize=None)
def reference_sweeps(npn, nt, row0=0, nrows=None, seed=SEED):
    """the shape's NSWEEPS sweeps with perm carried over: [(step, thermo, Sweep)], margins checked.  Computed once per shape and shared: read only"""
    nrows = npn - row0 if nrows is None else nrows
    et, pf = constants_lj(*grids(npn, nt), row0, nrows)
    out, perm = [], None
    for s in range(NSWEEPS):
        th = case_thermo(npn, nt, s, row0, nrows)
        step = case_step(npn, nt) + s
        res = sweep(npn, nt, row0, nrows, seed, step, th[:, 1] + th[:, 2], th[:, 4], et, pf, perm=perm)
        check_margins(res, '%dx%d rows %d+%d sweep %d' % (npn, nt, row0, nrows, s))
        out.append((step, th, res))
        perm = res.perm
    return out


# The edge set: a grid of rows with T = (1, 2), one pair per row (i = the slot at T = 2, j = the one at T = 1), equal volumes, so that
# dh = (Ei - Ej) (1/2 - 1) exactly.  Each entry: name, (Ej, Ei), uniform of the tape, swap expected
EDGE_T = (1.0, 2.0)
EDGE_PAIRS = [
    ('dh = 0, u = 1 - 2^-53',       (-1800.0, -1800.0), 1.0 - 2.0 ** -53, True),    # exp gives exactly 1: u <= 1
    ('dh = -1000, u = 0',           (-1000.0, 1000.0),  0.0,              True),    # exp underflows to 0: 0 <= 0
    ('dh = -1000, u = 2^-53',       (-1000.0, 1000.0),  2.0 ** -53,       False),
    ('dh = +800, u = 1 - 2^-53',    (800.0, -800.0),    1.0 - 2.0 ** -53, True),    # exp overflows to inf: min(1, inf) = 1
    ('dh = +800, u = 0',            (800.0, -800.0),    0.0,              True),
    ('dh = +800, u = 0.5',          (800.0, -800.0),    0.5,              True),
]
EDGE_DH = [0.0, -1000.0, -1000.0, 800.0, 800.0, 800.0]


def edge_pair_thermo():
    """thermo rows of the EDGE_PAIRS grid (len(EDGE_PAIRS) x 2): pe carries the energy, ke = 0, vol = 225"""
    th = np.zeros((2 * len(EDGE_PAIRS), 5))
    for r, (_, (ej, ei), _, _) in enumerate(EDGE_PAIRS):
        th[2 * r, 1], th[2 * r + 1, 1] = ej, ei
    th[:, 4] = 225.0
    return th


def edge_row_thermo(kind, nt=5, seed=5):
    """one row of nt slots on energies alone: kind 'nan' puts pe = NaN into slot 2; 'inf' puts +inf, -inf, +inf into slots 0, 1, 3 (the pairs
    among them give dh = +-inf and, inf - inf, NaN); 'finite' is the row both are made from"""
    th = synthetic(nt, seed)
    if kind == 'nan':
        th[2, 1] = np.nan
    elif kind == 'inf':
        th[0, 1], th[1, 1], th[3, 1] = np.inf, -np.inf, np.inf
    else:
        assert kind == 'finite'
    return th
