"""Exact all-pairs reference of the engine's two potentials, and seeded edge states to test the force kernels with.

The reference shares no machinery with the kernels or with the oracle: no neighbour list, no cutoff bookkeeping beyond the strict
r^2 < rc^2 test, minimum image by d - L rint(d / L) on the float64 positions, every pair term and every sum in np.longdouble.
Test infrastructure (plain helper module, imported by tests/test_exact_ref.py and tests/test_eval_edges_gpu.py)."""
import numpy as np

from neuralmelting_amd import lattice

LJ_RC = lattice.RC                                                # lj/cut 2.5, unshifted (remcmc:365)
SC_EPS, SC_A, SC_C, SC_RC = lattice.SC_EPS, lattice.SC_A, lattice.SC_C, lattice.SC_RC
RC = {'LJ': LJ_RC, 'Al': SC_RC}
DMIN = {'LJ': 0.8, 'Al': 0.8 * 4.046 / np.sqrt(2.0)}             # minimum separation of a random fluid: 0.8 sigma, 0.8 nearest fcc distance

_LD = np.longdouble


def skin(el, n):
    """the Verlet skin nm_create picks (nm_api.hip): the list radius is rc + skin"""
    if el == 'Al':
        return 0.6
    return 0.4 if n <= 512 else 0.55 if n <= 1024 else 0.6


def _pairs(x, L, rc, chunk=256):
    """every ordered pair (i, j != i) with r^2 < rc^2: i, j, d = x_i - x_j (minimum image), r^2, all in long double"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    n = len(x)
    xl, Ll, rc2 = x.astype(_LD), _LD(L), _LD(rc) * _LD(rc)
    out = []
    for a in range(0, n, chunk):
        d = xl[a:a + chunk, None, :] - xl[None, :, :]
        d -= Ll * np.rint(d / Ll)
        r2 = (d * d).sum(-1)
        ii, jj = np.nonzero(r2 < rc2)
        keep = (ii + a) != jj
        ii, jj = ii[keep], jj[keep]
        out.append((ii + a, jj, d[ii, jj], r2[ii, jj]))
    i = np.concatenate([o[0] for o in out]); j = np.concatenate([o[1] for o in out])
    d = np.concatenate([o[2] for o in out]); r2 = np.concatenate([o[3] for o in out])
    return n, i, j, d, r2


def _forces(n, i, d, fp):
    """f_i = sum_j fp_ij d_ij, and the per-atom sum of |fp_ij d_ij| (the scale of the rounding a kernel's sum can make)"""
    t = fp[:, None] * d
    f = np.zeros((n, 3), dtype=_LD)
    a = np.zeros((n, 3), dtype=_LD)
    np.add.at(f, i, t)
    np.add.at(a, i, np.abs(t))
    return f, a


def exact(el, x, L):
    """U, W = sum r.f, f[N][3], the number of (unordered) pairs inside rc, and abs[N][3] = sum_j |f_ij| per component.
    U, W are long double, f and abs float64 of long-double sums."""
    if el == 'LJ':
        n, i, j, d, r2 = _pairs(x, L, LJ_RC)
        r2i = 1 / r2
        r6i = r2i * r2i * r2i
        fp = r6i * (48 * r6i - 24) * r2i
        U = (r6i * (4 * r6i - 4)).sum() / 2
        W = (r2 * fp).sum() / 2
    else:
        n, i, j, d, r2 = _pairs(x, L, SC_RC)
        q2 = _LD(SC_A) * _LD(SC_A) / r2
        rm = q2 * q2 * q2                                          # (a/r)^6
        rn = rm * np.sqrt(q2)                                      # (a/r)^7
        rho = np.zeros(n, dtype=_LD)
        np.add.at(rho, i, rm)
        sq = np.sqrt(rho)
        isr = np.where(rho > 0, 1 / np.where(rho > 0, sq, 1), 0)   # only atoms with a pair inside rc are ever read
        dF = _LD(0.5) * _LD(SC_C) * (isr[i] + isr[j])
        fp = _LD(SC_EPS) * (7 * rn - 6 * dF * rm) / r2
        U = _LD(SC_EPS) * rn.sum() / 2 - _LD(SC_EPS) * _LD(SC_C) * sq.sum()
        W = (r2 * fp).sum() / 2
    f, a = _forces(n, i, d, fp)
    assert len(i) % 2 == 0
    return U, W, f.astype(np.float64), len(i) // 2, a.astype(np.float64)


U64 = 2.0 ** -53  # unit roundoff of float64
FIX_Q = 2.0 ** -37  # half a quantum of the half-list kernels' fixed-point force sums (2^-36 force units)


def force_bound(el, x, L, half=False):
    """per atom and component, a bound on |f_kernel - f_exact| derived from the kernels' arithmetic (nm_kernels.h pair_pre /
    pair_vec_half / pair_loop_sc):
      d    = fma(fract(fma(-x_j, 1/L, x_i / L + 1/2)), L, -L/2): at most 3 roundings of a quantity <= 2 in units of L, |dd| <= 3 u L;
      r^2  = sum d^2: |dr^2| <= 2 sum_c |d_c| 3 u L + 3 u r^2 <= (6 sqrt(3) L / r + 3) u r^2;
      fp   ~ r^-14 (LJ; EAM: r^-8, r^-9): |dfp| <= g (7 |dr^2| / r^2 + 10 u), g = the sum of the magnitudes of fp's terms (no credit
             for their cancellation; EAM: the densities' m-term sums add m u to dF);
      f_i  = sum over m_i terms, in order: (m_i - 1) u sum |t|.
    Per pair |dt_c| <= g (3 u L + |d_c| (7 (6 sqrt(3) L / r + 3) + 10 + m_i) u); half lists add 2^-37 per addend (one per pair of the row
    and per partner, and the row total)."""
    if el == 'LJ':
        n, i, j, d, r2 = _pairs(x, L, LJ_RC)
        r2i = 1 / r2
        r6i = r2i * r2i * r2i
        g = r6i * (48 * r6i + 24) * r2i
        m = np.bincount(i, minlength=n).astype(np.float64)
        extra = np.zeros(len(i))
    else:
        n, i, j, d, r2 = _pairs(x, L, SC_RC)
        q2 = _LD(SC_A) * _LD(SC_A) / r2
        rm = q2 * q2 * q2
        rn = rm * np.sqrt(q2)
        rho = np.zeros(n, dtype=_LD)
        np.add.at(rho, i, rm)
        isr = np.where(rho > 0, 1 / np.sqrt(np.where(rho > 0, rho, 1)), 0)
        dF = _LD(0.5) * _LD(SC_C) * (isr[i] + isr[j])
        g = _LD(SC_EPS) * (7 * rn + 6 * dF * rm) / r2
        m = np.bincount(i, minlength=n).astype(np.float64)
        extra = (m[i] + m[j]).astype(np.float64)                 # the densities' sums inside dF
    r = np.sqrt(r2.astype(np.float64))
    g = g.astype(np.float64)
    ad = np.abs(d.astype(np.float64))
    rel = 7 * (6 * np.sqrt(3.0) * L / r + 3) + 10 + m[i] + extra
    per = g[:, None] * (3 * L + ad * rel[:, None]) * U64
    b = np.zeros((n, 3))
    np.add.at(b, i, per)
    if half:
        b += (m[:, None] + 1) * FIX_Q
    return b


# ---------------------------------------------------------------------------------------------------------- edge states
def _mind(x, p, L):
    d = x - p
    d -= L * np.rint(d / L)
    return np.sqrt((d * d).sum(-1)) if len(x) else np.array([np.inf])


def fluid(n, L, rng, dmin, fixed=None, clear=()):
    """random placement with minimum-image separation >= dmin (a dilute gas up to ~1.0 sigma^-3): the atoms of `fixed` first (kept as
    given), then sites of a cubic grid of spacing a >= dmin taken at random, each moved by up to (a - dmin) / 2 per axis, none closer
    than dmin to a fixed atom; clear: [(point, radius)] that no random atom may come closer to"""
    fixed = np.zeros((0, 3)) if fixed is None else np.asarray(fixed, dtype=np.float64).reshape(-1, 3)
    m = int(np.floor(L / dmin))
    while m ** 3 > 4 * n + 64 and m > 1:      # (no finer than needed: the random moves stay large)
        m -= 1
    a = L / m
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing='ij'), -1).reshape(-1, 3)
    x = (g + 0.5) * a + rng.uniform(-0.5, 0.5, (len(g), 3)) * (a - dmin)
    keep = np.ones(len(x), dtype=bool)
    for p, r in [(f, dmin) for f in fixed] + list(clear):
        keep &= _mind(x, np.asarray(p), L) >= r
    x = x[keep]
    need = n - len(fixed)
    if need > len(x) or a < dmin:
        raise RuntimeError('fluid: cannot place %d atoms in a box of %g' % (n, L))
    return np.concatenate([fixed, x[rng.permutation(len(x))[:need]]])[:n]


def box_for(el, n, rho):
    """the box edge of n atoms at number density rho, never below the minimum-image limit 2 rc"""
    return max((n / rho) ** (1.0 / 3.0), 2.0 * RC[el] + 1e-3)


def edge_states(el, n, L, seed=0):
    """seeded states of n atoms, [(name, x[n][3], L)], of the kinds the kernels can get wrong:
    (a) random fluid; (b) planted pairs at the cutoff, at the list radius, through every periodic image, at L / 2, on the faces and
    unwrapped; (c) LJ close contacts; (e) Al: an atom whose only listed neighbour lies between rc and rc + skin.
    (d), the box edges, is box_edge_states.  A kind that does not fit n atoms is left out."""
    rng = np.random.default_rng(seed * 7919 + n)
    rc, sk, dmin = RC[el], skin(el, n), DMIN[el]
    Lg = box_for(el, n, 0.02 if el == 'LJ' else 0.002)
    out = [('fluid', fluid(n, L, rng, dmin), L), ('gas', fluid(n, Lg, rng, dmin), Lg)]
    if n < 2:
        return out
    # (b) pairs at rc (1 -+ 10^-k), k = 6..12, and at rc + skin - 10^-k, each along one axis across a face of the box (a periodic
    # image): x, y, z in turn, so that the images of all three axes are crossed
    plant = [rc * (1 + sg * 10.0 ** -k) for k in range(6, 13) for sg in (-1, 1)] + [rc + sk - 10.0 ** -k for k in (6, 9, 12)]
    fixed = []
    for q in range(min(len(plant), n // 2)):
        ax = q % 3
        for _ in range(100):                                                   # (a place clear of the pairs planted so far)
            p0 = rng.uniform(0.0, L, 3)
            p0[ax] = 0.3 * rng.uniform(0.2, 1.0)
            p1 = p0.copy()
            p1[ax] -= plant[q]                                                 # below 0: the pair crosses the face x_ax = 0
            if not fixed or min(_mind(np.array(fixed), p0, L).min(), _mind(np.array(fixed), p1, L).min()) >= dmin:
                fixed += [p0, p1]
                break
    try:
        out.append(('planted_cutoff', fluid(n, L, rng, dmin, fixed=fixed), L))
    except RuntimeError:
        pass
    # a pair at exactly L / 2 along one axis (outside rc for every L >= 2 rc), and the corner image: L / 2 along all three
    p0 = rng.uniform(0.0, L, 3)
    p1 = p0.copy(); p1[0] += 0.5 * L
    fx = [p0, p1]
    if n >= 4:
        p2 = rng.uniform(0.0, L, 3)
        fx += [p2, p2 + 0.5 * L]
    try:
        out.append(('half_box', fluid(n, L, rng, dmin, fixed=fx), L))
    except RuntimeError:
        pass
    # atoms on the faces x = 0 and x = L (the same plane), a pair across it, then every coordinate unwrapped into [-0.7 L, 1.7 L)
    y, z = rng.uniform(0.0, L, 2)
    fx = [[0.0, y, z], [L, (y + 1.375 * dmin) % L, z]][:n]
    try:
        x = fluid(n, L, rng, dmin, fixed=fx)
        out.append(('faces', x, L))
        xu = x + rng.integers(-1, 2, (n, 3)) * L
        xu = np.where(xu < -0.7 * L, xu + L, np.where(xu >= 1.7 * L, xu - L, xu))
        out.append(('unwrapped', xu, L))
    except RuntimeError:
        pass
    if el == 'LJ':
        # (c) one close contact inside an otherwise ordinary fluid
        for r in (0.8, 0.7, 0.65, 0.62, 0.6, 0.55):
            p0 = rng.uniform(0.0, L, 3)
            u = rng.normal(size=3); u /= np.linalg.norm(u)
            try:
                out.append(('contact_%g' % r, fluid(n, L, rng, dmin, fixed=[p0, p0 + r * u]), L))
            except RuntimeError:
                pass
    else:
        # (e) an atom whose only listed neighbour lies in (rc, rc + skin]: its density is zero, the pair is listed
        # (in a box that holds the pair's image beyond rc + skin, and room for the others outside the empty sphere)
        Ls = max(L, 2 * (rc + sk) + 1.0, ((n + 100) / 0.03) ** (1.0 / 3.0) if n > 2 else 0.0)
        p0 = rng.uniform(0.0, Ls, 3)
        p1 = p0.copy(); p1[0] += rc + 0.5 * sk
        if n == 2:
            out.append(('al_shell_pair', np.array([p0, p1]), Ls))
        else:
            try:
                out.append(('al_isolated', fluid(n, Ls, rng, dmin, fixed=[p0, p1], clear=[(p0, rc + sk + 0.1)]), Ls))
            except RuntimeError:
                pass
    return out


def box_edge_states(el, n, seed=0):
    """(d) boxes from the minimum-image limit 2 rc to just above 2 (rc + skin), n atoms of a random fluid in each:
    [(name, x, L)]; only n small enough that every atom's list fits (n <= 128)"""
    rc, sk = RC[el], skin(el, n)
    rng = np.random.default_rng(seed * 104729 + n)
    out = []
    for name, L in (('L=2rc', 2 * rc), ('L=2rc+1e-9', 2 * rc + 1e-9), ('L=2rc+skin', 2 * rc + sk), ('L=2(rc+skin)+1e-6', 2 * (rc + sk) + 1e-6)):
        if n / L ** 3 > (1.0 if el == 'LJ' else 0.05):
            continue
        out.append((name, fluid(n, L, rng, DMIN[el]), L))
    return out
