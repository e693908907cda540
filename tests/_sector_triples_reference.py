"""Plain-numpy restatement of the momentum-blocked (T) (pymes_amd/solver/ueg_cc.py, sector_triples_energy): the
tables of pymes_amd/solver/sectors.py (TriplesTables), the implied-index layouts, the W slab and the energy of a triple,
vectorised over (a,b).  TEST INFRASTRUCTURE ONLY: checked against tests/_triples_reference.py on the CPU, and what the HIP
kernels are compared with on the GPU."""
import numpy as np

from pymes_amd.solver.sectors import SectorTables, TriplesTables
from tests import _triples_reference as R


def tables_for(k_int, no):
    tab = SectorTables(k_int, no)
    return tab, TriplesTables(tab)


def triples_integrals(tt, V):
    """(Vv [o,v,v], Vo [o,o,v]) gathered from a dense V_pqrs; exact zeros where the implied orbital does not exist."""
    out = []
    for family, shape in (("vv", (tt.no, tt.nv, tt.nv)), ("vo", (tt.no, tt.no, tt.nv))):
        pqrs, valid = tt.list_pqrs(family)
        x = np.zeros(len(valid))
        p = pqrs[valid]
        x[valid] = V[p[:, 0], p[:, 1], p[:, 2], p[:, 3]]
        out.append(x.reshape(shape))
    return out


def third_virtual(tt, i, j, k):
    """c[a,b]: the virtual (counted from the first one) with k_i + k_j + k_k - k_a - k_b, -1 where there is none."""
    kk, no = tt.tables.k_int, tt.no
    kv = kk[no:]
    orb = tt.lookup(kk[i] + kk[j] + kk[k] - kv[:, None, :] - kv[None, :, :])
    return np.where(orb >= no, orb - no, -1)


def _w(tt, Vv, Vo, Tc, x, y, z, p, q, r):
    """w(xyz;pqr) = Vv[x,p,q] Tc[z,y,r] - (m = m_of[x,y,p]) >= 0 ? Vo[x,y,p] Tc[m,z,q] : 0 at index vectors p, q, r."""
    m = tt.m_of[x, y, p]
    return Vv[x, p, q] * Tc[z, y, r] - np.where(m >= 0, Vo[x, y, p] * Tc[np.maximum(m, 0), z, q], 0.0)


def W_slab(tt, Vv, Vo, Tc, i, j, k):
    """(Wt [v,v], c [v,v]): W_ijk[a,b,c(a,b)], 0 where c is no virtual."""
    c = third_virtual(tt, i, j, k)
    ok = c >= 0
    a, b = np.nonzero(ok)
    cc = c[ok]
    w = _w(tt, Vv, Vo, Tc, i, j, k, a, b, cc)
    w = w + _w(tt, Vv, Vo, Tc, i, k, j, a, cc, b)
    w = w + _w(tt, Vv, Vo, Tc, j, i, k, b, a, cc)
    w = w + _w(tt, Vv, Vo, Tc, j, k, i, b, cc, a)
    w = w + _w(tt, Vv, Vo, Tc, k, i, j, cc, a, b)
    w = w + _w(tt, Vv, Vo, Tc, k, j, i, cc, b, a)
    Wt = np.zeros((tt.nv, tt.nv))
    Wt[ok] = w
    return Wt, c


def triple_terms(tt, eps, Wt, c, i, j, k):
    """(Wt[a,b] R[a,b] / D[a,b] / 3, the same with every one of the six products of R taken by its absolute value), one
    entry per (a,b) with a virtual c.  The second is the sum of |terms| that bounds the rounding error of S_ijk: the terms
    that are added are the six products, and R cancels (to zero when i = j = k, where W is symmetric in a, b, c)."""
    ok = c >= 0
    a, b = np.nonzero(ok)
    cc = c[ok]
    r = 4.0 * Wt[a, b] + Wt[b, cc] + Wt[cc, a] - 2.0 * Wt[cc, b] - 2.0 * Wt[a, cc] - 2.0 * Wt[b, a]
    A = np.abs(Wt)
    ra = 4.0 * A[a, b] + A[b, cc] + A[cc, a] + 2.0 * A[cc, b] + 2.0 * A[a, cc] + 2.0 * A[b, a]
    ev = np.asarray(eps)[tt.no:]
    d = eps[i] + eps[j] + eps[k] - ev[a] - ev[b] - ev[cc]
    return Wt[a, b] * r / d / 3.0, A[a, b] * ra / np.abs(d) / 3.0


def per_triple(tt, eps, Vv, Vo, Tc, begin=0, end=None):
    """(m_ijk S_ijk, m_ijk sum |terms|) of the triples [begin, end) in the library's order."""
    val, scale = [], []
    for (i, j, k) in R.triples(tt.no)[begin:end]:
        Wt, c = W_slab(tt, Vv, Vo, Tc, i, j, k)
        terms, bound = triple_terms(tt, eps, Wt, c, i, j, k)
        m = R.multiplicity(i, j, k)
        val.append(m * float(terms.sum()))
        scale.append(m * float(bound.sum()))
    return np.array(val), np.array(scale)


def ordered_sum(values):
    """The values added in order with the rounding error of every add carried along (Neumaier), as the library returns
    the sum of a range of triples."""
    total, carry = 0.0, 0.0
    for x in map(float, values):
        s = total + x
        carry += (total - s) + x if abs(total) >= abs(x) else (x - s) + total
        total = s
    return total + carry


def conserving_V(k_int, seed, scale=0.1):
    """Seeded random V_pqrs, non-zero only where k_p + k_q = k_r + k_s, with V_pqrs = V_qpsr = V_rspq (four_fold_V, masked):
    needs no electron-gas formula, so any list of vectors will do."""
    k = np.asarray(k_int)
    n = len(k)
    pair = k[:, None, :] + k[None, :, :]
    mask = np.all(pair[:, :, None, None, :] == pair[None, None, :, :, :], axis=-1)
    V = R.four_fold_V(n, seed, scale) * mask
    V = 0.5 * (V + V.transpose(1, 0, 3, 2))               # the two symmetries to the bit (a sum of two terms commutes)
    return 0.5 * (V + V.transpose(2, 3, 0, 1))
