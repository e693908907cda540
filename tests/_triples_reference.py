"""numpy references of the closed-shell (T) correction (pymes_amd/solver/ccsd_t.py, include/pymes_amd.h, pymes_ccsd_t).

Notation of the code base: V[p,q,r,s] = <pq|rs>, T[a,b,i,j], t1[a,i]; eps = diag(f).  For an occupied triple (i,j,k):

    w_ijk[a,b,c] = sum_f V_iabc[i,f,a,b] T[c,f,k,j] - sum_m V_ijak[i,j,a,m] T[b,c,m,k]
    W_ijk[a,b,c] = w_ijk[abc] + w_ikj[acb] + w_jik[bac] + w_jki[bca] + w_kij[cab] + w_kji[cba]
    Y_ijk[a,b,c] = W_ijk[abc] + V_ijab[j,k,b,c] t1[a,i] + V_ijab[i,k,a,c] t1[b,j] + V_ijab[i,j,a,b] t1[c,k]
    R(Y)[a,b,c]  = 4Y[abc] + Y[bca] + Y[cab] - 2Y[cba] - 2Y[acb] - 2Y[bac]
    S_ijk        = 1/3 sum_abc W[abc] R(Y)[abc] / (e_i + e_j + e_k - e_a - e_b - e_c)
    E(T)         = sum_{i >= j >= k} m_ijk S_ijk,   m = 6 (i > j > k), 3 (two equal), 1 (i = j = k)

The hole term is <ij|am> T[b,c,m,k]: the often printed <im|aj> is the same number only for 8-fold symmetric integrals.
TEST INFRASTRUCTURE ONLY."""
import numpy as np


def triples(no):
    """The unique triples in the library's order: i ascending, then j <= i, then k <= j."""
    return [(i, j, k) for i in range(no) for j in range(i + 1) for k in range(j + 1)]


def n_triples(no):
    return no * (no + 1) * (no + 2) // 6


def multiplicity(i, j, k):
    if i == j == k:
        return 1
    if i == j or j == k:
        return 3
    return 6


def _w(Viabc, Vijak, T, i, j, k):
    return (np.einsum("fab,cf->abc", Viabc[i], T[:, :, k, j])
            - np.einsum("am,bcm->abc", Vijak[i, j], T[:, :, :, k]))


def W_ijk(Viabc, Vijak, T, i, j, k):
    return (_w(Viabc, Vijak, T, i, j, k)
            + _w(Viabc, Vijak, T, i, k, j).transpose(0, 2, 1)
            + _w(Viabc, Vijak, T, j, i, k).transpose(1, 0, 2)
            + _w(Viabc, Vijak, T, j, k, i).transpose(2, 0, 1)
            + _w(Viabc, Vijak, T, k, i, j).transpose(1, 2, 0)
            + _w(Viabc, Vijak, T, k, j, i).transpose(2, 1, 0))


def blocks(no, V):
    """(V_iabc, V_ijak, V_ijab) of a dense V_pqrs."""
    o, v = slice(0, no), slice(no, None)
    return V[o, v, v, v], V[o, o, v, o], V[o, o, v, v]


def blocks_from_factors(no, B):
    """The same blocks of V[p,q,r,s] = sum_Q B[Q,p,r] B[Q,q,s] without the n^4 array."""
    o, v = slice(0, no), slice(no, None)
    return (np.einsum("Qib,Qac->iabc", B[:, o, v], B[:, v, v], optimize=True),
            np.einsum("Qia,Qjk->ijak", B[:, o, v], B[:, o, o], optimize=True),
            np.einsum("Qia,Qjb->ijab", B[:, o, v], B[:, o, v], optimize=True))


def S_ijk(no, V, eps, t1, T, i, j, k):
    """S_ijk of the closed-shell formula (one triple, any order of i, j, k)."""
    return S_ijk_blocks(blocks(no, V), eps, t1, T, i, j, k)


def S_ijk_blocks(blk, eps, t1, T, i, j, k):
    Viabc, Vijak, Vijab = blk
    no = Vijak.shape[0]
    W = W_ijk(Viabc, Vijak, T, i, j, k)
    Y = W.copy()
    if t1 is not None:
        Y += (np.einsum("bc,a->abc", Vijab[j, k], t1[:, i]) + np.einsum("ac,b->abc", Vijab[i, k], t1[:, j])
              + np.einsum("ab,c->abc", Vijab[i, j], t1[:, k]))
    R = (4 * Y + Y.transpose(1, 2, 0) + Y.transpose(2, 0, 1) - 2 * Y.transpose(2, 1, 0) - 2 * Y.transpose(0, 2, 1)
         - 2 * Y.transpose(1, 0, 2))
    ev = eps[no:]
    D = eps[i] + eps[j] + eps[k] - ev[:, None, None] - ev[None, :, None] - ev[None, None, :]
    return float(np.sum(W * R / D)) / 3.0


def per_triple(no, V, eps, t1, T, begin=0, end=None, blk=None):
    """m_ijk S_ijk for the triples [begin, end) of the library's order (blk: the blocks in place of V)."""
    blk = blocks(no, V) if blk is None else blk
    tri = triples(no)[begin:end]
    return np.array([multiplicity(*t) * S_ijk_blocks(blk, eps, t1, T, *t) for t in tri])


def energy(no, V, eps, t1, T):
    """E(T) by the explicit loop over the unique triples."""
    return float(np.sum(per_triple(no, V, eps, t1, T)))


def spin_orbital_energy(no, V, eps, t1, T):
    """Textbook spin-orbital (T) for tiny sizes: E = 1/36 sum t(c) D (t(c) + t(d)) with antisymmetrised integrals
    (Crawford and Schaefer, Rev. Comp. Chem. 14 (2000), eqs. 271-273), built from the spatial quantities: spin orbital
    2p + s (s = 0 alpha, 1 beta) of spatial orbital p."""
    n = V.shape[0]
    nv = n - no
    s = np.arange(2 * n) % 2
    p = np.arange(2 * n) // 2
    same = (s[:, None] == s[None, :]).astype(float)
    Vs = V[np.ix_(p, p, p, p)] * same[:, None, :, None] * same[None, :, None, :]
    A = Vs - Vs.transpose(0, 1, 3, 2)                     # <pq||rs>
    O = 2 * no
    oo, vv = slice(0, O), slice(O, None)
    ps_o, ps_v = p[:O], p[O:] - no
    s_o, s_v = s[:O], s[O:]
    t1s = np.zeros((2 * nv, O))
    if t1 is not None:
        t1s = t1[np.ix_(ps_v, ps_o)] * (s_v[:, None] == s_o[None, :])
    d_ai = (s_v[:, None] == s_o[None, :]).astype(float)
    # t_ij^ab (spin orbitals, [a,b,i,j]) = T[a,b,i,j] d(a,i) d(b,j) - T[b,a,i,j] d(b,i) d(a,j)
    T2 = T[np.ix_(ps_v, ps_v, ps_o, ps_o)]
    Tba = T2.transpose(1, 0, 2, 3)
    t2s = np.einsum("abij,ai,bj->abij", T2, d_ai, d_ai) - np.einsum("abij,bi,aj->abij", Tba, d_ai, d_ai)
    Vvovv = A[vv, oo, vv, vv]         # <ei||bc> as [e,i,b,c]
    Vovoo = A[oo, vv, oo, oo]         # <ma||jk> as [m,a,j,k]
    Voovv = A[oo, oo, vv, vv]         # <jk||bc>
    # X(c)[i,j,k,a,b,c] before the permutations: sum_e t_jk^ae <ei||bc> - sum_m t_im^bc <ma||jk>
    Xc = np.einsum("aejk,eibc->ijkabc", t2s, Vvovv) - np.einsum("bcim,majk->ijkabc", t2s, Vovoo)
    Xd = np.einsum("ai,jkbc->ijkabc", t1s, Voovv)

    def P(X):
        # P(i/jk) P(a/bc): f(ijk) - f(jik) - f(kji) on both triples
        X = X - X.transpose(1, 0, 2, 3, 4, 5) - X.transpose(2, 1, 0, 3, 4, 5)
        return X - X.transpose(0, 1, 2, 4, 3, 5) - X.transpose(0, 1, 2, 5, 4, 3)
    Xc, Xd = P(Xc), P(Xd)
    e = eps[p]
    eo, ev = e[:O], e[O:]
    D = (eo[:, None, None, None, None, None] + eo[None, :, None, None, None, None] + eo[None, None, :, None, None, None]
         - ev[None, None, None, :, None, None] - ev[None, None, None, None, :, None] - ev[None, None, None, None, None, :])
    return float(np.sum(Xc * (Xc + Xd) / D)) / 36.0


# ---- inputs -------------------------------------------------------------------------------------------------------------
def four_fold_V(n, seed, scale=0.1):
    """Random real integrals with only V_pqrs = V_qpsr = V_rspq (the symmetry of plane-wave UEG integrals)."""
    X = np.random.default_rng(seed).standard_normal((n, n, n, n)) * scale
    return 0.25 * (X + X.transpose(1, 0, 3, 2) + X.transpose(2, 3, 0, 1) + X.transpose(3, 2, 1, 0))


def random_amplitudes(no, nv, seed, amp=0.05):
    """Random T1 and pair-symmetric T2 (T[a,b,i,j] = T[b,a,j,i])."""
    rng = np.random.default_rng(seed)
    t1 = rng.standard_normal((nv, no)) * amp
    t2 = rng.standard_normal((nv, nv, no, no)) * amp
    return t1, 0.5 * (t2 + t2.transpose(1, 0, 3, 2))
