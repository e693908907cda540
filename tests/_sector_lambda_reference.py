"""Plain-numpy restatement of the momentum-sector Lambda equations and of the two-slab Lambda-(T)
(pymes_amd/solver/ueg_cc.py, SectorLambda and sector_lambda_triples_energy): the transpose of the Jacobian of
tests/_sector_reference.residual, term by term and sector by sector as the device forms it, and the energy of a triple from a
right-hand and a left-hand W slab.  TEST INFRASTRUCTURE ONLY: checked on the CPU against finite differences of the residual
and against tests/_lambda_reference.py / tests/_lambda_triples_reference.py, and what the HIP path is compared with."""
import numpy as np

from pymes_amd.solver.sectors import BLOCKS
from tests import _sector_triples_reference as tr
from tests import _triples_reference as R
from tests._sector_reference import Blocks


def eta(ints):
    """dE/dT of E = 2 T.ed - T.ex on the compact vector."""
    return 2.0 * ints["ed"] - ints["ex"]


def jt_plain(tab, eps, T, ints, lam, is_dcd=False):
    """The adjoint of every product of ``_sector_reference.residual`` applied to `lam`, plain inner product over the compact
    elements.  The product list treats the two electrons differently (Rd = Tt X, Rc = Xc C are exchange-symmetric only as
    functions of a symmetric T), so this is not exchange-symmetric even for symmetric `lam`; ``jt_apply`` projects it."""
    quad = not is_dcd
    w = 1.0 if quad else 0.5
    no = tab.no
    nP, nq, neg = len(tab.P_keys), len(tab.q_keys), tab.neg
    B = lambda name: Blocks(tab, *BLOCKS[name][:2], data=ints[name])
    # ---- pp layout: G^P = lam^P hole^T + [CCD] klcd^T (T^T lam) + abcd^T lam
    Tp, Lp, G = Blocks(tab, "vv", "oo", T), Blocks(tab, "vv", "oo", lam), Blocks(tab, "vv", "oo")
    klij, klcd, abcd = B("klij"), B("klcd"), B("abcd")
    for s in range(nP):
        hole = klij[s] + (klcd[s] @ Tp[s] if quad else 0.0)
        G[s][...] = Lp[s] @ hole.T + abcd[s].T @ Lp[s]
        if quad:
            G[s][...] += klcd[s].T @ (Tp[s].T @ Lp[s])
    # ---- ph layouts of T (what the solver hoists) and the cotangents of Rd, Rc, Ed, Ec
    ph = lambda data=None: Blocks(tab, "ph", "ph-", data)
    sq = lambda: Blocks(tab, "ph", "ph")
    D, Cx = ph(T[tab.d_from_pp]), ph(T[tab.c_from_pp])
    Tt, CmD = ph(2.0 * D.data - Cx.data), ph(Cx.data - D.data)
    W1, Wx, Wa, W2 = B("w1"), B("wx"), B("wa"), B("w2")
    X, Y, Xc = sq(), sq(), sq()
    for q in range(nq):
        if neg[q] >= 0:
            X[q][...], Y[q][...], Xc[q][...] = W1[q] @ Tt[neg[q]], D[q] @ Wx[neg[q]], Cx[q] @ Wx[neg[q]]
    yRd, yRc = ph(lam[tab.d_from_pp]), ph(lam[tab.c_from_pp])
    yEd = ph(yRd.data + yRd.data[tab.d_partner])                          # Ed enters as Ed + Ed^T(1,0,3,2)
    yEc = ph(yRc.data + yRc.data[tab.d_partner])
    zTt, zD, zC, zM = ph(), ph(), ph(), ph()                                 # zM: the cotangent of C - D
    Z = sq()
    for q in range(nq):
        if neg[q] >= 0:
            Z[q][...] = Tt[neg[q]].T @ yRd[neg[q]]                           # the cotangent of X^q
    for q in range(nq):
        m = neg[q]
        if m < 0:
            continue
        zTt[q][...] = yRd[q] @ X[m].T + yEd[q] @ W2[m].T + W1[m].T @ Z[m]
        zD[q][...] = -(Wa[q].T @ yEd[q])
        zC[q][...] = -(yEc[q] @ Wa[m])
        if quad:
            zM[q][...] = Y[q].T @ yEd[q]
            zD[q][...] += (yEd[q] @ CmD[q].T) @ Wx[m].T
            zC[q][...] += Xc[q].T @ yRc[q] + (yRc[q] @ Cx[q].T) @ Wx[m].T
    # ---- the diagonal X_ac / X_ki term: Ed[g,:] += scale(T)[g] D[g,:], scale = x_vv[a] - x_oo[i]
    rows = list(zip(tab.row_start, tab.row_len))
    s_row = np.array([np.dot(Tt.data[a:a + n], W1.data[a:a + n]) for a, n in rows])
    s_ai = s_row[tab.ph_row].reshape(tab.nv, no)
    eps = np.asarray(eps, dtype=np.float64)
    x_vv, x_oo = eps[no:] - w * s_ai.sum(axis=1), eps[:no] + w * s_ai.sum(axis=0)
    row_scale = np.empty(tab.nv * no)
    row_scale[tab.ph_row] = (x_vv[:, None] - x_oo[None, :]).reshape(-1)
    zD.data += np.repeat(row_scale, tab.row_len) * yEd.data
    rho = np.array([np.dot(yEd.data[a:a + n], D.data[a:a + n]) for a, n in rows])
    r_ai = rho[tab.ph_row].reshape(tab.nv, no)
    back = np.empty(tab.nv * no)
    back[tab.ph_row] = (-w * (r_ai.sum(axis=1)[:, None] + r_ai.sum(axis=0)[None, :])).reshape(-1)
    zTt.data += np.repeat(back, tab.row_len) * W1.data
    # ---- back to the pp vector: D = T[d_from_pp], C = T[c_from_pp], Tt = 2 D - C
    out = G.data + zD.data[tab.pp_to_d] + zC.data[tab.pp_to_c] + 2.0 * zTt.data[tab.pp_to_d] - zTt.data[tab.pp_to_c]
    if quad:
        out += zM.data[tab.pp_to_c] - zM.data[tab.pp_to_d]
    return out


def jt_apply(tab, eps, T, ints, lam, is_dcd=False):
    """J(T)^T lam, J = dR/dT on the exchange-symmetric vectors: ``jt_plain`` projected on them, (x + x[pp_swap]) / 2 (the
    two have the same inner product with every symmetric vector)."""
    g = jt_plain(tab, eps, T, ints, lam, is_dcd)
    return 0.5 * g + 0.5 * g[tab.pp_swap]


def lambda_residual(tab, eps, T, ints, lam, is_dcd=False):
    """G(lam) = J^T lam + eta, the sum projected as a whole (eta is symmetric up to the rounding of the integrals), so that
    G is symmetric to the bit."""
    g = jt_plain(tab, eps, T, ints, lam, is_dcd) + eta(ints)
    return 0.5 * g + 0.5 * g[tab.pp_swap]


def solve_lambda(tab, eps, T, ints, is_dcd=False, tol=1e-12, max_iter=200):
    """lam <- lam + G / den from lam = 0, plain iteration with the oracle's DIIS; returns (lam, |G|)."""
    from oracle import cc_oracle as oc
    inv = 1.0 / tab.denominators(eps)
    lam, mixer, norm = np.zeros(tab.nnz), oc.Diis(6), np.inf
    for _ in range(max_iter):
        g = lambda_residual(tab, eps, T, ints, lam, is_dcd)
        norm = float(np.linalg.norm(g))
        if norm <= tol:
            break
        d = g * inv
        lam = mixer.mix([d], [lam + d])[0]
    return lam, norm


# ---- Lambda-(T) -----------------------------------------------------------------------------------------------------------
def right_integrals(tt, V):
    """(VvR [o,v,v], VoR [o,o,v]) gathered from a dense V_pqrs: VvR[i,a,b] = V[a,b,i,f*], VoR[i,j,a] = V[a,m*,i,j]; exact
    zeros where the implied orbital does not exist."""
    out = []
    for family, shape in (("vv_r", (tt.no, tt.nv, tt.nv)), ("vo_r", (tt.no, tt.no, tt.nv))):
        pqrs, valid = tt.list_pqrs(family)
        x = np.zeros(len(valid))
        p = pqrs[valid]
        x[valid] = V[p[:, 0], p[:, 1], p[:, 2], p[:, 3]]
        out.append(x.reshape(shape))
    return out


def left_amplitudes(tab, lam):
    """L = (2 lam + lam^x) / 3 on the compact vector, lam^x[a,b,i,j] = lam[b,a,i,j]."""
    a, b, i, j = tab.abij()
    return (2.0 * lam + lam[tab._pp_index(b, a, i, j)]) / 3.0


def triple_terms(tt, eps, WR, WL, c, i, j, k):
    """(WR[a,b] R(WL)[a,b] / D[a,b] / 3, the same with every product taken by its absolute value) per (a,b) with a virtual c."""
    ok = c >= 0
    a, b = np.nonzero(ok)
    cc = c[ok]
    r = 4.0 * WL[a, b] + WL[b, cc] + WL[cc, a] - 2.0 * WL[cc, b] - 2.0 * WL[a, cc] - 2.0 * WL[b, a]
    A = np.abs(WL)
    ra = 4.0 * A[a, b] + A[b, cc] + A[cc, a] + 2.0 * A[cc, b] + 2.0 * A[a, cc] + 2.0 * A[b, a]
    ev = np.asarray(eps)[tt.no:]
    d = eps[i] + eps[j] + eps[k] - ev[a] - ev[b] - ev[cc]
    return WR[a, b] * r / d / 3.0, np.abs(WR[a, b]) * ra / np.abs(d) / 3.0


def per_triple(tt, eps, VvR, VoR, VvL, VoL, Tc, Lc, begin=0, end=None):
    """(m_ijk S_ijk, m_ijk sum |terms|) of the triples [begin, end): WR from (VvR, VoR, Tc), WL from (VvL, VoL, Lc)."""
    val, scale = [], []
    for (i, j, k) in R.triples(tt.no)[begin:end]:
        WR, c = tr.W_slab(tt, VvR, VoR, Tc, i, j, k)
        WL, _ = tr.W_slab(tt, VvL, VoL, Lc, i, j, k)
        terms, bound = triple_terms(tt, eps, WR, WL, c, i, j, k)
        m = R.multiplicity(i, j, k)
        val.append(m * float(terms.sum()))
        scale.append(m * float(bound.sum()))
    return np.array(val), np.array(scale)
