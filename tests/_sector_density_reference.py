"""Plain-numpy restatement of the sector densities (pymes_amd/solver/ueg_cc.py, SectorDensity): gamma and the
density arena G, the derivatives of L(eps, V) = E(T; V) + <lam, R(T; eps, V)> with respect to the orbital energies and to every
stored integral element, as the term-by-term adjoint of the product list of tests/_sector_reference.residual with respect to
its integral operands; the transfer sums s(q) and the structure factor.  TEST INFRASTRUCTURE ONLY: checked on the CPU against
the definition (L is linear in eps and in the integrals) and against the dense densities, and what the HIP path is compared
with."""
import numpy as np

from pymes_amd.solver.sectors import BLOCKS, FOCK_LISTS
from tests import _sector_reference as sr
from tests._sector_reference import Blocks


def lagrangian(tab, eps, ints, T, lam, is_dcd=False):
    """L(eps, V) at fixed (T, lam), and the sum of the absolute values of its terms."""
    R = sr.residual(tab, eps, T, ints, is_dcd)
    e_dir, e_ex = sr.energy(T, ints)
    return float(e_dir + e_ex + lam @ R), float(abs(e_dir) + abs(e_ex) + np.abs(lam) @ np.abs(R))


def zero_integrals(tab):
    out = {name: np.zeros(int(tab.block_offsets(name)[-1])) for name in BLOCKS}
    out.update({name: np.zeros(tab.n * tab.no) for name in FOCK_LISTS})
    return out


def density(tab, T, lam, is_dcd=False):
    """(gamma [n], {family: G}) with every family of BLOCKS, ``abcd`` included."""
    quad = not is_dcd
    w = 1.0 if quad else 0.5
    no, nv = tab.no, tab.nv
    nP, nq, neg = len(tab.P_keys), len(tab.q_keys), tab.neg
    G = {name: Blocks(tab, *BLOCKS[name][:2]) for name in BLOCKS}
    G["abij"].data[:], G["ed"].data[:], G["ex"].data[:] = lam, 2.0 * T, -T
    # ---- pp layout: R^P = V_abij^P + T^P (V_klij^P + [CCD] V_klcd^P T^P) + V_abcd^P T^P
    Tp, Lp = Blocks(tab, "vv", "oo", T), Blocks(tab, "vv", "oo", lam)
    for s in range(nP):
        M = Tp[s].T @ Lp[s]
        G["klij"][s][...] = M
        G["abcd"][s][...] = Lp[s] @ Tp[s].T
        if quad:
            G["klcd"][s][...] = M @ Tp[s].T
    # ---- ph layouts of T and the cotangents of Rd, Rc, Ed, Ec (as tests/_sector_lambda_reference.jt_plain)
    ph = lambda data=None: Blocks(tab, "ph", "ph-", data)
    D, Cx = ph(T[tab.d_from_pp]), ph(T[tab.c_from_pp])
    Tt, CmD = ph(2.0 * D.data - Cx.data), ph(Cx.data - D.data)
    yRd, yRc = ph(lam[tab.d_from_pp]), ph(lam[tab.c_from_pp])
    yEd = ph(yRd.data + yRd.data[tab.d_partner])
    yEc = ph(yRc.data + yRc.data[tab.d_partner])
    for q in range(nq):
        m = neg[q]
        if m < 0:
            continue
        Z = Tt[m].T @ yRd[m]                                                  # the cotangent of X^q = W1^q Tt^{-q}
        G["w1"][q][...] = Z @ Tt[m].T
        G["w2"][q][...] = Tt[m].T @ yEd[m]                                    # Ed^{-q} = Tt^{-q} W2^q
        G["wa"][q][...] = -(yEd[q] @ D[q].T) - yEc[m].T @ Cx[m]               # Ed^q -= Wa^q D^q;  Ec^{-q} = -C^{-q} (Wa^q)^T
        if quad:
            G["wx"][q][...] = D[m].T @ (yEd[m] @ CmD[m].T) + Cx[m].T @ (yRc[m] @ Cx[m].T)
    # ---- the diagonal X_ac / X_ki term: gamma, and its W1 part
    rows = list(zip(tab.row_start, tab.row_len))
    rho = np.array([np.dot(yEd.data[a:a + n], D.data[a:a + n]) for a, n in rows])
    r_ai = rho[tab.ph_row].reshape(nv, no)
    gamma = np.concatenate((-r_ai.sum(axis=0), r_ai.sum(axis=1)))
    back = np.empty(nv * no)
    back[tab.ph_row] = (-w * (r_ai.sum(axis=1)[:, None] + r_ai.sum(axis=0)[None, :])).reshape(-1)
    G["w1"].data += np.repeat(back, tab.row_len) * Tt.data
    return gamma, {name: G[name].data for name in BLOCKS}


def expectation(tab, gamma, G, eps_w, W):
    """L(eps_w, W) = gamma . eps_w + <G, W> over every family."""
    return float(gamma @ eps_w + sum(G[name] @ W[name] for name in BLOCKS))


def transfer_bins(tab):
    """(bin vectors [bins,3] sorted lexicographically, the bin of -q, the bin of 0): every k_r - k_p over all orbital pairs."""
    k = tab.k_int
    q = np.unique((k[None, :, :] - k[:, None, :]).reshape(-1, 3), axis=0)
    index = {tuple(v): b for b, v in enumerate(q)}
    neg = np.array([index[tuple(-v)] for v in q])
    return q, neg, index[(0, 0, 0)]


def transfer_sums(tab, G, q, families=tuple(BLOCKS)):
    """s(q) per bin: G summed over the elements (p,q,r,s) of the families with k_r - k_p = q."""
    index = {tuple(v): b for b, v in enumerate(q)}
    k, s = tab.k_int, np.zeros(len(q))
    for name in families:
        pqrs = tab.block_pqrs(name)
        bins = np.array([index[tuple(v)] for v in k[pqrs[:, 2]] - k[pqrs[:, 0]]], dtype=np.int64)
        s += np.bincount(bins, weights=G[name], minlength=len(q))
    return s


def structure_factor(tab, gamma, s, q, neg, zero):
    """S(q) per bin in the convention of ``lambda_ccsd.full_rdm2``, from the plain s(q)."""
    k, no = tab.k_int, tab.no
    N = 2 * no
    index = {tuple(v): b for b, v in enumerate(q)}
    bracket = 2.0 * 0.5 * (s + s[neg])
    for i in range(no):
        for j in range(no):
            bracket[index[tuple(k[j] - k[i])]] -= 2.0
        for p in range(tab.n):
            bracket[index[tuple(k[i] - k[p])]] -= gamma[p]
            bracket[index[tuple(k[p] - k[i])]] -= gamma[p]
    bracket[zero] = N * (N - 1)
    return 1.0 + bracket / N
