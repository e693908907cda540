"""numpy reference of the CCSD two-particle response density.  TEST INFRASTRUCTURE ONLY.

``L(f, V) = E(f, V) + <l1, R1(f, V)> + <l2, R2(f, V)>`` is the Lagrangian of ``_lambda_reference.lagrangian_density`` with the
two-body integrals switched on: ``oracle/cc_oracle.py``'s energy and residuals at fixed (t1, t2, l1, l2).  It is linear and
homogeneous in (f, V).  ``G_pqrs = dL/dV_pqrs`` (f held fixed, all n^4 entries independent) and ``Gamma_pqrs = (G_pqrs + G_qpsr) / 2``:
``L(f, V) = sum gamma f + sum Gamma V`` for every V with V_pqrs = V_qpsr; no factor 1/2, nothing hermitian, nothing symmetrised.

``lagrangian_density2`` is the definition (n^4 evaluations of L), ``rdm2_terms`` the same blocks written out as the contractions
the device performs: densities of the six dressed blocks, their back-transformation through T1, the dressed-Fock part
and the direct terms.  Conventions as in ``_lambda_reference``; block names as ``cc_oracle.split_blocks``.
"""
import functools
import os

import numpy as np

from oracle import cc_oracle as cc
from tests import _lambda_reference as LR

ein = functools.partial(np.einsum, optimize=True)


def lagrangian(no, f, V, t1, t2, l1, l2):
    """One evaluation of L(f, V)."""
    Vb = cc.split_blocks(no, V)
    fd = cc.dressed_fock(no, f, t1, Vb)
    Vd = cc.dressed_V(t1, Vb)
    r1 = cc.singles_residual(no, fd, t1, t2, Vb)
    r2 = cc.ccsd_doubles_residual(no, fd, t2, Vd, ein=ein)
    return float(sum(cc.ccsd_energy(f[:no, no:], t1, t2, Vb["ijab"])) + (l1 * r1).sum() + (l2 * r2).sum())


def project(G):
    return 0.5 * (G + G.transpose(1, 0, 3, 2))


def lagrangian_density2(no, t1, t2, l1, l2):
    """Gamma [n,n,n,n] by definition: L(0, e_pqrs) for every unit tensor, then the projection."""
    n = no + t1.shape[0]
    f0 = np.zeros((n, n))
    G = np.zeros((n, n, n, n))
    e = np.zeros((n, n, n, n))
    for idx in np.ndindex(n, n, n, n):
        e[idx] = 1.0
        G[idx] = lagrangian(no, f0, e, t1, t2, l1, l2)
        e[idx] = 0.0
    return project(G)


# ---- the same, written out ---------------------------------------------------------------------------------------------------------
def dressed_densities(no, t1, t2, l1, l2):
    """Coefficients in L of the six dressed blocks the doubles residual reads (abij, klij, ijab, iajb, iabj, abcd); the ijab
    entry holds only what <l2, R2> contributes (the dressed ijab block is the undressed one)."""
    T, L = t2, l2
    Tt = 2.0 * T - T.transpose(1, 0, 2, 3)
    gvv = 2.0 * ein("abij,cbij->ac", L, T)
    goo = -2.0 * ein("abij,abkj->ki", L, T)
    Bn = ein("abij,abkl->klij", L, T)
    d = {"abij": L.copy(), "klij": Bn, "abcd": ein("abij,cdij->abcd", L, T)}
    d["iajb"] = -2.0 * ein("abij,cbkj->kaic", L, T) - 2.0 * ein("abij,ackj->kbic", L, T)
    d["iabj"] = 2.0 * ein("abij,acik->kbcj", L, Tt)
    J = ein("klij,cdij->klcd", Bn, T)
    J += ein("bidk,cbil->klcd", ein("abij,adkj->bidk", L, T), T)
    J += ein("bjck,dblj->klcd", ein("abij,acik->bjck", L, Tt), Tt)
    J -= ein("ad,aclk->klcd", gvv, Tt)
    J += ein("li,dcik->klcd", goo, Tt)
    J += 2.0 * ein("bjdk,bclj->klcd", ein("abij,daki->bjdk", L, T), T - T.transpose(1, 0, 2, 3))
    d["ijab"] = J
    return d, gvv, goo


def back_transform(no, key, D, t1, out):
    """The adjoint of ``cc_oracle.dressed_block``: adds the density D of the dressed block ``key`` to the undressed blocks it was
    built from.  A bra-virtual index sends -t[a,k] x D to the occupied source index, a ket-occupied one +t[c,i] x D to the
    virtual source; index by index, each subset of the transformable positions once."""
    def walk(pat, X, start):
        out[cc.NAME_OF_PATTERN[pat]] += X
        for pos in range(start, 4):
            sub = "pqrs"
            if pos < 2 and pat[pos] == "v":
                Y = -ein(sub + ",%sx->" % sub[pos] + sub.replace(sub[pos], "x"), X, t1)
                walk(pat[:pos] + "o" + pat[pos + 1:], Y, pos + 1)
            elif pos >= 2 and pat[pos] == "o":
                Y = ein(sub + ",x%s->" % sub[pos] + sub.replace(sub[pos], "x"), X, t1)
                walk(pat[:pos] + "v" + pat[pos + 1:], Y, pos + 1)
    walk(cc._pattern(key), D, 0)


def raw_density2(no, t1, t2, l1, l2):
    """G = dL/dV block by block (dictionary of the 16 blocks), before the projection."""
    nv = t1.shape[0]
    dim = {"o": no, "v": nv}
    G = {nm: np.zeros(tuple(dim[c] for c in cc._pattern(nm))) for nm in cc.BLOCK_NAMES}
    T = t2
    Tt = 2.0 * T - T.transpose(1, 0, 2, 3)
    # 1 + 2: the dressed-block densities, back-transformed
    d, gvv, goo = dressed_densities(no, t1, t2, l1, l2)
    for key, D in d.items():
        back_transform(no, key, D, t1, G)
    # 3: the dressed-Fock part.  C is gamma~ pulled back through the f terms of the dressing (the response density without the
    # energy's 2 t1); the direct sum over the occupied orbital j reads V[j,p,b,q], the exchange sum V[j,p,q,b].  The reference
    # dresses f_ov[i,a] with V_iabj[j,a,b,i] in place of V_ijab[j,i,b,a] (DESIGN 8d caveat): that term goes where it reads.
    gov = ein("ai,abij->jb", l1, Tt)
    n = no + nv
    C = np.zeros((n, n))
    C[no:, :no] = l1
    C[:no, :no] = goo - t1.T @ l1
    C[no:, no:] = gvv + l1 @ t1.T
    C[:no, no:] = gov - t1.T @ l1 @ t1.T + goo @ t1.T - t1.T @ gvv
    Cd = C.copy()
    Cd[:no, no:] -= gov
    o, v = slice(0, no), slice(no, None)
    for (P, p), (Q, q) in ((x, y) for x in (("o", o), ("v", v)) for y in (("o", o), ("v", v))):
        G[cc.NAME_OF_PATTERN["o" + P + "v" + Q]] += 2.0 * ein("bj,pq->jpbq", t1, Cd[p, q])
        G[cc.NAME_OF_PATTERN["o" + P + Q + "v"]] -= ein("bj,pq->jpqb", t1, C[p, q])
    G["iabj"] += 2.0 * ein("bj,ia->jabi", t1, gov)
    # 4: the direct V terms of the singles residual and of the energy
    G["aibc"] += ein("ai,bcij->ajbc", l1, Tt)
    G["ijab"] -= ein("ik,bcij->kjbc", ein("ai,ak->ik", l1, t1), Tt)
    G["ijka"] -= ein("ai,abjk->jkib", l1, Tt)
    G["ijab"] -= ein("ac,abjk->jkcb", ein("ai,ci->ac", l1, t1), Tt)
    tau = T + ein("ai,bj->abij", t1, t1)
    G["ijab"] += (2.0 * tau - tau.transpose(1, 0, 2, 3)).transpose(2, 3, 0, 1)
    return G


def project_blocks(G):
    """Gamma_pqrs = (G_pqrs + G_qpsr) / 2 on a dictionary of the 16 blocks."""
    out = {}
    for nm, X in G.items():
        pat = cc._pattern(nm)
        partner = cc.NAME_OF_PATTERN[pat[1] + pat[0] + pat[3] + pat[2]]
        out[nm] = 0.5 * (X + G[partner].transpose(1, 0, 3, 2))
    return out


def rdm2_terms(no, t1, t2, l1, l2):
    """The 16 blocks of Gamma as the device builds them."""
    return project_blocks(raw_density2(no, t1, t2, l1, l2))


def assemble(no, blocks):
    """[n,n,n,n] from a complete dictionary of blocks."""
    nv = blocks["abij"].shape[0]
    n = no + nv
    out = np.zeros((n, n, n, n))
    for nm, view in cc.split_blocks(no, out).items():
        view[...] = blocks[nm]
    return out


def contract_blocks(Gb, Wb):
    return float(sum((Gb[nm] * Wb[nm]).sum() for nm in Gb))


def sym_problem(no, nv, seed, eight):
    """(f, V) of _lambda_reference.random_problem (8-fold symmetric, or V_pqrs = V_qpsr only)."""
    return LR.random_problem(no, nv, seed, eight=eight)


# ---- the density by definition at (3,5): 4096 evaluations of the Lagrangian, recorded
# (python -m tests._rdm2_reference rewrites tests/golden/lambda_rdm2_3_5.npz) ---------------------------------------------------
GOLDEN_RDM2 = ("lambda_rdm2_3_5.npz", 3, 5, 11)          # file, no, nv, seed
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_rdm2():
    name, no, nv, seed = GOLDEN_RDM2
    return no, nv, LR.density_inputs(no, nv, seed), np.load(os.path.join(GOLD, name))["rdm2"]


if __name__ == "__main__":
    name, no, nv, seed = GOLDEN_RDM2
    np.savez_compressed(os.path.join(GOLD, name), rdm2=lagrangian_density2(no, *LR.density_inputs(no, nv, seed)))
