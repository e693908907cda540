"""Plain-numpy restatement of the momentum-sector CCD / DCD residual (pymes_amd/solver/ueg_cc.py; DESIGN "Momentum
sectors"): the same tables (pymes_amd/solver/sectors.py), the same product list, one numpy matmul per sector.  TEST
INFRASTRUCTURE ONLY: checked against oracle.cc_oracle on the CPU, and what the HIP path is compared with on the GPU."""
import numpy as np

from pymes_amd.solver.sectors import BLOCKS, FOCK_LISTS, SectorTables


def tables_for(k_int, no):
    return SectorTables(k_int, no)


def sector_integrals(tab, V):
    """Every block family gathered from a dense V_pqrs."""
    out = {}
    for name in tuple(BLOCKS) + FOCK_LISTS:
        idx = tab.block_pqrs(name)
        out[name] = V[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]
    return out


def hf_orbital_energies(tab, ints, kinetic):
    return np.asarray(kinetic) + (2.0 * ints["pipi"] - ints["piip"]).reshape(tab.n, tab.no).sum(axis=1)


class Blocks:
    """Views of one block family stored sector after sector (row-major)."""

    def __init__(self, tab, rows, cols, data=None):
        self.nr, self.nc, self.off = tab._sizes[rows], tab._sizes[cols], tab.offsets(rows, cols)
        self.data = np.zeros(int(self.off[-1])) if data is None else data
        assert len(self.data) == self.off[-1]

    def __getitem__(self, s):
        return self.data[self.off[s]:self.off[s + 1]].reshape(self.nr[s], self.nc[s])


def residual(tab, eps, T, ints, is_dcd=False):
    """The compact residual of ccd.py:164-254 for a diagonal Fock matrix `eps` (all orbitals), term by term as the device
    path forms it."""
    quad = not is_dcd
    w = 1.0 if quad else 0.5
    no = tab.no
    nP, nq, neg = len(tab.P_keys), len(tab.q_keys), tab.neg
    B = lambda name, data=None: Blocks(tab, *BLOCKS[name][:2], data=ints[name] if data is None else data)
    # ---- pp layout: hole ladder, particle ladder
    Tp, R = Blocks(tab, "vv", "oo", T), Blocks(tab, "vv", "oo", ints["abij"].copy())
    klij, klcd, abcd = B("klij"), B("klcd"), B("abcd")
    for s in range(nP):
        hole = klij[s] + (klcd[s] @ Tp[s] if quad else 0.0)
        R[s][...] += Tp[s] @ hole + abcd[s] @ Tp[s]
    # ---- ph layouts
    ph = lambda data=None: Blocks(tab, "ph", "ph-", data)
    D, Cx = ph(T[tab.d_from_pp]), ph(T[tab.c_from_pp])
    Tt = ph(2.0 * D.data - Cx.data)
    W1, Wx, Wa, W2 = B("w1"), B("wx"), B("wa"), B("w2")
    Rd, Ed, Rc, Ec = ph(), ph(), ph(), ph()
    X = Blocks(tab, "ph", "ph")
    for q in range(nq):
        X[q][...] = W1[q] @ Tt[neg[q]] if neg[q] >= 0 else 0.0
    for q in range(nq):
        m = neg[q]
        if m < 0:
            continue
        Rd[q][...] += Tt[q] @ X[m]                                          # ccd.py:202-204
        Ed[q][...] += Tt[q] @ W2[m] - Wa[q] @ D[q]
        Ec[q][...] -= Cx[q] @ Wa[m].T
        if quad:
            Ed[q][...] += (D[q] @ Wx[m]) @ (Cx[q] - D[q])                  # :237-240
            Rc[q][...] += (Cx[q] @ Wx[m]) @ Cx[q]                          # :189-191
    # ---- the diagonal X_ac, X_ki (row sums of Tt o W1 in the direct layout)
    s_row = np.array([np.dot(Tt.data[a:a + n], W1.data[a:a + n]) for a, n in zip(tab.row_start, tab.row_len)])
    s_ai = s_row[tab.ph_row].reshape(tab.nv, no)
    eps = np.asarray(eps, dtype=np.float64)
    x_vv, x_oo = eps[no:] - w * s_ai.sum(axis=1), eps[:no] + w * s_ai.sum(axis=0)
    scale = (x_vv[:, None] - x_oo[None, :]).reshape(-1)
    row_scale = np.empty(tab.nv * no)
    row_scale[tab.ph_row] = scale
    Ed.data += np.repeat(row_scale, tab.row_len) * D.data
    # ---- Ex + Ex^T(1,0,3,2), and everything back to the pp vector
    return (R.data + Rd.data[tab.pp_to_d] + Rc.data[tab.pp_to_c] + Ed.data[tab.pp_to_d] + Ed.data[tab.pp_to_dT]
            + Ec.data[tab.pp_to_c] + Ec.data[tab.pp_to_cT])


def energy(T, ints):
    return 2.0 * np.dot(T, ints["ed"]), -np.dot(T, ints["ex"])


def solve(tab, eps, ints, is_dcd=False, delta_e=1e-8, max_iter=50, level_shift=0.0, mixer=None):
    """cc_oracle.ccd_solve on the compact vector (the oracle's own DIIS bookkeeping); returns the energy of every pass."""
    from oracle import cc_oracle as oc
    inv = 1.0 / (tab.denominators(eps) + level_shift)
    T = ints["abij"] * inv
    e_last = sum(energy(T, ints))
    mixer = mixer or oc.Diis(6)
    dE, it, hist = abs(e_last), 0, []
    while abs(dE) > delta_e and it <= max_iter:
        it += 1
        dT = residual(tab, eps, T, ints, is_dcd) * inv
        T = mixer.mix([dT], [T + dT])[0]
        e = float(sum(energy(T, ints)))
        dE, e_last = e - e_last, e
        hist.append(e)
    return {"e": e_last, "t2": T, "history": hist, "iterations": it}
