"""Plain-numpy restatement of the sector IP- / EA-EOM-CCD sigma (pymes_amd/solver/ueg_eom.py) on the host copies of
the sector data: the integral families of tests/_sector_reference.sector_integrals, the four implied-index lists of the
triples tables, the compact amplitudes.  Independent of the device code's factorisation: the blocks the term tables of
tests/_ipea_reference.py name are rebuilt as coordinate lists from the sector data, and every one of the 7 + 32 terms of an
operator is contracted as it is written there, by a small sparse einsum (joins on the shared labels, smallest operand first).
Here t1 = 0, f_ov = 0 and the Fock matrix is diagonal.  TEST INFRASTRUCTURE ONLY: checked against tests/_ipea_reference.py on
the CPU (tests/test_sector_ipea_reference.py), and what the HIP path is compared with on the GPU."""
import numpy as np

from pymes_amd.solver.sectors import QuasiparticleTables
from tests import _ipea_reference as ip
from tests import _sector_lambda_reference as sl
from tests import _sector_triples_reference as tr


class Coo:
    """A sparse array: `idx` [nnz, ndim] int64 (one column per label of `labels`) and `val` [nnz]."""

    def __init__(self, labels, idx, val):
        self.labels, self.idx, self.val = labels, np.asarray(idx, dtype=np.int64).reshape(len(val), len(labels)), \
            np.asarray(val, dtype=np.float64)

    def sum_out(self, keep, base):
        """Summed over every label that is not in `keep`; equal coordinates merged (every index is below `base`)."""
        cols = [n for n, l in enumerate(self.labels) if l in keep]
        labels = "".join(self.labels[n] for n in cols)
        idx = self.idx[:, cols]
        if not len(self.val):
            return Coo(labels, idx, self.val)
        _, first, inv = np.unique(_key(idx, range(len(cols)), base), return_index=True, return_inverse=True)
        return Coo(labels, idx[first], np.bincount(inv.reshape(-1), weights=self.val, minlength=len(first)))


def _key(idx, cols, base):
    assert base ** len(cols) < 2 ** 62, "the coordinates of a sparse product do not fit one int64 key"
    key = np.zeros(len(idx), dtype=np.int64)
    for c in cols:
        key = key * base + idx[:, c]
    return key


def join(a, b, base):
    """The product of two sparse arrays over their shared labels (a relational join; nothing is summed)."""
    shared = [l for l in a.labels if l in b.labels]
    ka = _key(a.idx, [a.labels.index(l) for l in shared], base)
    kb = _key(b.idx, [b.labels.index(l) for l in shared], base)
    order = np.argsort(kb, kind="stable")
    kb = kb[order]
    lo, hi = np.searchsorted(kb, ka, side="left"), np.searchsorted(kb, ka, side="right")
    n = hi - lo
    ia = np.repeat(np.arange(len(ka)), n)
    ib = order[np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(lo, n)]
    rest = [c for c, l in enumerate(b.labels) if l not in shared]
    return Coo(a.labels + "".join(b.labels[c] for c in rest), np.hstack([a.idx[ia], b.idx[ib][:, rest]]), a.val[ia] * b.val[ib])


def sparse_einsum(spec, operands, base):
    """einsum of sparse operands into a sparse result (labels of the output in its order)."""
    ins, out = spec.split("->")
    todo = [Coo(l, o.idx, o.val) for l, o in zip(ins.split(","), operands)]
    todo.sort(key=lambda o: len(o.val))
    cur = todo.pop(0)
    while todo:
        nxt = max(todo, key=lambda o: (len(set(o.labels) & set(cur.labels)), -len(o.val)))
        todo.remove(nxt)
        needed = set(out) | set("".join(o.labels for o in todo))
        cur = join(cur, nxt, base).sum_out(needed, base)
    cur = cur.sum_out(set(out), base)
    return Coo(out, cur.idx[:, [cur.labels.index(l) for l in out]], cur.val)


# ---- the blocks of the term tables from the sector data ------------------------------------------------------------------
def triples_lists(tt, V):
    """The four implied-index lists from a dense V (what UEG.eval_2b_triples(..., both_sides=True) holds)."""
    Vv, Vo = tr.triples_integrals(tt, V)
    VvR, VoR = sl.right_integrals(tt, V)
    return dict(Vv=Vv, Vo=Vo, VvR=VvR, VoR=VoR)


def blocks(tab, tt, ints, lists, ladder=None):
    """name -> Coo [4 labels "pqrs"] of every block the term tables read, indices local to the block (virtuals from 0), from
    the sector families `ints`, the implied-index `lists` and, for the V_abcd at pair momenta without a pp sector, `ladder`
    (a list of (pqrs, values) pairs, one per EA target; absent: those elements are not needed or not given)."""
    no, nv, k = tab.no, tab.nv, tab.k_int
    shift = {"o": 0, "v": no}

    def family(name, kinds):
        pqrs = tab.block_pqrs(name).astype(np.int64) - np.array([shift[c] for c in kinds])
        return pqrs, np.asarray(ints[name], dtype=np.float64)

    out = {}
    for name, fam, kinds, perm in (("klij", "klij", "oooo", (0, 1, 2, 3)), ("ijab", "klcd", "oovv", (0, 1, 2, 3)),
                                   ("iajb", "wa", "ovov", (0, 1, 2, 3)), ("iabj", "w2", "ovvo", (0, 1, 2, 3))):
        pqrs, val = family(fam, kinds)
        out[name] = Coo("pqrs", pqrs[:, perm], val)
    pqrs, val = family("abcd", "vvvv")
    if ladder:
        extra = np.concatenate([p.astype(np.int64) - no for p, _ in ladder])
        pqrs, val = np.concatenate([pqrs, extra]), np.concatenate([val] + [np.asarray(x, dtype=np.float64) for _, x in ladder])
        pqrs, first = np.unique(pqrs, axis=0, return_index=True)
        val = val[first]
    out["abcd"] = Coo("pqrs", pqrs, val)
    # Vo[x,y,a] = V[x,y,a,m],  VoR[x,y,a] = V[a,m,x,y]
    x, y, a = np.nonzero(tt.m_of >= 0)
    m = tt.m_of[x, y, a].astype(np.int64)
    vo, vor = lists["Vo"][x, y, a], lists["VoR"][x, y, a]
    out["ijak"] = Coo("pqrs", np.stack([x, y, a, m], axis=1), vo)
    out["ijka"] = Coo("pqrs", np.stack([y, x, m, a], axis=1), vo)               # V[y,x,m,a] = V[x,y,a,m]
    out["iajk"] = Coo("pqrs", np.stack([m, a, y, x], axis=1), vor)              # V[m,a,y,x] = V[a,m,x,y]
    # Vv[i,a,b] = V[i,f,a,b],  VvR[i,a,b] = V[a,b,i,f]
    i, a, b = np.meshgrid(np.arange(no), np.arange(nv), np.arange(nv), indexing="ij")
    f = tt.lookup(k[no + a] + k[no + b] - k[i]) - no
    ok = f >= 0
    i, a, b, f = i[ok], a[ok], b[ok], f[ok]
    out["iabc"] = Coo("pqrs", np.stack([i, f, a, b], axis=1), lists["Vv"][i, a, b])
    out["abic"] = Coo("pqrs", np.stack([a, b, i, f], axis=1), lists["VvR"][i, a, b])
    return out


def amplitudes(tab, T):
    a, b, i, j = tab.abij()
    return Coo("abij", np.stack([a, b, i, j], axis=1), T)


def tables(tt, kind, target):
    return QuasiparticleTables(tt, kind, target)


def sigma(qt, eps, blk, T, r1, R):
    """(s1 [k], S [k, nx, no]) of the k stacked vectors (r1 [k], R [k, nx, no]) of the block of `qt`: every term of the tables
    of tests/_ipea_reference.py.  Returns also `leak`, the largest element a term puts outside the block (exactly 0)."""
    tab, kind, p = qt.tables, qt.kind, qt.target
    no, nv = tab.no, tab.nv
    r1, R = np.atleast_1d(np.asarray(r1, dtype=np.float64)), np.asarray(R, dtype=np.float64).reshape((-1,) + qt.shape)
    nk = len(r1)
    eps = np.asarray(eps, dtype=np.float64)
    z = np.arange(nk)
    pl = p if kind == "ip" else p - no
    pos = np.flatnonzero(qt.inside)
    x, y, b = pos // no, pos % no, qt.b_of[pos].astype(np.int64)
    zz, xx, yy, bb = np.repeat(z, len(pos)), np.tile(x, nk), np.tile(y, nk), np.tile(b, nk)
    vals = R.reshape(nk, -1)[:, pos].reshape(-1)
    second = np.stack([zz, xx, yy, bb] if kind == "ip" else [zz, xx, bb, yy], axis=1)       # r2[i,j,b] / r2[a,b,j]
    env = dict(blk)
    env.update(t=amplitudes(tab, T), r1=Coo("zi", np.stack([z, np.full(nk, pl)], axis=1), r1), r2=Coo("zijb", second, vals),
               foo=Coo("pq", np.stack([np.arange(no)] * 2, axis=1), eps[:no]),
               fvv=Coo("pq", np.stack([np.arange(nv)] * 2, axis=1), eps[no:]), fov=Coo("pq", np.zeros((0, 2)), np.zeros(0)))
    n1, shape2 = ip.shapes(kind, no, nv)
    s1, s2 = np.zeros((nk,) + n1), np.zeros((nk,) + shape2)
    for table, acc in zip(ip.TABLES[kind], (s1, s2)):
        for c, spec, names in table:
            ins, out = spec.split("->")
            parts = ins.split(",")
            parts[-1] = "Z" + parts[-1]                          # the vector index rides along with r1 / r2
            term = sparse_einsum(",".join(parts) + "->Z" + out, [env[n] for n in names], tab.n + nk)
            np.add.at(acc, tuple(term.idx.T), c * term.val)
    # what is inside the block, and the leak
    if kind == "ip":
        S = s2[:, x, y, b]
        s2[:, x, y, b] = 0.0
    else:
        S = s2[:, x, b, y]
        s2[:, x, b, y] = 0.0
    got1 = s1[:, pl].copy()
    s1[:, pl] = 0.0
    out = np.zeros((nk, qt.npos))
    out[:, pos] = S
    return got1, out.reshape((nk,) + qt.shape), max(np.abs(s1).max(), np.abs(s2).max())


def matrix(qt, eps, blk, T):
    """The block as a matrix over [r1 | R row-major], zero rows and columns at the positions outside the space."""
    n = 1 + qt.npos
    eye = np.eye(n)
    s1, S, leak = sigma(qt, eps, blk, T, eye[:, 0], eye[:, 1:])
    assert leak == 0.0
    return np.hstack([s1[:, None], S.reshape(n, -1)]).T


def diagonals(qt, eps, ints, T):
    """(d1, d2 [nx, no], L [n], m1, m2 [nx, no], mL [n]): d1 = -L_pp / L_pp, d2 = L_b* - L_i - L_j / L_a + L_b* - L_j with the L
    of tests/_ipea_reference.diagonals, L_oo[i] = eps_i + sum_a s[a,i], L_vv[a] = eps_a - sum_i s[a,i], s the row sums of
    (2 D - C) o W1 in the direct layout; the positions outside the space hold QuasiparticleTables.OUTSIDE.  The implied
    virtual of a position is found here by comparing momenta with every virtual, not through the tables' b_of.  m1, m2, mL are
    the sums of the magnitudes of all terms that enter an element (|eps| and every |product|): what a bound in ulps has to
    refer to, since eps of either sign and signed products cancel in L, and three L in d2."""
    tab = qt.tables
    no, nv, k = tab.no, tab.nv, tab.k_int
    eps = np.asarray(eps, dtype=np.float64)
    D, Cx = T[tab.d_from_pp], T[tab.c_from_pp]
    prod = (2.0 * D - Cx) * np.asarray(ints["w1"])
    rows = np.array([prod[s:s + n].sum() for s, n in zip(tab.row_start, tab.row_len)])
    mags = np.array([np.abs(prod[s:s + n]).sum() for s, n in zip(tab.row_start, tab.row_len)])
    s_ai, m_ai = rows[tab.ph_row].reshape(nv, no), mags[tab.ph_row].reshape(nv, no)
    L = np.concatenate([eps[:no] + s_ai.sum(axis=0), eps[no:] - s_ai.sum(axis=1)])
    mL = np.concatenate([np.abs(eps[:no]) + m_ai.sum(axis=0), np.abs(eps[no:]) + m_ai.sum(axis=1)])
    x, y = np.divmod(np.arange(qt.npos), no)
    p = qt.target
    want_k = k[x] + k[y] - k[p] if qt.kind == "ip" else k[p] + k[y] - k[no + x]
    hit = (want_k[:, None, :] == k[None, no:, :]).all(axis=2)                  # [position, virtual]
    inside, b = hit.any(axis=1), hit.argmax(axis=1)
    if qt.kind == "ip":
        d1, d2, m2 = -L[p], L[no + b] - L[x] - L[y], mL[no + b] + mL[x] + mL[y]
    else:
        d1, d2, m2 = L[p], L[no + x] + L[no + b] - L[y], mL[no + x] + mL[no + b] + mL[y]
    return (d1, np.where(inside, d2, qt.OUTSIDE).reshape(qt.shape), L, mL[p], np.where(inside, m2, 0.0).reshape(qt.shape), mL)
