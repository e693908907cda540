"""Momentum-sector tables of a closed-shell Hamiltonian whose orbitals carry a conserved integer vector (the electron gas,
with or without twist).  Host side, numpy only.

Every integral and amplitude conserves the vector: V_pqrs != 0 only if k_p + k_q = k_r + k_s, and T_abij only if
k_a + k_b = k_i + k_j.  The same ~ o^2 v non-zeros of T are held in three block-diagonal layouts:

  pp       one sector per P in {k_i + k_j}: T^P[(a,b),(i,j)] = T_abij, rows VV_P (ordered virtual pairs with k_a + k_b = P),
           columns OO_P, row-major; the sectors concatenated are the canonical compact amplitude vector
  direct   one sector per q in {k_a - k_i}: D^q[(a,i),(b,j)] = T_abij, rows PH_q, columns PH_{-q}
  crossed  C^q[(a,j),(b,i)] = T_abij, the same row and column lists (read as [(a,i),(b,j)] it is T_baij)

A sector without virtual pairs (or a q whose -q does not occur: twisted bases) is legal and empty.  The integral blocks
each product reads are described by `BLOCKS`; `block_pqrs` lists their (p,q,r,s) sector by sector.  `gemm_tasks` writes the
task table of one sector-batched product (include/pymes_amd.h, pymes_sector_gemm)."""
import numpy as np

# name -> (row set, column set, (p,q,r,s) from the row pair (r0,r1) and the column pair (c0,c1); virtuals already
# shifted by no).  Sets: "oo" / "vv" pairs of pp sector P; "ph" = PH_q, "ph-" = PH_{-q} of ph sector q.
BLOCKS = {
    "klij": ("oo", "oo", lambda r0, r1, c0, c1: (r0, r1, c0, c1)),        # I^P[(k,l),(i,j)]
    "klcd": ("oo", "vv", lambda r0, r1, c0, c1: (r0, r1, c0, c1)),        # V_klcd^P[(k,l),(c,d)]
    "abij": ("vv", "oo", lambda r0, r1, c0, c1: (r0, r1, c0, c1)),        # pp layout of V_abij
    "abcd": ("vv", "vv", lambda r0, r1, c0, c1: (r0, r1, c0, c1)),        # the ladder block
    "ed":   ("vv", "oo", lambda r0, r1, c0, c1: (c0, c1, r0, r1)),        # V_ijab at T_abij (direct energy)
    "ex":   ("vv", "oo", lambda r0, r1, c0, c1: (c0, c1, r1, r0)),        # V_ijba at T_abij (exchange energy)
    "w1":   ("ph", "ph-", lambda c, k, d, l: (k, l, c, d)),               # W1^q[(c,k),(d,l)] = V_klcd
    "wx":   ("ph", "ph-", lambda d, k, c, l: (k, l, c, d)),               # Wx^q[(d,k),(c,l)] = V_klcd
    "wa":   ("ph", "ph", lambda a, i, c, k: (k, a, i, c)),                # Wa^q[(a,i),(c,k)] = V_kaic (Wb = Wa^T)
    "w2":   ("ph", "ph", lambda c, k, b, j: (k, b, c, j)),                # W2^q[(c,k),(b,j)] = V_kbcj
}
FOCK_LISTS = ("pipi", "piip")       # diagonal of hf.construct_hf_matrix: f_pp = h_pp + sum_i (2 V_pipi - V_piip)


def _expand(nr, nc, s0, s1):
    """Sector, local row and local column of every element of the row-major blocks nr[s] x nc[s], s0 <= s < s1."""
    size = nr[s0:s1] * nc[s0:s1]
    sec = np.repeat(np.arange(s0, s1), size)
    start = np.concatenate(([0], np.cumsum(size)))[:-1]
    local = np.arange(int(size.sum())) - np.repeat(start, size)
    w = np.maximum(nc[sec], 1)
    return sec, local // w, local % w


class SectorTables:
    def __init__(self, k_int, no):
        k = np.ascontiguousarray(k_int, dtype=np.int64)
        if k.ndim != 2 or k.shape[1] != 3:
            raise ValueError("SectorTables: k_int must be [n, 3] integers")
        n, no = k.shape[0], int(no)
        if not 0 < no < n:
            raise ValueError("SectorTables: need 0 < no < n")
        if len(np.unique(k, axis=0)) != n:
            raise ValueError("SectorTables: two orbitals carry the same vector")
        self.k_int, self.no, self.nv, self.n = k, no, n - no, n
        nv = self.nv
        bound = 2 * int(np.abs(k).max()) + 1
        side = 2 * bound + 1

        def key(v):
            return ((v[..., 0] + bound) * side + v[..., 1] + bound) * side + v[..., 2] + bound

        def unkey(x):
            return np.stack([x // (side * side) - bound, x // side % side - bound, x % side - bound], axis=-1)

        ko, kv = k[:no], k[no:]
        # ---- pp sectors: P in {k_i + k_j}
        oo_key = key(ko[:, None, :] + ko[None, :, :]).reshape(-1)
        self.P_keys = np.unique(oo_key)
        self.P = unkey(self.P_keys)
        nP = len(self.P_keys)
        self.oo_pairs, self.oo_off, self.oo_sec, self.oo_pos = self._group(oo_key, no, nP)
        self.vv_pairs, self.vv_off, self.vv_sec, self.vv_pos = self._group(key(kv[:, None, :] + kv[None, :, :]).reshape(-1), nv, nP)
        self.n_oo, self.n_vv = np.diff(self.oo_off), np.diff(self.vv_off)
        # ---- ph sectors: q in {k_a - k_i}
        ph_key = key(kv[:, None, :] - ko[None, :, :]).reshape(-1)
        self.q_keys = np.unique(ph_key)
        self.q = unkey(self.q_keys)
        nq = len(self.q_keys)
        sec = np.searchsorted(self.q_keys, ph_key)
        order = np.argsort(sec, kind="stable")
        self.ph_pairs = np.stack([order // no, order % no], axis=1)             # (a, i), a counted from the first virtual
        self.ph_off = np.concatenate(([0], np.cumsum(np.bincount(sec, minlength=nq))))
        self.ph_row = np.empty(nv * no, dtype=np.int64)                          # (a, i) -> global row
        self.ph_row[order] = np.arange(nv * no)
        neg_key = key(-self.q)
        pos = np.minimum(np.searchsorted(self.q_keys, neg_key), nq - 1)
        self.neg = np.where(self.q_keys[pos] == neg_key, pos, -1)               # sector of -q, -1: it does not occur
        self.n_ph = np.diff(self.ph_off)
        self.n_hp = np.where(self.neg >= 0, self.n_ph[np.maximum(self.neg, 0)], 0)     # |PH_{-q}|
        # ---- element offsets of the block families
        self._sizes = {"oo": self.n_oo, "vv": self.n_vv, "ph": self.n_ph, "ph-": self.n_hp}
        self._off = {}
        self.pp_off = self.offsets("vv", "oo")
        self.nnz = int(self.pp_off[-1])
        self._maps()

    def _group(self, pair_key, m, nP):
        """Ordered pairs (x, y), x, y < m, grouped by the pp sector their key belongs to (pairs of other keys dropped)."""
        pos = np.minimum(np.searchsorted(self.P_keys, pair_key), nP - 1)
        sec = np.where(self.P_keys[pos] == pair_key, pos, -1)
        keep = np.flatnonzero(sec >= 0)
        order = keep[np.argsort(sec[keep], kind="stable")]
        off = np.concatenate(([0], np.cumsum(np.bincount(sec[keep], minlength=nP))))
        where = np.full(m * m, -1, dtype=np.int64)
        where[order] = np.arange(len(order)) - off[sec[order]]
        return np.stack([order // m, order % m], axis=1), off, sec, where

    def offsets(self, rows, cols):
        """Element offsets (len = sectors + 1) of the concatenated row-major blocks |rows_s| x |cols_s|."""
        if (rows, cols) not in self._off:
            self._off[rows, cols] = np.concatenate(([0], np.cumsum(self._sizes[rows] * self._sizes[cols]))).astype(np.int64)
        return self._off[rows, cols]

    def _pairs(self, kind, sec, local):
        if kind == "oo":
            return self.oo_pairs[self.oo_off[sec] + local]
        if kind == "vv":
            return self.vv_pairs[self.vv_off[sec] + local]
        if kind == "ph-":
            sec = self.neg[sec]
        return self.ph_pairs[self.ph_off[sec] + local]

    def _pp_index(self, a, b, i, j):
        ab, ij = a * self.nv + b, i * self.no + j
        sec = self.oo_sec[ij]
        assert np.array_equal(sec, self.vv_sec[ab])
        return self.pp_off[sec] + self.vv_pos[ab] * self.n_oo[sec] + self.oo_pos[ij]

    def _maps(self):
        """The gather maps between the layouts (int64, one entry per non-zero)."""
        nq = len(self.q_keys)
        self.d_off = self.offsets("ph", "ph-")
        sec, lr, lc = _expand(self.n_ph, self.n_hp, 0, nq)
        if len(sec) != self.nnz:
            raise AssertionError("sector layouts disagree: pp holds %d elements, ph %d" % (self.nnz, len(sec)))
        row, col = self._pairs("ph", sec, lr), self._pairs("ph-", sec, lc)
        self.d_from_pp = self._pp_index(row[:, 0], col[:, 0], row[:, 1], col[:, 1])       # D^q[(a,i),(b,j)] = T_abij
        self.c_from_pp = self._pp_index(row[:, 0], col[:, 0], col[:, 1], row[:, 1])       # C^q[(a,j),(b,i)] = T_abij
        partner = self.d_off[self.neg[sec]] + lc * self.n_ph[sec] + lr                     # block -q, transposed
        self.d_partner = partner
        self.pp_to_d, self.pp_to_c = self._inverse(self.d_from_pp), self._inverse(self.c_from_pp)
        self.pp_to_dT, self.pp_to_cT = partner[self.pp_to_d], partner[self.pp_to_c]       # Ex^T(1,0,3,2) at each pp element
        a, b, i, j = self.abij()
        self.pp_swap = self._pp_index(b, a, j, i)                                          # T_baji at each pp element
        # rows of the direct layout: where each starts, how long it is, which (a, i) it belongs to
        g = np.arange(self.nv * self.no)
        s = np.searchsorted(self.ph_off, g, side="right") - 1
        self.row_start = self.d_off[s] + (g - self.ph_off[s]) * self.n_hp[s]
        self.row_len = self.n_hp[s].astype(np.int64)

    def _inverse(self, perm):
        inv = np.full(self.nnz, -1, dtype=np.int64)
        inv[perm] = np.arange(self.nnz)
        if len(perm) != self.nnz or (inv < 0).any():
            raise AssertionError("sector layouts are not permutations of one another")
        return inv

    def abij(self):
        """(a, b, i, j) of every element of the compact vector (a, b counted from the first virtual)."""
        sec, lr, lc = _expand(self.n_vv, self.n_oo, 0, len(self.P_keys))
        ab, ij = self._pairs("vv", sec, lr), self._pairs("oo", sec, lc)
        return ab[:, 0], ab[:, 1], ij[:, 0], ij[:, 1]

    # ---- integrals ---------------------------------------------------------------------------------------------
    def n_sectors(self, name):
        return len(self.P_keys) if BLOCKS[name][0] in ("oo", "vv") else len(self.q_keys)

    def block_offsets(self, name):
        return self.offsets(*BLOCKS[name][:2])

    def block_pqrs(self, name, s0=0, s1=None):
        """(p,q,r,s) (int32 [count, 4]) of the elements of block family `name`, sectors s0 <= s < s1, in storage order."""
        if name in FOCK_LISTS:
            p, i = np.repeat(np.arange(self.n), self.no), np.tile(np.arange(self.no), self.n)
            return np.stack([p, i, p, i] if name == "pipi" else [p, i, i, p], axis=1).astype(np.int32)
        rows, cols, spec = BLOCKS[name]
        s1 = self.n_sectors(name) if s1 is None else s1
        sec, lr, lc = _expand(self._sizes[rows], self._sizes[cols], s0, s1)
        r, c = self._pairs(rows, sec, lr), self._pairs(cols, sec, lc)
        shift = lambda kind: self.no if kind == "vv" else 0
        if rows.startswith("ph"):
            idx = spec(r[:, 0] + self.no, r[:, 1], c[:, 0] + self.no, c[:, 1])
        else:
            idx = spec(r[:, 0] + shift(rows), r[:, 1] + shift(rows), c[:, 0] + shift(cols), c[:, 1] + shift(cols))
        return np.stack(idx, axis=1).astype(np.int32)

    def ladder_rows(self):
        """What the direct ladder (include/pymes_amd.h, pymes_sector_ladder_direct) reads in place of the ``abcd`` lists: the vv
        pair list as absolute orbital indices (int32 [rows, 2], the order of ``vv_pairs``) and the first row of every pp
        sector in it (int64, one per sector).  Element (r, c) of ``abcd`` sector s is <pq|rs> with (p,q) = rows[first[s] + r]
        and (r,s) = rows[first[s] + c]."""
        return (self.vv_pairs + self.no).astype(np.int32), self.vv_off[:-1].astype(np.int64)

    def conserving(self, pqrs):
        k = self.k_int
        return np.all(k[pqrs[:, 0]] + k[pqrs[:, 1]] == k[pqrs[:, 2]] + k[pqrs[:, 3]], axis=1)

    # ---- amplitudes --------------------------------------------------------------------------------------------
    def compact(self, dense, name="T2"):
        """The compact vector of a dense [v,v,o,o] array; weight outside the support is refused."""
        dense = np.asarray(dense)
        if dense.shape != (self.nv, self.nv, self.no, self.no):
            raise ValueError("%s: expected a [v,v,o,o] array of shape %s" % (name, ((self.nv,) * 2 + (self.no,) * 2,)))
        idx = self.abij()
        out = np.ascontiguousarray(dense[idx], dtype=np.float64)
        if np.count_nonzero(dense) != np.count_nonzero(out):
            raise ValueError("%s has weight outside the momentum-conserving support" % name)
        return out

    def to_dense(self, vec):
        out = np.zeros((self.nv, self.nv, self.no, self.no))
        out[self.abij()] = vec
        return out

    def denominators(self, eps):
        """e_i + e_j - e_a - e_b at every element of the compact vector (eps: all n orbital energies)."""
        a, b, i, j = self.abij()
        eps = np.asarray(eps, dtype=np.float64)
        return eps[i] + eps[j] - eps[self.no + a] - eps[self.no + b]

    # ---- products ----------------------------------------------------------------------------------------------
    def gemm_tasks(self, a, b, c, alpha=1.0, beta=0.0, trans_b=False, trans_a=False):
        """Task table of C^s = alpha A^s' B^s'' + beta C^s over all sectors.  a, b, c = (rows, cols, negated): the block
        family of the operand as stored (before `trans_a` / `trans_b`), and whether the operand of sector q is block -q."""
        nsec = len(self.P_keys) if a[0] in ("oo", "vv") else len(self.q_keys)
        ident = np.arange(nsec)

        def view(op):
            rows, cols, negated = op
            src = self.neg if negated else ident
            flip = {"ph": "ph-", "ph-": "ph"}
            if negated:       # block -q of a family (rows, cols) has the sizes of (flip rows, flip cols) at q
                rows, cols = flip[rows], flip[cols]
            off = np.where(src >= 0, self.offsets(*op[:2])[np.maximum(src, 0)], 0)
            return self._sizes[rows], self._sizes[cols], off

        ar, ac, ao = view(a)
        br, bc, bo = view(b)
        cr, cc, co = view(c)
        lda, ldb = ac, bc
        if trans_a:
            ar, ac = ac, ar
        if trans_b:
            br, bc = bc, br
        if not (np.array_equal(ar, cr) and np.array_equal(bc, cc) and np.array_equal(ac, br)):
            raise AssertionError("gemm_tasks: the operand shapes do not chain")
        return make_tasks(ar, bc, ac, ao, bo, co, lda, ldb, cc, alpha, beta, trans_a=trans_a, trans_b=trans_b)


class TriplesTables:
    """The implied-index tables of the momentum-blocked (T), from a `SectorTables`.  Host side, numpy only.

    With k_p + k_q = k_r + k_s every sum of w_ijk[a,b,c] = sum_f V_iabc[i,f,a,b] T[c,f,k,j] - sum_m V_ijak[i,j,a,m] T[b,c,m,k]
    has at most one term, so each operand is held with its implied index left out:

      Vv[i,a,b] = V[i, f*, a, b]   f* the virtual with k_a + k_b - k_i        list family "vv", shape [o,v,v]
      Vo[i,j,a] = V[i, j, a, m*]   m* the occupied with k_i + k_j - k_a       list family "vo", shape [o,o,v]; m_of = m*
      Tc[i,j,a] = T[a, b*, i, j]   b* the virtual with k_i + k_j - k_a        `implied_map` into the compact pp vector

    Lambda-(T) also reads the excitation-type integrals with the same implied orbitals:

      VvR[i,a,b] = V[a, b, i, f*]                                              list family "vv_r", shape [o,v,v]
      VoR[i,j,a] = V[a, m*, i, j]                                              list family "vo_r", shape [o,o,v]

    A position whose implied orbital does not exist holds an exact 0 (in m_of: -1).  `orb_of` is the dense lookup grid
    vector -> orbital over the box [lo, lo + dims) of the orbitals' own vectors, -1 where no orbital sits; a vector outside
    the box names no orbital and is never wrapped into it (`lookup` checks every axis)."""

    FAMILIES = ("vv", "vo")
    RIGHT_FAMILIES = ("vv_r", "vo_r")       # the same positions and implied orbitals, V with bra and ket exchanged

    def __init__(self, tables):
        if not isinstance(tables, SectorTables):
            raise TypeError("TriplesTables: a SectorTables is needed")
        self.tables = tables
        k, no, nv = tables.k_int, tables.no, tables.nv
        self.no, self.nv, self.n = no, nv, tables.n
        self.lo = k.min(axis=0).astype(np.int64)
        self.dims = (k.max(axis=0) - self.lo + 1).astype(np.int64)
        if int(np.prod(self.dims)) > 0x7fffffff:
            raise ValueError("TriplesTables: the box of the orbital vectors holds more than 2^31 points")
        self.orb_of = np.full(tuple(self.dims), -1, dtype=np.int32)
        rel = k - self.lo
        self.orb_of[rel[:, 0], rel[:, 1], rel[:, 2]] = np.arange(tables.n, dtype=np.int32)
        self.box = np.concatenate((self.lo, self.dims)).astype(np.int32)         # what the kernel takes: lo[3], dims[3]
        ko, kv = k[:no], k[no:]
        m = self.lookup(ko[:, None, None, :] + ko[None, :, None, :] - kv[None, None, :, :])
        self.m_of = np.where(m < no, m, -1).astype(np.int32)                      # [o,o,v]: occupied or -1
        b = self.b_of = np.where(m >= no, m - no, -1)                             # [o,o,v]: b* counted from the first virtual
        ok = b >= 0
        i, j, a = np.nonzero(ok)
        self.implied_map = np.full((no, no, nv), tables.nnz, dtype=np.int64)      # invalid: the appended zero slot
        self.implied_map[ok] = tables._pp_index(a, b[ok], i, j)
        self.sizes = {"vv": no * nv * nv, "vo": no * no * nv}

    def lookup(self, vec):
        """Orbital index of every integer vector of `vec` [..., 3], -1 where there is none (outside the box included)."""
        rel = np.asarray(vec, dtype=np.int64) - self.lo
        inside = np.all((rel >= 0) & (rel < self.dims), axis=-1)
        rel = np.where(inside[..., None], rel, 0)
        return np.where(inside, self.orb_of[rel[..., 0], rel[..., 1], rel[..., 2]], -1).astype(np.int64)

    def list_pqrs(self, family, e0=0, e1=None):
        """((p,q,r,s) int32 [count, 4], valid bool [count]) of the positions e0 <= e < e1 of list family "vv" or "vo" (or
        their right-hand partners "vv_r", "vo_r": (r,s,p,q) of the same position) in storage order.  Where `valid` is False the implied orbital does not exist: the row then names orbital 0 in its place
        and must not be evaluated (the stored value there is an exact 0)."""
        no, nv, k = self.no, self.nv, self.tables.k_int
        if family in self.RIGHT_FAMILIES:
            pqrs, valid = self.list_pqrs(family[:2], e0, e1)
            return np.ascontiguousarray(pqrs[:, [2, 3, 0, 1]]), valid
        e1 = self.sizes[family] if e1 is None else e1
        e = np.arange(e0, e1, dtype=np.int64)
        if family == "vv":                      # Vv[i,a,b] = V[i, f*, a, b]
            i, a, b = e // (nv * nv), e // nv % nv + no, e % nv + no
            f = self.lookup(k[a] + k[b] - k[i])
            valid = f >= no
            idx = (i, np.where(valid, f, 0), a, b)
        elif family == "vo":                    # Vo[i,j,a] = V[i, j, a, m*]
            i, j, a = e // (no * nv), e // nv % no, e % nv + no
            m = self.lookup(k[i] + k[j] - k[a])
            valid = (m >= 0) & (m < no)
            idx = (i, j, a, np.where(valid, m, 0))
        else:
            raise KeyError(family)
        return np.stack(idx, axis=1).astype(np.int32), valid

    def implied(self, T):
        """Tc [o,o,v] of a compact pp vector."""
        T = np.asarray(T, dtype=np.float64)
        if T.shape != (self.tables.nnz,):
            raise ValueError("TriplesTables.implied: a compact vector of %d elements is needed" % self.tables.nnz)
        return np.append(T, 0.0)[self.implied_map]


class QuasiparticleTables:
    """The tables of one momentum block of the sector IP- / EA-EOM-CCD operator, from a `TriplesTables`.  Host side,
    numpy only.

    H-bar conserves the momentum, so the operator is block diagonal in the momentum of the removed (IP: -k_p, `target` p
    occupied) or added (EA: +k_p, p virtual, counted over all n) electron.  A block is the singles element r1[p] and the doubles
    with their implied index left out:

      IP   R[i,j] = r2[i, j, b*], shape [o,o], b* the virtual with k_i + k_j - k_p
      EA   R[a,j] = r2[a, b*, j], shape [v,o], b* the virtual with k_p + k_j - k_a

    A position (x,y) whose implied orbital does not exist is not part of the space (`b_of` = -1 there, every map below too).
    With `count` = dim - 1 positions inside:

      b_of       b* counted from the first virtual (int32)
      partner    the position of the exchanged element: IP (j,i), EA (b*,j)   (r2[j,i,b] resp. r2[b,a,j]; an involution)
      ph         position -> [0, count): row x of R is a vector over PH_q, q = k_x - k_p (IP) / k_p - k_x (EA), its element
                 (b*, y); the rows follow each other, each in the order of PH_q
      ph_partner ph[partner]
      pair       position -> [0, count): IP the element (i,j) of OO_P, the pair sectors P with a b* one after the other; EA the
                 element (a,b*) of VV_P, P = k_p + k_j, column after column of R

    All four maps are bijections of the space.  `tasks(k)` writes the task tables of the products of one apply for k stacked
    vectors, every operand in the views above with the vector index running fastest ([count, k])."""

    KINDS = ("ip", "ea")
    # the preconditioner's diagonal at a position outside the space: far below every eigenvalue, so that w - d + shift of the
    # Davidson correction is positive there and (s - w r) / (w - d + shift) = +0.0 / 1e30 stays an exact +0.0
    OUTSIDE = -1.0e30

    def __init__(self, ttab, kind, target):
        if not isinstance(ttab, TriplesTables):
            raise TypeError("QuasiparticleTables: a TriplesTables is needed")
        if kind not in self.KINDS:
            raise ValueError("QuasiparticleTables: kind must be 'ip' or 'ea'")
        tab = ttab.tables
        no, nv, n, k = tab.no, tab.nv, tab.n, tab.k_int
        p = int(target)
        if kind == "ip" and not 0 <= p < no:
            raise ValueError("QuasiparticleTables: the IP target %d is not an occupied orbital (0 <= p < %d)" % (p, no))
        if kind == "ea" and not no <= p < n:
            raise ValueError("QuasiparticleTables: the EA target %d is not a virtual orbital (%d <= p < %d)" % (p, no, n))
        self.ttab, self.tables, self.kind, self.target = ttab, tab, kind, p
        nx = no if kind == "ip" else nv
        self.shape, self.npos = (nx, no), nx * no
        x, y = np.repeat(np.arange(nx), no), np.tile(np.arange(no), nx)
        orb = ttab.lookup(k[x] + k[y] - k[p] if kind == "ip" else k[p] + k[y] - k[no + x])
        b = np.where(orb >= no, orb - no, -1)
        inside = b >= 0
        self.b_of, self.inside, self.count = b.astype(np.int32), inside, int(inside.sum())
        self.dim = self.count + 1
        pos = np.flatnonzero(inside)
        xi, yi, bi = x[pos], y[pos], b[pos]
        self.partner = np.full(self.npos, -1, dtype=np.int64)
        self.partner[pos] = yi * no + xi if kind == "ip" else bi * no + yi
        # rows of R as vectors over PH_q: the element (b*, y) of the sector it lies in
        g = tab.ph_row[bi * no + yi]
        sec = np.searchsorted(tab.ph_off, g, side="right") - 1
        self.row_sec = np.full(nx, -1, dtype=np.int64)
        self.row_sec[xi] = sec
        if not np.array_equal(self.row_sec[xi], sec):
            raise AssertionError("QuasiparticleTables: a row of R spans two ph sectors")
        self.row_len = np.where(self.row_sec >= 0, tab.n_ph[np.maximum(self.row_sec, 0)], 0)
        self.row_off = np.concatenate(([0], np.cumsum(self.row_len))).astype(np.int64)
        self.ph = np.full(self.npos, -1, dtype=np.int64)
        self.ph[pos] = self.row_off[xi] + g - tab.ph_off[sec]
        self.ph_partner = np.full(self.npos, -1, dtype=np.int64)
        self.ph_partner[pos] = self.ph[self.partner[pos]]
        # the pair view: OO_P of the sectors with a b* (IP), VV_P of P = k_p + k_j column by column (EA)
        self.pair = np.full(self.npos, -1, dtype=np.int64)
        if kind == "ip":
            sec = tab.oo_sec[pos]                                   # (position i no + j is the pair index of oo_sec)
            self.pair_sec = np.unique(sec)
            self.pair_len = tab.n_oo[self.pair_sec]
            self.pair_off = np.concatenate(([0], np.cumsum(self.pair_len))).astype(np.int64)
            self.pair[pos] = self.pair_off[np.searchsorted(self.pair_sec, sec)] + tab.oo_pos[pos]
        else:
            # one block per column j, its virtual pairs (a, b*) in ascending a: the order of VV_P where P is a pp sector.  A
            # pair momentum k_p + k_j that is no sum of two occupied momenta has no pp sector (no T, no V_klcd, no stored
            # V_abcd there): its ladder block is the `extra` family, `extra_pqrs` lists it.
            order = np.lexsort((xi, yi))
            self.pair[pos[order]] = np.arange(self.count)
            self.pair_len = np.bincount(yi, minlength=no).astype(np.int64)
            self.pair_off = np.concatenate(([0], np.cumsum(self.pair_len))).astype(np.int64)
            self.pair_a, self.pair_b = xi[order], bi[order]
            ab = xi * nv + bi
            sec = tab.vv_sec[ab]
            self.pair_sec = np.full(no, -1, dtype=np.int64)
            self.pair_sec[yi] = sec
            stored = sec >= 0
            if not np.array_equal(self.pair_sec[yi], sec) or \
                    not np.array_equal(self.pair[pos[stored]], self.pair_off[yi[stored]] + tab.vv_pos[ab[stored]]) or \
                    not np.array_equal(tab.n_vv[sec[stored]], self.pair_len[yi[stored]]):
                raise AssertionError("QuasiparticleTables: a column of R is not the row list of its pp sector")
            self.mid_len = np.where(self.pair_sec >= 0, tab.n_oo[np.maximum(self.pair_sec, 0)], 0)
            self.mid_off = np.concatenate(([0], np.cumsum(self.mid_len))).astype(np.int64)
            self.extra_len = np.where(self.pair_sec < 0, self.pair_len, 0)
            self.extra_off = np.concatenate(([0], np.cumsum(self.extra_len ** 2))).astype(np.int64)
        self.check()

    @property
    def extra_size(self):
        """Elements of the `extra` ladder family (EA): V_abcd at the pair momenta k_p + k_j that are no pp sector."""
        return int(self.extra_off[-1]) if self.kind == "ea" else 0

    def extra_columns(self):
        """The columns j of an EA block whose pair momentum k_p + k_j is no pp sector (and that are not empty)."""
        return np.flatnonzero(self.extra_len) if self.kind == "ea" else np.zeros(0, dtype=np.int64)

    def extra_pqrs(self, column=None):
        """(p,q,r,s) int32 [count, 4] of the `extra` ladder family: per column j without a pp sector the block V[a,b,c,d],
        rows (a,b) and columns (c,d) the column's pairs, row-major, from element `extra_off[j]` on.  `column`: that block
        alone; None: all of them, one after the other."""
        out = [np.zeros((0, 4), dtype=np.int32)]
        for j in (self.extra_columns() if column is None else [int(column)]):
            lo, hi = self.pair_off[j], self.pair_off[j + 1]
            a, b = (self.pair_a[lo:hi] + self.tables.no).astype(np.int32), (self.pair_b[lo:hi] + self.tables.no).astype(np.int32)
            m = hi - lo
            out.append(np.stack([np.repeat(a, m), np.repeat(b, m), np.tile(a, m), np.tile(b, m)], axis=1))
        return np.concatenate(out)

    def check(self):
        """Every map lies in range and is a bijection of the space onto [0, count) (the kernels trust them)."""
        for name in ("ph", "ph_partner", "pair"):
            m = getattr(self, name)
            if (m[~self.inside] != -1).any() or not np.array_equal(np.sort(m[self.inside]), np.arange(self.count)):
                raise AssertionError("QuasiparticleTables: the map '%s' is no bijection of the space" % name)
        q = self.partner[self.inside]
        if (self.partner[~self.inside] != -1).any() or not self.inside[q].all() \
                or not np.array_equal(self.partner[q], np.flatnonzero(self.inside)):
            raise AssertionError("QuasiparticleTables: the exchange partner is no involution of the space")
        if int(self.row_off[-1]) != self.count or int(self.pair_off[-1]) != self.count:
            raise AssertionError("QuasiparticleTables: a view does not hold the space")

    def tasks(self, k):
        """name -> (task table, lengths of A, B, C) of the products of one apply of k stacked vectors:

          ring   G^x = S^q(x) X^x per row x, S a square [(a,i),(d,l)] of ph sector q(x) (PA, PB, MDU), X and G in the ph view;
                 ring_add the same with beta = 1
          IP  hole    H^P = (I^P)^T R^P for the pair sectors with a b*
          EA  ladder  H^j = V_abcd^P R^j, P = k_p + k_j;  quad: M^j = V_klcd^P R^j;  quad_back: H^j += T^P M^j"""
        tab, k = self.tables, int(k)
        if k < 1:
            raise ValueError("QuasiparticleTables.tasks: at least one vector is needed")
        total, nsq = self.count * k, int(tab.offsets("ph", "ph")[-1])
        rows = np.flatnonzero(self.row_sec >= 0)
        rs, rl, ro = self.row_sec[rows], self.row_len[rows], self.row_off[rows] * k
        sq = tab.offsets("ph", "ph")[rs]
        out = {"ring": (make_tasks(rl, k, rl, sq, ro, ro, rl, k, k), nsq, total, total),
               "ring_add": (make_tasks(rl, k, rl, sq, ro, ro, rl, k, k, beta=1.0), nsq, total, total)}
        if self.kind == "ip":
            ps, pl, po = self.pair_sec, self.pair_len, self.pair_off[:-1] * k
            out["hole"] = (make_tasks(pl, k, pl, tab.offsets("oo", "oo")[ps], po, po, pl, k, k, trans_a=True),
                           int(tab.offsets("oo", "oo")[-1]), total, total)
        else:
            cols = np.flatnonzero(self.pair_sec >= 0)
            ps, pl, po = self.pair_sec[cols], self.pair_len[cols], self.pair_off[cols] * k
            ml, mo, mid = self.mid_len[cols], self.mid_off[cols] * k, int(self.mid_off[-1]) * k
            out["ladder"] = (make_tasks(pl, k, pl, tab.offsets("vv", "vv")[ps], po, po, pl, k, k),
                             int(tab.offsets("vv", "vv")[-1]), total, total)
            out["quad"] = (make_tasks(ml, k, pl, tab.offsets("oo", "vv")[ps], po, mo, pl, k, k),
                           int(tab.offsets("oo", "vv")[-1]), total, mid)
            out["quad_back"] = (make_tasks(pl, k, ml, tab.pp_off[ps], mo, po, ml, k, k, beta=1.0), tab.nnz, mid, total)
            cols = np.flatnonzero(self.extra_len)
            pl, po = self.pair_len[cols], self.pair_off[cols] * k
            out["ladder_extra"] = (make_tasks(pl, k, pl, self.extra_off[cols], po, po, pl, k, k), self.extra_size, total, total)
        return out


def square_transpose(tables):
    """The gather map that transposes every block of a ("ph", "ph") family: out[(r,c) of sector q] = in[(c,r) of sector q]."""
    sec, lr, lc = _expand(tables.n_ph, tables.n_ph, 0, len(tables.q_keys))
    return tables.offsets("ph", "ph")[sec] + lc * tables.n_ph[sec] + lr


class TransferBins:
    """The bins of the momentum transfer q = k_r - k_p of an element (p,q,r,s), for the transfer sums and the structure
    factor of the sector densities, from a `SectorTables`.  Host side, numpy only.

      q, neg, zero    the bin vectors (every k_r - k_p over all orbital pairs, sorted by key: closed under negation, also on
                      twisted bases), the bin of -q, the bin of q = 0
      csr[name]       per stored family of `BLOCKS`: (offsets int64 [bins + 1], element indices int64 grouped by bin, each
                      group ascending).  ``abcd`` has none: its sums come from the rows of the pp layout (``pair_rows``)
      oo_count        per bin, the number of occupied pairs (i,j) with k_j - k_i = q
      ip_off, ip_orb  per bin, the orbitals p of the pairs (i occupied, p) with k_i - k_p = q
    """

    STORED = tuple(nm for nm in BLOCKS if nm != "abcd")

    def __init__(self, tables):
        if not isinstance(tables, SectorTables):
            raise TypeError("TransferBins: a SectorTables is needed")
        self.tables = tables
        k, no, n = tables.k_int, tables.no, tables.n
        bound = 2 * int(np.abs(k).max()) + 1
        side = 2 * bound + 1
        self._key = lambda v: ((v[..., 0] + bound) * side + v[..., 1] + bound) * side + v[..., 2] + bound
        diff = self._key(k[None, :, :] - k[:, None, :])                        # [p, r]: k_r - k_p
        self.keys = np.unique(diff)
        x = self.keys
        self.q = np.stack([x // (side * side) - bound, x // side % side - bound, x % side - bound], axis=-1)
        self.nbins = len(x)
        self.neg = np.searchsorted(x, self._key(-self.q))
        if not np.array_equal(x[self.neg], self._key(-self.q)):
            raise AssertionError("TransferBins: the bins are not closed under negation")
        self.zero = int(np.searchsorted(x, self._key(np.zeros(3, dtype=np.int64))))
        self.csr = {}
        for name in self.STORED:
            pqrs = tables.block_pqrs(name)
            self.csr[name] = self._group(np.searchsorted(x, self._key(k[pqrs[:, 2]] - k[pqrs[:, 0]])))
        oo = np.searchsorted(x, diff[:no, :no].reshape(-1))
        self.oo_count = np.bincount(oo, minlength=self.nbins).astype(np.int64)
        ip = np.searchsorted(x, diff[:, :no].reshape(-1))                       # [p, i]: k_i - k_p
        self.ip_off, order = self._group(ip)
        self.ip_orb = order // no

    def _group(self, bins):
        off = np.concatenate(([0], np.cumsum(np.bincount(bins, minlength=self.nbins)))).astype(np.int64)
        return off, np.argsort(bins, kind="stable").astype(np.int64)

    def bin_of(self, vec):
        """The bin of every integer vector of `vec` [..., 3], -1 where it is no bin."""
        key = self._key(np.asarray(vec, dtype=np.int64))
        pos = np.minimum(np.searchsorted(self.keys, key), self.nbins - 1)
        return np.where(self.keys[pos] == key, pos, -1)

    def pair_rows(self):
        """The rows of the pp layout as ``pymes_sector_pair_transfer`` takes them: (vv_pairs int32 [rows,2], row_start int64,
        row_len int64, row_of_pair int64 [nv nv], -1 where a virtual pair has no row)."""
        t = self.tables
        sec = np.repeat(np.arange(len(t.P_keys)), t.n_vv)
        local = np.arange(len(sec)) - t.vv_off[sec]
        row_start = (t.pp_off[sec] + local * t.n_oo[sec]).astype(np.int64)
        row_of_pair = np.full(t.nv * t.nv, -1, dtype=np.int64)
        row_of_pair[t.vv_pairs[:, 0] * t.nv + t.vv_pairs[:, 1]] = np.arange(len(sec))
        return t.vv_pairs.astype(np.int32), row_start, t.n_oo[sec].astype(np.int64), row_of_pair

    def shells(self):
        """(|q|^2 of every shell, ascending; the shell of every bin): the bins grouped for the spherical average."""
        q2 = (self.q * self.q).sum(axis=1)
        values, shell = np.unique(q2, return_inverse=True)
        return values, shell.reshape(-1)

    def reference_terms(self, gamma):
        """Per bin, the part of N (S(q) - 1) that the reference determinant and gamma give at q != 0 (``full_rdm2``):
        -2 #{(i,j): k_j - k_i = q} - sum_{i,p: k_i - k_p = q} gamma_p - sum_{i,p: k_p - k_i = q} gamma_p."""
        which = np.repeat(np.arange(self.nbins), np.diff(self.ip_off))
        g = np.bincount(which, weights=np.asarray(gamma, dtype=np.float64)[self.ip_orb], minlength=self.nbins)
        return -2.0 * self.oo_count - (g + g[self.neg])          # (even in q to the bit: the sum of two terms commutes)


TASK_DTYPE = np.dtype([("m", "<i8"), ("n", "<i8"), ("k", "<i8"), ("a", "<i8"), ("b", "<i8"), ("c", "<i8"), ("lda", "<i8"),
                       ("ldb", "<i8"), ("ldc", "<i8"), ("flags", "<i8"), ("tile0", "<i8"), ("alpha", "<f8"), ("beta", "<f8"),
                       ("reserved", "<i8")])       # pymes_sector_task of include/pymes_amd.h
TILE_M, TILE_N = 32, 16
TRANS_A, TRANS_B = 1, 2


def make_tasks(m, n, k, a, b, c, lda, ldb, ldc, alpha=1.0, beta=0.0, trans_a=False, trans_b=False):
    """pymes_sector_task records (numpy structured array) with the tile prefix filled in; scalars broadcast."""
    m = np.atleast_1d(np.asarray(m, dtype=np.int64))
    t = np.zeros(len(m), dtype=TASK_DTYPE)
    for name, val in (("m", m), ("n", n), ("k", k), ("a", a), ("b", b), ("c", c), ("lda", lda), ("ldb", ldb), ("ldc", ldc),
                      ("alpha", alpha), ("beta", beta)):
        t[name] = val
    t["flags"] = np.asarray(trans_a, dtype=np.int64) * TRANS_A + np.asarray(trans_b, dtype=np.int64) * TRANS_B
    tiles = -(-t["m"] // TILE_M) * -(-t["n"] // TILE_N)
    t["tile0"] = np.concatenate(([0], np.cumsum(tiles)))[:-1]
    return t


def task_tiles(tasks):
    return int((-(-tasks["m"] // TILE_M) * -(-tasks["n"] // TILE_N)).sum())


def check_tasks(tasks, len_a, len_b, len_c):
    """Every element a task reads or writes lies inside its arena (the kernel trusts the table)."""
    t = tasks
    if len(t) == 0:
        return
    if (t["m"] < 0).any() or (t["n"] < 0).any() or (t["k"] < 0).any() or (t["flags"] & ~3).any():
        raise ValueError("sector_gemm: negative extent or unknown flag in the task table")
    ta, tb = (t["flags"] & TRANS_A) != 0, (t["flags"] & TRANS_B) != 0
    live = (t["m"] > 0) & (t["n"] > 0)

    def span(rows, cols, ld, off, on):
        on = on & (rows > 0) & (cols > 0)
        if ((ld < cols) & on).any() or ((off < 0) & on).any():
            raise ValueError("sector_gemm: leading dimension below the row length, or a negative offset")
        return np.where(on, off + (rows - 1) * ld + cols, 0)

    ends = (span(np.where(ta, t["k"], t["m"]), np.where(ta, t["m"], t["k"]), t["lda"], t["a"], live),
            span(np.where(tb, t["n"], t["k"]), np.where(tb, t["k"], t["n"]), t["ldb"], t["b"], live),
            span(t["m"], t["n"], t["ldc"], t["c"], live))
    for end, cap, nm in zip(ends, (len_a, len_b, len_c), "ABC"):
        if end.max() > cap:
            raise ValueError("sector_gemm: a task reaches past the end of operand %s" % nm)
    if task_tiles(t) > 0x7fffffff:
        raise ValueError("sector_gemm: too many tiles for one launch")
