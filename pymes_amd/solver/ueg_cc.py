"""Momentum-blocked closed-shell CCD / DCD for Hamiltonians whose orbitals carry a conserved integer vector (the electron
gas, with or without twist): the loop of ``CCD.solve`` on the ~ o^2 v non-zero amplitudes, never an array of size n^4, v^4
or v^2 o^2.  Singles vanish by the same symmetry, so DCD here is also DCSD.

The tables (``pymes_amd.solver.sectors``) hold the non-zeros in three block-diagonal layouts; every contraction of
ccd.py:164-254 is one launch of the ragged batched product ``pymes_sector_gemm`` over all sectors, the moves between the
layouts are gathers, and the diagonal X_ac / X_ki terms, the update and the energy are element-wise tails (DESIGN "Momentum
sectors"; the numpy restatement the tests compare with is tests/_sector_reference.py).  The dense path (``CCD``, ``CCSD``) is
untouched."""
import ctypes as C
import os
import time

import numpy as np

from pymes_amd import _lib
from pymes_amd import dist as pdist
from pymes_amd.device import Context, DeviceArray
from pymes_amd.log import print_logging_info
from pymes_amd.mixer import diis
from pymes_amd.solver import sectors
from pymes_amd.solver.ccd import quiet_collector
from pymes_amd.solver import ccsd_t
from pymes_amd.solver.sectors import BLOCKS, FOCK_LISTS, SectorTables, TriplesTables

__all__ = ["SectorTables", "SectorIntegrals", "SectorAmplitudes", "SectorCCD", "TriplesTables", "SectorTriplesIntegrals",
           "sector_triples_energy"]


def upload_raw(ctx, host):
    """A host array of any 4- or 8-byte dtype as device bytes (held in a DeviceArray of doubles)."""
    host = np.ascontiguousarray(host)
    if host.nbytes % 8:
        raise ValueError("upload_raw: a whole number of doubles is needed")
    arr = ctx.empty((max(host.nbytes // 8, 1),))
    if host.nbytes:
        ctx.lib.call("pymes_upload", ctx.handle, C.c_void_p(arr.ptr), host.ctypes.data_as(C.c_void_p), host.nbytes)
    return arr


def view(arr, offset, n):
    return DeviceArray(arr.ctx, arr.ptr + 8 * int(offset), (int(n),), owned=False, keepalive=arr)


class Tasks:
    """A task table of ``pymes_sector_gemm`` on the device, checked against the operand lengths before the upload."""

    def __init__(self, ctx, tasks, len_a, len_b, len_c):
        sectors.check_tasks(tasks, len_a, len_b, len_c)
        self.ctx, self.count, self.tiles = ctx, len(tasks), sectors.task_tiles(tasks)
        self.lens = (int(len_a), int(len_b), int(len_c))
        self.dev = upload_raw(ctx, tasks.view(np.int64) if len(tasks) else np.zeros(14, dtype=np.int64))

    def run(self, A, B, Cm):
        if any(x.size < n for x, n in zip((A, B, Cm), self.lens)):
            raise ValueError("sector_gemm: an operand is shorter than the task table was checked for")
        self.ctx.lib.call("pymes_sector_gemm", self.ctx.handle, C.c_void_p(self.dev.ptr), self.count, self.tiles,
                          C.c_void_p(A.ptr), C.c_void_p(B.ptr), C.c_void_p(Cm.ptr))


def gather(ctx, dst, s1, m1, a1=1.0, s2=None, m2=None, a2=0.0, beta=0.0):
    """dst[i] = beta dst[i] + a1 s1[m1[i]] (+ a2 s2[m2[i]])."""
    if dst.size < m1.count or (m2 is not None and m2.count != m1.count):
        raise ValueError("sector_gather: the maps and the destination differ in length")
    ctx.lib.call("pymes_sector_gather", ctx.handle, C.c_void_p(dst.ptr), m1.count, float(beta),
                 float(a1), C.c_void_p(s1.ptr), C.c_void_p(m1.ptr), float(a2), C.c_void_p(s2.ptr if s2 is not None else 0),
                 C.c_void_p(m2.ptr if m2 is not None else 0))


class DeviceTables:
    """The gather maps, row tables and task tables of one ``SectorTables`` in one context (uploaded once, kept with the
    integrals)."""

    def __init__(self, ctx, tab):
        self.ctx, self.tab = ctx, tab

        def imap(host, limit):
            host = np.ascontiguousarray(host, dtype=np.int64)
            if len(host) and (host.min() < 0 or host.max() >= limit):
                raise AssertionError("sector tables: a gather map points outside its source")
            arr = upload_raw(ctx, host)
            arr.count = len(host)
            return arr

        nnz, rows = tab.nnz, tab.no * tab.nv
        for name in ("d_from_pp", "c_from_pp", "pp_to_d", "pp_to_c", "pp_to_dT", "pp_to_cT"):
            setattr(self, name, imap(getattr(tab, name), nnz))
        self.row_start, self.row_len = imap(tab.row_start, nnz + 1), imap(tab.row_len, nnz + 1)
        ai = np.empty(rows, dtype=np.int64)
        ai[tab.ph_row] = np.arange(rows)
        self.row_of, self.ai_of = imap(tab.ph_row, rows), imap(ai, rows)
        F, S, Fn, Sn = ("ph", "ph-", False), ("ph", "ph", False), ("ph", "ph-", True), ("ph", "ph", True)
        vo, oo, ov, vv = ("vv", "oo", False), ("oo", "oo", False), ("oo", "vv", False), ("vv", "vv", False)
        self.nsq = int(tab.offsets("ph", "ph")[-1])
        size = lambda op: int(tab.offsets(*op[:2])[-1])

        def table(a, b, c, **kw):
            return Tasks(ctx, tab.gemm_tasks(a, b, c, **kw), size(a), size(b), size(c))
        self.hole_quad = table(ov, vo, oo, beta=1.0)            # I^P += V_klcd^P T^P
        self.hole = table(vo, oo, vo, beta=1.0)                 # R^P += T^P I^P
        self.ladder = table(vv, vo, vo, beta=1.0)               # R^P += V_abcd^P T^P
        self.to_square = table(F, Fn, S)                        # X^q = W1^q Tt^{-q};  Y^q = D^q Wx^{-q};  Xc^q = C^q Wx^{-q}
        self.from_square_neg = table(F, Sn, F)                  # Rd^q = Tt^q X^{-q};  Ed^q = Tt^q W2^{-q}
        self.from_square_neg_t = table(F, Sn, F, alpha=-1.0, trans_b=True)      # Ec^q = -C^q (Wa^{-q})^T
        self.square_left_sub = table(S, F, F, alpha=-1.0, beta=1.0)              # Ed^q -= Wa^q D^q
        self.square_left_add = table(S, F, F, beta=1.0)                           # Ed^q += Y^q (C^q - D^q)
        self.square_left = table(S, F, F)                                         # Rc^q = Xc^q C^q


class SectorIntegrals:
    """The integral sectors of one Hamiltonian on the device: every block family of ``sectors.BLOCKS`` in the layout its
    product reads, plus the ``pipi`` / ``piip`` lists of the (diagonal) Fock matrix, in one arena.  Supports ``+`` and
    scaling (the transcorrelated Hamiltonian is ``only_2b + effect_2b``)."""

    NAMES = tuple(BLOCKS) + FOCK_LISTS

    def __init__(self, ctx, tables, arena=None, own_ctx=False):
        self.ctx, self.tables, self._own = ctx, tables, own_ctx
        sizes = [int(tables.block_offsets(nm)[-1]) if nm in BLOCKS else tables.n * tables.no for nm in self.NAMES]
        self.offsets = dict(zip(self.NAMES, np.concatenate(([0], np.cumsum(sizes)))[:-1]))
        self.sizes = dict(zip(self.NAMES, sizes))
        self.total = int(sum(sizes))
        self.arena = ctx.empty((self.total,)) if arena is None else arena
        self._dev = None

    def __getitem__(self, name):
        return view(self.arena, self.offsets[name], self.sizes[name])

    @property
    def nbytes(self):
        return 8 * self.total

    def device_tables(self):
        if self._dev is None:
            self._dev = DeviceTables(self.ctx, self.tables)
        return self._dev

    def _combine(self, terms):
        out = SectorIntegrals(self.ctx, self.tables)
        self.ctx.lincomb(out.arena, [t.arena for t, _ in terms], [c for _, c in terms])
        return out

    def __add__(self, other):
        if not isinstance(other, SectorIntegrals) or other.tables is not self.tables or other.ctx is not self.ctx:
            raise ValueError("SectorIntegrals: only integrals of the same tables and context can be added")
        return self._combine([(self, 1.0), (other, 1.0)])

    def __mul__(self, factor):
        return self._combine([(self, float(factor))])

    __rmul__ = __mul__

    def hf_orbital_energies(self, kinetic):
        """The diagonal of ``hf.construct_hf_matrix`` (the Fock matrix is diagonal here): h_pp + sum_i (2 V_pipi - V_piip)."""
        tab = self.tables
        kinetic = np.asarray(kinetic, dtype=np.float64)
        if kinetic.shape != (tab.n,):
            raise ValueError("hf_orbital_energies: one kinetic energy per orbital is needed")
        return kinetic + (2.0 * self["pipi"].get() - self["piip"].get()).reshape(tab.n, tab.no).sum(axis=1)

    def close(self):
        if self._own and self.ctx.handle:
            self.ctx.close()


class SectorAmplitudes:
    """Doubles amplitudes on their momentum-conserving support: the compact pp-layout vector and its tables."""

    def __init__(self, tables, vector):
        self.tables, self.vector = tables, vector

    def get(self):
        return self.vector.get() if isinstance(self.vector, DeviceArray) else np.asarray(self.vector)

    def to_dense(self):
        t = self.tables
        if 8 * t.nv ** 2 * t.no ** 2 > (8 << 30):
            raise MemoryError("SectorAmplitudes.to_dense: the [v,v,o,o] array would take more than 8 GiB")
        return t.to_dense(self.get())


class SectorTriplesIntegrals:
    """The two integral families of the momentum-blocked (T) on the device (``UEG.eval_2b_triples``), with their
    ``TriplesTables``:

      Vv[i,a,b] = V[i, f*, a, b], shape [o,v,v], f* the virtual with k_a + k_b - k_i
      Vo[i,j,a] = V[i, j, a, m*], shape [o,o,v], m* the occupied with k_i + k_j - k_a

    Contract: a position whose implied orbital does not exist holds an exact 0.0 (never a NaN, never left unwritten); the
    kernel multiplies it with the equally exact 0 of ``Tc`` there.  No ``+`` and no scaling (left out)."""

    def __init__(self, ctx, ttab, own_ctx=False):
        self.ctx, self.tables, self._own = ctx, ttab, own_ctx
        self.Vv = ctx.empty((ttab.no, ttab.nv, ttab.nv))
        self.Vo = ctx.empty((ttab.no, ttab.no, ttab.nv))
        self._dev = None

    @property
    def nbytes(self):
        return self.Vv.nbytes + self.Vo.nbytes

    def device_tables(self):
        """(k_int, orb_of, m_of as int32 device bytes; the implied map of ``Tc`` as an int64 gather map)"""
        if self._dev is None:
            t = self.tables
            if t.m_of.max(initial=-1) >= t.no or t.orb_of.max() >= t.n or t.implied_map.min() < 0 or \
                    t.implied_map.max() > t.tables.nnz:
                raise AssertionError("triples tables: an index points outside its array")
            i32 = lambda x: upload_raw(self.ctx, np.append(np.ascontiguousarray(x, dtype=np.int32).reshape(-1),
                                                           np.zeros(x.size % 2, dtype=np.int32)))
            imap = upload_raw(self.ctx, t.implied_map.reshape(-1))
            imap.count = t.implied_map.size
            self._dev = (i32(t.tables.k_int), i32(t.orb_of), i32(t.m_of), imap)
        return self._dev

    def close(self):
        if self._own and self.ctx.handle:
            self.ctx.close()


TRIPLES_WS_ENV, TRIPLES_WS_DEFAULT = "PYMES_SECTOR_TRIPLES_BYTES", 1 << 30


def triple_bytes(nv):
    """Workspace bytes of one triple in ``pymes_sector_triples``: the v x v slab, one partial per 32 x 32 tile, the value."""
    return 8 * (nv * nv + (-(-nv // 32)) ** 2 + 1)


def _hermitian(ints, rtol=1e-12):
    """V_klcd = V_cdkl, sector by sector: ``klcd``^P against ``abij``^P transposed."""
    tab = ints.tables
    sec, lr, lc = sectors._expand(tab.n_oo, tab.n_vv, 0, len(tab.P_keys))
    kl, ab = ints["klcd"].get(), ints["abij"].get()
    if not len(kl):
        return True
    return np.abs(kl - ab[tab.pp_off[sec] + lc * tab.n_oo[sec] + lr]).max() <= rtol * max(np.abs(ab).max(), 1e-300)


def _check_triples(who, ints, tints):
    """The refusals of the (T) inputs that need no amplitudes (``SectorCCD.solve`` makes them before it iterates)."""
    if not isinstance(ints, SectorIntegrals):
        raise TypeError(who + ": ints must be SectorIntegrals (UEG.eval_2b_sectors)")
    if not isinstance(tints, SectorTriplesIntegrals):
        raise TypeError(who + ": the triples integrals must be SectorTriplesIntegrals (UEG.eval_2b_triples)")
    tab, other = ints.tables, tints.tables.tables
    same = other is tab or (other.no == tab.no and np.array_equal(other.k_int, tab.k_int))
    if not same or tints.ctx is not ints.ctx:
        raise ValueError(who + ": the triples integrals belong to other tables or another context than the integrals")
    if ints.ctx.recording:
        raise RuntimeError(who + ": the context is recording a launch graph")
    if not _hermitian(ints):
        raise ValueError(who + ": the integrals are not Hermitian (V_pqrs = V_rspq fails between the klcd and abij sectors); "
                         "(T) is not defined for transcorrelated integrals, and Lambda-(T) does not exist on sectors yet")


def sector_triples_energy(eps, ints, tints, amps, triple_range=None, per_triple=False, workspace_bytes=None):
    """E(T) of doubles amplitudes on the momentum sectors (singles vanish there, so CCD(T) is CCSD(T)): the sum of m_ijk S_ijk
    of tests/_triples_reference.py by ``pymes_sector_triples``, never an array larger than ``tints``.

    eps: the orbital energies (or a diagonal Fock matrix); ints: the ``SectorIntegrals``; tints: the
    ``SectorTriplesIntegrals`` of the same tables and context (``UEG.eval_2b_triples``); amps: ``SectorAmplitudes``, a compact
    vector or a dense [v,v,o,o] array with T_abij = T_baji.  ``triple_range=(begin, end)``: only those triples (the order of
    ``pymes_ccsd_t``), no collective; otherwise all of them, split over the ranks by ``ccsd_t.rank_range`` and all-reduced
    when ``torch.distributed`` runs one process per GPU.  The triples are worked off in batches of as many v x v slabs as
    ``workspace_bytes`` hold (default: the environment's PYMES_SECTOR_TRIPLES_BYTES, else 1 GiB; at least one triple); the
    value of a triple does not depend on it.  Returns the energy, or (energy, per-triple values of the range as a host
    array) with ``per_triple=True``.  Refused: integrals without V_pqrs = V_rspq (transcorrelated ones)."""
    who = "sector_triples_energy"
    _check_triples(who, ints, tints)
    tab, ctx, tt = ints.tables, ints.ctx, tints.tables
    eps = np.asarray(eps, dtype=np.float64)
    if eps.ndim == 2:
        if np.count_nonzero(eps - np.diag(eps.diagonal())):
            raise ValueError(who + ": the Fock matrix must be diagonal (it is for a momentum-conserving Hamiltonian)")
        eps = eps.diagonal().copy()
    if eps.shape != (tab.n,):
        raise ValueError(who + ": %d orbital energies for %d orbitals" % (eps.size, tab.n))
    vec = SectorCCD._compact(tab, amps)
    if len(vec) and np.abs(vec - vec[tab.pp_swap]).max() > 1e-13 * max(np.abs(vec).max(), 1e-300):
        raise ValueError(who + ": the amplitudes are not exchange-symmetric (T_abij = T_baji)")
    no, nv = tab.no, tab.nv
    lo, hi, reduce = ccsd_t._triple_chunk(no, triple_range)
    if not 0 <= lo <= hi <= ccsd_t.n_triples(no):
        raise ValueError(who + ": triple range [%d, %d) outside [0, %d]" % (lo, hi, ccsd_t.n_triples(no)))
    if workspace_bytes is None:
        workspace_bytes = int(os.environ.get(TRIPLES_WS_ENV, TRIPLES_WS_DEFAULT))
    each = triple_bytes(nv)
    ws_bytes = each * max(1, min(int(workspace_bytes) // each, max(hi - lo, 1)))
    k_dev, orb_dev, m_dev, imap = tints.device_tables()
    temps = [ctx.array(np.append(vec, 0.0)), ctx.empty((no, no, nv)), ctx.array(eps), ctx.empty((ws_bytes // 8,))]
    src, Tc, eps_dev, ws = temps
    out = ctx.empty((max(hi - lo, 1),)) if per_triple else None
    e = C.c_double()
    try:
        gather(ctx, Tc, src, imap)
        ctx.lib.call("pymes_sector_triples", ctx.handle, no, nv, C.c_void_p(eps_dev.ptr), C.c_void_p(k_dev.ptr),
                     C.c_void_p(orb_dev.ptr), tt.box.ctypes.data_as(C.c_void_p), C.c_void_p(m_dev.ptr), C.c_void_p(Tc.ptr),
                     C.c_void_p(tints.Vv.ptr), C.c_void_p(tints.Vo.ptr), int(lo), int(hi), C.c_void_p(ws.ptr), int(ws_bytes),
                     C.c_void_p(out.ptr if out is not None else None), C.byref(e))
        values = out.get()[:hi - lo] if out is not None else None
    finally:
        for t in temps + ([out] if out is not None else []):
            t.free()
    energy = float(e.value)
    if reduce:
        energy = float(pdist.allreduce_sum([energy])[0])
    return (energy, values) if per_triple else energy


class SectorCCD:
    def __init__(self, no, delta_e=1.e-8, is_dcd=False, is_diis=True, is_dr_ccd=False, is_bruekner=False, device=0):
        if is_dr_ccd or is_bruekner:
            raise NotImplementedError("dr-CCD and Brueckner energies (ccd.py:95-121) are outside the HIP hot path")
        self.no, self.delta_e, self.is_dcd, self.is_diis, self.device = no, delta_e, is_dcd, is_diis, device
        self.max_iter = 50
        if self.is_diis:
            self.mixer = diis.DIIS(dim_space=6)

    # ---- one residual: ccd.py:164-254 as sector-batched products (term by term: tests/_sector_reference.py) ------------
    def residual(self, ints, eps_dev, T, R, ws):
        ctx, dt = ints.ctx, ints.device_tables()
        quad = not self.is_dcd
        D, Cx, Tt, Rd, Ed, Ec, sq, scratch = (ws[k] for k in ("D", "C", "Tt", "Rd", "Ed", "Ec", "sq", "x"))
        # pp layout: R^P = V_abij^P + T^P (V_klij^P + [CCD] V_klcd^P T^P) + V_abcd^P T^P
        R.copy_from(ints["abij"])
        hole = ints["klij"]
        if quad:
            hole = ws["I"].copy_from(hole)
            dt.hole_quad.run(ints["klcd"], T, hole)
        dt.hole.run(T, hole, R)
        dt.ladder.run(ints["abcd"], T, R)
        # direct and crossed layouts of T, and Tt = 2 D - C
        gather(ctx, D, T, dt.d_from_pp)
        gather(ctx, Cx, T, dt.c_from_pp)
        gather(ctx, Tt, T, dt.d_from_pp, 2.0, T, dt.c_from_pp, -1.0)
        dt.to_square.run(ints["w1"], Tt, sq)                     # X^q = W1^q Tt^{-q}
        dt.from_square_neg.run(Tt, sq, Rd)                       # Rd^q = Tt^q X^{-q}                  (:202-204)
        dt.from_square_neg.run(Tt, ints["w2"], Ed)               # Ed^q = Tt^q W2^{-q}
        dt.square_left_sub.run(ints["wa"], D, Ed)                # Ed^q -= Wa^q D^q
        dt.from_square_neg_t.run(Cx, ints["wa"], Ec)             # Ec^q = -C^q Wb^{-q},  Wb = Wa^T
        if quad:
            CmD, Rc = ws["CmD"], ws["Rc"]
            gather(ctx, CmD, T, dt.c_from_pp, 1.0, T, dt.d_from_pp, -1.0)
            dt.to_square.run(D, ints["wx"], sq)                  # Y^q = D^q Wx^{-q}
            dt.square_left_add.run(sq, CmD, Ed)                  # Ed^q += Y^q (C^q - D^q)             (:237-240)
            dt.to_square.run(Cx, ints["wx"], sq)                 # Xc^q = C^q Wx^{-q}
            dt.square_left.run(sq, Cx, Rc)                       # Rc^q = Xc^q C^q                     (:189-191)
        tab = ints.tables
        ctx.lib.call("pymes_sector_xdiag", ctx.handle, C.c_void_p(Tt.ptr), C.c_void_p(ints["w1"].ptr), C.c_void_p(D.ptr),
                     C.c_void_p(Ed.ptr), C.c_void_p(eps_dev.ptr), 1.0 if quad else 0.5, tab.no, tab.nv,
                     C.c_void_p(dt.row_start.ptr), C.c_void_p(dt.row_len.ptr), C.c_void_p(dt.row_of.ptr),
                     C.c_void_p(dt.ai_of.ptr), C.c_void_p(scratch.ptr))
        # Ex + Ex^T(1,0,3,2) (block q against the transpose of block -q), everything back to the pp vector
        gather(ctx, R, Ed, dt.pp_to_d, 1.0, Ed, dt.pp_to_dT, 1.0, beta=1.0)
        gather(ctx, R, Ec, dt.pp_to_c, 1.0, Ec, dt.pp_to_cT, 1.0, beta=1.0)
        if quad:
            gather(ctx, R, Rd, dt.pp_to_d, 1.0, ws["Rc"], dt.pp_to_c, 1.0, beta=1.0)
        else:
            gather(ctx, R, Rd, dt.pp_to_d, beta=1.0)
        return R

    def workspace(self, ints):
        ctx, tab = ints.ctx, ints.tables
        nnz = max(tab.nnz, 1)
        ws = {k: ctx.empty((nnz,)) for k in ("D", "C", "Tt", "Rd", "Ed", "Ec")}
        ws["sq"] = ctx.empty((max(ints.device_tables().nsq, 1),))
        ws["x"] = ctx.empty((tab.no * tab.nv + tab.n,))
        if not self.is_dcd:
            ws.update({k: ctx.empty((nnz,)) for k in ("CmD", "Rc")})
            ws["I"] = ctx.empty((max(ints.sizes["klij"], 1),))
        return ws

    def get_residual(self, eps, ints, amps):
        """The compact residual of compact (or dense) amplitudes, as a host vector."""
        tab, ctx = ints.tables, ints.ctx
        T = ctx.array(self._compact(tab, amps))
        R = self.residual(ints, ctx.array(np.asarray(eps, dtype=np.float64)), T, ctx.empty((tab.nnz,)), self.workspace(ints))
        return R.get()

    @staticmethod
    def _compact(tab, amps):
        if isinstance(amps, SectorAmplitudes):
            if amps.tables is not tab and not (np.array_equal(amps.tables.k_int, tab.k_int) and amps.tables.no == tab.no):
                raise ValueError("SectorCCD: the tables of the amplitudes do not match the integrals")
            vec = amps.get()
        else:
            vec = np.asarray(amps)
            vec = tab.compact(vec, "amps") if vec.ndim == 4 else vec
        vec = np.ascontiguousarray(vec, dtype=np.float64)
        if vec.shape != (tab.nnz,):
            raise ValueError("SectorCCD: the tables of the amplitudes do not match the integrals")
        return vec

    def _checks(self, eps, ints):
        if not isinstance(ints, SectorIntegrals):
            raise TypeError("SectorCCD.solve: ints must be SectorIntegrals (UEG.eval_2b_sectors); the dense path is CCD")
        tab, ctx = ints.tables, ints.ctx
        if ctx.recording:
            raise RuntimeError("SectorCCD.solve: the context is recording a launch graph")
        eps = np.asarray(eps, dtype=np.float64)
        if eps.ndim == 2:
            if np.count_nonzero(eps - np.diag(eps.diagonal())):
                raise ValueError("SectorCCD.solve: the Fock matrix must be diagonal (it is for a momentum-conserving Hamiltonian)")
            eps = eps.diagonal().copy()
        if tab.no != self.no or eps.shape != (tab.n,):
            raise ValueError("SectorCCD.solve: the tables of the integrals (no = %d, n = %d) do not match the solver (no = %d) "
                             "and the %d orbital energies" % (tab.no, tab.n, self.no, eps.size))
        # the product list needs V_klcd = V_lkdc (the X_ac / X_ki sums read W1 where ccd.py:213-220 reads V_lkdc)
        w1 = ints["w1"].get()
        if len(w1) and np.abs(w1 - w1[tab.d_partner]).max() > 1e-12 * max(np.abs(w1).max(), 1e-300):
            raise ValueError("SectorCCD.solve: the integrals are not symmetric under the exchange of the two electrons "
                             "(V_pqrs = V_qpsr), which the sector residual needs")
        return eps

    def solve(self, eps, ints, level_shift=0., amps=None, triples=None, **kwargs):
        """The loop of ``CCD.solve`` (ccd.py:24-162) on the compact vector.  eps: the orbital energies (or a diagonal Fock
        matrix); ints: ``SectorIntegrals``.  ``triples``: the ``SectorTriplesIntegrals`` of the same tables; the result then
        also holds "(t) e" (``sector_triples_energy`` of the final amplitudes) and "ccd(t) e"."""
        algo_name = "ccd.solve"
        time_ccd = time.time()
        eps = self._checks(eps, ints)
        if triples is not None:
            _check_triples("SectorCCD.solve", ints, triples)
        tab, ctx, no = ints.tables, ints.ctx, self.no
        max_iter, delta_e = kwargs.get("max_iter", self.max_iter), kwargs.get("delta_e", self.delta_e)
        with quiet_collector():
            print_logging_info(algo_name)
            print_logging_info("Using DCD: ", self.is_dcd, level=1)
            print_logging_info("Using dr-CCD: ", False, level=1)
            print_logging_info("Solving doubles amplitude equation", level=1)
            print_logging_info("Using data type %s" % np.float64, level=1)
            print_logging_info("Using DIIS mixer: ", self.is_diis, level=1)
            print_logging_info("Using Bruekner quasi-particle energy: ", False, level=1)
            print_logging_info("Iteration = 0", level=1)
            n = tab.nnz
            eps_dev, den = ctx.array(eps), ctx.array(tab.denominators(eps))
            ws = self.workspace(ints)
            t2, r2 = ctx.pool_get((n,)), ctx.pool_get((n,))
            dt_fixed = None if self.is_diis else ctx.pool_get((n,))
            self._update(ctx, t2, None, None, ints["abij"], den, level_shift)        # mp2.py:9-22
            e_dir, e_exc = self._energy(ctx, ints, t2)[:2]
            e_mp2 = e_dir + e_exc
            print("MP2 energy = ", e_mp2)
            if amps is not None:
                vec = self._compact(tab, amps)
                if np.abs(vec - vec[tab.pp_swap]).max() > 1e-13 * max(np.abs(vec).max(), 1e-300):
                    raise ValueError("SectorCCD.solve: the amplitudes are not exchange-symmetric (T_abij = T_baji), which the "
                                     "sector residual needs")
                t2.set(vec)
            dE, iteration, e_last = np.abs(e_mp2), 0, e_mp2
            e_ccd = e_dir_ccd = e_ex_ccd = 0.
            while np.abs(dE) > delta_e and iteration <= max_iter:
                iteration += 1
                self.residual(ints, eps_dev, t2, r2, ws)                              # ccd.py:100-102
                if self.is_diis:
                    t2n, dt2 = ctx.pool_get((n,)), ctx.pool_get((n,))
                    self._update(ctx, t2n, dt2, t2, r2, den, level_shift)             # :123-124
                    self.mixer.mix([dt2], [t2n], release=ctx.pool_put, out=[t2], defer_log=True, native=True)   # :126-127
                else:
                    dt2 = dt_fixed
                    self._update(ctx, t2, dt2, t2, r2, den, level_shift)
                e_dir_ccd, e_ex_ccd, nt2, nr2 = self._energy(ctx, ints, t2, dt2)      # :132 and the norms, one pass
                if self.is_diis:
                    self.mixer.log_last()
                e_ccd = e_dir_ccd + e_ex_ccd
                dE = e_ccd - e_last
                e_last = e_ccd
                if iteration <= max_iter:
                    print_logging_info("Iteration = ", iteration, level=1)
                    print_logging_info("Correlation Energy = {:.12f}".format(e_ccd), level=2)
                    print_logging_info("dE = {:.12e}".format(dE), level=2)
                    print_logging_info("L1 Norm of T2 = {:.12f}".format(np.sqrt(nt2)), level=2)
                    print_logging_info("Norm Residual = {:.12f}".format(np.sqrt(nr2)), level=2)
                else:
                    print_logging_info("A converged solution is not found!", level=1)
            print_logging_info("Direct contribution = {:.12f}".format(e_dir_ccd), level=1)
            print_logging_info("Exchange contribution = {:.12f}".format(e_ex_ccd), level=1)
            print_logging_info("CCD correlation energy = {:.12f}".format(e_ccd), level=1)
            print_logging_info("{:.3f} seconds spent on CCD".format((time.time() - time_ccd)), level=1)
            self.iterations = iteration
            result = ctx.empty((n,)).copy_from(t2)       # (t2 itself goes back to the pool; the mixer may hold the rest)
            ctx.pool_put(t2)
            ctx.pool_put(r2)
            out = {"ccd e": e_ccd, "t2 amp": SectorAmplitudes(tab, result), "hole e": eps[:no], "particle e": eps[no:],
                   "dE": dE}
            if triples is not None:
                out["(t) e"] = sector_triples_energy(eps, ints, triples, out["t2 amp"])
                out["ccd(t) e"] = e_ccd + out["(t) e"]
                print_logging_info("(T) correction = {:.12f}".format(out["(t) e"]), level=1)
            return out

    @staticmethod
    def _update(ctx, t_out, dt, t_in, r, den, shift):
        ctx.lib.call("pymes_sector_update", ctx.handle, C.c_void_p(t_out.ptr), C.c_void_p(dt.ptr if dt is not None else 0),
                     C.c_void_p(t_in.ptr if t_in is not None else 0), C.c_void_p(r.ptr), C.c_void_p(den.ptr), float(shift),
                     t_out.size)

    @staticmethod
    def _energy(ctx, ints, t2, dt2=None):
        """(direct, exchange, |T|^2, |dT|^2): ccd.py:256-262 on the compact vector, one launch and one synchronisation."""
        xs, ys = [t2, t2, t2], [ints["ed"], ints["ex"], t2]
        if dt2 is not None:
            xs, ys = xs + [dt2], ys + [dt2]
        d = ctx.dots(xs, ys)
        return 2.0 * d[0], -d[1], d[2], (d[3] if dt2 is not None else 0.0)
