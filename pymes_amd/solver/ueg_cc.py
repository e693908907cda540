"""Momentum-blocked closed-shell CCD / DCD for Hamiltonians whose orbitals carry a conserved integer vector (the electron
gas, with or without twist): the loop of ``CCD.solve`` on the ~ o^2 v non-zero amplitudes, never an array of size n^4, v^4
or v^2 o^2.  Singles vanish by the same symmetry, so DCD here is also DCSD.

The tables (``pymes_amd.solver.sectors``) hold the non-zeros in three block-diagonal layouts; every contraction of
ccd.py:164-254 is one launch of the ragged batched product ``pymes_sector_gemm`` over all sectors, the moves between the
layouts are gathers, and the diagonal X_ac / X_ki terms, the update and the energy are element-wise tails (DESIGN "Momentum
sectors"; the numpy restatement the tests compare with is tests/_sector_reference.py).  The dense path (``CCD``, ``CCSD``) is
untouched.

On the same tables: the perturbative triples (``sector_triples_energy``), and for integrals without
V_pqrs = V_rspq (the transcorrelated electron gas) the Lambda equations of CCD and DCD as the transposed Jacobian of that
residual (``SectorLambda``) with the Lambda-(T) correction on top (``sector_lambda_triples_energy``); and from
the amplitudes and their Lambda the response densities (``sector_density`` / ``SectorDensity``): the momentum
distribution n(k), the expectation value of a second two-body operator, the transfer sums and the static structure factor S(q).
The ladder block V_abcd is either stored like every other family or, for ``UEG.eval_2b_sectors(..., ladder="direct")``, generated
inside the ladder product from ``LadderTerm`` objects (``SectorIntegrals.ladder``)."""
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

__all__ = ["SectorTables", "SectorIntegrals", "LadderTerm", "SectorAmplitudes", "SectorCCD", "TriplesTables",
           "SectorTriplesIntegrals", "sector_triples_energy", "SectorLambda", "sector_lambda_triples_energy", "SectorDensity", "sector_density",
           "SectorIPEAHoist", "SectorIPEASigma", "SectorIP_EOM_CCD", "SectorEA_EOM_CCD", "SectorLadderIntegrals",
           "SectorSpectralFunction"]
_EOM_NAMES = ("SectorIPEAHoist", "SectorIPEASigma", "SectorIP_EOM_CCD", "SectorEA_EOM_CCD", "SectorLadderIntegrals",
              "SectorSpectralFunction")


def __getattr__(name):
    """The sector EOM (``ueg_eom``) is re-exported here; it imports this module, so it is bound on first use."""
    if name in _EOM_NAMES:
        from pymes_amd.solver import ueg_eom
        return getattr(ueg_eom, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


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
        self.extent = np.maximum(tasks["m"], tasks["k"]) if len(tasks) else np.zeros(0, dtype=np.int64)    # rows / columns of A
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


def upload_map(ctx, host, limit, who="sector tables: a gather map points outside its source", lowest=0):
    """An int64 gather map (or index list) on the device with its length as ``.count``, refused unless every entry lies in
    [lowest, limit): the kernels trust it."""
    host = np.ascontiguousarray(host, dtype=np.int64).reshape(-1)
    if len(host) and (host.min() < lowest or host.max() >= limit):
        raise AssertionError(who)
    arr = upload_raw(ctx, host)
    arr.count = len(host)
    return arr


def upload_i32(ctx, host):
    """An int32 table on the device, padded with a 0 to a whole number of doubles."""
    host = np.ascontiguousarray(host, dtype=np.int32).reshape(-1)
    return upload_raw(ctx, np.append(host, np.zeros(host.size % 2, dtype=np.int32)))


class DeviceTables:
    """The gather maps, row tables and task tables of one ``SectorTables`` in one context (uploaded once, kept with the
    integrals)."""

    # the operands of ``SectorTables.gemm_tasks`` (rows, columns, block -q in place of q): F, S, Fn, Sn of the ph layouts and
    # vo, oo, ov, vv of the pp layout, in the order every table list below unpacks them
    OPERANDS = (("ph", "ph-", False), ("ph", "ph", False), ("ph", "ph-", True), ("ph", "ph", True),
                ("vv", "oo", False), ("oo", "oo", False), ("oo", "vv", False), ("vv", "vv", False))

    def size(self, op):
        return int(self.tab.offsets(*op[:2])[-1])

    def table(self, a, b, c, **kw):
        return Tasks(self.ctx, self.tab.gemm_tasks(a, b, c, **kw), self.size(a), self.size(b), self.size(c))

    def __init__(self, ctx, tab):
        self.ctx, self.tab = ctx, tab
        nnz, rows = tab.nnz, tab.no * tab.nv
        for name in ("d_from_pp", "c_from_pp", "pp_to_d", "pp_to_c", "pp_to_dT", "pp_to_cT"):
            setattr(self, name, upload_map(ctx, getattr(tab, name), nnz))
        self.row_start, self.row_len = upload_map(ctx, tab.row_start, nnz + 1), upload_map(ctx, tab.row_len, nnz + 1)
        ai = np.empty(rows, dtype=np.int64)
        ai[tab.ph_row] = np.arange(rows)
        self.row_of, self.ai_of = upload_map(ctx, tab.ph_row, rows), upload_map(ctx, ai, rows)
        table, (F, S, Fn, Sn, vo, oo, ov, vv) = self.table, self.OPERANDS
        self.nsq = self.size(S)
        self.hole_quad = table(ov, vo, oo, beta=1.0)            # I^P += V_klcd^P T^P
        self.hole = table(vo, oo, vo, beta=1.0)                 # R^P += T^P I^P
        self.ladder = table(vv, vo, vo, beta=1.0)               # R^P += V_abcd^P T^P
        self.to_square = table(F, Fn, S)                        # X^q = W1^q Tt^{-q};  Y^q = D^q Wx^{-q};  Xc^q = C^q Wx^{-q}
        self.from_square_neg = table(F, Sn, F)                  # Rd^q = Tt^q X^{-q};  Ed^q = Tt^q W2^{-q}
        self.from_square_neg_t = table(F, Sn, F, alpha=-1.0, trans_b=True)      # Ec^q = -C^q (Wa^{-q})^T
        self.square_left_sub = table(S, F, F, alpha=-1.0, beta=1.0)              # Ed^q -= Wa^q D^q
        self.square_left_add = table(S, F, F, beta=1.0)                           # Ed^q += Y^q (C^q - D^q)
        self.square_left = table(S, F, F)                                         # Rc^q = Xc^q C^q
        self._adjoint = None
        self._density = None

    def layouts(self, T, D=None, Cx=None, Tt=None, CmD=None):
        """The direct and crossed layouts of a compact vector into the caller's buffers, those that are given, in this
        order: D = T[d_from_pp], C = T[c_from_pp], Tt = 2 D - C, CmD = C - D (one gather each)."""
        ctx, d, c = self.ctx, self.d_from_pp, self.c_from_pp
        if D is not None:
            gather(ctx, D, T, d)
        if Cx is not None:
            gather(ctx, Cx, T, c)
        if Tt is not None:
            gather(ctx, Tt, T, d, 2.0, T, c, -1.0)
        if CmD is not None:
            gather(ctx, CmD, T, c, 1.0, T, d, -1.0)

    def cotangents(self, lam, yRd, yRc, yEd, yEc):
        """The cotangents of Rd, Rc and of Ed, Ec (which enter as Ex + Ex^T(1,0,3,2)) into the caller's buffers: gathers of
        lambda through the inverse maps (the first rows of the table of DESIGN 8k)."""
        ctx, at = self.ctx, self.adjoint()
        gather(ctx, yRd, lam, self.d_from_pp)
        gather(ctx, yRc, lam, self.c_from_pp)
        gather(ctx, yEd, lam, self.d_from_pp, 1.0, lam, at.dT_from_pp, 1.0)
        gather(ctx, yEc, lam, self.c_from_pp, 1.0, lam, at.cT_from_pp, 1.0)

    def adjoint(self):
        """The task tables and maps of the Lambda residual (``SectorLambda``): every product of the list above
        with the operand that held T exchanged for the output, built on first use.  In the ph layouts the adjoint of a
        product that read block -q of an operand writes the cotangent of that block, so the tables below are written for
        the output sector q and read blocks -q where the forward product wrote them."""
        if self._adjoint is not None:
            return self._adjoint
        ctx, tab = self.ctx, self.tab
        table, (F, S, Fn, Sn, vo, oo, ov, vv) = self.table, self.OPERANDS

        class Adjoint:
            pass
        at = Adjoint()
        at.ladder_t = table(vv, vo, vo, beta=1.0, trans_a=True)                # G^P += (V_abcd^P)^T lam^P
        at.hole_t = table(vo, oo, vo, beta=1.0, trans_b=True)                  # G^P += lam^P (I^P)^T
        at.t_lam = table(vo, vo, oo, trans_a=True)                             # M^P = (T^P)^T lam^P
        at.hole_quad_t = table(ov, oo, vo, beta=1.0, trans_a=True)             # G^P += (V_klcd^P)^T M^P
        at.sq_tn = table(Fn, Fn, S, trans_a=True)                              # Z^q = (Tt^{-q})^T yRd^{-q}  (cotangent of X^q)
        at.right_t = table(F, Sn, F, trans_b=True)                             # zTt^q = yRd^q (X^{-q})^T
        at.right_t_add = table(F, Sn, F, beta=1.0, trans_b=True)               # zTt^q += yEd^q (W2^{-q})^T
        at.left_tn_add = table(Fn, Sn, F, beta=1.0, trans_a=True)              # zTt^q += (W1^{-q})^T Z^{-q}
        at.sq_t_left_neg = table(S, F, F, alpha=-1.0, trans_a=True)            # zD^q = -(Wa^q)^T yEd^q
        at.sq_t_left = table(S, F, F, trans_a=True)                            # zM^q = (Y^q)^T yEd^q
        at.sq_t_left_add = table(S, F, F, beta=1.0, trans_a=True)              # zC^q += (Xc^q)^T yRc^q
        at.right_neg = table(F, Sn, F, alpha=-1.0)                             # zC^q = -yEc^q Wa^{-q}
        at.outer = table(F, F, S, trans_b=True)                                # zY^q = yEd^q (C^q - D^q)^T;  zXc^q = yRc^q (C^q)^T
        at.sq_right_t_add = table(S, Fn, F, beta=1.0, trans_b=True)            # zD^q += zY^q (Wx^{-q})^T;  zC^q += zXc^q (Wx^{-q})^T
        at.dT_from_pp = upload_map(ctx, tab.d_from_pp[tab.d_partner], tab.nnz)
        at.cT_from_pp = upload_map(ctx, tab.c_from_pp[tab.d_partner], tab.nnz)
        at.pp_swap = upload_map(ctx, tab.pp_swap, tab.nnz)
        self._adjoint = at
        return at

    def density(self):
        """The task tables of ``SectorDensity``: every product of the list above with the operand that held an
        integral block exchanged for the output (outer-product shapes), next to those of ``adjoint()``; built on first use."""
        if self._density is not None:
            return self._density
        at, table, (F, S, Fn, Sn, vo, oo, ov, _) = self.adjoint(), self.table, self.OPERANDS

        class Density:
            pass
        dn = Density()
        dn.t_lam, dn.sq_tn, dn.outer, dn.left_tn_add = at.t_lam, at.sq_tn, at.outer, at.left_tn_add
        dn.m_tt = table(oo, vo, ov, trans_b=True)                              # G_klcd^P = M^P (T^P)^T
        dn.sq_right_t = table(S, Fn, F, trans_b=True)                          # G_w1^q = Z^q (Tt^{-q})^T
        dn.outer_neg = table(F, F, S, alpha=-1.0, trans_b=True)                # G_wa^q = -yEd^q (D^q)^T
        dn.sq_tn_sub = table(Fn, Fn, S, alpha=-1.0, beta=1.0, trans_a=True)    # G_wa^q -= (yEc^{-q})^T C^{-q}
        dn.left_tn = table(Fn, Sn, F, trans_a=True)                            # G_wx^q = (D^{-q})^T zY^{-q}
        self._density = dn
        return dn


class LadderTerm:
    """One term of the direct particle ladder on the device (include/pymes_amd.h, pymes_ueg_ladder_term_create): what one
    ``UEG.eval_2b_sectors(..., ladder="direct")`` call prepared instead of the ``abcd`` blocks.  Shared by the
    ``SectorIntegrals`` that sum or scale it and freed with the last of them, or with the context."""

    def __init__(self, ctx, handle, k_int):
        self.ctx, self.handle, self.k_int = ctx, handle, np.array(k_int, dtype=np.int32)
        nbytes = C.c_int64()
        ctx.lib.call("pymes_ueg_ladder_term_bytes", ctx.handle, handle, C.byref(nbytes))
        self.nbytes = int(nbytes.value)

    def free(self):
        if self.handle and self.ctx.handle:           # (a closed context has released its terms)
            self.ctx.lib.call("pymes_ueg_ladder_term_free", self.ctx.handle, self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SectorIntegrals:
    """The integral sectors of one Hamiltonian on the device: every block family of ``sectors.BLOCKS`` in the layout its
    product reads, plus the ``pipi`` / ``piip`` lists of the (diagonal) Fock matrix, in one arena.  Supports ``+`` and
    scaling (the transcorrelated Hamiltonian is ``only_2b + effect_2b``).

    ``ladder_terms``: a list of (coefficient, ``LadderTerm``) makes it a direct object: the ``abcd`` family has
    size 0 and ``ladder`` evaluates V_abcd = sum coefficient * term inside the product.  ``+`` of two direct objects
    concatenates their lists (at most ``MAX_LADDER_TERMS`` terms), ``*`` scales the coefficients."""

    NAMES = tuple(BLOCKS) + FOCK_LISTS
    MAX_LADDER_TERMS = 4            # PYMES_SECTOR_LADDER_MAX_TERMS

    def __init__(self, ctx, tables, arena=None, own_ctx=False, ladder_terms=None):
        self.ctx, self.tables, self._own = ctx, tables, own_ctx
        self.ladder_terms = None if ladder_terms is None else self._checked_terms(ctx, tables, ladder_terms)
        sizes = [int(tables.block_offsets(nm)[-1]) if nm in BLOCKS else tables.n * tables.no for nm in self.NAMES]
        if self.direct:
            sizes[self.NAMES.index("abcd")] = 0
        self.offsets = dict(zip(self.NAMES, np.concatenate(([0], np.cumsum(sizes)))[:-1]))
        self.sizes = dict(zip(self.NAMES, sizes))
        self.total = int(sum(sizes))
        self.arena = ctx.empty((self.total,)) if arena is None else arena
        self._dev = None
        self._ladder_dev = None

    @classmethod
    def _checked_terms(cls, ctx, tables, terms):
        terms = [(float(c), t) for c, t in terms]
        if not 1 <= len(terms) <= cls.MAX_LADDER_TERMS:
            raise ValueError("SectorIntegrals: a direct ladder takes between 1 and %d terms, %d were given"
                             % (cls.MAX_LADDER_TERMS, len(terms)))
        for _, t in terms:
            if not isinstance(t, LadderTerm) or t.ctx is not ctx or not t.handle:
                raise ValueError("SectorIntegrals: a ladder term must be a live LadderTerm of the same context")
            if t.k_int.shape != tables.k_int.shape or not np.array_equal(t.k_int, tables.k_int):
                raise ValueError("SectorIntegrals: a ladder term was made for another basis (its k_int differs from the tables')")
        return terms

    @property
    def direct(self):
        return self.ladder_terms is not None

    def __getitem__(self, name):
        return view(self.arena, self.offsets[name], self.sizes[name])

    @property
    def nbytes(self):
        """Device bytes of the integrals: the arena, and for a direct object what its (distinct) ladder terms hold."""
        terms = {id(t): t.nbytes for _, t in self.ladder_terms or ()}
        return 8 * self.total + sum(terms.values())

    def device_tables(self):
        if self._dev is None:
            self._dev = DeviceTables(self.ctx, self.tables)
        return self._dev

    def _combine(self, terms):
        ladder = None
        if self.direct:
            ladder = [(c * lc, t) for obj, c in terms for lc, t in obj.ladder_terms]
        out = SectorIntegrals(self.ctx, self.tables, ladder_terms=ladder)
        self.ctx.lincomb(out.arena, [t.arena for t, _ in terms], [c for _, c in terms])
        return out

    def __add__(self, other):
        if not isinstance(other, SectorIntegrals) or other.tables is not self.tables or other.ctx is not self.ctx:
            raise ValueError("SectorIntegrals: only integrals of the same tables and context can be added")
        if self.direct != other.direct:
            raise ValueError("SectorIntegrals: integrals with a direct ladder and integrals with a stored ladder cannot be "
                             "added (evaluate both with the same ladder=)")
        return self._combine([(self, 1.0), (other, 1.0)])

    def __mul__(self, factor):
        return self._combine([(self, float(factor))])

    __rmul__ = __mul__

    def ladder(self, tasks, X, Y):
        """The particle-ladder product of a task table built on the (vv, vv) family -- ``DeviceTables.ladder`` or
        ``adjoint().ladder_t`` --: Y^P = alpha op(V_abcd^P) X^P + beta Y^P.  A stored object reads its ``abcd`` blocks
        (``pymes_sector_gemm``); a direct one generates them inside ``pymes_sector_ladder_direct``."""
        if not self.direct:
            tasks.run(self["abcd"], X, Y)
            return
        ctx, tab = self.ctx, self.tables
        if ctx.recording:
            raise RuntimeError("SectorIntegrals.ladder: the context is recording a launch graph (direct ladder)")
        if self._ladder_dev is None:
            rows, first = tab.ladder_rows()
            if len(rows) and (rows.min() < tab.no or rows.max() >= tab.n):
                raise AssertionError("sector tables: the vv pair list names an orbital that is no virtual")
            self._ladder_dev = (upload_i32(ctx, rows), upload_raw(ctx, first if len(first) else np.zeros(1, dtype=np.int64)),
                                upload_i32(ctx, tab.k_int), first, len(rows))
        rows_dev, first_dev, k_dev, first, nrows = self._ladder_dev
        if tasks.ctx is not ctx or tasks.count != len(first) or (len(first) and (first + tasks.extent).max() > nrows):
            raise ValueError("SectorIntegrals.ladder: the task table is not one of the (vv, vv) family of these tables")
        if X.size < tasks.lens[1] or Y.size < tasks.lens[2]:
            raise ValueError("sector_ladder_direct: an operand is shorter than the task table was checked for")
        coef = (C.c_double * len(self.ladder_terms))(*[c for c, _ in self.ladder_terms])
        ctx.lib.call("pymes_sector_ladder_direct", ctx.handle, C.c_void_p(tasks.dev.ptr), tasks.count, tasks.tiles,
                     C.c_void_p(first_dev.ptr), C.c_void_p(rows_dev.ptr), C.c_void_p(k_dev.ptr), tab.n,
                     len(self.ladder_terms), _lib.ptr_array([t.handle.value for _, t in self.ladder_terms]), coef,
                     C.c_void_p(X.ptr), C.c_void_p(Y.ptr))

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


def _refuse_direct_ea(who, ints, *options):
    """The EA particle ladder reads V_abcd blocks of its own: not yet in direct form."""
    if getattr(ints, "direct", False) and any(isinstance(o, dict) and len(o.get("ea") or ()) for o in options):
        raise ValueError(who + ": the integrals carry a direct ladder, and the EA particle ladder reads stored V_abcd blocks: "
                         "evaluate them with ladder=\"stored\" for 'ea' targets")


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
    kernel multiplies it with the equally exact 0 of ``Tc`` there.

    ``both_sides`` (``UEG.eval_2b_triples(..., both_sides=True)``) adds the excitation-type partners that
    Lambda-(T) reads, VvR[i,a,b] = V[a, b, i, f*] and VoR[i,j,a] = V[a, m*, i, j]; they are None otherwise.  ``+`` and scaling
    (the transcorrelated Hamiltonian is ``only_2b + effect_2b``) go through ``ctx.lincomb``, so exact zeros stay exact zeros."""

    SIDES = ("Vv", "Vo", "VvR", "VoR")

    def __init__(self, ctx, ttab, own_ctx=False, both_sides=False):
        self.ctx, self.tables, self._own, self.both_sides = ctx, ttab, own_ctx, bool(both_sides)
        self.Vv = ctx.empty((ttab.no, ttab.nv, ttab.nv))
        self.Vo = ctx.empty((ttab.no, ttab.no, ttab.nv))
        self.VvR = ctx.empty((ttab.no, ttab.nv, ttab.nv)) if both_sides else None
        self.VoR = ctx.empty((ttab.no, ttab.no, ttab.nv)) if both_sides else None
        self._dev = None

    @property
    def nbytes(self):
        return sum(getattr(self, nm).nbytes for nm in self.SIDES if getattr(self, nm) is not None)

    def _combine(self, terms):
        out = SectorTriplesIntegrals(self.ctx, self.tables, both_sides=self.both_sides)
        out._dev = self._dev
        for nm in self.SIDES:
            if getattr(self, nm) is not None:
                self.ctx.lincomb(getattr(out, nm), [getattr(t, nm) for t, _ in terms], [c for _, c in terms])
        return out

    def __add__(self, other):
        if not isinstance(other, SectorTriplesIntegrals) or other.tables.tables is not self.tables.tables \
                or other.ctx is not self.ctx or other.both_sides != self.both_sides:
            raise ValueError("SectorTriplesIntegrals: only integrals of the same tables, context and sides can be added")
        return self._combine([(self, 1.0), (other, 1.0)])

    def __mul__(self, factor):
        return self._combine([(self, float(factor))])

    __rmul__ = __mul__

    def device_tables(self):
        """(k_int, orb_of, m_of as int32 device bytes; the implied map of ``Tc`` as an int64 gather map)"""
        if self._dev is None:
            t = self.tables
            outside = "triples tables: an index points outside its array"
            if t.m_of.max(initial=-1) >= t.no or t.orb_of.max() >= t.n:
                raise AssertionError(outside)
            imap = upload_map(self.ctx, t.implied_map, t.tables.nnz + 1, outside)
            self._dev = tuple(upload_i32(self.ctx, x) for x in (t.tables.k_int, t.orb_of, t.m_of)) + (imap,)
        return self._dev

    def close(self):
        if self._own and self.ctx.handle:
            self.ctx.close()


TRIPLES_WS_ENV, TRIPLES_WS_DEFAULT = "PYMES_SECTOR_TRIPLES_BYTES", 1 << 30


def triple_bytes(nv):
    """Workspace bytes of one triple in ``pymes_sector_triples``: the v x v slab, one partial per 32 x 32 tile, the value."""
    return 8 * (nv * nv + (-(-nv // 32)) ** 2 + 1)


def lambda_triple_bytes(nv):
    """Workspace bytes of one triple in ``pymes_sector_triples_lambda``: two v x v slabs, one partial per tile, the value."""
    return 8 * (2 * nv * nv + (-(-nv // 32)) ** 2 + 1)


def _hermitian(ints, rtol=1e-12):
    """V_klcd = V_cdkl, sector by sector: ``klcd``^P against ``abij``^P transposed."""
    tab = ints.tables
    sec, lr, lc = sectors._expand(tab.n_oo, tab.n_vv, 0, len(tab.P_keys))
    kl, ab = ints["klcd"].get(), ints["abij"].get()
    if not len(kl):
        return True
    return np.abs(kl - ab[tab.pp_off[sec] + lc * tab.n_oo[sec] + lr]).max() <= rtol * max(np.abs(ab).max(), 1e-300)


def _diagonal_eps(who, tab, eps, check_length=True):
    """The orbital energies as a vector, from a vector or from a diagonal Fock matrix."""
    eps = np.asarray(eps, dtype=np.float64)
    if eps.ndim == 2:
        if np.count_nonzero(eps - np.diag(eps.diagonal())):
            raise ValueError(who + ": the Fock matrix must be diagonal (it is for a momentum-conserving Hamiltonian)")
        eps = eps.diagonal().copy()
    if check_length and eps.shape != (tab.n,):
        raise ValueError(who + ": %d orbital energies for %d orbitals" % (eps.size, tab.n))
    return eps


def _exchange_symmetric(ints):
    """V_pqrs = V_qpsr where the product list needs it: the X_ac / X_ki sums read W1 where ccd.py:213-220 reads V_lkdc."""
    w1 = ints["w1"].get()
    return not len(w1) or np.abs(w1 - w1[ints.tables.d_partner]).max() <= 1e-12 * max(np.abs(w1).max(), 1e-300)


def _check_solver_inputs(who, no, eps, ints, dense_hint):
    """The refusals that ``SectorCCD.solve`` and ``SectorLambda.solve`` share; returns the orbital energies as a vector."""
    if not isinstance(ints, SectorIntegrals):
        raise TypeError(who + ": ints must be SectorIntegrals (UEG.eval_2b_sectors); the dense path is " + dense_hint)
    tab = ints.tables
    if ints.ctx.recording:
        raise RuntimeError(who + ": the context is recording a launch graph")
    eps = _diagonal_eps(who, tab, eps, check_length=False)
    if tab.no != no or eps.shape != (tab.n,):
        raise ValueError(who + ": the tables of the integrals (no = %d, n = %d) do not match the solver (no = %d) "
                         "and the %d orbital energies" % (tab.no, tab.n, no, eps.size))
    if not _exchange_symmetric(ints):
        raise ValueError(who + ": the integrals are not symmetric under the exchange of the two electrons "
                         "(V_pqrs = V_qpsr), which the sector residual needs")
    return eps


def _symmetric_compact(who, tab, amps, what, identity="(X_abij = X_baji)"):
    vec = SectorCCD._compact(tab, amps, "lambda" if what.startswith("lambda") else "amps")
    if len(vec) and np.abs(vec - vec[tab.pp_swap]).max() > 1e-13 * max(np.abs(vec).max(), 1e-300):
        raise ValueError(who + ": %s not exchange-symmetric %s" % (what, identity))
    return vec


def _check_triples(who, ints, tints, left=False):
    """The refusals of the (T) inputs that need no amplitudes (``SectorCCD.solve`` makes them before it iterates).  ``left``:
    for Lambda-(T), which needs both sides of the triples integrals and no Hermitian V."""
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
    if left:
        if not tints.both_sides:
            raise ValueError(who + ": the triples integrals lack the right-hand families VvR / VoR "
                             "(UEG.eval_2b_triples(..., both_sides=True))")
    elif not _hermitian(ints):
        raise ValueError(who + ": the integrals are not Hermitian (V_pqrs = V_rspq fails between the klcd and abij sectors); "
                         "(T) is not defined for transcorrelated integrals, and Lambda-(T) does not exist on sectors yet under "
                         "this keyword: pass the integrals of UEG.eval_2b_triples(..., both_sides=True) as lambda_triples= "
                         "to SectorCCD.solve, or call sector_lambda_triples_energy")


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
    return _triples_energy("sector_triples_energy", eps, ints, tints, amps, None, triple_range, per_triple, workspace_bytes)


def sector_lambda_triples_energy(eps, ints, tints, amps, lam, triple_range=None, per_triple=False, workspace_bytes=None):
    """E_Lambda(T) on the momentum sectors: the triples correction for integrals without V_pqrs = V_rspq (transcorrelated
    ones), the formulas of tests/_lambda_triples_reference.py with lam1 = None (singles vanish on the sectors), by
    ``pymes_sector_triples_lambda``.  With a Hermitian V and lam = 2 T - T^x it is the (T) of
    ``sector_triples_energy``.

    tints: ``UEG.eval_2b_triples(..., both_sides=True)``; amps and lam: ``SectorAmplitudes``, a compact vector or a dense
    [v,v,o,o] array, lam in the library's normalisation (``SectorLambda``; A^T lam + eta = 0).  Everything else as
    ``sector_triples_energy``: triple ranges, the split over ranks and the all-reduce, batches of as many triples as
    ``workspace_bytes`` hold (``lambda_triple_bytes(nv)`` each: two slabs).  Nothing asks for V_pqrs = V_rspq."""
    return _triples_energy("sector_lambda_triples_energy", eps, ints, tints, amps, lam, triple_range, per_triple,
                           workspace_bytes)


def _triples_energy(who, eps, ints, tints, amps, lam, triple_range, per_triple, workspace_bytes):
    """The driver behind ``sector_triples_energy`` (``lam`` None: one slab per triple, ``pymes_sector_triples``) and
    ``sector_lambda_triples_energy`` (two slabs, ``pymes_sector_triples_lambda``)."""
    left = lam is not None
    _check_triples(who, ints, tints, left=left)
    tab, ctx, tt = ints.tables, ints.ctx, tints.tables
    eps = _diagonal_eps(who, tab, eps)
    vec = _symmetric_compact(who, tab, amps, "the amplitudes are", "(X_abij = X_baji)" if left else "(T_abij = T_baji)")
    lvec = _symmetric_compact(who, tab, lam, "lambda is") if left else None
    no, nv = tab.no, tab.nv
    lo, hi, reduce = ccsd_t._triple_chunk(no, triple_range)
    if not 0 <= lo <= hi <= ccsd_t.n_triples(no):
        raise ValueError(who + ": triple range [%d, %d) outside [0, %d]" % (lo, hi, ccsd_t.n_triples(no)))
    if workspace_bytes is None:
        workspace_bytes = int(os.environ.get(TRIPLES_WS_ENV, TRIPLES_WS_DEFAULT))
    each = lambda_triple_bytes(nv) if left else triple_bytes(nv)
    ws_bytes = each * max(1, min(int(workspace_bytes) // each, max(hi - lo, 1)))
    k_dev, orb_dev, m_dev, imap = tints.device_tables()
    temps = []

    def temp(make, *args):                   # one at a time, so that whatever was allocated is freed if a later one fails
        temps.append(make(*args))
        return temps[-1]
    ptr = lambda arr: C.c_void_p(arr.ptr if arr is not None else None)
    e = C.c_double()
    try:
        src, Tc = temp(ctx.array, np.append(vec, 0.0)), temp(ctx.empty, (no, no, nv))
        operands = [Tc, tints.Vv, tints.Vo]
        if left:
            # Lc[i,j,a] = L[a,b*,i,j], L = (2 lam + lam^x) / 3: the implied map, and the same map behind the exchange of a and b
            a, b, i, j = tab.abij()
            swapped = temp(upload_map, ctx, np.append(tab._pp_index(b, a, i, j), tab.nnz)[tt.implied_map.reshape(-1)],
                           tab.nnz + 1)
            lsrc, Lc = temp(ctx.array, np.append(lvec, 0.0)), temp(ctx.empty, (no, no, nv))
            operands = [Tc, Lc, tints.VvR, tints.VoR, tints.Vv, tints.Vo]
        eps_dev, ws = temp(ctx.array, eps), temp(ctx.empty, (ws_bytes // 8,))
        out = temp(ctx.empty, (max(hi - lo, 1),)) if per_triple else None
        gather(ctx, Tc, src, imap)
        if left:
            gather(ctx, Lc, lsrc, imap, 2.0 / 3.0, lsrc, swapped, 1.0 / 3.0)
        ctx.lib.call("pymes_sector_triples_lambda" if left else "pymes_sector_triples", ctx.handle, no, nv, ptr(eps_dev),
                     ptr(k_dev), ptr(orb_dev), tt.box.ctypes.data_as(C.c_void_p), ptr(m_dev), *map(ptr, operands), int(lo),
                     int(hi), ptr(ws), int(ws_bytes), ptr(out), C.byref(e))
        values = out.get()[:hi - lo] if out is not None else None
    finally:
        for t in temps:
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
        ints.ladder(dt.ladder, T, R)
        # direct and crossed layouts of T, and Tt = 2 D - C
        dt.layouts(T, D, Cx, Tt)
        dt.to_square.run(ints["w1"], Tt, sq)                     # X^q = W1^q Tt^{-q}
        dt.from_square_neg.run(Tt, sq, Rd)                       # Rd^q = Tt^q X^{-q}                  (:202-204)
        dt.from_square_neg.run(Tt, ints["w2"], Ed)               # Ed^q = Tt^q W2^{-q}
        dt.square_left_sub.run(ints["wa"], D, Ed)                # Ed^q -= Wa^q D^q
        dt.from_square_neg_t.run(Cx, ints["wa"], Ec)             # Ec^q = -C^q Wb^{-q},  Wb = Wa^T
        if quad:
            CmD, Rc = ws["CmD"], ws["Rc"]
            dt.layouts(T, CmD=CmD)
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
    def _compact(tab, amps, name="amps"):
        if isinstance(amps, SectorAmplitudes):
            if amps.tables is not tab and not (np.array_equal(amps.tables.k_int, tab.k_int) and amps.tables.no == tab.no):
                raise ValueError("SectorCCD: the tables of the amplitudes do not match the integrals")
            vec = amps.get()
        else:
            vec = np.asarray(amps)
            vec = tab.compact(vec, name) if vec.ndim == 4 else vec
        vec = np.ascontiguousarray(vec, dtype=np.float64)
        if vec.shape != (tab.nnz,):
            raise ValueError("SectorCCD: the tables of the amplitudes do not match the integrals")
        return vec

    def _checks(self, eps, ints):
        return _check_solver_inputs("SectorCCD.solve", self.no, eps, ints, "CCD")

    def solve(self, eps, ints, level_shift=0., amps=None, triples=None, lambda_triples=None, density=False, quasiparticles=None,
              spectral=None, **kwargs):
        """The loop of ``CCD.solve`` (ccd.py:24-162) on the compact vector.  eps: the orbital energies (or a diagonal Fock
        matrix); ints: ``SectorIntegrals``.  ``triples``: the ``SectorTriplesIntegrals`` of the same tables; the result then
        also holds "(t) e" (``sector_triples_energy`` of the final amplitudes) and "ccd(t) e".  ``lambda_triples``: the
        ``SectorTriplesIntegrals`` with both sides (``UEG.eval_2b_triples(..., both_sides=True)``), for integrals without
        V_pqrs = V_rspq: Lambda is solved after the amplitudes (``SectorLambda``, threshold ``lambda_threshold``, default
        1e-8) and the result also holds "lambda2", "lambda (t) e" (``sector_lambda_triples_energy``) and "ccd(t)_lambda e".
        ``density``: Lambda is solved (once; shared with ``lambda_triples``) and the result also holds "lambda2", "lambda
        residual", "density" (the ``SectorDensity``), "n(k)", "density e" (L(eps, ints): the correlation energy again, from
        the densities), "structure factor" and "structure factor q" (DESIGN 8l).  ``quasiparticles``: a dictionary
        ``dict(tints=..., ip=[...], ea=[...], n_roots=1, ladders=...)`` -- ``tints`` the ``SectorTriplesIntegrals`` with both
        sides (it may be the object passed as ``lambda_triples``), ``ip`` / ``ea`` the target orbitals, ``ladders`` the
        ``SectorLadderIntegrals`` of the EA targets -- adds "ip e", "ea e" [targets, n_roots], "ip singles weight", "ea singles
        weight" and, with both lists, "qp gap" (``ueg_eom.sector_quasiparticles``).  ``spectral``: a dictionary
        ``dict(tints=..., omegas=..., eta=..., ip=[...], ea=[...], ladders=..., max_dim=...)`` adds the keys of
        ``ueg_eom.SectorSpectralFunction.solve`` (G, A(k, w), pole strengths); Lambda and the density are solved
        once, shared with ``density=True`` and ``lambda_triples``."""
        algo_name = "ccd.solve"
        time_ccd = time.time()
        eps = self._checks(eps, ints)
        _refuse_direct_ea("SectorCCD.solve", ints, quasiparticles, spectral)
        if triples is not None:
            _check_triples("SectorCCD.solve", ints, triples)
        if lambda_triples is not None:
            _check_triples("SectorCCD.solve", ints, lambda_triples, left=True)
        if quasiparticles is not None:
            if not isinstance(quasiparticles, dict) or "tints" not in quasiparticles:
                raise ValueError("SectorCCD.solve: quasiparticles must be a dictionary with 'tints' and the target lists 'ip' / 'ea'")
            _check_triples("SectorCCD.solve", ints, quasiparticles["tints"], left=True)
        if spectral is not None:
            if not isinstance(spectral, dict) or not {"tints", "omegas", "eta"} <= set(spectral):
                raise ValueError("SectorCCD.solve: spectral must be a dictionary with 'tints', 'omegas', 'eta' and the target lists "
                                 "'ip' / 'ea'")
            _check_triples("SectorCCD.solve", ints, spectral["tints"], left=True)
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
                t2.set(_symmetric_compact("SectorCCD.solve", tab, amps, "the amplitudes are",
                                          "(T_abij = T_baji), which the sector residual needs"))
            dE, iteration, e_last = np.abs(e_mp2), 0, e_mp2
            e_ccd = e_dir_ccd = e_ex_ccd = 0.
            while np.abs(dE) > delta_e and iteration <= max_iter:
                iteration += 1
                self.residual(ints, eps_dev, t2, r2, ws)                              # ccd.py:100-102
                dt2 = self._step(ctx, t2, r2, den, level_shift, dt_fixed)           # :123-127
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
            if lambda_triples is not None or density or spectral is not None:
                left = SectorLambda(no, kwargs.get("lambda_threshold", 1.e-8), is_dcd=self.is_dcd, is_diis=self.is_diis)
                lam = left.solve(eps, ints, out["t2 amp"], level_shift=level_shift, max_iter=kwargs.get("lambda_max_iter", 100))
                out["lambda2"] = lam["lambda2"]
            if density:
                out["lambda residual"] = lam["lambda residual"]
                dens = sector_density(eps, ints, out["t2 amp"], lam["lambda2"], is_dcd=self.is_dcd)
                out["density"], out["n(k)"] = dens, dens.momentum_distribution()
                out["density e"] = dens.lagrangian(eps, ints)
                out["structure factor"], out["structure factor q"] = dens.structure_factor()
                print_logging_info("Energy from the densities = {:.12f}".format(out["density e"]), level=1)
            if lambda_triples is not None:
                out["lambda (t) e"] = sector_lambda_triples_energy(eps, ints, lambda_triples, out["t2 amp"], lam["lambda2"])
                out["ccd(t)_lambda e"] = e_ccd + out["lambda (t) e"]
                print_logging_info("Lambda residual norm = {:.3e} after {} iterations".format(lam["lambda residual"],
                                                                                               lam["iterations"]), level=1)
                print_logging_info("Lambda-(T) correction = {:.12f}".format(out["lambda (t) e"]), level=1)
            if quasiparticles is not None:
                from pymes_amd.solver.ueg_eom import sector_quasiparticles
                out.update(sector_quasiparticles(no, eps, ints, out["t2 amp"], **quasiparticles))
            if spectral is not None:
                from pymes_amd.solver.ueg_eom import sector_spectral
                dens = out["density"] if density else sector_density(eps, ints, out["t2 amp"], lam["lambda2"], is_dcd=self.is_dcd)
                out.update(sector_spectral(no, eps, ints, out["t2 amp"], dens, **spectral))
            return out

    @staticmethod
    def _update(ctx, t_out, dt, t_in, r, den, shift):
        ctx.lib.call("pymes_sector_update", ctx.handle, C.c_void_p(t_out.ptr), C.c_void_p(dt.ptr if dt is not None else 0),
                     C.c_void_p(t_in.ptr if t_in is not None else 0), C.c_void_p(r.ptr), C.c_void_p(den.ptr), float(shift),
                     t_out.size)

    def _step(self, ctx, x, r, den, shift, dx_fixed):
        """x <- x + r / (den + shift), through the DIIS mixer if there is one (its log line is the caller's:
        ``mixer.log_last()``); returns the step dx.  The step of ``SectorCCD.solve`` and of ``SectorLambda.solve``."""
        if not self.is_diis:
            SectorCCD._update(ctx, x, dx_fixed, x, r, den, shift)
            return dx_fixed
        xn, dx = ctx.pool_get(x.shape), ctx.pool_get(x.shape)
        SectorCCD._update(ctx, xn, dx, x, r, den, shift)
        self.mixer.mix([dx], [xn], release=ctx.pool_put, out=[x], defer_log=True, native=True)
        return dx

    @staticmethod
    def _energy(ctx, ints, t2, dt2=None):
        """(direct, exchange, |T|^2, |dT|^2): ccd.py:256-262 on the compact vector, one launch and one synchronisation."""
        xs, ys = [t2, t2, t2], [ints["ed"], ints["ex"], t2]
        if dt2 is not None:
            xs, ys = xs + [dt2], ys + [dt2]
        d = ctx.dots(xs, ys)
        return 2.0 * d[0], -d[1], d[2], (d[3] if dt2 is not None else 0.0)


def hoist_amplitudes(ints, T, quad):
    """What depends on the amplitudes alone, shared by ``SectorLambda`` and the sector EOM (``ueg_eom.SectorIPEASigma``): the three
    layouts of T, X = W1 Tt, the hole intermediate I^P = V_klij^P (+ V_klcd^P T^P) and, with ``quad`` (CCD; always for the EOM,
    whose H-bar has the quadratic pieces also for DCD amplitudes), C - D and the squares Y = D Wx, Xc = C Wx."""
    ctx, tab, dt = ints.ctx, ints.tables, ints.device_tables()
    nnz, nsq = max(tab.nnz, 1), max(dt.nsq, 1)
    h = {"T": T, "D": ctx.empty((nnz,)), "C": ctx.empty((nnz,)), "Tt": ctx.empty((nnz,)), "X": ctx.empty((nsq,))}
    dt.layouts(T, h["D"], h["C"], h["Tt"])
    dt.to_square.run(ints["w1"], h["Tt"], h["X"])                      # X^q = W1^q Tt^{-q}
    h["hole"] = ints["klij"]
    if quad:
        h["hole"] = ctx.empty((max(ints.sizes["klij"], 1),)).copy_from(ints["klij"])
        dt.hole_quad.run(ints["klcd"], T, h["hole"])                   # I^P = V_klij^P + V_klcd^P T^P
        h["CmD"], h["Y"], h["Xc"] = ctx.empty((nnz,)), ctx.empty((nsq,)), ctx.empty((nsq,))
        dt.layouts(T, CmD=h["CmD"])
        dt.to_square.run(h["D"], ints["wx"], h["Y"])                   # Y^q = D^q Wx^{-q}
        dt.to_square.run(h["C"], ints["wx"], h["Xc"])                  # Xc^q = C^q Wx^{-q}
    return h


class SectorLambda:
    """The Lambda equations of the momentum-sector CCD / DCD: J(T)^T lam + eta = 0, J = dR/dT of the compact
    residual of ``SectorCCD.residual`` on the exchange-symmetric vectors, eta = 2 ed - ex, plain inner product over the
    compact elements (the dense library's convention: for CCD, ``lambda2.to_dense()`` is the lambda2 of ``Lambda_CCSD``;
    lambda1 vanishes like T1).  Lambda is the transpose of the Jacobian of the sector residual itself, so DCD has one too.
    The integrals need V_pqrs = V_qpsr only: no V_pqrs = V_rspq."""

    def __init__(self, no, threshold=1.e-8, is_dcd=False, is_diis=True):
        self.no, self.threshold, self.is_dcd, self.is_diis = no, threshold, is_dcd, is_diis
        self.max_iter = 100
        if self.is_diis:
            self.mixer = diis.DIIS(dim_space=6)

    def _checks(self, eps, ints, amps):
        who = "SectorLambda.solve"
        eps = _check_solver_inputs(who, self.no, eps, ints, "Lambda_CCSD")
        return eps, _symmetric_compact(who, ints.tables, amps, "the amplitudes are")

    _step = SectorCCD._step

    # ---- what depends on T alone (``hoist_amplitudes``), and eta ----------------------------------------------------------
    def hoist(self, ints, T):
        ctx, tab = ints.ctx, ints.tables
        h = hoist_amplitudes(ints, T, not self.is_dcd)
        h["eta"] = ctx.empty((max(tab.nnz, 1),))
        ctx.lincomb(h["eta"], [ints["ed"], ints["ex"]], [2.0, -1.0])
        h["zero"] = ctx.zeros((tab.n,))
        return h

    def workspace(self, ints):
        ctx, tab = ints.ctx, ints.tables
        nnz = max(tab.nnz, 1)
        ws = {k: ctx.empty((nnz,)) for k in ("yRd", "yRc", "yEd", "yEc", "zTt", "zD", "zC", "Gp", "Gs")}
        ws["Z"] = ctx.empty((max(ints.device_tables().nsq, 1),))
        ws["x"] = ctx.empty((tab.no * tab.nv + tab.n,))
        if not self.is_dcd:
            ws["zM"] = ctx.empty((nnz,))
            ws["sq"] = ctx.empty((max(ints.device_tables().nsq, 1),))
            ws["M"] = ctx.empty((max(ints.sizes["klij"], 1),))
        return ws

    # ---- G = J(T)^T lam + eta: the adjoint of every product of SectorCCD.residual (tests/_sector_lambda_reference.py) ------
    def residual(self, ints, eps_dev, h, lam, G, ws):
        ctx, tab, dt = ints.ctx, ints.tables, ints.device_tables()
        at = dt.adjoint()
        quad = not self.is_dcd
        w = 1.0 if quad else 0.5
        yRd, yRc, yEd, yEc, zTt, zD, zC, Gp, Z = (ws[k] for k in ("yRd", "yRc", "yEd", "yEc", "zTt", "zD", "zC", "Gp", "Z"))
        dt.cotangents(lam, yRd, yRc, yEd, yEc)
        # pp layout: G^P = eta^P + V_abcd^P^T lam^P + lam^P I^P^T + [CCD] V_klcd^P^T (T^P^T lam^P)
        Gp.copy_from(h["eta"])
        ints.ladder(at.ladder_t, lam, Gp)
        at.hole_t.run(lam, h["hole"], Gp)
        if quad:
            at.t_lam.run(h["T"], lam, ws["M"])
            at.hole_quad_t.run(ints["klcd"], ws["M"], Gp)
        # ph layouts: the cotangents of Tt, D and C
        at.sq_tn.run(h["Tt"], yRd, Z)                            # Z^q = Tt^{-q}^T yRd^{-q}             (of X, from Rd = Tt X)
        at.right_t.run(yRd, h["X"], zTt)                         # zTt^q = yRd^q X^{-q}^T
        at.right_t_add.run(yEd, ints["w2"], zTt)                 # zTt^q += yEd^q W2^{-q}^T
        at.left_tn_add.run(ints["w1"], Z, zTt)                   # zTt^q += W1^{-q}^T Z^{-q}            (X = W1 Tt)
        at.sq_t_left_neg.run(ints["wa"], yEd, zD)                # zD^q = -Wa^q^T yEd^q
        at.right_neg.run(yEc, ints["wa"], zC)                    # zC^q = -yEc^q Wa^{-q}                (Ec = -C Wa^T)
        if quad:
            sq = ws["sq"]
            at.sq_t_left.run(h["Y"], yEd, ws["zM"])              # zM^q = Y^q^T yEd^q                   (of C - D)
            at.outer.run(yEd, h["CmD"], sq)                      # zY^q = yEd^q (C^q - D^q)^T
            at.sq_right_t_add.run(sq, ints["wx"], zD)            # zD^q += zY^q Wx^{-q}^T               (Y = D Wx)
            at.sq_t_left_add.run(h["Xc"], yRc, zC)               # zC^q += Xc^q^T yRc^q
            at.outer.run(yRc, h["C"], sq)                        # zXc^q = yRc^q C^q^T
            at.sq_right_t_add.run(sq, ints["wx"], zC)            # zC^q += zXc^q Wx^{-q}^T              (Xc = C Wx)
        # the diagonal X_ac / X_ki term, Ed[g,:] += scale(T)[g] D[g,:]: zD[g,:] += scale(T)[g] yEd[g,:] is the forward call
        # with yEd in the place of D; zTt[g,:] -= w (rho_a + rho_i) W1[g,:], rho the row sums of yEd o D, is the same call with
        # the operands exchanged and eps = 0
        rows = (C.c_void_p(dt.row_start.ptr), C.c_void_p(dt.row_len.ptr), C.c_void_p(dt.row_of.ptr), C.c_void_p(dt.ai_of.ptr),
                C.c_void_p(ws["x"].ptr))
        ctx.lib.call("pymes_sector_xdiag", ctx.handle, C.c_void_p(h["Tt"].ptr), C.c_void_p(ints["w1"].ptr), C.c_void_p(yEd.ptr),
                     C.c_void_p(zD.ptr), C.c_void_p(eps_dev.ptr), w, tab.no, tab.nv, *rows)
        ctx.lib.call("pymes_sector_xdiag", ctx.handle, C.c_void_p(yEd.ptr), C.c_void_p(h["D"].ptr), C.c_void_p(ints["w1"].ptr),
                     C.c_void_p(zTt.ptr), C.c_void_p(h["zero"].ptr), w, tab.no, tab.nv, *rows)
        # back to the pp vector through the inverse maps (D = T[d_from_pp], C = T[c_from_pp], Tt = 2 D - C) ...
        gather(ctx, Gp, zD, dt.pp_to_d, 1.0, zC, dt.pp_to_c, 1.0, beta=1.0)
        gather(ctx, Gp, zTt, dt.pp_to_d, 2.0, zTt, dt.pp_to_c, -1.0, beta=1.0)
        if quad:
            gather(ctx, Gp, ws["zM"], dt.pp_to_c, 1.0, ws["zM"], dt.pp_to_d, -1.0, beta=1.0)
        # ... and on the exchange-symmetric vectors: the plain adjoint is not symmetric.  0.5 x + 0.5 y is one
        # rounding of the exact mean whichever comes first, so G is symmetric to the bit
        gather(ctx, ws["Gs"], Gp, at.pp_swap)
        ctx.lincomb(G, [Gp, ws["Gs"]], [0.5, 0.5])
        return G

    def get_residual(self, eps, ints, amps, lam):
        """G(lam) = J(T)^T lam + eta for compact (or dense) amplitudes and lambda, as a host vector."""
        tab, ctx = ints.tables, ints.ctx
        T, L = ctx.array(SectorCCD._compact(tab, amps)), ctx.array(SectorCCD._compact(tab, lam, "lambda"))
        G = self.residual(ints, ctx.array(np.asarray(eps, dtype=np.float64)), self.hoist(ints, T), L, ctx.empty((tab.nnz,)),
                          self.workspace(ints))
        return G.get()

    def solve(self, eps, ints, amps, level_shift=0., lam=None, **kwargs):
        """lam <- lam + G(lam) / (den + level_shift) with the DIIS mixer, from lam = 0 (or ``lam``), until |G| is below the
        threshold.  Returns {"lambda2": SectorAmplitudes, "lambda residual": |G|, "iterations", "converged"}."""
        eps, vec = self._checks(eps, ints, amps)
        tab, ctx = ints.tables, ints.ctx
        max_iter, threshold = kwargs.get("max_iter", self.max_iter), kwargs.get("threshold", self.threshold)
        n = tab.nnz
        start = np.zeros(n) if lam is None else _symmetric_compact("SectorLambda.solve", tab, lam, "lambda is")
        with quiet_collector():
            eps_dev, den = ctx.array(eps), ctx.array(tab.denominators(eps))
            h, ws = self.hoist(ints, ctx.array(vec)), self.workspace(ints)
            l2, g2 = ctx.pool_get((n,)), ctx.pool_get((n,))
            l2.set(start)
            dl_fixed = None if self.is_diis else ctx.pool_get((n,))
            iteration, norm, converged = 0, np.inf, False
            while True:
                self.residual(ints, eps_dev, h, l2, g2, ws)
                norm = float(np.sqrt(ctx.dots([g2], [g2])[0]))
                print_logging_info("Lambda iteration = ", iteration, " |G| = {:.6e}".format(norm), level=2)
                converged = norm <= threshold
                if converged or iteration >= max_iter:
                    break
                iteration += 1
                self._step(ctx, l2, g2, den, level_shift, dl_fixed)
                if self.is_diis:
                    self.mixer.log_last()
            if not converged:
                print_logging_info("A converged Lambda is not found!", level=1)
            self.iterations = iteration
            result = ctx.empty((n,)).copy_from(l2)
            ctx.pool_put(l2)
            ctx.pool_put(g2)
            return {"lambda2": SectorAmplitudes(tab, result), "lambda residual": norm, "iterations": iteration,
                    "converged": converged}


def sector_density(eps, ints, amps, lam, is_dcd=False):
    """The one- and two-particle response densities of the momentum-sector CCD / DCD (``SectorDensity``) for
    amplitudes and their Lambda (``SectorLambda``; both ``SectorAmplitudes``, a compact vector or a dense [v,v,o,o] array,
    exchange-symmetric).  eps: the orbital energies (or a diagonal Fock matrix); ints: the ``SectorIntegrals`` whose tables
    and context the density lives in (the densities themselves do not read the integrals).  Refused: anything but
    ``SectorIntegrals``, amplitudes of other tables, off the support or not symmetric, a non-diagonal Fock matrix, a recording
    context."""
    who = "sector_density"
    if not isinstance(ints, SectorIntegrals):
        raise TypeError(who + ": ints must be SectorIntegrals (UEG.eval_2b_sectors); the dense path is Lambda_CCSD.rdm2")
    tab = ints.tables
    if ints.ctx.recording:
        raise RuntimeError(who + ": the context is recording a launch graph")
    eps = _diagonal_eps(who, tab, eps)
    vec = _symmetric_compact(who, tab, amps, "the amplitudes are")
    lvec = _symmetric_compact(who, tab, lam, "lambda is")
    return SectorDensity(ints, eps, vec, lvec, is_dcd)


class SectorDensity:
    """gamma and the density arena G of L(eps, V) = E(T; V) + <lam, R(T; eps, V)> at fixed (T, lam) on the momentum sectors
    (DESIGN 8l): gamma_p = dL/d eps_p (diagonal: momentum is conserved), G = dL/d(arena), one number per stored integral element
    of every family of ``sectors.BLOCKS`` but ``abcd``, whose part is formed on the fly (<lam, W_abcd T> through the ladder
    product; the fused ``pymes_sector_pair_transfer`` for the transfer sums).  L is linear in (eps, V), so for every operator W
    held as ``SectorIntegrals``, L(eps_W, W) = gamma . eps_W + <G, W>.  Built as the term-by-term adjoint of the product list of
    ``SectorCCD.residual`` with respect to its integral operands (tests/_sector_density_reference.py), so DCD has one too.
    Made by ``sector_density``."""

    FAMILIES = sectors.TransferBins.STORED

    def __init__(self, ints, eps, vec, lvec, is_dcd=False):
        ctx, tab = ints.ctx, ints.tables
        self.ctx, self.tables, self.is_dcd, self.eps = ctx, tab, bool(is_dcd), eps
        self._dt = ints.device_tables()
        sizes = [ints.sizes[nm] for nm in self.FAMILIES]
        self.offsets = dict(zip(self.FAMILIES, np.concatenate(([0], np.cumsum(sizes)))[:-1]))
        self.sizes = dict(zip(self.FAMILIES, sizes))
        self.arena = ctx.empty((max(int(sum(sizes)), 1),))
        self.gamma = ctx.empty((tab.n,))
        self.T, self.lam = ctx.array(vec), ctx.array(lvec)
        self._bins = self._bins_dev = None
        self._build()

    def __getitem__(self, name):
        return view(self.arena, self.offsets[name], self.sizes[name])

    def _build(self):
        ctx, tab, dt = self.ctx, self.tables, self._dt
        dn = dt.density()
        quad = not self.is_dcd
        nnz, nsq = max(tab.nnz, 1), max(dt.nsq, 1)
        T, lam = self.T, self.lam
        D, Cx, Tt, yRd, yRc, yEd, yEc = (ctx.empty((nnz,)) for _ in range(7))
        Z = ctx.empty((nsq,))
        # the simple members: G_abij = lam, G_ed = 2 T, G_ex = -T, and the pp layout
        self["abij"].copy_from(lam)
        ctx.lincomb(self["ed"], [T], [2.0])
        ctx.lincomb(self["ex"], [T], [-1.0])
        M = self["klij"]
        dn.t_lam.run(T, lam, M)                                  # G_klij^P = M^P = (T^P)^T lam^P
        if quad:
            dn.m_tt.run(M, T, self["klcd"])                      # G_klcd^P = M^P (T^P)^T
        else:
            self["klcd"].zero_()
            self["wx"].zero_()
        # the ph layouts of T and the cotangents of Rd, Rc, Ed, Ec (the first rows of the table of DESIGN 8k)
        dt.layouts(T, D, Cx, Tt)
        dt.cotangents(lam, yRd, yRc, yEd, yEc)
        dn.sq_tn.run(Tt, yRd, Z)                                 # Z^q = (Tt^{-q})^T yRd^{-q}          (of X = W1 Tt)
        dn.sq_right_t.run(Z, Tt, self["w1"])                     # G_w1^q = Z^q (Tt^{-q})^T
        dn.sq_tn.run(Tt, yEd, self["w2"])                        # G_w2^q = (Tt^{-q})^T yEd^{-q}       (Ed = Tt W2)
        dn.outer_neg.run(yEd, D, self["wa"])                     # G_wa^q = -yEd^q (D^q)^T             (Ed -= Wa D)
        dn.sq_tn_sub.run(yEc, Cx, self["wa"])                    # G_wa^q -= (yEc^{-q})^T C^{-q}       (Ec = -C Wa^T)
        if quad:
            CmD = ctx.empty((nnz,))
            dt.layouts(T, CmD=CmD)
            dn.outer.run(yEd, CmD, Z)                            # zY^q = yEd^q (C^q - D^q)^T
            dn.left_tn.run(D, Z, self["wx"])                     # G_wx^q = (D^{-q})^T zY^{-q}         (Y = D Wx)
            dn.outer.run(yRc, Cx, Z)                             # zXc^q = yRc^q (C^q)^T
            dn.left_tn_add.run(Cx, Z, self["wx"])                # G_wx^q += (C^{-q})^T zXc^{-q}       (Xc = C Wx)
        # the diagonal X_ac / X_ki term: rho the row sums of yEd o D; gamma is rho summed by orbital, and its W1 part
        # G_w1[g,:] -= w (rho_a + rho_i) Tt[g,:] is the second call of SectorLambda.residual with W1 and Tt exchanged
        rows = (C.c_void_p(dt.row_start.ptr), C.c_void_p(dt.row_len.ptr), C.c_void_p(dt.row_of.ptr))
        scratch, zero = ctx.empty((tab.no * tab.nv + tab.n,)), ctx.zeros((tab.n,))
        ctx.lib.call("pymes_sector_gamma", ctx.handle, C.c_void_p(yEd.ptr), C.c_void_p(D.ptr), tab.no, tab.nv, *rows,
                     C.c_void_p(self.gamma.ptr), C.c_void_p(scratch.ptr))
        ctx.lib.call("pymes_sector_xdiag", ctx.handle, C.c_void_p(yEd.ptr), C.c_void_p(D.ptr), C.c_void_p(Tt.ptr),
                     C.c_void_p(self["w1"].ptr), C.c_void_p(zero.ptr), 1.0 if quad else 0.5, tab.no, tab.nv, *rows,
                     C.c_void_p(dt.ai_of.ptr), C.c_void_p(scratch.ptr))

    # ---- one-body ---------------------------------------------------------------------------------------------------
    def momentum_distribution(self):
        """n(k_p) = gamma_p + 2 [p occupied], per orbital (host array)."""
        n = self.gamma.get()
        n[:self.tables.no] += 2.0
        return n

    # ---- expectation values -----------------------------------------------------------------------------------------
    def _operator(self, who, W):
        if not isinstance(W, SectorIntegrals):
            raise TypeError(who + ": W must be SectorIntegrals (UEG.eval_2b_sectors)")
        if W.tables is not self.tables or W.ctx is not self.ctx:
            raise ValueError(who + ": W belongs to other tables or another context than the density")
        if self.ctx.recording:
            raise RuntimeError(who + ": the context is recording a launch graph")
        if not _exchange_symmetric(W):
            raise ValueError(who + ": W is not symmetric under the exchange of the two electrons (W_pqrs = W_qpsr), which "
                             "the sector densities need")

    def lagrangian(self, eps, W):
        """L(eps, W) = gamma . eps + <G, W>: one fixed-tree dot per stored family, <lam, W_abcd T> for the ladder block."""
        who = "SectorDensity.lagrangian"
        self._operator(who, W)
        return self._lagrangian(_diagonal_eps(who, self.tables, eps), W)

    def _lagrangian(self, eps, W):
        ctx, tab = self.ctx, self.tables
        ladder = ctx.zeros((max(tab.nnz, 1),))
        W.ladder(self._dt.ladder, self.T, ladder)
        live = [nm for nm in self.FAMILIES if self.sizes[nm]]
        xs, ys = [self[nm] for nm in live], [W[nm] for nm in live]
        if tab.nnz:
            xs, ys = xs + [self.lam], ys + [view(ladder, 0, tab.nnz)]
        d = ctx.dots(xs + [self.gamma], ys + [ctx.array(eps)])
        return float(np.sum(d))

    def expectation(self, W, one_body=None, mean_field=True):
        """The expectation value of the two-body operator W (``SectorIntegrals`` with W_pqrs = W_qpsr) and, if given, of the
        diagonal one-body operator ``one_body`` (one number per orbital): L(one_body + f_HF[W], W), f_HF[W]_p =
        sum_i (2 W_pipi - W_piip) as in ``hf_orbital_energies``, without the reference determinant's own value.  With W the
        Hamiltonian's integrals and the kinetic energies it is the correlation energy of converged amplitudes.
        ``mean_field=False`` leaves f_HF[W] out, L(one_body, W): the derivative of the energy along W when the orbital
        energies are held fixed."""
        who = "SectorDensity.expectation"
        self._operator(who, W)
        kinetic = np.zeros(self.tables.n) if one_body is None else np.asarray(one_body, dtype=np.float64)
        if kinetic.shape != (self.tables.n,):
            raise ValueError(who + ": one number per orbital is needed for the one-body operator")
        return self._lagrangian(W.hf_orbital_energies(kinetic) if mean_field else kinetic, W)

    # ---- transfer sums and the structure factor ---------------------------------------------------------------------
    def bins(self):
        if self._bins is None:
            self._bins = sectors.TransferBins(self.tables)
        return self._bins

    def _bin_tables(self):
        """The CSR of every stored family, the bin vectors and the rows of the pp layout on the device, checked first (the
        kernels trust them)."""
        if self._bins_dev is None:
            ctx, tab, tb = self.ctx, self.tables, self.bins()
            imap = lambda host, limit: upload_map(ctx, host, limit, "transfer bins: an index points outside its array", -1)
            i32 = lambda host: upload_i32(ctx, host)
            csr = {}
            for nm in self.FAMILIES:
                off, order = tb.csr[nm]
                if off[0] != 0 or off[-1] != self.sizes[nm] or (np.diff(off) < 0).any() or len(order) != self.sizes[nm] \
                        or (len(order) and order.min() < 0):
                    raise AssertionError("transfer bins: the lists of family %s do not cover it" % nm)
                csr[nm] = (imap(off, self.sizes[nm] + 1), imap(order, max(self.sizes[nm], 1)))
            tt = TriplesTables(tab)
            vv, start, length, of_pair = tb.pair_rows()
            if len(vv) and (vv.min() < 0 or vv.max() >= tab.nv or start.min() < 0 or (start + length).max() > tab.nnz
                            or tt.orb_of.max() >= tab.n):
                raise AssertionError("transfer bins: a row of the pp layout points outside the compact vector")
            self._bins_dev = {"csr": csr, "q": i32(tb.q), "k": i32(tab.k_int), "orb": i32(tt.orb_of), "box": tt.box,
                              "rows": len(vv), "vv": i32(vv), "start": imap(start, tab.nnz + 1),
                              "len": imap(length, tab.nnz + 1), "of_pair": imap(of_pair, max(len(vv), 1))}
        return self._bins_dev

    def stored_transfer(self, out=None):
        """The stored families' part of s(q) on the device: one launch of ``pymes_sector_bin_sums`` per family."""
        ctx, tb, bd = self.ctx, self.bins(), self._bin_tables()
        out = ctx.empty((tb.nbins,)) if out is None else out
        for n, nm in enumerate(self.FAMILIES):
            off, order = bd["csr"][nm]
            ctx.lib.call("pymes_sector_bin_sums", ctx.handle, C.c_void_p(out.ptr), tb.nbins, C.c_void_p(off.ptr),
                         C.c_void_p(order.ptr), C.c_void_p(self[nm].ptr), 1.0, 0.0 if n == 0 else 1.0)
        return out

    def pair_transfer(self, out=None, max_groups=0):
        """The ``abcd`` part of s(q) on the device (``pymes_sector_pair_transfer``)."""
        ctx, tab, tb, bd = self.ctx, self.tables, self.bins(), self._bin_tables()
        out = ctx.empty((tb.nbins,)) if out is None else out
        ctx.lib.call("pymes_sector_pair_transfer", ctx.handle, C.c_void_p(out.ptr), tb.nbins, C.c_void_p(bd["q"].ptr),
                     C.c_void_p(bd["k"].ptr), C.c_void_p(bd["orb"].ptr), bd["box"].ctypes.data_as(C.c_void_p), tab.no, tab.nv,
                     bd["rows"], C.c_void_p(bd["vv"].ptr), C.c_void_p(bd["start"].ptr), C.c_void_p(bd["len"].ptr),
                     C.c_void_p(bd["of_pair"].ptr), C.c_void_p(self.lam.ptr), C.c_void_p(self.T.ptr), int(max_groups))
        return out

    def transfer_sums(self, symmetrize=True):
        """(s per bin, the bin vectors [bins,3]): s(q) = the sum of G over all families and elements (p,q,r,s) with
        k_r - k_p = q.  The plain s is not even in q (the product list treats the two electrons differently);
        ``symmetrize`` returns S2(q) = (s(q) + s(-q)) / 2, which goes with Gamma_pqrs = (G_pqrs + G_qpsr) / 2."""
        if self.ctx.recording:
            raise RuntimeError("SectorDensity.transfer_sums: the context is recording a launch graph")
        tb = self.bins()
        s = self.stored_transfer().get() + self.pair_transfer().get()
        if symmetrize:
            s = 0.5 * s + 0.5 * s[tb.neg]
        return s, tb.q

    def structure_factor(self, shells=False):
        """(S(q) per bin, the bin vectors), in the convention of ``lambda_ccsd.full_rdm2``: for q != 0
        S(q) = 1 + [-2 #{(i,j): k_j - k_i = q} - sum_{i,p: k_i - k_p = +-q} gamma_p + 2 S2(q)] / N, and S(0) = N.  ``shells``:
        (the average of S over the bins of equal |q|^2, those |q|^2 in units of the integer vectors)."""
        tb, N = self.bins(), 2 * self.tables.no
        s2, q = self.transfer_sums(symmetrize=True)
        bracket = tb.reference_terms(self.gamma.get()) + 2.0 * s2
        bracket[tb.zero] = N * (N - 1)
        S = 1.0 + bracket / N
        if not shells:
            return S, q
        values, shell = tb.shells()
        return np.bincount(shell, weights=S) / np.bincount(shell), values
