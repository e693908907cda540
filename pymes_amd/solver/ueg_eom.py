"""Momentum-blocked IP- and EA-EOM-CCD for the electron gas on the sector path: ionisation and attachment energies
per momentum, E(N -+ 1; -+ k_p) - E(N), at sizes where no dense V fits; also for integrals without V_pqrs = V_rspq (the
transcorrelated Hamiltonian).

The operator is the one of ``eom_ip_ea`` (the term tables of tests/_ipea_reference.py) with t1 = 0 and a diagonal Fock matrix:
"the CCD-type H-bar with the amplitudes given", a function of (eps, V, T) for any exchange-symmetric T on the support, whether it
came from CCD or DCD.  H-bar conserves the momentum, so the operator is block diagonal in the momentum of the removed or added
electron; one block is the singles element r1[p] of the target orbital p and the doubles with their implied virtual left out,

  IP  R[i,j] = r2[i, j, b*], [o,o], k_b* = k_i + k_j - k_p        EA  R[a,j] = r2[a, b*, j], [v,o], k_b* = k_p + k_j - k_a

(``sectors.QuasiparticleTables``).  ``SectorIPEASigma`` applies it to stacked vectors: what depends on T alone is hoisted once per
object (``ueg_cc.hoist_amplitudes``, shared with ``SectorLambda``, the three ring squares PA / PB / MDU of DESIGN 8c and L_oo, L_vv),
what depends on the target once per target (``pymes_sector_ipea_prepare``), and one apply is a pack kernel, the ragged products
``pymes_sector_gemm`` with task tables per (kind, target, k), and an assembly kernel.  ``SectorIP_EOM_CCD`` / ``SectorEA_EOM_CCD``
run ``subspace.block_davidson`` once per target.  The numpy restatement the tests compare with is
tests/_sector_ipea_reference.py."""
import ctypes as C
import functools
import time
from types import SimpleNamespace

import numpy as np

from pymes_amd import _lib
from pymes_amd.log import print_logging_info
from pymes_amd.solver import sectors, subspace
from pymes_amd.solver.ccd import quiet_collector
from pymes_amd.solver.sectors import QuasiparticleTables, TriplesTables
from pymes_amd.solver.ueg_cc import (SectorIntegrals, Tasks, _check_solver_inputs, _check_triples, _refuse_direct_ea,
                                     _symmetric_compact, gather, hoist_amplitudes, upload_i32, upload_map, view)

__all__ = ["SectorLadderIntegrals", "SectorIPEAHoist", "SectorIPEASigma", "SectorIP_EOM_CCD", "SectorEA_EOM_CCD",
           "sector_quasiparticles", "SectorSpectralFunction", "KrylovBasis", "sector_spectral"]

MAX_STACK = 32          # vectors per launch of the pack and assembly kernels (kQpMax of kernels_sector.hip)


class SectorLadderIntegrals:
    """The one block family of the EA operator that ``SectorIntegrals`` does not hold (``UEG.eval_2b_ladder``): its particle ladder
    sum_cd V_abcd r2[c,d,j] runs over the virtual pairs of the pair momentum P = k_p + k_j, p the virtual target, and such a P need
    not be the sum of two occupied momenta -- the only pair momenta for which ``SectorIntegrals`` stores V_abcd.  Per target: the
    blocks V[(a,b),(c,d)] of the columns j without a pp sector (``QuasiparticleTables.extra_pqrs``), one arena.  Every other term
    of either operator reads a stored family.  Supports ``+`` and scaling like the other sector integrals."""

    def __init__(self, ctx, ttab, targets):
        self.ctx, self.tables = ctx, ttab
        self.qtabs = {int(p): QuasiparticleTables(ttab, "ea", int(p)) for p in targets}
        self.arenas = {p: ctx.empty((max(qt.extra_size, 1),)) for p, qt in self.qtabs.items()}

    @property
    def nbytes(self):
        return 8 * sum(qt.extra_size for qt in self.qtabs.values())

    def _combine(self, terms):
        out = SectorLadderIntegrals(self.ctx, self.tables, [])
        out.qtabs = self.qtabs
        for p in self.qtabs:
            out.arenas[p] = self.ctx.empty(self.arenas[p].shape)
            self.ctx.lincomb(out.arenas[p], [t.arenas[p] for t, _ in terms], [c for _, c in terms])
        return out

    def __add__(self, other):
        if not isinstance(other, SectorLadderIntegrals) or other.ctx is not self.ctx \
                or other.tables.tables is not self.tables.tables or sorted(other.qtabs) != sorted(self.qtabs):
            raise ValueError("SectorLadderIntegrals: only integrals of the same tables, context and targets can be added")
        return self._combine([(self, 1.0), (other, 1.0)])

    def __mul__(self, factor):
        return self._combine([(self, float(factor))])

    __rmul__ = __mul__

    def close(self):
        """Frees the arenas."""
        for arr in self.arenas.values():
            arr.free()
        self.arenas = {}


def _triples_tables(tints):
    return tints.tables if isinstance(tints.tables, TriplesTables) else TriplesTables(tints.tables)


class SectorIPEAHoist:
    """What the sector IP and EA operators need of (eps, V, T) alone, built once and shared by all targets and both kinds: the
    checks of the inputs, ``hoist_amplitudes`` (the layouts of T, I^P, X, Y, Xc: the function ``SectorLambda.hoist`` calls too),
    the three ring squares PA, PB, MDU of DESIGN 8c on the ph sectors, L_oo and L_vv (the x of ``pymes_sector_xdiag`` with
    w = 1), and Tc as the triples read it.  Arguments as ``SectorIPEASigma``; ``close()`` frees it (its owner's job: a
    ``SectorIPEASigma`` closes only a hoist it made itself)."""

    def __init__(self, eps, ints, tints, amps, who="SectorIPEAHoist"):
        no = ints.tables.no if isinstance(ints, SectorIntegrals) else 0
        eps = _check_solver_inputs(who, no, eps, ints, "IP_EOM_CCSD / EA_EOM_CCSD")
        _check_triples(who, ints, tints, left=True)
        tab, ctx = ints.tables, ints.ctx
        vec = _symmetric_compact(who, tab, amps, "the amplitudes are")
        self.ctx, self.ints, self.tints, self.tables, self.ttab = ctx, ints, tints, tab, _triples_tables(tints)
        self._own = []
        dt = ints.device_tables()
        keep = self._own.append
        T = ctx.array(vec)
        h = hoist_amplitudes(ints, T, True)
        self._own += list(h.values())
        self.T, self.hole = T, h["hole"]
        nsq, nnz = max(dt.nsq, 1), max(tab.nnz, 1)
        ident = upload_map(ctx, np.arange(dt.nsq), nsq)
        trans = upload_map(ctx, sectors.square_transpose(tab), nsq)
        m1 = ctx.empty((nsq,))                             # M1^T = W2 + X as [(d,l),(a,i)]
        self.PA, self.PB, self.MDU = (ctx.empty((nsq,)) for _ in range(3))
        for arr in (self.PA, self.PB, self.MDU):
            keep(arr)
        if dt.nsq:
            ctx.lincomb(m1, [ints["w2"], h["X"]], [1.0, 1.0])
            ctx.lincomb(self.MDU, [h["Xc"], ints["wa"]], [1.0, -1.0])                   # MDU = Xc - Wa
            gather(ctx, self.PB, h["Y"], ident, 1.0, m1, trans, -1.0)                   # PB = Y - M1
            gather(ctx, self.PA, m1, trans, 2.0, h["Y"], ident, -2.0)                   # PA = 2 M1 - 2 Y + MDU
            gather(ctx, self.PA, self.MDU, ident, beta=1.0)
        # L_oo, L_vv: the x of pymes_sector_xdiag with w = 1 (its row scaling goes into a vector nobody reads)
        ws, junk, eps_dev = ctx.empty((tab.no * tab.nv + tab.n,)), ctx.zeros((nnz,)), ctx.array(eps)
        keep(ws)
        ctx.lib.call("pymes_sector_xdiag", ctx.handle, C.c_void_p(h["Tt"].ptr), C.c_void_p(ints["w1"].ptr), C.c_void_p(h["D"].ptr),
                     C.c_void_p(junk.ptr), C.c_void_p(eps_dev.ptr), 1.0, tab.no, tab.nv, C.c_void_p(dt.row_start.ptr),
                     C.c_void_p(dt.row_len.ptr), C.c_void_p(dt.row_of.ptr), C.c_void_p(dt.ai_of.ptr), C.c_void_p(ws.ptr))
        self.L = view(ws, tab.no * tab.nv, tab.n)
        self.L_host = self.L.get()
        # Tc[i,j,a] = T[a,b*,i,j], as the triples read it
        self.k_dev, self.orb_dev, _, imap = tints.device_tables()
        src = ctx.array(np.append(vec, 0.0))
        self.Tc = ctx.empty((tab.no, tab.no, tab.nv))
        keep(self.Tc)
        gather(ctx, self.Tc, src, imap)
        for arr in (ident, trans, m1, junk, eps_dev, src):
            arr.free()

    def close(self):
        for arr in self._own:
            if getattr(arr, "_owned", True):           # (a view belongs to whoever owns its arena)
                arr.free()
        self._own = []


class SectorIPEASigma:
    """sigma = H-bar r on the momentum blocks of the IP (``kind`` "ip") or EA ("ea") operator, for stacked vectors.

    eps: the orbital energies (or a diagonal Fock matrix); ints: ``SectorIntegrals``; tints: the ``SectorTriplesIntegrals`` with
    both sides (``UEG.eval_2b_triples(..., both_sides=True)``) of the same tables and context -- they hold the complete ooov /
    vooo / ovvv / vvov blocks, which couple the singles element to the doubles; amps: ``SectorAmplitudes``, a compact vector or a
    dense [v,v,o,o] array with T_abij = T_baji (from CCD or DCD: the quadratic pieces of H-bar are always built).  ladders: the
    ``SectorLadderIntegrals`` of ``UEG.eval_2b_ladder`` for the EA targets whose particle ladder needs pair momenta outside the
    stored V_abcd sectors.  hoist: a ``SectorIPEAHoist`` of the same (eps, ints, tints, amps), so that an IP and an EA operator
    share one; without it the object builds (and closes) its own.  Needs V_pqrs = V_qpsr and no hermiticity.

    A target is an orbital index over all n: occupied for IP, virtual for EA.  A vector of its block is (r1 [1], R ``shape(target)``);
    a position outside the space holds an exact 0.0 and its sigma is an exact +0.0.  No atomics: identical applies give identical
    bits, and a vector's sigma does not depend on the vectors it is stacked with."""

    def __init__(self, kind, eps, ints, tints, amps, ladders=None, hoist=None):
        who = "SectorIPEASigma"
        if kind not in QuasiparticleTables.KINDS:
            raise ValueError(who + ": kind must be 'ip' or 'ea'")
        if hoist is not None and (not isinstance(hoist, SectorIPEAHoist) or hoist.ints is not ints or hoist.tints is not tints):
            raise ValueError(who + ": the hoist belongs to other integrals")
        if kind == "ea":
            _refuse_direct_ea(who, ints, {"ea": [0]})
        self._own_hoist = hoist is None
        self.hoist = h = SectorIPEAHoist(eps, ints, tints, amps, who) if hoist is None else hoist
        tab, ctx = h.tables, h.ctx
        if ladders is not None and (not isinstance(ladders, SectorLadderIntegrals) or ladders.ctx is not ctx
                                    or not np.array_equal(ladders.tables.tables.k_int, tab.k_int) or kind != "ea"):
            if self._own_hoist:
                h.close()
            raise ValueError(who + ": ladders must be the SectorLadderIntegrals (UEG.eval_2b_ladder) of the same tables and "
                             "context, and only the EA operator reads them")
        self.kind, self.ctx, self.ints, self.tints, self.ladders = kind, ctx, ints, tints, ladders
        self.tables, self.ttab, self.L_host = tab, h.ttab, h.L_host
        self._targets = {}

    # ---- per target ------------------------------------------------------------------------------------------------------
    def _target(self, target):
        """What one target holds: ``qt`` its QuasiparticleTables; ``ph``, ``ph_partner``, ``pair``, ``partner`` the maps on the
        device; ``layout`` and ``d`` the flat layout and the flat diagonal; ``d1``; ``U``, ``W`` the couplings to the singles
        element; ``extra`` the arena of the extra ladder family or None; ``own`` the device arrays to free with it; ``work`` per
        number of stacked vectors k the task tables and the buffers of one apply."""
        p = int(target)
        if p in self._targets:
            return self._targets[p]
        if self.ctx.recording:
            raise RuntimeError("SectorIPEASigma: the context is recording a launch graph")
        who, ctx, tab, tt, h = "SectorIPEASigma", self.ctx, self.tables, self.ttab, self.hoist
        if self.kind == "ip" and not 0 <= p < tab.no:
            raise ValueError(who + ": the IP target %d is not an occupied orbital (0 <= p < %d)" % (p, tab.no))
        if self.kind == "ea" and not tab.no <= p < tab.n:
            raise ValueError(who + ": the EA target %d is not a virtual orbital (%d <= p < %d)" % (p, tab.no, tab.n))
        qt = QuasiparticleTables(tt, self.kind, p)
        outside = "quasiparticle tables: a map points outside the space"
        if qt.b_of.max(initial=-1) >= tab.nv:
            raise AssertionError(outside)
        cap = max(qt.count, 1)
        ph, ph_partner, pair = (upload_map(ctx, m, cap, outside, lowest=-1) for m in (qt.ph, qt.ph_partner, qt.pair))
        partner = upload_map(ctx, qt.partner, qt.npos, outside, lowest=-1)
        layout = subspace.FlatLayout(ctx, (1,), qt.shape)
        d, U, W = layout.padded(), ctx.empty((qt.npos,)), ctx.empty((qt.npos,))
        extra = self.ladders.arenas[p] if qt.extra_size and self.ladders is not None and p in self.ladders.qtabs else None
        d1 = float(-h.L_host[p] if self.kind == "ip" else h.L_host[p])
        tg = SimpleNamespace(qt=qt, ph=ph, ph_partner=ph_partner, pair=pair, partner=partner, layout=layout, d=d, d1=d1, U=U, W=W,
                             extra=extra, own=[ph, ph_partner, pair, partner, d, U, W], work={})
        b_dev = upload_i32(ctx, qt.b_of)
        ptr = lambda a: C.c_void_p(a.ptr)
        ti = self.tints
        ctx.lib.call("pymes_sector_ipea_prepare", ctx.handle, 0 if self.kind == "ip" else 1, p, tab.no, tab.nv, ptr(h.k_dev),
                     ptr(h.orb_dev), tt.box.ctypes.data_as(C.c_void_p), ptr(b_dev), ptr(h.L), ptr(h.Tc), ptr(ti.Vv), ptr(ti.Vo),
                     ptr(ti.VvR), ptr(ti.VoR), float(qt.OUTSIDE), ptr(U), ptr(W), ptr(layout.part2(d)))
        layout.part1(d).set(np.array([d1]))
        b_dev.free()
        self._targets[p] = tg
        return tg

    def _work(self, tg, k):
        """The task tables and the buffers of one apply of k stacked vectors, built on first use and kept with the target:
        (tasks by name, XR, XX, XP, G1, G2, H, M)."""
        if k not in tg.work:
            ctx, size = self.ctx, max(tg.qt.count, 1) * k
            tasks = {nm: Tasks(ctx, *spec) for nm, spec in tg.qt.tasks(k).items()}
            bufs = [ctx.empty((size,)) for _ in range(6)]
            bufs.append(ctx.empty((max(tasks["quad"].lens[2], 1),)) if self.kind == "ea" else None)
            tg.work[k] = (tasks, *bufs)
        return tg.work[k]

    def forget(self, target):
        """Frees what the object holds for one target (it is built again on the next use)."""
        tg = self._targets.pop(int(target), None)
        if tg is None:
            return
        for tasks, *bufs in tg.work.values():
            for arr in [t.dev for t in tasks.values()] + [b for b in bufs if b is not None]:
                arr.free()
        for arr in tg.own:
            arr.free()

    def tables_of(self, target):
        return self._target(target).qt

    def shape(self, target):
        return self._target(target).qt.shape

    def layout(self, target):
        """The ``subspace.FlatLayout`` [r1 (1) | zero pad | R] of the target's vectors."""
        return self._target(target).layout

    def diagonals(self, target):
        """The preconditioner's diagonal as a flat device vector of ``layout(target)``: d1 = -L_pp (IP) / L_pp (EA), d2 = L_b* - L_i -
        L_j / L_a + L_b* - L_j, and ``QuasiparticleTables.OUTSIDE`` at the positions outside the space."""
        return self._target(target).d

    # ---- one apply -------------------------------------------------------------------------------------------------------
    def apply_many(self, target, r1s, r2s, out1=None, out2=None):
        """sigma of the stacked device vectors (r1s[z] of one element, r2s[z] of ``shape(target)``) into out1 / out2 (made if not
        given); returns the list of (s1, s2).  At most 32 vectors go into one launch; more are worked off in groups."""
        tg = self._target(target)
        ctx, qt = self.ctx, tg.qt
        if ctx.recording:
            raise RuntimeError("SectorIPEASigma.apply_many: the context is recording a launch graph")
        n = len(r1s)
        if len(r2s) != n or any(x.size != 1 for x in r1s) or any(x.size != qt.npos for x in r2s):
            raise ValueError("SectorIPEASigma.apply_many: the vectors do not have the lengths of the target's block (1 and %d)"
                             % qt.npos)
        out1 = [ctx.empty((1,)) for _ in range(n)] if out1 is None else list(out1)
        out2 = [ctx.empty(qt.shape) for _ in range(n)] if out2 is None else list(out2)
        if len(out1) != n or len(out2) != n or any(x.size != 1 for x in out1) or any(x.size != qt.npos for x in out2):
            raise ValueError("SectorIPEASigma.apply_many: the outputs do not have the lengths of the target's block")
        for lo in range(0, n, MAX_STACK):
            hi = min(n, lo + MAX_STACK)
            self._apply(tg, r1s[lo:hi], r2s[lo:hi], out1[lo:hi], out2[lo:hi])
        return list(zip(out1, out2))

    def _apply(self, tg, r1s, r2s, s1s, s2s):
        ctx, qt, h, k = self.ctx, tg.qt, self.hoist, len(r1s)
        if qt.extra_size and tg.extra is None:
            raise ValueError("SectorIPEASigma: the particle ladder of the EA target %d reads V_abcd at pair momenta k_p + k_j that "
                             "are no sum of two occupied momenta, which the integrals do not store: pass "
                             "ladders=UEG.eval_2b_ladder(tables, targets)" % qt.target)
        tasks, XR, XX, XP, G1, G2, H, M = self._work(tg, k)
        ptr, pp = (lambda a: C.c_void_p(a.ptr)), (lambda xs: _lib.ptr_array([x.ptr for x in xs]))
        ctx.lib.call("pymes_sector_ipea_pack", ctx.handle, k, pp(r2s), qt.npos, ptr(tg.ph), ptr(tg.partner), ptr(tg.pair), ptr(XR),
                     ptr(XX), ptr(XP))
        tasks["ring"].run(h.PA, XR, G1)                             # G1 = PA XR + PB XX
        tasks["ring_add"].run(h.PB, XX, G1)
        tasks["ring"].run(h.MDU, XX, G2)                            # G2 = MDU XX
        if self.kind == "ip":
            tasks["hole"].run(h.hole, XP, H)                        # H^P = (I^P)^T R^P
        else:
            tasks["ladder"].run(self.ints["abcd"], XP, H)           # H^j = V_abcd^P R^j, P = k_p + k_j
            if tg.extra is not None:
                tasks["ladder_extra"].run(tg.extra, XP, H)          # (the columns whose P is no pp sector)
            tasks["quad"].run(self.ints["klcd"], XP, M)             # M^j = V_klcd^P R^j
            tasks["quad_back"].run(h.T, M, H)                       # H^j += T^P M^j
        ctx.lib.call("pymes_sector_ipea_assemble", ctx.handle, k, pp(r1s), pp(r2s), pp(s1s), pp(s2s), qt.npos, ptr(tg.ph),
                     ptr(tg.ph_partner), ptr(tg.pair), ptr(tg.layout.part2(tg.d)), ptr(tg.U), ptr(tg.W), tg.d1, ptr(G1), ptr(G2),
                     ptr(H))

    def get_sigma(self, target, r1, R):
        """One apply for host arrays: (s1, S) of (r1, R), or of k stacked vectors (r1 [k], R [k, ...]) as (s1 [k], S [k, ...])."""
        qt = self._target(target).qt
        R = np.asarray(R, dtype=np.float64)
        single = R.ndim == 2
        r1 = np.asarray(r1, dtype=np.float64).reshape(-1)
        R = R.reshape((-1,) + qt.shape)
        if len(r1) != len(R):
            raise ValueError("SectorIPEASigma.get_sigma: as many r1 as R are needed")
        ins = [(self.ctx.array(a.reshape(1)), self.ctx.array(b)) for a, b in zip(r1, R)]
        out = self.apply_many(target, [a for a, _ in ins], [b for _, b in ins])
        s1, S = np.array([a.get()[0] for a, _ in out]), np.array([b.get() for _, b in out]).reshape((-1,) + qt.shape)
        for a, b in ins + out:
            a.free()
            b.free()
        return (s1[0], S[0]) if single else (s1, S)

    def correction(self, target):
        """The ``correction`` argument of ``subspace.block_davidson`` for the target's layout: the element-wise correction kernel
        of the dense EOM drivers through ``pymes_sector_ipea_correction``, which takes the lengths as they are."""
        lay, ctx = self._target(target).layout, self.ctx

        def run(ss, rs, w, d, shift, qs):
            n = len(rs)
            ww, out = np.ascontiguousarray(w, dtype=np.float64), np.zeros(2 * max(n, 1))
            pp = lambda xs: _lib.ptr_array([x.ptr for x in xs])
            ctx.lib.call("pymes_sector_ipea_correction", ctx.handle, n, pp(ss), pp(rs), _lib.host_ptr(ww), C.c_void_p(d.ptr),
                         float(shift), pp(qs), lay.n1, lay.off2, lay.nflat, _lib.host_ptr(out))
            return out[0:2 * n:2].copy(), out[1:2 * n:2].copy()
        return run

    def close(self):
        """Frees what the object holds on the device: its targets, and the hoist if it made it (the integrals and the amplitudes
        handed in stay the caller's)."""
        for p in list(self._targets):
            self.forget(p)
        if self._own_hoist:
            self.hoist.close()


class _SectorEOM:
    """One block Davidson (``subspace.block_davidson``, ``DROP_NULL``) per target on the blocks of ``SectorIPEASigma``."""
    KIND = NAME = None

    def __init__(self, no, n_roots=1, r_epsilon=1.e-6, max_iter=100, max_dim=None, shift=1.e-5):
        if n_roots < 1:
            raise ValueError("%s: at least one root is needed" % self.NAME)
        self.no, self.n_roots, self.r_epsilon, self.max_iter, self.shift = no, int(n_roots), r_epsilon, max_iter, shift
        self.max_dim = 8 * self.n_roots if max_dim is None else int(max_dim)

    def solve(self, eps, ints, tints, amps, targets, ladders=None, keep_vectors=False, hoist=None):
        """The ``n_roots`` lowest roots of the Krylov space of the start vectors in the block of every target (orbital indices over
        all n: occupied for IP, virtual for EA), in the sign convention of ``eom_ip_ea``: E(N -+ 1) - E(N).

        Start vectors: the singles unit vector and, for n_roots > 1, unit vectors on the n_roots - 1 smallest d2 inside the space.
        Returns, with K = "ip" or "ea": "K e" [targets, n_roots] ascending per target, "singles weight" = r1^2 / |r|^2 (the
        quasi-particle root has the largest), "residuals" = |s - w r| / |r|, "converged" [targets], "passes" [targets], "targets",
        and with ``keep_vectors`` "K vectors": per target and root the host pair (r1, R) of unit norm.  ``hoist``: a
        ``SectorIPEAHoist`` of the same inputs, shared with the solver of the other kind.  Refused by name: n_roots
        above the dimension of a block, and everything ``SectorIPEASigma`` refuses."""
        who, K, nr = self.NAME + ".solve", self.KIND, self.n_roots
        if isinstance(ints, SectorIntegrals) and ints.tables.no != self.no:
            raise ValueError(who + ": the tables of the integrals (no = %d) do not match the solver (no = %d)"
                             % (ints.tables.no, self.no))
        t_start = time.time()
        targets = [int(p) for p in np.atleast_1d(targets)]
        sig = SectorIPEASigma(K, eps, ints, tints, amps, ladders=ladders, hoist=hoist)
        ctx = sig.ctx
        out = {K + " e": np.zeros((len(targets), nr)), "singles weight": np.zeros((len(targets), nr)),
               "residuals": np.zeros((len(targets), nr)), "converged": np.zeros(len(targets), dtype=bool),
               "passes": np.zeros(len(targets), dtype=np.int64), "targets": np.array(targets, dtype=np.int64)}
        if keep_vectors:
            out[K + " vectors"] = []
        try:
            with quiet_collector():
                for n, p in enumerate(targets):
                    qt, lay, d = sig.tables_of(p), sig.layout(p), sig.diagonals(p)
                    if nr > qt.dim:
                        raise ValueError(who + ": n_roots = %d exceeds the dimension %d of the block of target %d" % (nr, qt.dim, p))
                    start = [lay.unit(0)]
                    if nr > 1:
                        d2 = lay.part2(d).get().reshape(-1)
                        inside = np.flatnonzero(qt.inside)
                        for t in inside[np.argsort(d2[inside], kind="stable")[:nr - 1]]:
                            vec = ctx.zeros((lay.nflat,))
                            one = np.zeros(qt.npos)
                            one[t] = 1.0
                            lay.part2(vec).set(one.reshape(qt.shape))
                            start.append(vec)
                    flat = functools.partial(subspace.apply_flat, lay, functools.partial(sig.apply_many, p))
                    dav = subspace.block_davidson(ctx, lay, flat, sig.correction(p), d, start, nr, max(self.max_dim, nr + 1),
                                                  self.max_iter, self.r_epsilon, self.shift,
                                                  label="%s target %d" % (self.NAME, p), on_null=subspace.DROP_NULL)
                    order = np.argsort(dav.theta, kind="stable")
                    out[K + " e"][n], out["residuals"][n] = dav.theta[order], dav.rel[order]
                    out["converged"][n], out["passes"][n] = dav.converged, dav.passes
                    w1 = np.array([lay.part1(dav.rz[r]).get()[0] ** 2 for r in order])
                    out["singles weight"][n] = w1 / dav.nrm[order]
                    if keep_vectors:
                        out[K + " vectors"].append([(lay.part1(dav.rz[r]).get() / np.sqrt(dav.nrm[r]),
                                                     lay.part2(dav.rz[r]).get() / np.sqrt(dav.nrm[r])) for r in order])
                    for r in range(nr):
                        print_logging_info("{} target {:d} root {:d} energy = {:.12f}  singles weight = {:.4f}".format(
                            self.NAME, p, r, out[K + " e"][n, r], out["singles weight"][n, r]), level=2)
            print_logging_info("{} finished in {:.3f} seconds".format(self.NAME, time.time() - t_start), level=1)
            return out
        finally:
            sig.close()


class SectorIP_EOM_CCD(_SectorEOM):
    """Ionisation energies E(N-1; -k_p) - E(N) per occupied target p; r1[p], R[i,j] = r2[i,j,b*]."""
    KIND, NAME = "ip", "SectorIP_EOM_CCD"


class SectorEA_EOM_CCD(_SectorEOM):
    """Attachment energies E(N+1; +k_p) - E(N) per virtual target p (counted over all n); r1[p], R[a,j] = r2[a,b*,j]."""
    KIND, NAME = "ea", "SectorEA_EOM_CCD"


def sector_quasiparticles(no, eps, ints, amps, tints=None, ip=None, ea=None, n_roots=1, ladders=None, **kwargs):
    """What ``SectorCCD.solve(..., quasiparticles=dict(tints=..., ip=[...], ea=[...], n_roots=1, ladders=...))`` adds to its result:
    "ip e" / "ea e" [targets, n_roots], "ip singles weight" / "ea singles weight", and with both lists "qp gap" = lowest "ip e"
    + lowest "ea e", as the dense solve does.  Further keywords go to the solvers (r_epsilon, max_iter, max_dim)."""
    out = {}
    hoist = SectorIPEAHoist(eps, ints, tints, amps, "sector_quasiparticles")          # one for both kinds
    try:
        for kind, cls, targets in (("ip", SectorIP_EOM_CCD, ip), ("ea", SectorEA_EOM_CCD, ea)):
            if targets is None:
                continue
            res = cls(no, n_roots=n_roots, **kwargs).solve(eps, ints, tints, amps, targets, ladders=ladders if kind == "ea" else None,
                                                           hoist=hoist)
            out[kind + " e"], out[kind + " singles weight"] = res[kind + " e"], res["singles weight"]
    finally:
        hoist.close()
    if "ip e" in out and "ea e" in out:
        out["qp gap"] = float(out["ip e"].min() + out["ea e"].min())
    return out


# ---- spectral functions A(k, w) and pole strengths Z_k -----------------------------------------------------------------
ARNOLDI_MAX = 512       # PYMES_SECTOR_ARNOLDI_MAX of include/pymes_amd.h: the most basis vectors pymes_sector_arnoldi_step takes
_SIGN = {"ip": 1.0, "ea": -1.0}


def arnoldi_workspace(ctx, length, j):
    """The doubles of scratch that ``pymes_sector_arnoldi_step`` needs for vectors of ``length`` at step ``j`` (its query form)."""
    size = C.c_int64(0)
    ctx.lib.call("pymes_sector_arnoldi_step", ctx.handle, None, 0, int(length), int(j), None, 0, 0.0, None, C.byref(size), None)
    return int(size.value)


def arnoldi_step(ctx, basis, pitch, length, j, hess, ldh, breakdown, ws, status):
    """One step of the device Arnoldi process (include/pymes_amd.h): CGS2 of row j+1 of ``basis`` against the rows 0..j, column j
    of ``hess``; nothing is read back.  ``status``: a device array of one 8-byte integer, zero before the first step."""
    ctx.lib.call("pymes_sector_arnoldi_step", ctx.handle, C.c_void_p(basis.ptr), int(pitch), int(length), int(j),
                 C.c_void_p(hess.ptr), int(ldh), float(breakdown), C.c_void_p(ws.ptr), C.byref(C.c_int64(ws.size)),
                 C.c_void_p(status.ptr))


def shifted_hessenberg(Hbar, kind, z, chunk=64):
    """(y_1(z), y_k(z)) of (z + s H_k) y = e_1 for the shifts z, s = +1 (IP) / -1 (EA), from the [k+1, k] Hessenberg matrix."""
    k, z = Hbar.shape[1], np.atleast_1d(z).astype(np.complex128)
    e1 = np.zeros((k, 1), dtype=np.complex128)
    e1[0] = 1.0
    first, last = np.zeros(len(z), dtype=np.complex128), np.zeros(len(z), dtype=np.complex128)
    sH, eye = _SIGN[kind] * Hbar[:k], np.eye(k)
    for lo in range(0, len(z), chunk):
        zz = z[lo:lo + chunk]
        y = np.linalg.solve(zz[:, None, None] * eye[None] + sH[None], e1[None])[:, :, 0]
        first[lo:lo + chunk], last[lo:lo + chunk] = y[:, 0], y[:, -1]
    return first, last


class KrylovBasis:
    """What ``SectorSpectralFunction.solve(..., keep_basis=True)`` keeps per target: the basis on the device and its Hessenberg
    matrix.  ``close()`` frees the device arrays."""

    def __init__(self, ctx):
        self.ctx, self._targets = ctx, {}

    def _add(self, kind, target, layout, basis, pitch, Hbar):
        self._targets[int(target)] = SimpleNamespace(kind=kind, layout=layout, basis=basis, pitch=pitch, Hbar=Hbar)

    def hessenberg(self, target):
        """The [k+1, k] Hessenberg matrix of the target (host); its last row holds h_{k+1,k} alone, 0.0 after a breakdown."""
        return self._targets[int(target)].Hbar.copy()

    def rows(self, target):
        """The k+1 basis rows of the target as flat device vectors of its layout (views; the last one is zero after a breakdown)."""
        t = self._targets[int(target)]
        return [subspace.view(self.ctx, t.basis, i * t.pitch, (t.layout.nflat,)) for i in range(t.Hbar.shape[0])]

    def solution(self, target, z):
        """x(z) = V_k y(z), (z + s H_k) y = e_1, as two flat device vectors (real part, imaginary part) of the target's layout:
        G(z) = N_p x_1(z)."""
        t = self._targets[int(target)]
        k, sH = t.Hbar.shape[1], _SIGN[t.kind] * t.Hbar[:t.Hbar.shape[1]]
        e1 = np.zeros(k, dtype=np.complex128)
        e1[0] = 1.0
        y = np.linalg.solve(complex(z) * np.eye(k) + sH, e1)
        out = [t.layout.empty(), t.layout.empty()]
        self.ctx.lincomb_multi(out, self.rows(target)[:k], np.stack([y.real, y.imag], axis=1))
        return tuple(out)

    def close(self):
        for t in self._targets.values():
            t.basis.free()
        self._targets = {}


class SectorSpectralFunction:
    """The diagonal one-particle Green's function of the electron gas on the sector path, its spectral function A(k, w) and the
    pole strengths Z_k.  H-bar conserves momentum, t1 = lambda1 = 0 and no two orbitals share a momentum, so the Dyson
    amplitudes of DESIGN 8f collapse to the singles element: for an occupied target p

        G_pp(z) = N_p [(z + H_IP)^-1]_11,  N_p = n(k_p) / 2        (the hole part, poles at -w_k)

    and for a virtual one G_pp(z) = N_p [(z - H_EA)^-1]_11, N_p = 1 - n(k_p) / 2 (the particle part), with H the momentum block that
    ``SectorIPEASigma`` applies and n(k) from the ``SectorDensity``: the only place Lambda enters.  All frequencies share the
    Krylov space K_m(H, e_1): one Arnoldi run per target (m real applies, each followed by ``pymes_sector_arnoldi_step`` on the
    device, no host round trip per step), G from the m x m Hessenberg matrix alone, the residual of every shift h_{m+1,m} |y_m(z)|.
    Only the majority part of a momentum is computed: the particle part of an occupied momentum (weight 1 - n(k)/2) and the hole
    part of a virtual one are left out; "K norm" says how much weight the computed part holds.

    max_dim: the most basis vectors per target (at most ``ARNOLDI_MAX``); r_epsilon: the run stops when the residual of every
    shift lies below it; check_every: steps between two read-backs of the Hessenberg matrix; breakdown: the relative norm below
    which a new direction counts as none (the space is invariant and the result exact)."""

    def __init__(self, no, max_dim=256, r_epsilon=1.e-6, check_every=16, breakdown=1.e-10):
        who = "SectorSpectralFunction"
        if not 1 <= int(max_dim) <= ARNOLDI_MAX:
            raise ValueError(who + ": max_dim must lie in [1, %d] (the cap of pymes_sector_arnoldi_step)" % ARNOLDI_MAX)
        if int(check_every) < 1:
            raise ValueError(who + ": check_every must be at least 1")
        self.no, self.max_dim, self.r_epsilon = no, int(max_dim), float(r_epsilon)
        self.check_every, self.breakdown = int(check_every), float(breakdown)

    @staticmethod
    def _occupations(who, ints, density):
        """n(k) over all orbitals from a ``SectorDensity`` of the same tables and context, or from an array."""
        tab = ints.tables
        if hasattr(density, "momentum_distribution"):
            if density.tables is not tab or density.ctx is not ints.ctx:
                raise ValueError(who + ": the density belongs to other tables or another context")
            return np.asarray(density.momentum_distribution(), dtype=np.float64)
        nk = np.asarray(density, dtype=np.float64)
        if nk.shape != (tab.n,):
            raise ValueError(who + ": n(k) must hold one number per orbital (%d), not %s" % (tab.n, nk.shape))
        return nk

    def solve(self, eps, ints, tints, amps, density, omegas, eta, ip=None, ea=None, ladders=None, hoist=None, keep_basis=False):
        """G(w + i eta) for the frequencies ``omegas`` and the targets ``ip`` (occupied orbitals) and / or ``ea`` (virtual, counted
        over all n).  eps, ints, tints, amps, ladders, hoist: as ``SectorIPEASigma``; density: the ``SectorDensity`` of the same
        amplitudes and their Lambda, or n(k) over all n orbitals.

        Returns, with K = "ip" / "ea": "K G" complex [targets, omegas]; "K A" = -Im G / pi; "K residuals" [targets, omegas], the
        residual h_{m+1,m} |y_m(z)| of (z +- H) x = e_1; "K converged" (all residuals below r_epsilon, or breakdown), "K krylov
        dim", "K breakdown", "K norm" (N_p), "K targets"; per target the lists "K poles" (the Ritz values in the energy convention
        of DESIGN 8f D3: -theta for IP, +theta for EA), "K pole strengths" (Z_j = N_p S_1j (S^-1)_j1) and "K pole residuals"
        (h_{m+1,m} |S_mj| / |S_:j|), complex128 because a non-Hermitian block may hold conjugate pairs; "K qp e" / "K qp z": the
        real pole of largest |Z_j| among those with a residual below r_epsilon, NaN where there is none; "A" [all targets, omegas]
        (the IP targets, then the EA targets: "targets") and "omegas".  With ``keep_basis`` also "K basis", a ``KrylovBasis``.
        Refused by name: everything ``SectorIPEASigma`` refuses, a density of other tables or context or n(k) of the wrong length,
        eta <= 0, neither ip nor ea."""
        who = "SectorSpectralFunction.solve"
        if ip is None and ea is None:
            raise ValueError(who + ": give the targets ip= and / or ea=")
        if not float(eta) > 0.0:
            raise ValueError(who + ": eta must be positive")
        if isinstance(ints, SectorIntegrals) and ints.tables.no != self.no:
            raise ValueError(who + ": the tables of the integrals (no = %d) do not match the solver (no = %d)"
                             % (ints.tables.no, self.no))
        omegas = np.atleast_1d(np.asarray(omegas, dtype=np.float64))
        z = omegas + 1j * float(eta)
        t_start = time.time()
        own_hoist = hoist is None
        if own_hoist:
            hoist = SectorIPEAHoist(eps, ints, tints, amps, who)
        out = {"omegas": omegas}
        try:
            nk = self._occupations(who, ints, density)
            for kind, targets in (("ip", ip), ("ea", ea)):
                if targets is None:
                    continue
                sig = SectorIPEASigma(kind, eps, ints, tints, amps, ladders=ladders if kind == "ea" else None, hoist=hoist)
                try:
                    with quiet_collector():
                        out.update(self._run(sig, kind, [int(p) for p in np.atleast_1d(targets)], nk, z, keep_basis))
                finally:
                    sig.close()
        finally:
            if own_hoist:
                hoist.close()
        kinds = [K for K in ("ip", "ea") if K + " A" in out]
        out["A"] = np.vstack([out[K + " A"] for K in kinds])
        out["targets"] = np.concatenate([out[K + " targets"] for K in kinds])
        print_logging_info("SectorSpectralFunction finished in {:.3f} seconds".format(time.time() - t_start), level=1)
        return out

    def _run(self, sig, K, targets, nk, z, keep_basis):
        ctx, nt, nz = sig.ctx, len(targets), len(z)
        res = {K + " G": np.zeros((nt, nz), dtype=np.complex128), K + " residuals": np.zeros((nt, nz)),
               K + " converged": np.zeros(nt, dtype=bool), K + " krylov dim": np.zeros(nt, dtype=np.int64),
               K + " breakdown": np.zeros(nt, dtype=bool), K + " norm": np.zeros(nt), K + " targets": np.array(targets, dtype=np.int64),
               K + " poles": [], K + " pole strengths": [], K + " pole residuals": [],
               K + " qp e": np.full(nt, np.nan), K + " qp z": np.full(nt, np.nan)}
        kept = KrylovBasis(ctx) if keep_basis else None
        for n, p in enumerate(targets):
            qt, lay = sig.tables_of(p), sig.layout(p)
            norm = 0.5 * nk[p] if K == "ip" else 1.0 - 0.5 * nk[p]
            basis, pitch, Hbar, broke = self._arnoldi(sig, p, qt, lay, K, z)
            k = Hbar.shape[1]
            first, last = shifted_hessenberg(Hbar, K, z)
            res[K + " G"][n], res[K + " residuals"][n] = norm * first, abs(Hbar[k, k - 1]) * np.abs(last)
            res[K + " krylov dim"][n], res[K + " breakdown"][n], res[K + " norm"][n] = k, broke, norm
            res[K + " converged"][n] = broke or bool(np.all(res[K + " residuals"][n] < self.r_epsilon))
            theta, S = np.linalg.eig(Hbar[:k])
            strength = (norm * S[0, :] * np.linalg.inv(S)[:, 0]).astype(np.complex128)
            pres = abs(Hbar[k, k - 1]) * np.abs(S[-1, :]) / np.linalg.norm(S, axis=0)
            energy = (-_SIGN[K] * theta).astype(np.complex128)
            res[K + " poles"].append(energy)
            res[K + " pole strengths"].append(strength)
            res[K + " pole residuals"].append(pres)
            ok = (pres < self.r_epsilon) & (np.abs(energy.imag) <= 1e-12 * np.maximum(1.0, np.abs(energy.real)))
            if ok.any():
                best = np.flatnonzero(ok)[np.argmax(np.abs(strength[ok]))]
                res[K + " qp e"][n], res[K + " qp z"][n] = energy[best].real, strength[best].real
            print_logging_info("SectorSpectralFunction {} target {:d}: Krylov dimension {:d}, largest residual {:.3e}, N_p = {:.6f}, "
                               "quasi-particle pole {:.10f} with Z = {:.6f}".format(K, p, k, res[K + " residuals"][n].max(), norm,
                                                                                    res[K + " qp e"][n], res[K + " qp z"][n]), level=2)
            if keep_basis:
                kept._add(K, p, lay, basis, pitch, Hbar)
            else:
                basis.free()
            sig.forget(p)
        res[K + " A"] = -res[K + " G"].imag / np.pi
        if keep_basis:
            res[K + " basis"] = kept
        return res

    def _arnoldi(self, sig, p, qt, lay, K, z):
        """The Arnoldi run of one target: (basis on the device, its pitch, the [k+1, k] Hessenberg matrix on the host, breakdown).
        The basis is zero-filled first, so the pad of the layout and of the pitch stays zero in every row; one read-back of the
        Hessenberg matrix and the status every ``check_every`` steps and at the end."""
        ctx = sig.ctx
        m_cap = min(self.max_dim, qt.dim)            # the Krylov dimension cannot exceed the dimension of the block
        length, pitch = lay.nflat, -(-lay.nflat // 32) * 32
        basis = ctx.zeros(((m_cap + 1) * pitch,))
        ldh = m_cap
        state = ctx.zeros(((m_cap + 1) * ldh + 1,))   # the Hessenberg matrix, row-major, and the status word behind it
        status = subspace.view(ctx, state, (m_cap + 1) * ldh, (1,))
        ws = ctx.empty((arnoldi_workspace(ctx, length, m_cap - 1),))
        row = lambda i: subspace.view(ctx, basis, i * pitch, (length,))
        lay.part1(row(0)).set(np.ones(lay.shape1))
        try:
            j = 0
            while True:
                stop = min(j + self.check_every, m_cap)
                for jj in range(j, stop):
                    src, dst = row(jj), row(jj + 1)
                    sig.apply_many(p, [lay.part1(src)], [lay.part2(src)], out1=[lay.part1(dst)], out2=[lay.part2(dst)])
                    arnoldi_step(ctx, basis, pitch, length, jj, state, ldh, self.breakdown, ws, status)
                j = stop
                host = state.get()
                flag = int(host[-1:].view(np.int64)[0])
                k = flag if flag else j
                Hbar = np.ascontiguousarray(host[:-1].reshape(m_cap + 1, ldh)[:k + 1, :k])
                if flag or j >= m_cap:
                    return basis, pitch, Hbar, bool(flag)
                last = shifted_hessenberg(Hbar, K, z)[1]
                if np.all(abs(Hbar[k, k - 1]) * np.abs(last) < self.r_epsilon):
                    return basis, pitch, Hbar, False
        except Exception:
            basis.free()
            raise
        finally:
            state.free()
            ws.free()


def sector_spectral(no, eps, ints, amps, density, *, tints, omegas, eta, ip=None, ea=None, ladders=None, **kwargs):
    """What ``SectorCCD.solve(..., spectral=dict(tints=..., omegas=..., eta=..., ip=[...], ea=[...], ladders=..., max_dim=...))``
    adds to its result: the keys of ``SectorSpectralFunction.solve``.  Further keywords go to the constructor (max_dim,
    r_epsilon, check_every, breakdown)."""
    return SectorSpectralFunction(no, **kwargs).solve(eps, ints, tints, amps, density, omegas, eta, ip=ip, ea=ea, ladders=ladders)
