"""3D uniform electron gas (pymes/model/ueg.py): plane-wave basis, Coulomb and transcorrelated
two-body integrals, mean-field pieces of the three-body operator.

Drop-in for the parts of ``pymes.model.ueg.UEG`` that feed the CCD/DCSD path (BASELINE config 4):
``init_single_basis``, ``eval_2b_integrals`` (Coulomb, ``is_only_2b``, ``is_effect_2b``,
``is_rpa_approx``; the reference's correlators ``trunc``, ``yukawa``, ``gaskell``, ``gaskell_modified``, ``smooth``,
``coulomb``, ``stg`` are evaluated inside the kernels from the same float k^2 the reference forms, a callable of the
caller's own is tabulated over the lattice shells and looked up on the device), ``double_contractions_in_3_body``,
``triple_contractions_in_3_body``.  The O(n_pw^3) integral evaluation — a Python triple loop with a
(2*30+1)^3 lattice sum per (p,r) pair in the reference — runs as HIP kernels (``pymes_ueg_eval_2b``);
the O(n_occ^2 n_pw) mean-field contractions stay on the host like the reference's.
"""
import contextlib
import ctypes as C
import time
import warnings

import numpy as np

from pymes_amd import _lib
from pymes_amd.basis_set import planewave
from pymes_amd.device import Context
from pymes_amd.log import print_logging_info


class UEG:
    def __init__(self, n_ele, n_alpha, n_beta, rs, device=0):
        if n_ele % 2 != 0 or n_alpha != n_beta:
            warnings.warn("only closed-shell systems are supported")
        self.n_ele, self.n_alpha, self.n_beta = int(n_ele), int(n_alpha), int(n_beta)
        self.rs = rs
        self.L = self.rs * ((4 * np.pi * self.n_ele) / 3) ** (1.0 / 3.0)
        self.Omega = self.L ** 3
        self.basis_fns = None
        self.imax = 0
        self.cutoff = 0.
        self.basis_indices_map = None
        self.kPrime = None
        self.correlator = None
        self.k_cutoff = None
        self.gamma = None
        self.device = device
        self._k_shift = np.zeros(3)

    # ---- basis (ueg.py:82-172) -----------------------------------------------------------------
    def is_k_in_basis(self, ke):
        return ke <= self.cutoff * (2 * np.pi / self.L) ** 2 / 2.

    def init_basis_indices_map(self):
        m = self.imax * 2 + 1
        self.basis_indices_map = -1 * np.ones(m ** 3).astype(int)
        for i in range(len(self.basis_fns) // 2):
            k = self.basis_fns[i * 2].k
            self.basis_indices_map[m * m * (k[0] + self.imax) + m * (k[1] + self.imax) + k[2] + self.imax] = i

    def init_single_basis(self, cutoff, k_shift=(0., 0., 0.)):
        k_shift = np.array(k_shift, dtype=float)
        self._k_shift = k_shift
        self.cutoff = cutoff
        self.imax = int(np.ceil(np.sqrt(cutoff + k_shift.dot(k_shift)))) + 1
        fns = []
        rng = range(-self.imax, self.imax + 1)
        for i in rng:
            for j in rng:
                for k in rng:
                    bfn = planewave.BasisFunc(i, j, k, self.L, 1, k_shift)
                    if self.is_k_in_basis(bfn.kinetic):
                        fns.append(bfn)
                        fns.append(planewave.BasisFunc(i, j, k, self.L, -1, k_shift))
        fns.sort()                               # stable: degenerate shells keep their generation order
        self.basis_fns = tuple(fns)
        self.init_basis_indices_map()
        return self.basis_fns

    def density_operator(self, q):
        """rho_q in the spatial plane-wave basis, for an integer momentum transfer q (in units of 2 pi / L): O[p,r] = 1 where
        k_p - k_r = q, so that rho_-q is its transpose.  The one-body operator of the density response chi(q, w) =
        <<rho_q; rho_-q>>_w (pymes_amd/solver/response.py)."""
        if self.basis_fns is None:
            raise RuntimeError("density_operator: call init_single_basis first")
        q = np.asarray(q)
        if q.shape != (3,) or not np.all(np.equal(np.mod(q, 1), 0)):
            raise ValueError("density_operator: q must be three integers (units of 2 pi / L), not %r" % (q,))
        k = np.array([self.basis_fns[2 * i].k for i in range(len(self.basis_fns) // 2)], dtype=np.int64)
        diff = k[:, None, :] - k[None, :, :]
        return np.all(diff == q.astype(np.int64)[None, None, :], axis=2).astype(np.float64)

    # ---- correlator (ueg.py:772-800); like the reference it zeroes the small entries of an array argument
    def trunc(self, kSquare):
        if self.k_cutoff is None:
            self.k_cutoff = int(np.ceil(np.sqrt(self.cutoff)))
        if self.gamma is None:
            self.gamma = 1.0
        kc2 = (self.k_cutoff * 2 * np.pi / self.L) ** 2
        if not isinstance(kSquare, np.ndarray):
            if kSquare <= kc2 * (1 + 0.00001):
                kSquare = 0.
        else:
            kSquare[kSquare <= kc2 * (1 + 0.00001)] = 0.
        result = np.divide(-4. * np.pi, kSquare ** 2, out=np.zeros_like(kSquare), where=(kSquare > 1e-12))
        return result * self.gamma

    # ---- the other correlators of the reference, with its two call forms: an ndarray argument goes through np.divide
    # masks, a float through an if/else — the two agree except AT the cut-off of gaskell / gaskell_modified
    @staticmethod
    def _masked(num, den, keep):
        den = np.asarray(den, dtype=np.float64)
        return np.divide(num, den, out=np.zeros_like(den), where=keep)

    def yukawa(self, kSquare, multiply_by_k_square=False):
        """ueg.py:740-770: -4 pi / (k^2 + gamma), gamma in units of sqrt(rho pi / 4)."""
        if multiply_by_k_square:
            raise NotImplementedError("multiply_by_k_square is not used by the integral builder")
        g0 = np.sqrt(self.n_ele / self.Omega / 4. * np.pi)
        g = g0 if self.gamma is None else self.gamma * g0
        floor = self.k_cutoff * (2 * np.pi / self.L) ** 2 + g if self.k_cutoff is not None else 1e-12
        b = kSquare + g
        return self._masked(-4. * np.pi, b, np.abs(b) > floor)

    def gaskell(self, kSquare, multiply_by_k_square=False):
        """ueg.py:836-883: -mu / k^2 below k_cutoff^2 k_F^2 (default 4 k_F^2), mu = gamma sqrt(4 pi / rho)."""
        mu = np.sqrt(4. * np.pi / (self.n_ele / self.Omega)) * (self.gamma if self.gamma is not None else 1.)
        kf = self.basis_fns[int(self.n_ele / 2) * 2].kp
        cut = (self.k_cutoff ** 2 if self.k_cutoff is not None else 4.) * kf.dot(kf)
        if not isinstance(kSquare, np.ndarray):
            return -(mu / kSquare) if (kSquare < cut and kSquare > 1e-12) else -0.
        res = self._masked(mu, kSquare, kSquare > 1e-12)
        res[kSquare > cut] = 0.
        return -res

    def gaskell_modified(self, kSquare, multiply_by_k_square=False):
        """ueg.py:802-834: -4 pi / k^4 from (k_cutoff 2 pi / L)^2 (default 2) on."""
        cut = (self.k_cutoff * (2 * np.pi / self.L)) ** 2 if self.k_cutoff is not None else 2
        if not isinstance(kSquare, np.ndarray):
            if kSquare < cut and kSquare > 1e-12:
                return -0.
            with np.errstate(divide="ignore"):
                return -(4 * np.pi / np.float64(kSquare) ** 2)
        return -self._masked(4 * np.pi, kSquare ** 2, kSquare >= cut)

    def smooth(self, kSquare, multiply_by_k_square=False):
        """ueg.py:885-903: trunc with an error-function switch of relative width gamma (default 0.01)."""
        from scipy import special
        if self.k_cutoff is None:
            self.k_cutoff = int(np.ceil(np.sqrt(self.cutoff)))
        if self.gamma is None:
            self.gamma = 0.01
        kc = np.sqrt((self.k_cutoff * 2 * np.pi / self.L) ** 2)
        k = np.sqrt(kSquare)
        return self._masked(-4. * np.pi * (1. + special.erf((k - kc) / (kc * self.gamma))) / 2., np.asarray(kSquare) ** 2,
                            kSquare > (kc * self.gamma) ** 2)

    def coulomb(self, kSquare, multiply_by_k_square=False):
        """ueg.py:905-915: -4 pi gamma / k^2."""
        return self._masked(-4. * np.pi * (1. if self.gamma is None else self.gamma), kSquare, np.asarray(kSquare) > 1e-12)

    def stg(self, kSquare, multiply_by_k_square=False):
        """ueg.py:917-935: Slater-type geminal, -4 pi / gamma / (k^2 + gamma^2)^2, gamma default sqrt(4 pi rho)."""
        g = np.sqrt(4. * np.pi * self.n_ele / self.Omega) if self.gamma is None else self.gamma
        floor = (self.k_cutoff * (2 * np.pi / self.L) ** 2 + g ** 2) ** 2 if self.k_cutoff is not None else 1e-12
        b = (kSquare + g ** 2) ** 2
        return self._masked(-4. * np.pi / g, b, np.abs(b) > floor)

    def _correlator_spec(self, correlator):
        """(kind, params) of pymes_ueg_eval_2b_corr for the reference's named correlators bound to this model, with the
        parameters formed by the same float expressions as the methods above; None for anything else (-> tables)."""
        if getattr(correlator, "__self__", None) is not self:
            return None
        name = getattr(correlator, "__name__", "")
        tw2 = (2 * np.pi / self.L) ** 2
        if name == "gaskell":
            mu = np.sqrt(4. * np.pi / (self.n_ele / self.Omega)) * (self.gamma if self.gamma is not None else 1.)
            kf = self.basis_fns[int(self.n_ele / 2) * 2].kp
            return 1, [mu, (self.k_cutoff ** 2 if self.k_cutoff is not None else 4.) * kf.dot(kf)]
        if name == "gaskell_modified":
            return 2, [(self.k_cutoff * (2 * np.pi / self.L)) ** 2 if self.k_cutoff is not None else 2.]
        if name == "coulomb":
            return 3, [-4. * np.pi * (1. if self.gamma is None else self.gamma)]
        if name == "yukawa":
            g0 = np.sqrt(self.n_ele / self.Omega / 4. * np.pi)
            g = g0 if self.gamma is None else self.gamma * g0
            return 4, [g, self.k_cutoff * tw2 + g if self.k_cutoff is not None else 1e-12]
        if name == "stg":
            g = np.sqrt(4. * np.pi * self.n_ele / self.Omega) if self.gamma is None else self.gamma
            return 5, [g ** 2, (self.k_cutoff * tw2 + g ** 2) ** 2 if self.k_cutoff is not None else 1e-12, -4. * np.pi / g]
        if name == "smooth":
            kc = np.sqrt((self.k_cutoff * 2 * np.pi / self.L) ** 2)
            return 6, [kc, kc * self.gamma, (kc * self.gamma) ** 2]
        return None

    def _correlator_tables(self, correlator, lattice_cutoff=30):
        """u over the lattice shells m = |n|^2 (every argument the integral builder passes to the correlator is
        |2 pi n / L|^2 for an integer n): (called with a float, called with an ndarray).  The argument of shell m is the
        reference's own float expression kp.dot(kp) for the first vector of the shell; a correlator with a jump exactly
        on a shell whose members round differently would be evaluated at that member's value."""
        r = lattice_cutoff + 2 * self.imax
        g = np.arange(-r, r + 1)
        vec = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        m_all = np.einsum("ni,ni->n", vec, vec)
        m_max = 3 * r * r
        shells, first = np.unique(m_all, return_index=True)
        x = (2 * np.pi / self.L) ** 2 * np.arange(m_max + 1, dtype=np.float64)     # shells without a vector: never looked up
        kp = vec[first] * 2 * np.pi / self.L
        x[shells] = np.einsum("ni,ni->n", kp, kp)
        with np.errstate(all="ignore"):
            arr = np.asarray(correlator(x.copy()), dtype=np.float64)
            try:
                sca = np.array([float(correlator(np.float64(v))) for v in x])
            except (TypeError, IndexError, ValueError):      # a callable written for arrays only
                sca = arr.copy()
        arr[~np.isfinite(arr)] = 0.0          # u(0) of a float call may divide by zero; k = 0 terms are never used
        sca[~np.isfinite(sca)] = 0.0
        return np.ascontiguousarray(sca), np.ascontiguousarray(arr)

    # ---- two-body integrals (ueg.py:265-516) on the device -----------------------------------------
    def _mode(self, correlator, flags):
        if correlator is None:
            return 0
        if not callable(correlator):
            raise TypeError("correlator must be a callable u(k^2)")
        on = [k for k, v in flags.items() if v]
        if on == ["is_rpa_approx"] or (flags["is_rpa_approx"]):
            return 3
        if flags["is_only_2b"]:
            return 1
        if flags["is_effect_2b"]:
            return 2
        raise NotImplementedError("supported TC modes: is_only_2b, is_effect_2b, is_rpa_approx "
                                  "(is_only_(non_)hermi_2b and is_exchange_1..3 are the reference's test-only switches)")

    def eval_2b_integrals(self, correlator=None, is_rpa_approx=False, is_only_2b=False, is_only_non_hermi_2b=False,
                          is_only_hermi_2b=False, is_effect_2b=False, is_exchange_1=False, is_exchange_2=False,
                          is_exchange_3=False, dtype=np.float64, sp=1, on_device=False, ctx=None):
        """Returns V_pqrs (numpy [n_p]^4 as the reference; a DeviceArray with ``on_device=True``)."""
        start_time = time.time()
        print_logging_info(__name__, level=0)
        if self.basis_fns is None:
            raise ValueError("Basis functions not initialized!")
        # (a twist k_shift of init_single_basis moves the kinetic energies and the shell order of the basis; every integral
        # below depends on DIFFERENCES of the integer plane-wave vectors only, so the kernels take the shifted basis as it is
        # — checked against the reference: tests/golden/ueg_twist.npz)
        if is_only_non_hermi_2b or is_only_hermi_2b or is_exchange_1 or is_exchange_2 or is_exchange_3:
            raise NotImplementedError("test-only switches of the reference are not on the HIP path")
        mode = self._mode(correlator, dict(is_rpa_approx=is_rpa_approx, is_only_2b=is_only_2b, is_effect_2b=is_effect_2b))
        is_trunc = correlator is not None and getattr(correlator, "__name__", "") == "trunc" and \
            getattr(correlator, "__self__", None) is self
        if correlator is not None:
            self.correlator = correlator
            print_logging_info("Using TC method", level=1)
            print_logging_info("Using correlator: ", getattr(correlator, "__name__", repr(correlator)), level=1)
            if self.k_cutoff is not None:
                print_logging_info("k_cutoff in correlator = {:.8f}".format(self.k_cutoff), level=1)
            if self.gamma is not None:
                print_logging_info("Gamma in correlator = {:.8f}".format(self.gamma), level=1)
            correlator(np.float64(1.0))          # fixes the correlator's k_cutoff / gamma defaults like its first call would
        n_p = len(self.basis_fns) // 2
        k_int = np.ascontiguousarray([self.basis_fns[2 * i].k for i in range(n_p)], dtype=np.int32)
        imap = np.ascontiguousarray(self.basis_indices_map, dtype=np.int32)
        own = ctx is None
        if own:
            ctx = Context(1, 1, device=self.device, workspace_bytes=1 << 20)
        try:
            V = ctx.empty((n_p,) * 4)
            if correlator is None or is_trunc:       # trunc is evaluated inside the kernels
                ctx.lib.call("pymes_ueg_eval_2b", ctx.handle, n_p, self.n_ele, self.imax, mode, float(self.L),
                             float(self.k_cutoff or 0.0), float(self.gamma or 1.0), 30,
                             k_int.ctypes.data_as(C.c_void_p), imap.ctypes.data_as(C.c_void_p), C.c_void_p(V.ptr))
            elif self._correlator_spec(correlator) is not None:       # the reference's other correlators, in the kernels
                kind, prm = self._correlator_spec(correlator)
                prm = (C.c_double * 4)(*(list(map(float, prm)) + [0.0] * (4 - len(prm))))
                ctx.lib.call("pymes_ueg_eval_2b_corr", ctx.handle, n_p, self.n_ele, self.imax, mode, float(self.L), 30, kind,
                             prm, k_int.ctypes.data_as(C.c_void_p), imap.ctypes.data_as(C.c_void_p), C.c_void_p(V.ptr))
            else:                                    # a u(k^2) of the caller's own: tabulated over the lattice shells
                tab_s, tab_a = self._correlator_tables(correlator, 30)
                ctx.lib.call("pymes_ueg_eval_2b_tab", ctx.handle, n_p, self.n_ele, self.imax, mode, float(self.L), 30,
                             k_int.ctypes.data_as(C.c_void_p), imap.ctypes.data_as(C.c_void_p),
                             tab_s.ctypes.data_as(C.c_void_p), tab_a.ctypes.data_as(C.c_void_p), len(tab_a),
                             C.c_void_p(V.ptr))
            if mode == 2:                        # ueg.py:509-513: symmetrise w.r.t. the electron labels
                Vs = ctx.permute("pqrs->pqrs", V, alpha=0.5)
                ctx.permute("qpsr->pqrs", V, out=Vs, alpha=0.5, beta=1.0)
                V = Vs
            print_logging_info("{:.3f} s spent on ".format(time.time() - start_time) + __name__, level=1)
            if on_device:
                if own:
                    raise ValueError("on_device=True needs the caller's ctx (the array lives in its context)")
                return V
            return V.get().astype(dtype, copy=False)
        finally:
            if own:
                ctx.close()

    # ---- the same integrals sector by sector (pymes_amd/solver/ueg_cc.py): never an [n_p]^4 array -------------------
    SECTOR_CHUNK = 1 << 23        # integrals per pymes_ueg_eval_2b_list call (16 bytes of index list each)

    def sector_tables(self):
        """The momentum-sector tables of this basis (pymes_amd.solver.sectors.SectorTables)."""
        from pymes_amd.solver.sectors import SectorTables
        if self.basis_fns is None:
            raise ValueError("Basis functions not initialized!")
        n_p = len(self.basis_fns) // 2
        return SectorTables(np.array([self.basis_fns[2 * i].k for i in range(n_p)], dtype=np.int64), self.n_ele // 2)

    def _list_evaluator(self, k_int, correlator, flags):
        """``pymes_ueg_eval_2b_list`` with this basis and correlator bound: f(ctx, pqrs_ptr, count, out_ptr)."""
        n_p = len(k_int)
        mode = self._mode(correlator, flags)
        kind, prm, tab_s, tab_a = 0, [0.0] * 4, None, None
        if correlator is not None:
            self.correlator = correlator
            correlator(np.float64(1.0))          # fixes the correlator's k_cutoff / gamma defaults like its first call would
            is_trunc = getattr(correlator, "__name__", "") == "trunc" and getattr(correlator, "__self__", None) is self
            spec = None if is_trunc else self._correlator_spec(correlator)
            if spec is not None:
                kind, prm = spec[0], list(map(float, spec[1])) + [0.0] * (4 - len(spec[1]))
            elif not is_trunc:
                tab_s, tab_a = self._correlator_tables(correlator, 30)
        prm_c = (C.c_double * 4)(*prm)

        def bound(ctx):
            return (ctx.handle, n_p, self.n_ele, self.imax, mode, float(self.L), float(self.k_cutoff or 0.0),
                    float(self.gamma or 1.0), 30, kind, prm_c, k_int.ctypes.data_as(C.c_void_p),
                    tab_s.ctypes.data_as(C.c_void_p) if tab_s is not None else None,
                    tab_a.ctypes.data_as(C.c_void_p) if tab_a is not None else None, len(tab_a) if tab_a is not None else 0)

        def eval_list(ctx, pqrs_ptr, count, out_ptr):
            ctx.lib.call("pymes_ueg_eval_2b_list", *bound(ctx), C.c_void_p(pqrs_ptr), count, C.c_void_p(out_ptr))

        def make_term(ctx):
            """The same state kept on the device as a term of the direct ladder (``pymes_ueg_ladder_term_create``)."""
            from pymes_amd.solver.ueg_cc import LadderTerm
            handle = C.c_void_p()
            ctx.lib.call("pymes_ueg_ladder_term_create", *bound(ctx), C.byref(handle))
            return LadderTerm(ctx, handle, k_int)
        eval_list.make_term = make_term
        return eval_list

    @contextlib.contextmanager
    def _sector_frame(self, who, tables, correlator, flags, ctx):
        """What ``eval_2b_sectors`` and ``eval_2b_triples`` share around their bodies: the ``SectorTables`` must belong to
        this basis; the list evaluator is bound; without ``ctx`` a context of its own is made; a recording context is
        refused; and a context of its own is closed again if the body raises.  Yields (ctx, whether it is its own, f)."""
        if self.basis_fns is None:
            raise ValueError("Basis functions not initialized!")
        n_p = len(self.basis_fns) // 2
        k_int = np.ascontiguousarray([self.basis_fns[2 * i].k for i in range(n_p)], dtype=np.int32)
        if tables.n != n_p or tables.no != self.n_ele // 2 or not np.array_equal(tables.k_int, k_int):
            raise ValueError(who + ": the tables do not belong to this basis")
        eval_list = self._list_evaluator(k_int, correlator, flags)
        own = ctx is None
        if own:
            ctx = Context(tables.no, tables.nv, device=self.device, workspace_bytes=1 << 20)
        try:
            if ctx.recording:
                raise RuntimeError(who + ": the context is recording a launch graph")
            yield ctx, own, eval_list
        except BaseException:
            if own:
                ctx.close()
            raise

    def eval_2b_sectors(self, tables, correlator=None, is_rpa_approx=False, is_only_2b=False, is_effect_2b=False, ctx=None,
                        ladder="stored"):
        """The integral sectors of ``tables`` as ``SectorIntegrals`` (``ctx``: the context they live in; its own otherwise).
        Same modes and correlators as ``eval_2b_integrals``; is_effect_2b comes out already symmetrised (ueg.py:509-513).
        Momentum conservation is exact here: the few non-conserving elements the dense builder sets at some bases through
        its flattened lookup (like the reference) do not exist on this path.  ``ladder="direct"``: no ``abcd`` block is
        listed, evaluated or stored -- the object carries one ladder term instead, from which the ladder product generates
        the same elements."""
        from pymes_amd.solver.sectors import BLOCKS
        from pymes_amd.solver.ueg_cc import SectorIntegrals, upload_raw
        start_time = time.time()
        if ladder not in ("stored", "direct"):
            raise ValueError("eval_2b_sectors: ladder must be \"stored\" or \"direct\"")
        flags = dict(is_rpa_approx=is_rpa_approx, is_only_2b=is_only_2b, is_effect_2b=is_effect_2b)
        with self._sector_frame("eval_2b_sectors", tables, correlator, flags, ctx) as (ctx, own, eval_list):
            terms = [(1.0, eval_list.make_term(ctx))] if ladder == "direct" else None
            ints = SectorIntegrals(ctx, tables, own_ctx=own, ladder_terms=terms)
            pieces = []             # (name, first sector, end sector, items), in arena order
            for name in ints.NAMES:
                if name not in BLOCKS or not ints.sizes[name]:        # (a list; or the ladder block of a direct object)
                    pieces.append((name, 0, 0, ints.sizes[name]))
                    continue
                off, s0 = tables.block_offsets(name), 0
                while s0 < len(off) - 1:        # as many whole sectors as fit the chunk (at least one)
                    s1 = max(int(np.searchsorted(off, off[s0] + self.SECTOR_CHUNK, side="right")) - 1, s0 + 1)
                    pieces.append((name, s0, s1, int(off[s1] - off[s0])))
                    s0 = s1
            done = 0
            while pieces:
                batch, count = [pieces.pop(0)], 0
                while pieces and sum(p[3] for p in batch) + pieces[0][3] <= self.SECTOR_CHUNK:
                    batch.append(pieces.pop(0))
                pqrs = np.concatenate([tables.block_pqrs(nm, s0, s1) for nm, s0, s1, _ in batch])
                count = len(pqrs)
                assert count == sum(p[3] for p in batch)
                if count:
                    lst = upload_raw(ctx, pqrs)
                    eval_list(ctx, lst.ptr, count, ints.arena.ptr + 8 * done)
                    lst.free()
                done += count
            assert done == ints.total
            print_logging_info("{:.3f} s spent on ".format(time.time() - start_time) + __name__, level=1)
            return ints

    def eval_2b_triples(self, tables, correlator=None, is_rpa_approx=False, is_only_2b=False, is_effect_2b=False, ctx=None,
                        both_sides=False):
        """The two integral families of the momentum-blocked (T), ``SectorTriplesIntegrals`` (Vv[i,a,b] = V[i,f*,a,b] and
        Vo[i,j,a] = V[i,j,a,m*]; pymes_amd.solver.ueg_cc), for the ``SectorTables`` (or ``TriplesTables``) of this
        basis.  Modes, correlators and ``ctx`` as ``eval_2b_sectors``.  The lists are evaluated in chunks of SECTOR_CHUNK
        positions: the entries whose implied orbital exists by ``pymes_ueg_eval_2b_list``, then placed; every other
        position is an exact 0.  ``both_sides``: also the excitation-type partners VvR[i,a,b] = V[a,b,i,f*] and
        VoR[i,j,a] = V[a,m*,i,j] that Lambda-(T) reads (list families "vv_r", "vo_r")."""
        from pymes_amd.solver.sectors import TriplesTables
        from pymes_amd.solver.ueg_cc import SectorTriplesIntegrals, gather, upload_raw, view
        start_time = time.time()
        if self.basis_fns is None:
            raise ValueError("Basis functions not initialized!")
        ttab = tables if isinstance(tables, TriplesTables) else TriplesTables(tables)
        flags = dict(is_rpa_approx=is_rpa_approx, is_only_2b=is_only_2b, is_effect_2b=is_effect_2b)
        with self._sector_frame("eval_2b_triples", ttab.tables, correlator, flags, ctx) as (ctx, own, eval_list):
            tints = SectorTriplesIntegrals(ctx, ttab, own_ctx=own, both_sides=both_sides)
            families = [("vv", tints.Vv), ("vo", tints.Vo)] + ([("vv_r", tints.VvR), ("vo_r", tints.VoR)] if both_sides else [])
            for family, dst in families:
                for e0 in range(0, dst.size, self.SECTOR_CHUNK):
                    e1 = min(e0 + self.SECTOR_CHUNK, dst.size)
                    pqrs, valid = ttab.list_pqrs(family, e0, e1)
                    nvalid = int(valid.sum())
                    vals = ctx.zeros((nvalid + 1,))                           # the last slot stays 0: what invalid positions read
                    if nvalid:
                        lst = upload_raw(ctx, pqrs[valid])
                        eval_list(ctx, lst.ptr, nvalid, vals.ptr)
                        lst.free()
                    place = upload_raw(ctx, np.where(valid, np.cumsum(valid) - 1, nvalid).astype(np.int64))
                    place.count = e1 - e0
                    gather(ctx, view(dst, e0, e1 - e0), vals, place)
                    place.free()
                    vals.free()
            print_logging_info("{:.3f} s spent on ".format(time.time() - start_time) + __name__, level=1)
            return tints

    def eval_2b_ladder(self, tables, targets, correlator=None, is_rpa_approx=False, is_only_2b=False, is_effect_2b=False, ctx=None):
        """The V_abcd blocks that the particle ladder of the sector EA-EOM-CCD reads outside the stored pair sectors, as
        ``SectorLadderIntegrals`` (pymes_amd.solver.ueg_eom): per virtual target p (an index over all orbitals) the
        blocks at the pair momenta k_p + k_j that are no sum of two occupied momenta (``QuasiparticleTables.extra_pqrs``).
        ``tables``: the ``SectorTables`` (or ``TriplesTables``) of this basis; modes, correlators and ``ctx`` as
        ``eval_2b_sectors``.  The lists are evaluated in chunks of SECTOR_CHUNK elements by ``pymes_ueg_eval_2b_list``."""
        from pymes_amd.solver.sectors import TriplesTables
        from pymes_amd.solver.ueg_cc import upload_raw
        from pymes_amd.solver.ueg_eom import SectorLadderIntegrals
        start_time = time.time()
        if self.basis_fns is None:
            raise ValueError("Basis functions not initialized!")
        ttab = tables if isinstance(tables, TriplesTables) else TriplesTables(tables)
        flags = dict(is_rpa_approx=is_rpa_approx, is_only_2b=is_only_2b, is_effect_2b=is_effect_2b)
        with self._sector_frame("eval_2b_ladder", ttab.tables, correlator, flags, ctx) as (ctx, own, eval_list):
            lad = SectorLadderIntegrals(ctx, ttab, targets)
            try:
                for p, qt in lad.qtabs.items():
                    for j in qt.extra_columns():                                # one block at a time: the lists stay small
                        pqrs, off = qt.extra_pqrs(j), int(qt.extra_off[j])
                        for e0 in range(0, len(pqrs), self.SECTOR_CHUNK):
                            e1 = min(e0 + self.SECTOR_CHUNK, len(pqrs))
                            lst = upload_raw(ctx, pqrs[e0:e1])
                            try:
                                eval_list(ctx, lst.ptr, e1 - e0, lad.arenas[p].ptr + 8 * (off + e0))
                            finally:
                                lst.free()
            except BaseException:
                lad.close()
                raise
            print_logging_info("{:.3f} s spent on ".format(time.time() - start_time) + __name__, level=1)
            return lad

    # ---- host mirrors of the per-element helpers (ueg.py:518-596) ----------------------------------
    def _occ_kp(self):
        return np.array([self.basis_fns[i * 2].kp for i in range(self.n_ele // 2)])

    def contract_exchange_3_body(self, p_vec, kVec):
        d = p_vec - self._occ_kp()
        return np.sum((d @ kVec) * self.correlator(kVec @ kVec) * self.correlator(np.einsum("ni,ni->n", d, d))) / self.Omega

    def contractP_KWithQ(self, pVec, kVec):
        v1, v2 = pVec - kVec - self._occ_kp(), pVec - self._occ_kp()
        return np.sum(np.einsum("ni,ni->n", v1, v2) * self.correlator(np.einsum("ni,ni->n", v1, v1))
                      * self.correlator(np.einsum("ni,ni->n", v2, v2))) / self.Omega

    def sumNablaUSquare(self, k, cutoff=30):
        if self.kPrime is None:
            g = np.arange(-cutoff, cutoff + 1)
            self.kPrime = np.array([[a, b, c] for a in g for b in g for c in g])
        k1 = 2 * np.pi * self.kPrime / self.L
        k2 = k - k1
        val = np.einsum("ni,ni->n", k1, k2) * self.correlator(np.einsum("ni,ni->n", k1, k1)) \
            * self.correlator(np.einsum("ni,ni->n", k2, k2))
        return np.sum(val) / self.Omega

    # ---- mean-field pieces of the 3-body operator (ueg.py:598-733), O(n_occ^2 n_pw) on the host --------
    def triple_contractions_in_3_body(self):
        print_logging_info("UEG.triple_contractions_in_3_body", level=1)
        occ = self._occ_kp()
        d = occ[:, None, :] - occ[None, :, :]
        d2 = np.einsum("pqi,pqi->pq", d, d)
        u = self.correlator(d2)                  # zeroes the sub-cutoff entries of d2 as well (reference behaviour)
        dirE = np.sum(u ** 2 * d2) * self.n_ele / 2 / self.Omega ** 2 * 2
        excE = -2 * 2 * np.einsum("pqo,pqo->", np.einsum("poi,pqi->pqo", d, d), np.einsum("pq,po->pqo", u, u)) \
            / 2. / self.Omega ** 2
        print_logging_info("Direct E = {:.8f}".format(dirE), level=2)
        print_logging_info("Exchange E = {:.8f}".format(excE), level=2)
        return dirE + excE

    def double_contractions_in_3_body(self):
        print_logging_info("UEG.double_contractions_in_3_body", level=1)
        no, n_p = self.n_ele // 2, len(self.basis_fns) // 2
        kp = np.array([self.basis_fns[i * 2].kp for i in range(n_p)])
        ki = kp[:no]
        dpi = kp[:, None, :] - ki[None, :, :]
        dpi2 = np.einsum("pij,pij->pi", dpi, dpi)
        u_pi = self.correlator(dpi2)             # dpi2 is cut in place, as in the reference
        e_perl = 2.0 * self.n_ele / self.Omega ** 2 / 2 * np.sum(u_pi ** 2 * dpi2, axis=1)
        e_wave = -np.einsum("pij,pij->p", np.einsum("pik,pjk->pij", dpi, dpi), np.einsum("pi,pj->pij", u_pi, u_pi)) \
            * 2 / self.Omega ** 2 / 2
        dij = ki[:, None, :] - ki[None, :, :]
        dij2 = np.einsum("ijk,ijk->ij", dij, dij)
        u_ij = self.correlator(dij2)
        e_shield = np.ones(n_p) * np.einsum("ij,ij->", u_ij ** 2, dij2) * 2 / 2 / self.Omega ** 2
        e_frog = -np.einsum("ijp,ijp->p", np.einsum("ijk,pik->ijp", dij, -dpi), np.einsum("ij,pi->ijp", u_ij, u_pi)) \
            * 4 / self.Omega ** 2 / 2
        return e_perl + e_wave + e_shield + e_frog
