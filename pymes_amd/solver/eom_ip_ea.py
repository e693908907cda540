"""IP- and EA-EOM-CCSD on the MI355X engine: ionisation potentials and electron affinities of a closed-shell CCSD state.

``IP_EOM_CCSD(no, n_roots).solve(f_dressed, dict_or_DressedDeviceIntegrals, t2)`` returns the ``n_roots`` lowest eigenvalues
``E(N-1) - E(N)`` of the IP operator, ``EA_EOM_CCSD`` those of ``E(N+1) - E(N)``, ascending; doublet final states, right
eigenvectors.  Vectors: IP ``r1[i], r2[i,j,b]`` (``i`` the orbital the electron leaves), EA ``r1[a], r2[a,b,j]``.

The operator is the EE-EOM-CCSD sigma (eom_ccsd.py:268-385) restricted to the sector with one extra orbital that interacts
with nothing (formulas: include/pymes_amd.h, ``pymes_ipea_sigma_*``).  The sigma build runs in the engine
(csrc/eom.cpp, ``IpEaSigma``): everything that does not depend on the trial vector is hoisted once per solve, all vectors of a
call go through each product as one GEMM.  The driver is the block Davidson on flat device vectors of ``subspace.py``;
unlike the EE driver — which is pinned to the reference pass by pass — it preconditions element-wise with the diagonals and
stops on the relative residual norm of every root.
"""
import ctypes as C
import time

import numpy as np

from pymes_amd import _lib
from pymes_amd.device import PymesError
from pymes_amd.log import print_logging_info, print_title
from pymes_amd.solver import subspace

KIND_IP, KIND_EA = 0, 1           # PYMES_IPEA_IP / PYMES_IPEA_EA of include/pymes_amd.h


class IPEASigma(subspace.LibraryHandle):
    """Device-resident IP / EA sigma build: a handle of the engine's ``IpEaSigma`` (``pymes_ipea_sigma_prepare / _apply /
    _diagonals / _correction``)."""

    # the dressed blocks each operator reads (the IP operator never reads abcd or abic: it runs on a sharded context)
    BLOCKS = {KIND_IP: ("ijab", "iabj", "iajb", "ijka", "ijak", "iabc", "iajk", "klij"),
              KIND_EA: ("ijab", "iabj", "iajb", "ijka", "iabc", "abic", "abcd")}
    DESTROY, NOUN = "pymes_ipea_sigma_destroy", "IP / EA sigma"

    def __init__(self, ctx, kind, f, t2, dressed=False):
        self.ctx, self.kind = ctx, int(kind)
        self.no, self.nv = ctx.no, ctx.nv
        self.dressed = bool(dressed)
        self.T = t2                                   # (kept alive: the handle reads it in every build)
        self._f = np.ascontiguousarray(f, dtype=np.float64)
        if self._f.shape != (ctx.n, ctx.n):
            raise ValueError("the dressed Fock matrix must be [n, n]")
        o, v = self.no, self.nv
        lay = self.layout = subspace.FlatLayout(ctx, *(((o,), (o, o, v)) if self.kind == KIND_IP else ((v,), (v, v, o))))
        for name in ("shape1", "shape2", "n1", "n2", "off2", "nflat", "part1", "part2"):      # flat vectors [r1 | zero pad | r2]
            setattr(self, name, getattr(lay, name))
        h = C.c_void_p()
        ctx.lib.call("pymes_ipea_sigma_prepare", ctx.handle, _lib.host_ptr(self._f), C.c_void_p(t2.ptr), int(self.dressed),
                     self.kind, C.byref(h))
        self._bind(h)

    def apply_many(self, r1s, r2s, out1=None, out2=None):
        """[(sigma1_z, sigma2_z)] for the trial vectors (r1s[z], r2s[z]), device arrays; one library call."""
        h, c, k = self._handle(), self.ctx, len(r1s)
        s1 = [out1[z] if out1 is not None else c.empty(self.shape1) for z in range(k)]
        s2 = [out2[z] if out2 is not None else c.empty(self.shape2) for z in range(k)]
        c.lib.call("pymes_ipea_sigma_apply", h, k, _lib.ptr_array([u.ptr for u in r1s]), _lib.ptr_array([u.ptr for u in r2s]),
                   _lib.ptr_array([x.ptr for x in s1]), _lib.ptr_array([x.ptr for x in s2]))
        return list(zip(s1, s2))

    def apply_left_many(self, l1s, l2s, out1=None, out2=None):
        """[((H^T l_z)_1, (H^T l_z)_2)] for the left vectors (l1s[z], l2s[z]), device arrays; one library call
        (``pymes_ipea_sigma_apply_left``: the products of ``apply_many`` once each, trial-vector operand and output exchanged)."""
        h, c, k = self._handle(), self.ctx, len(l1s)
        o1 = [out1[z] if out1 is not None else c.empty(self.shape1) for z in range(k)]
        o2 = [out2[z] if out2 is not None else c.empty(self.shape2) for z in range(k)]
        c.lib.call("pymes_ipea_sigma_apply_left", h, k, _lib.ptr_array([u.ptr for u in l1s]), _lib.ptr_array([u.ptr for u in l2s]),
                   _lib.ptr_array([x.ptr for x in o1]), _lib.ptr_array([x.ptr for x in o2]))
        return list(zip(o1, o2))

    def dyson(self, t1, lam1, lam2, l1s, l2s, r1s, r2s):
        """(psiL [k,n], psiR [k,n]) as host arrays (``pymes_ipea_dyson``); every input a device array of the handle's context."""
        k, n = len(l1s), self.ctx.n
        pl, pr = np.zeros((k, n)), np.zeros((k, n))
        self.ctx.lib.call("pymes_ipea_dyson", self._handle(), C.c_void_p(t1.ptr), C.c_void_p(lam1.ptr), C.c_void_p(lam2.ptr), k,
                          _lib.ptr_array([x.ptr for x in l1s]), _lib.ptr_array([x.ptr for x in l2s]),
                          _lib.ptr_array([x.ptr for x in r1s]), _lib.ptr_array([x.ptr for x in r2s]), _lib.host_ptr(pl),
                          _lib.host_ptr(pr))
        return pl, pr

    def diagonals(self):
        """The flat diagonal [d1 | 0 | d2] (device)."""
        h = self._handle()
        d = self.ctx.zeros((self.nflat,))
        self.ctx.lib.call("pymes_ipea_sigma_diagonals", h, C.c_void_p(d.ptr), C.c_void_p(d.ptr + 8 * self.off2))
        return d

    def correction(self, ss, rs, w, d, shift, qs):
        """q_n = (s_n - w_n r_n) / (w_n - d + shift) into qs for all roots in one launch; returns (|s_n - w_n r_n|^2,
        |r_n|^2) per root (one synchronisation)."""
        return subspace.correction(self.ctx.lib, "pymes_ipea_sigma_correction", self._handle(), self.layout, ss, rs, w, d, shift,
                                   qs)


class _IPEA_EOM_CCSD:
    """The lowest right eigenpairs of the IP / EA operator by ``subspace.block_davidson``."""
    KIND = None
    NAME = None

    def __init__(self, no, n_roots=3, device=0):
        self.algo_name = self.NAME
        self.no = no
        self.n_roots = int(n_roots)
        self.device = device
        self.max_dim = 8 * self.n_roots
        self.r_epsilon = 1.e-6
        self.max_iter = 200
        self.shift = 1.e-5
        self.e = np.zeros(self.n_roots)
        self.r_singles, self.r_doubles = [], []
        self.residual_norms = np.full(self.n_roots, np.inf)
        self.singles_weight = np.zeros(self.n_roots)
        self.iterations, self.converged, self.history = 0, False, []

    def check_context(self, ctx):
        """The EA operator reads the whole V_abcd: a context that shards its integrals is refused, by the name of the mode."""
        if self.KIND == KIND_EA and getattr(ctx, "shard", None) is not None:
            raise PymesError("EA-EOM-CCSD sigma: not available with integral sharding (shard=%s): the operator reads the "
                             "whole V_abcd" % (ctx.shard,))

    def _sigma(self, f, V, t2):
        """(ctx, sigma handle, owns the context) for the two call forms."""
        make = lambda ctx, f, t2, dressed: IPEASigma(ctx, self.KIND, f, t2, dressed)
        return subspace.open_handle(self.no, self.device, f, V, t2, self.BLOCKS, make, self.NAME, self.check_context)[1:]

    def apply(self, f_dressed, V_dressed, t2, r1, r2):
        """One sigma build for host arrays: (sigma1, sigma2) of (r1, r2), or lists of them for lists (stacked build)."""
        many = isinstance(r1, (list, tuple))
        r1s, r2s = (list(r1), list(r2)) if many else ([r1], [r2])
        ctx, sig, own = self._sigma(f_dressed, V_dressed, t2)
        try:
            out = sig.apply_many([ctx.array(np.asarray(x, dtype=np.float64).reshape(sig.shape1)) for x in r1s],
                                 [ctx.array(np.asarray(x, dtype=np.float64).reshape(sig.shape2)) for x in r2s])
            out = [(a.get(), b.get()) for a, b in out]
            return out if many else out[0]
        finally:
            sig.close()
            if own:
                ctx.close()

    def apply_left(self, f_dressed, V_dressed, t2, l1, l2):
        """One adjoint build for host arrays: (H^T l)_1, (H^T l)_2 of (l1, l2), or lists of them for lists (stacked build)."""
        many = isinstance(l1, (list, tuple))
        l1s, l2s = (list(l1), list(l2)) if many else ([l1], [l2])
        ctx, sig, own = self._sigma(f_dressed, V_dressed, t2)
        try:
            out = sig.apply_left_many([ctx.array(np.asarray(x, dtype=np.float64).reshape(sig.shape1)) for x in l1s],
                                      [ctx.array(np.asarray(x, dtype=np.float64).reshape(sig.shape2)) for x in l2s])
            out = [(a.get(), b.get()) for a, b in out]
            return out if many else out[0]
        finally:
            sig.close()
            if own:
                ctx.close()

    def solve(self, f_dressed, V_dressed, t2):
        """The ``n_roots`` lowest eigenvalues, ascending.  Call forms as ``EOM_CCSD.solve``: (dressed Fock matrix, dictionary
        of dressed host blocks, host T2) — a context is built and dies with the call —, or the device hand-over of a CCSD
        solve (``DressedDeviceIntegrals`` from ``CCSD.get_T1_dressed_V(t1, DeviceIntegrals, BLOCKS)``, T2 a DeviceArray of
        that context): nothing of size o^2 v crosses PCIe.

        Block Davidson: start from unit vectors on the n_roots smallest d1; per pass sigma of the NEW vectors only, the
        subspace matrix extended by their rows and columns, the Ritz pairs of the n_roots lowest eigenvalues, their
        residuals and element-wise preconditioned corrections from one launch (one synchronisation for all norms);
        converged when every root has |s - w r| / |r| < r_epsilon; collapse to the Ritz vectors at max_dim = 8 n_roots.
        Complex Ritz pairs: real parts are taken, the imaginary parts are logged.  The roots are the lowest ones of the
        Krylov space of the start vectors: a state without any singles component (a pure 2h1p / 2p1h satellite that a
        symmetry decouples from every Koopmans vector) cannot be reached from them and is not returned."""
        print_title(self.NAME + " Solver", )
        t_start = time.time()
        from pymes_amd.solver.ccd import quiet_collector
        ctx, sig, own = self._sigma(f_dressed, V_dressed, t2)
        collector = quiet_collector().__enter__()
        nr = self.n_roots
        try:
            if nr < 1 or nr > sig.n1:
                raise ValueError("%s: 1 <= n_roots <= %d (the number of singles)" % (self.NAME, sig.n1))
            lay = sig.layout
            d = sig.diagonals()
            d1 = sig.part1(d).get().ravel()
            start = [lay.unit(p) for p in np.argsort(d1, kind="stable")[:nr]]
            flat = lambda vecs: subspace.apply_flat(lay, sig.apply_many, vecs)
            # a vector that brings nothing new is dropped, not replaced: the roots are those of the Krylov space of the start
            dav = subspace.block_davidson(ctx, lay, flat, sig.correction, d, start, nr, self.max_dim, self.max_iter, self.r_epsilon,
                                          self.shift, label=self.NAME, on_null=subspace.DROP_NULL)
            e, rel, rz, nrm = dav.theta, dav.rel, dav.rz, dav.nrm
            self.history, self.converged, self.iterations = dav.history, dav.converged, dav.passes
            print_logging_info("{} finished in {:.3f} seconds".format(self.NAME, time.time() - t_start), level=1)
            order = np.argsort(e, kind="stable")
            self.e = e[order]
            self.residual_norms = rel[order]
            scale = 1.0 / np.sqrt(nrm[order])
            r1s = [sig.part1(rz[n]) for n in order]
            w1 = np.array([ctx.gram([x], [x])[0, 0] for x in r1s])
            self.singles_weight = w1 / nrm[order]
            vecs = []
            for j, n in enumerate(order):                                      # unit norm
                ctx.lincomb_multi([rz[n]], [], np.zeros((0, 1)), beta=[scale[j]])
                vecs.append(rz[n])
            self.r_singles = [sig.part1(x) for x in vecs]
            self.r_doubles = [sig.part2(x) for x in vecs]
            if own:
                self.r_singles = [x.get() for x in self.r_singles]
                self.r_doubles = [x.get() for x in self.r_doubles]
            for r in range(nr):
                print_logging_info("Root {:d} energy = {:.12f}".format(r, self.e[r]), level=2)
            return self.e
        finally:
            collector.__exit__()
            sig.close()
            if own:
                ctx.close()


class IP_EOM_CCSD(_IPEA_EOM_CCSD):
    """Ionisation potentials E(N-1) - E(N); r1[i], r2[i,j,b]."""
    KIND, NAME = KIND_IP, "IP-EOM-CCSD"
    BLOCKS = IPEASigma.BLOCKS[KIND_IP]             # for DressedDeviceIntegrals.require and CCSD.get_T1_dressed_V(t1, ints, BLOCKS)


class EA_EOM_CCSD(_IPEA_EOM_CCSD):
    """Electron affinities E(N+1) - E(N); r1[a], r2[a,b,j]."""
    KIND, NAME = KIND_EA, "EA-EOM-CCSD"
    BLOCKS = IPEASigma.BLOCKS[KIND_EA]
