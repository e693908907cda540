"""IP- and EA-EOM-CCSD on the MI355X engine: ionisation potentials and electron affinities of a closed-shell CCSD state.

``IP_EOM_CCSD(no, n_roots).solve(f_dressed, dict_or_DressedDeviceIntegrals, t2)`` returns the ``n_roots`` lowest eigenvalues
``E(N-1) - E(N)`` of the IP operator, ``EA_EOM_CCSD`` those of ``E(N+1) - E(N)``, ascending; doublet final states, right
eigenvectors.  Vectors: IP ``r1[i], r2[i,j,b]`` (``i`` the orbital the electron leaves), EA ``r1[a], r2[a,b,j]``.

The operator is the EE-EOM-CCSD sigma (eom_ccsd.py:268-385) restricted to the sector with one extra orbital that interacts
with nothing (formulas: include/pymes_amd.h, ``pymes_ipea_sigma_*``).  The sigma build runs in the engine
(csrc/eom.cpp, ``IpEaSigma``): everything that does not depend on the trial vector is hoisted once per solve, all vectors of a
call go through each product as one GEMM.  The driver is a block Davidson on flat device vectors with the subspace tools of
the EE driver; unlike that one — which is pinned to the reference pass by pass — it preconditions element-wise with the
diagonals and stops on the relative residual norm of every root.
"""
import ctypes as C
import time

import numpy as np

from pymes_amd import _lib
from pymes_amd.device import Context, DeviceArray, PymesError
from pymes_amd.integral.device import DressedDeviceIntegrals
from pymes_amd.log import print_logging_info, print_title
from pymes_amd.mixer.diis import _single_threaded_blas
from pymes_amd.solver.eom_ccsd import EOM_CCSD

KIND_IP, KIND_EA = 0, 1           # PYMES_IPEA_IP / PYMES_IPEA_EA of include/pymes_amd.h


class IPEASigma:
    """Device-resident IP / EA sigma build: a handle of the engine's ``IpEaSigma`` (``pymes_ipea_sigma_prepare / _apply /
    _diagonals / _correction``)."""

    # the dressed blocks each operator reads (the IP operator never reads abcd or abic: it runs on a sharded context)
    BLOCKS = {KIND_IP: ("ijab", "iabj", "iajb", "ijka", "ijak", "iabc", "iajk", "klij"),
              KIND_EA: ("ijab", "iabj", "iajb", "ijka", "iabc", "abic", "abcd")}

    def __init__(self, ctx, kind, f, t2, dressed=False):
        self.ctx, self.kind = ctx, int(kind)
        self.no, self.nv = ctx.no, ctx.nv
        self.dressed = bool(dressed)
        self.T = t2                                   # (kept alive: the handle reads it in every build)
        self._f = np.ascontiguousarray(f, dtype=np.float64)
        if self._f.shape != (ctx.n, ctx.n):
            raise ValueError("the dressed Fock matrix must be [n, n]")
        o, v = self.no, self.nv
        self.shape1, self.shape2 = ((o,), (o, o, v)) if self.kind == KIND_IP else ((v,), (v, v, o))
        self.n1, self.n2 = int(np.prod(self.shape1)), int(np.prod(self.shape2))
        self.off2 = -(-self.n1 // 32) * 32            # the doubles part on a 256-byte boundary
        self.nflat = self.off2 + self.n2
        self._h = None
        h = C.c_void_p()
        ctx.lib.call("pymes_ipea_sigma_prepare", ctx.handle, _lib.host_ptr(self._f), C.c_void_p(t2.ptr), int(self.dressed),
                     self.kind, C.byref(h))
        self._h = h
        ctx.on_close(self._ctx_closing)               # the handle dies before its context

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            self.ctx.lib.call("pymes_ipea_sigma_destroy", h)

    def _ctx_closing(self, ctx):
        try:
            self.close()
        except Exception:
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise PymesError("the IP / EA sigma handle has been destroyed (its context was closed)")
        return self._h

    # ---- flat vectors [r1 | zero pad | r2] -----------------------------------------------------------------------------
    def part1(self, vec):
        return DeviceArray(self.ctx, vec.ptr, self.shape1, owned=False, keepalive=vec)

    def part2(self, vec):
        return DeviceArray(self.ctx, vec.ptr + 8 * self.off2, self.shape2, owned=False, keepalive=vec)

    def zero_pad(self, vec):
        if self.off2 > self.n1:
            DeviceArray(self.ctx, vec.ptr + 8 * self.n1, (self.off2 - self.n1,), owned=False, keepalive=vec).zero_()
        return vec

    def apply_many(self, r1s, r2s, out1=None, out2=None):
        """[(sigma1_z, sigma2_z)] for the trial vectors (r1s[z], r2s[z]), device arrays; one library call."""
        h, c, k = self._handle(), self.ctx, len(r1s)
        s1 = [out1[z] if out1 is not None else c.empty(self.shape1) for z in range(k)]
        s2 = [out2[z] if out2 is not None else c.empty(self.shape2) for z in range(k)]
        c.lib.call("pymes_ipea_sigma_apply", h, k, _lib.ptr_array([u.ptr for u in r1s]), _lib.ptr_array([u.ptr for u in r2s]),
                   _lib.ptr_array([x.ptr for x in s1]), _lib.ptr_array([x.ptr for x in s2]))
        return list(zip(s1, s2))

    def apply_flat(self, vecs):
        """sigma of flat vectors, as new flat vectors (zero pad)."""
        outs = [self.zero_pad(self.ctx.empty((self.nflat,))) for _ in vecs]
        self.apply_many([self.part1(u) for u in vecs], [self.part2(u) for u in vecs],
                        out1=[self.part1(w) for w in outs], out2=[self.part2(w) for w in outs])
        return outs

    def diagonals(self):
        """The flat diagonal [d1 | 0 | d2] (device)."""
        h = self._handle()
        d = self.ctx.zeros((self.nflat,))
        self.ctx.lib.call("pymes_ipea_sigma_diagonals", h, C.c_void_p(d.ptr), C.c_void_p(d.ptr + 8 * self.off2))
        return d

    def correction(self, ss, rs, w, d, shift, qs):
        """q_n = (s_n - w_n r_n) / (w_n - d + shift) into qs for all roots in one launch; returns (|s_n - w_n r_n|^2,
        |r_n|^2) per root (one synchronisation)."""
        n = len(rs)
        ww = np.ascontiguousarray(w, dtype=np.float64)
        out = np.zeros(2 * max(n, 1))
        self.ctx.lib.call("pymes_ipea_sigma_correction", self._handle(), n, _lib.ptr_array([x.ptr for x in ss]),
                          _lib.ptr_array([x.ptr for x in rs]), _lib.host_ptr(ww), C.c_void_p(d.ptr), float(shift),
                          _lib.ptr_array([x.ptr for x in qs]), self.off2, self.nflat, _lib.host_ptr(out))
        return out[0:2 * n:2].copy(), out[1:2 * n:2].copy()


class _IPEA_EOM_CCSD(EOM_CCSD):
    """Block Davidson for the lowest right eigenpairs of the IP / EA operator (the subspace tools of ``EOM_CCSD``:
    ``ctx.gram``, ``ctx.lincomb_multi``, ``_orthonormalise_block``)."""
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

    # ---- device plumbing ----------------------------------------------------------------------------------------------
    def _open(self, f, V, t2):
        """(ctx, sigma handle, owns the context) for the two call forms."""
        if isinstance(f, DeviceArray):
            f = f.get()
        f = np.asarray(f, dtype=np.float64)
        nv = f.shape[0] - self.no
        if isinstance(V, DressedDeviceIntegrals):
            ctx = V.ctx
            self.check_context(ctx)
            if ctx.no != self.no or ctx.nv != nv:
                raise ValueError("the integrals' context does not match (no, nv) of the Fock matrix")
            if isinstance(t2, DeviceArray) and t2.ctx is not ctx:
                raise ValueError("t2 lives in another context than the dressed integrals")
            V.require(self.BLOCKS)
            t2d = t2 if isinstance(t2, DeviceArray) else ctx.array(t2)
            return ctx, IPEASigma(ctx, self.KIND, f, t2d, dressed=True), False
        ctx = Context(self.no, nv, device=self.device)
        try:
            for name in self.BLOCKS:
                blk = V.get(name)
                if blk is None:
                    raise KeyError("%s: the dressed block '%s' is missing from the dictionary" % (self.NAME, name))
                ctx.set_V_block(name, np.ascontiguousarray(blk, dtype=np.float64))
            return ctx, IPEASigma(ctx, self.KIND, f, ctx.array(np.asarray(t2, dtype=np.float64)), dressed=False), True
        except Exception:
            ctx.close()
            raise

    def apply(self, f_dressed, V_dressed, t2, r1, r2):
        """One sigma build for host arrays: (sigma1, sigma2) of (r1, r2), or lists of them for lists (stacked build)."""
        many = isinstance(r1, (list, tuple))
        r1s, r2s = (list(r1), list(r2)) if many else ([r1], [r2])
        ctx, sig, own = self._open(f_dressed, V_dressed, t2)
        try:
            out = sig.apply_many([ctx.array(np.asarray(x, dtype=np.float64).reshape(sig.shape1)) for x in r1s],
                                 [ctx.array(np.asarray(x, dtype=np.float64).reshape(sig.shape2)) for x in r2s])
            out = [(a.get(), b.get()) for a, b in out]
            return out if many else out[0]
        finally:
            sig.close()
            if own:
                ctx.close()

    # ---- the fall-back of _orthonormalise_block for this vector layout: Gram-Schmidt one by one, null vectors dropped ----
    def _orthonormalise_sequential(self, ctx, us, ys, lay, shadows=None):
        if shadows is not None:
            raise np.linalg.LinAlgError("linearly dependent Ritz vectors in the Davidson collapse")
        done = list(us)
        for y in ys:
            q = ctx.empty((lay[2],)).copy_from(y)
            nrm0 = np.sqrt(ctx.gram([q], [q])[0, 0])
            for _ in range(2):
                if done:
                    proj = ctx.gram(done, [q])[:, 0]
                    ctx.lincomb_multi([q], done, -proj[:, None], beta=[1.0])
            nrm = np.sqrt(ctx.gram([q], [q])[0, 0])
            if not (np.isfinite(nrm) and nrm > 1e-10 * max(nrm0, 1e-300) and nrm > 0.0):
                continue                                       # nothing new in this direction
            ctx.lincomb_multi([q], [], np.zeros((0, 1)), beta=[1.0 / nrm])
            done.append(q)
        return done[len(us):]

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
        ctx, sig, own = self._open(f_dressed, V_dressed, t2)
        collector = quiet_collector().__enter__()
        nr = self.n_roots
        try:
            if nr < 1 or nr > sig.n1:
                raise ValueError("%s: 1 <= n_roots <= %d (the number of singles)" % (self.NAME, sig.n1))
            lay = (sig.n1, sig.off2, sig.nflat)
            fresh = lambda: ctx.empty((sig.nflat,))
            d = sig.diagonals()
            d1 = sig.part1(d).get().ravel()
            new = []
            for p in np.argsort(d1, kind="stable")[:nr]:
                vec = ctx.zeros((sig.nflat,))
                one = np.zeros(sig.n1)
                one[p] = 1.0
                sig.part1(vec).set(one.reshape(sig.shape1))
                new.append(vec)
            us, ws, B = [], [], np.zeros((0, 0))
            self.history, self.converged = [], False
            e, rel, rz, nrm = np.zeros(nr), np.full(nr, np.inf), [], np.ones(nr)
            for it in range(self.max_iter):
                t_it = time.time()
                new = self._orthonormalise_block(ctx, us, new, lay) if new else []
                if new:
                    wn = sig.apply_flat(new)                                    # sigma of the new vectors only
                    d0 = len(us)
                    us, ws = us + new, ws + wn
                    Bn = np.zeros((len(us), len(us)))
                    Bn[:d0, :d0] = B
                    Bn[:, d0:] = ctx.gram(us, wn)
                    if d0:
                        Bn[d0:, :d0] = ctx.gram(new, ws[:d0])
                    B = Bn
                elif it > 0:
                    print_logging_info("No new direction left: the subspace is invariant.", level=1)
                    break
                with _single_threaded_blas():
                    lam, vec = np.linalg.eig(B)
                pick = np.argsort(lam.real, kind="stable")[:nr]
                e, e_imag = np.real(lam[pick]), np.imag(lam[pick])
                v = np.real(vec[:, pick])
                v = v / np.linalg.norm(v, axis=0)[None, :]
                rz, sz, qs = [fresh() for _ in range(nr)], [fresh() for _ in range(nr)], [fresh() for _ in range(nr)]
                ctx.lincomb_multi(rz, us, v)
                ctx.lincomb_multi(sz, ws, v)
                res, nrm = sig.correction(sz, rz, e, d, self.shift, qs)
                rel = np.sqrt(res / nrm)
                self.history.append(np.array(e))
                self.iterations = it + 1
                print_logging_info("Iteration = ", it, level=1)
                for r in range(nr):
                    print_logging_info("Root {:d} energy = {:.12f}  |residual| / |r| = {:.3e}".format(r, e[r], rel[r]), level=2)
                if np.abs(e_imag).max() > 0.0:
                    print_logging_info("Ritz values imaginary part = ", e_imag, level=2)
                print_logging_info("Took {:.3f} seconds ".format(time.time() - t_it), level=2)
                if np.all(rel < self.r_epsilon):
                    self.converged = True
                    print_logging_info("Iterative solver converged.", level=1)
                    break
                todo = [n for n in range(nr) if not rel[n] < self.r_epsilon]
                if len(us) + len(todo) > self.max_dim:                         # collapse to the Ritz vectors
                    us, ws = self._orthonormalise_block(ctx, [], rz, lay, shadows=sz)
                    B = ctx.gram(us, ws)
                new = [qs[n] for n in todo]
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
