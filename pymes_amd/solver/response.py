"""EOM-CCSD linear response functions and polarizabilities at real and complex frequencies.

``EOM_CCSD_Response(no).solve(f_dressed, dict_or_DressedDeviceIntegrals, t2, t1, operators, omegas, gamma=0.0, lam=None)`` gives

  <<X;Y>>_z = sum_k [ <0|X|k><k|Y|0> / (z - w_k) - <0|Y|k><k|X|0> / (z + w_k) ],   z = w + i gamma,   polarizability = -<<X;Y>>_z

in its resolvent form, without a single root: with the property vectors xi(O), eta(O) of ``pymes_response_vectors`` (definitions
and written-out formulas in include/pymes_amd.h) and x^O(z) = (z - A)^-1 xi(O) on the exchange-symmetric subspace,

  <<X;Y>>_z = <eta(X), x^Y(z)> + <eta(Y), x^X(-z)>.

Everything runs on ONE hoisted sigma handle (csrc/eom.cpp, ``EomSigma``): Lambda (unless ``lam`` is given), then the linear
systems (operator, +z) and (operator, -z) of every frequency together.  The method is GCR with a truncated, per-system subspace
(Orthomin(m), m = ``history``) and the diagonal preconditioner 1 / (z - d), d from ``pymes_eom_diagonals``.  Per sweep: sigma of
the preconditioned directions of all unconverged systems in ONE stacked ``apply_many`` (real and imaginary parts stacked in the
same call; with gamma = 0 everything stays real), the dots of the orthogonalisation of all systems from one launch
(``pymes_response_dots``, one synchronisation), and the fused step — orthogonalisation against the stored directions, update of x
and r, the next preconditioned direction and |r|^2 of all systems in one launch and one pass (``pymes_response_update``, one
synchronisation).  A system stops at |xi - (z - A) x| <= r_epsilon |xi|; the residuals reported are measured again with a fresh
sigma build.  A system that does not converge is reported (``"converged": False``), not raised.
"""
import ctypes as C
import time

import numpy as np

from pymes_amd import _lib
from pymes_amd.device import DeviceArray, PymesError
from pymes_amd.log import print_logging_info, print_title
from pymes_amd.solver import lambda_ccsd, subspace

OPS_MAX = 64           # operators per pymes_response_vectors call
STACK_MAX = 4096       # vectors per pymes_eom_sigma_apply call
SYSTEMS_MAX = 4096     # systems per pymes_response_dots / _update call


def check_occupied(no):
    lambda_ccsd.check_occupied(no, "EOM_CCSD_Response")


def check_context(ctx, no):
    """The refusals that need no allocation (as ``eom_transitions.check_context``)."""
    if getattr(ctx, "shard", None) is not None:
        raise PymesError("EOM_CCSD_Response: not available with integral sharding (shard=%s): the sigma builds read the whole "
                         "V_abcd" % (ctx.shard,))
    if getattr(ctx, "direct", None):
        raise PymesError("EOM_CCSD_Response: not available on a factor-direct context: the sigma builds read the whole V_abcd")
    if getattr(ctx, "recording", False):
        raise PymesError("EOM_CCSD_Response: the context is recording a launch graph")
    check_occupied(no)


def check_operators(operators, n, name="EOM_CCSD_Response"):
    """The operators as a float64 [m,n,n] array; anything else is refused by name (no conversion of dtype: a complex or integer
    array is a mistake of the caller's)."""
    ops = np.asarray(operators)
    if ops.dtype != np.float64:
        raise ValueError("%s: operators must be float64 (real one-body operators), not %s" % (name, ops.dtype))
    if ops.ndim == 2:
        ops = ops[None]
    if ops.ndim != 3 or ops.shape[1:] != (n, n) or ops.shape[0] < 1:
        raise ValueError("%s: operators must be [m, n, n] with n = %d (occupied orbitals first), not %s" % (name, n, ops.shape))
    return np.ascontiguousarray(ops)


def device_response_vectors(ctx, t1, t2, lam1, lam2, operators, out=None):
    """(xi1, xi2, eta1, eta2, g0): lists of device arrays and g0 [k] (host) for the operators [k,n,n] (``pymes_response_vectors``);
    every input a device array of ctx.  ``out``: (xi1s, xi2s, eta1s, eta2s) device arrays to write to instead of fresh ones."""
    ops = check_operators(operators, ctx.n, "response_vectors")
    nv, no = ctx.nv, ctx.no
    if out is None:
        out = tuple([ctx.empty(shape) for _ in range(len(ops))] for shape in ((nv, no), (nv, nv, no, no)) * 2)
    g0 = np.zeros(len(ops))
    for lo in range(0, len(ops), OPS_MAX):
        sl = slice(lo, lo + OPS_MAX)
        chunk = np.ascontiguousarray(ops[sl])
        ctx.lib.call("pymes_response_vectors", ctx.handle, C.c_void_p(t1.ptr), C.c_void_p(t2.ptr), C.c_void_p(lam1.ptr),
                     C.c_void_p(lam2.ptr), len(chunk), _lib.host_ptr(chunk), *[_lib.ptr_array([x.ptr for x in part[sl]]) for part in out],
                     _lib.host_ptr(g0[sl]))
    return out[0], out[1], out[2], out[3], g0


class _System:
    """One linear system (z - A) x = xi(O): its vectors as (re, im) pairs of flat device vectors (im None: real)."""

    def __init__(self, op, z, cplx):
        self.op, self.z, self.cplx = op, complex(z), cplx
        self.x = self.r = self.p = self.ap = self.pn = None
        self.alpha, self.inv, self.g = 0j, 1.0, []
        self.hp, self.hq = [], []
        self.norm0 = self.norm = np.inf
        self.iterations, self.active, self.broke = 0, True, False

    def parts(self):
        return 2 if self.cplx else 1


def _pair(struct_field, vec):
    struct_field[0] = vec[0].ptr if vec is not None else None
    struct_field[1] = vec[1].ptr if vec is not None and vec[1] is not None else None


class EOM_CCSD_Response:
    BLOCKS = lambda_ccsd.Lambda_CCSD.BLOCKS
    DRIFT = 1.01           # a system stops on the recurrence's |r|; the fresh residual may exceed r_epsilon by its rounding drift

    def __init__(self, no, r_epsilon=1.e-8, max_iter=200, device=0):
        self.algo_name = "EOM-CCSD response"
        self.no = no
        self.r_epsilon = float(r_epsilon)
        self.max_iter = int(max_iter)
        self.device = device
        self.history = 12                     # m of Orthomin(m): stored direction pairs per system (<= _lib.RESPONSE_HIST)
        self.floor = 1.e-3                    # the floor of |z - d| in the preconditioner
        self.lambda_r_epsilon = None          # (default: r_epsilon)
        self.keep_solutions = False           # True: the result also holds "x", the solutions as host (singles, doubles) pairs
        self.result = None
        self.lambda_solver = None
        self.sweeps = 0
        self.calls = {"apply": 0, "dots": 0, "update": 0}      # library calls of the last solve's sweeps

    # ---- the sweep's library calls --------------------------------------------------------------------------------------------------
    def _describe(self, systems, with_step, with_coeff=True):
        """The systems as the library's array of structures (``with_step`` False: no direction, the start of a solve;
        ``with_coeff`` False: before the step's coefficients exist, for the dots)."""
        arr = (_lib.ResponseSystem * len(systems))()
        for s, sy in zip(arr, systems):
            _pair(s.x, sy.x)
            _pair(s.r, sy.r)
            _pair(s.p, sy.p if with_step else None)
            _pair(s.ap, sy.ap if with_step else None)
            _pair(s.pn, sy.pn)
            s.nh = len(sy.hp) if with_step else 0
            for j in range(s.nh):
                _pair(s.hp[j], sy.hp[j])
                _pair(s.hq[j], sy.hq[j])
                if with_coeff:
                    s.g[j][0], s.g[j][1] = sy.g[j].real, sy.g[j].imag
            if with_coeff:
                s.alpha[0], s.alpha[1] = sy.alpha.real, sy.alpha.imag
            s.z[0], s.z[1] = sy.z.real, sy.z.imag
            s.inv = sy.inv
        return arr

    def _dots(self, ctx, lay, systems):
        out = np.zeros((len(systems), _lib.RESPONSE_DOTS))
        for lo in range(0, len(systems), SYSTEMS_MAX):
            chunk = systems[lo:lo + SYSTEMS_MAX]
            ctx.lib.call("pymes_response_dots", ctx.handle, len(chunk), C.byref(self._describe(chunk, True, False)), lay.off2,
                         lay.nflat, _lib.host_ptr(out[lo:lo + SYSTEMS_MAX]))
            self.calls["dots"] += 1
        return out

    def _update(self, ctx, lay, d, systems, with_step):
        out = np.zeros(len(systems))
        for lo in range(0, len(systems), SYSTEMS_MAX):
            chunk = systems[lo:lo + SYSTEMS_MAX]
            ctx.lib.call("pymes_response_update", ctx.handle, len(chunk), C.byref(self._describe(chunk, with_step)), C.c_void_p(d.ptr),
                         self.floor, lay.off2, lay.nflat, _lib.host_ptr(out[lo:lo + SYSTEMS_MAX]))
            self.calls["update"] += 1
        return out

    def _apply(self, lay, sig, vecs):
        """A of flat vectors, ONE stacked call (chunked only beyond what a call accepts)."""
        outs = []
        for lo in range(0, len(vecs), STACK_MAX):
            chunk = vecs[lo:lo + STACK_MAX]
            outs += subspace.apply_flat(lay, sig.apply_many, chunk, [True] * len(chunk))
            self.calls["apply"] += 1
        return outs

    def _sweep(self, ctx, lay, sig, d, todo):
        """One sweep over the unconverged systems ``todo``: one stacked sigma build, the dots (synchronisation 1), the fused step
        (synchronisation 2)."""
        cplx = todo[0].cplx
        for sy in todo:
            sy.p, sy.pn = sy.pn, None
        flat = [v for sy in todo for v in sy.p[:sy.parts()]]
        aps = self._apply(lay, sig, flat)                                          # ONE stacked sigma build
        at = 0
        for sy in todo:
            sy.ap = (aps[at], aps[at + 1] if cplx else None)
            at += sy.parts()
        dots = self._dots(ctx, lay, todo)                                          # synchronisation 1
        step = []
        for sy, row in zip(todo, dots):
            nh = len(sy.hp)
            g = row[0:2 * nh:2] + 1j * row[1:2 * nh:2]
            qq, qr = row[2 * nh], complex(row[2 * nh + 2], row[2 * nh + 3])
            left = qq - float((np.abs(g) ** 2).sum())                              # |q - sum_j g_j hq_j|^2, hq orthonormal
            if not np.isfinite(left) or left <= 1e-12 * max(qq, 1e-300):     # (below that the one-round Gram-Schmidt has lost it)
                sy.active, sy.broke = False, True                                 # nothing new in this direction: reported
                continue
            sy.g, sy.inv = list(g), 1.0 / np.sqrt(left)
            sy.alpha = qr * sy.inv                                                 # <qh, r>: r is orthogonal to the stored hq
            sy.pn = (lay.empty(), lay.empty() if cplx else None)
            step.append(sy)
        if step:
            norms = self._update(ctx, lay, d, step, True)                          # synchronisation 2
            for sy, nrm in zip(step, norms):
                sy.norm = float(np.sqrt(nrm))
                sy.iterations += 1
                sy.hp.append(sy.p)                                                 # (the update left ph, qh in p and ap)
                sy.hq.append(sy.ap)
                if len(sy.hp) > self.history:
                    sy.hp.pop(0)
                    sy.hq.pop(0)
                sy.p = sy.ap = None
                if not np.isfinite(sy.norm):
                    sy.active, sy.broke = False, True
                elif sy.norm <= self.r_epsilon * sy.norm0:
                    sy.active = False
                if not sy.active:
                    sy.hp, sy.hq = [], []                                          # (its stored directions go back to the pool)

    # ---- the solve --------------------------------------------------------------------------------------------------------------------
    def solve(self, f_dressed, V_dressed, t2, t1, operators, omegas, gamma=0.0, lam=None, eps=None, level_shift=0.0):
        """Call forms as ``EOM_CCSD.solve``: (dressed Fock matrix, dictionary of dressed host blocks, host T2) — a context is
        built and dies with the call — or the device hand-over of a CCSD solve (``DressedDeviceIntegrals``, T2 a host array or a
        DeviceArray of that context).  ``t1`` [v,o]: the converged singles; ``operators`` [m,n,n]: real one-body operators in
        the basis of f (occupied orbitals first; they need not be symmetric); ``omegas``: the frequencies w; ``gamma``: the
        damping, z = w + i gamma; ``lam = (lambda1, lambda2)``: a Lambda solution the caller has (else solved here; ``eps`` /
        ``level_shift`` as ``Lambda_CCSD.solve``).  Returns the result dictionary (host arrays): "response" [nf,m,m] (complex
        only when gamma != 0), "polarizability" (its negative), "omegas", "residuals", "iterations", "converged" ([nf,m,2]: the
        systems (operator, +z) and (operator, -z); relative residuals re-measured with a fresh sigma build), "xi", "eta" (lists
        of (singles, doubles)), "g0", "lambda1", "lambda2"."""
        print_title("EOM-CCSD response solver", )
        t_start = time.time()
        from pymes_amd.integral.device import DressedDeviceIntegrals
        from pymes_amd.solver.ccd import quiet_collector
        if isinstance(V_dressed, DressedDeviceIntegrals):
            check_context(V_dressed.ctx, self.no)
        else:
            check_occupied(self.no)
        ops = check_operators(operators, int(np.shape(f_dressed)[0]))
        omegas = np.atleast_1d(np.asarray(omegas, dtype=np.float64)).copy()
        if omegas.ndim != 1 or omegas.size < 1 or not np.all(np.isfinite(omegas)):
            raise ValueError("EOM_CCSD_Response: omegas must be a non-empty list of finite real frequencies")
        gamma = float(gamma)
        if not np.isfinite(gamma):
            raise ValueError("EOM_CCSD_Response: gamma must be finite")
        if not 1 <= int(self.history) <= _lib.RESPONSE_HIST:
            raise ValueError("EOM_CCSD_Response: 1 <= history <= %d" % _lib.RESPONSE_HIST)
        f, ctx, sig, own = subspace.open_handle(self.no, self.device, f_dressed, V_dressed, t2, self.BLOCKS, lambda_ccsd.LeftSigma,
                                                self.algo_name)
        collector = quiet_collector().__enter__()
        try:
            # (a frame of its own: its device vectors are released when it returns, before the pool is trimmed below)
            return self._solve_on(ctx, sig, f, V_dressed, t2, t1, ops, omegas, gamma, lam, eps, level_shift, t_start)
        finally:
            collector.__exit__()
            sig.close()
            if not isinstance(t2, DeviceArray):
                sig.T = None             # (the copy made for this solve: the context's close list keeps the closed handle itself alive)
            if own:
                ctx.close()
            elif ctx.handle is not None:
                ctx.trim()

    def _solve_on(self, ctx, sig, f, V_dressed, t2, t1, ops, omegas, gamma, lam, eps, level_shift, t_start):
        """The solve on an open handle (``solve`` owns its lifetime)."""
        no, nv, m, nf, cplx = self.no, ctx.nv, len(ops), len(omegas), gamma != 0.0
        lay = subspace.FlatLayout(ctx, (nv, no), (nv, nv, no, no))
        d = ctx.zeros((lay.nflat,))
        ctx.lib.call("pymes_eom_diagonals", ctx.handle, _lib.host_ptr(np.ascontiguousarray(f)), C.c_void_p(sig.T.ptr),
                     int(sig.dressed), C.c_void_p(d.ptr), C.c_void_p(d.ptr + 8 * lay.off2))
        # ---- Lambda, on the same handle -----------------------------------------------------------------------------------------
        if lam is None:
            solver = lambda_ccsd.Lambda_CCSD(no, r_epsilon=self.lambda_r_epsilon or self.r_epsilon, device=self.device)
            out = solver.solve(f, V_dressed, t2, eps=eps, level_shift=level_shift, handle=(ctx, sig))
            solver.t2 = None
            self.lambda_solver = solver
            lam, lam_ok = (out["lambda1"], out["lambda2"]), bool(out["converged"])
        else:
            lam, lam_ok = (np.asarray(lam[0], dtype=np.float64), np.asarray(lam[1], dtype=np.float64)), True
        # ---- the property vectors, straight into flat vectors --------------------------------------------------------------------
        t1d = t1 if isinstance(t1, DeviceArray) and t1.ctx is ctx else ctx.array(
            np.ascontiguousarray(t1.get() if isinstance(t1, DeviceArray) else t1, dtype=np.float64))
        xi, eta = [lay.padded() for _ in range(m)], [lay.padded() for _ in range(m)]
        *_, g0 = device_response_vectors(ctx, t1d, sig.T, ctx.array(lam[0]), ctx.array(lam[1]), ops,
                                         out=([lay.part1(x) for x in xi], [lay.part2(x) for x in xi],
                                              [lay.part1(x) for x in eta], [lay.part2(x) for x in eta]))
        # ---- the systems (operator, +z) and (operator, -z) of every frequency ------------------------------------------------------
        systems = [_System(o, sign * complex(w, gamma), cplx) for w in omegas for o in range(m) for sign in (1.0, -1.0)]
        for sy in systems:
            sy.x = (ctx.zeros((lay.nflat,)), ctx.zeros((lay.nflat,)) if cplx else None)
            sy.r = (lay.empty().copy_from(xi[sy.op]), ctx.zeros((lay.nflat,)) if cplx else None)
            sy.pn = (lay.empty(), lay.empty() if cplx else None)
            sy.alpha, sy.inv, sy.g = 0j, 1.0, []
        self.calls = {"apply": 0, "dots": 0, "update": 0}
        for sy, nrm in zip(systems, self._update(ctx, lay, d, systems, False)):       # p_0 = r_0 / (z - d), |xi|^2
            sy.norm0 = sy.norm = float(np.sqrt(nrm))
            sy.active = sy.norm0 > 0.0
        self.calls = {"apply": 0, "dots": 0, "update": 0}
        sweeps = 0
        while sweeps < self.max_iter:
            todo = [sy for sy in systems if sy.active]
            if not todo:
                break
            t_it = time.time()
            self._sweep(ctx, lay, sig, d, todo)
            sweeps += 1
            print_logging_info("Response sweep %d: %d systems, max |r| / |xi| = %.3e" % (
                sweeps, len(todo), max(sy.norm / sy.norm0 for sy in todo)), level=1)
            print_logging_info("Took {:.3f} seconds ".format(time.time() - t_it), level=2)
        self.sweeps = sweeps
        for sy in systems:
            sy.hp, sy.hq, sy.p, sy.pn, sy.r = [], [], None, None, None
        # ---- certificates from one fresh stacked build; the response function -----------------------------------------------------
        flat = [v for sy in systems for v in sy.x[:sy.parts()]]
        ax = self._apply(lay, sig, flat)
        # res = xi - z x + A x, written over A x (the Gram matrix of these vectors would lose it to cancellation)
        np_ = 2 if cplx else 1
        for s, sy in enumerate(systems):
            z, mine = sy.z, slice(np_ * s, np_ * s + np_)
            coef = np.array([[1.0, 0.0], [-z.real, -z.imag], [z.imag, -z.real], [1.0, 0.0], [0.0, 1.0]]) if cplx else \
                np.array([[1.0], [-z.real], [1.0]])
            ctx.lincomb_multi(ax[mine], [xi[sy.op]] + flat[mine] + ax[mine], coef)
        r2 = ctx.dots(ax, ax).reshape(len(systems), np_).sum(axis=1)
        rel = np.array([np.sqrt(r2[s]) / sy.norm0 if sy.norm0 > 0.0 else 0.0 for s, sy in enumerate(systems)])
        G = ctx.gram(eta, flat)                                                        # <eta(X), Re / Im x_s>
        dtype = np.complex128 if cplx else np.float64
        resp = np.zeros((nf, m, m), dtype=dtype)

        def braket(X, s):       # <eta(X), x_s>
            return G[X, np_ * s] + (1j * G[X, np_ * s + 1] if cplx else 0.0)
        index = {(w, o, sg): 2 * (w * m + o) + sg for w in range(nf) for o in range(m) for sg in (0, 1)}
        for w in range(nf):
            for X in range(m):
                for Y in range(m):
                    resp[w, X, Y] = braket(X, index[(w, Y, 0)]) + braket(Y, index[(w, X, 1)])
        shape = (nf, m, 2)
        ok = np.array([(rel[s] <= self.DRIFT * self.r_epsilon) and not sy.broke or sy.norm0 == 0.0 for s, sy in enumerate(systems)])
        self.result = {"response": resp, "polarizability": -resp, "omegas": omegas, "gamma": gamma,
                       "residuals": rel.reshape(shape), "iterations": np.array([sy.iterations for sy in systems]).reshape(shape),
                       "converged": bool(lam_ok and np.all(ok)), "converged systems": ok.reshape(shape), "sweeps": sweeps,
                       "xi": [(lay.part1(x).get(), lay.part2(x).get()) for x in xi],
                       "eta": [(lay.part1(x).get(), lay.part2(x).get()) for x in eta], "g0": g0,
                       "lambda1": lam[0], "lambda2": lam[1]}
        if self.keep_solutions:
            def host(vec, part):
                return part(vec[0]).get() + (1j * part(vec[1]).get() if cplx else 0.0)
            self.result["x"] = [(host(sy.x, lay.part1), host(sy.x, lay.part2)) for sy in systems]
        print_logging_info("EOM-CCSD response finished in {:.3f} seconds".format(time.time() - t_start), level=1)
        return self.result

    # ---- what users ask of the tensor ---------------------------------------------------------------------------------------------------
    def isotropic(self):
        """The mean of the diagonal of the polarizability, per frequency."""
        if self.result is None:
            raise RuntimeError("isotropic: needs a finished solve()")
        a = self.result["polarizability"]
        return np.trace(a, axis1=1, axis2=2) / a.shape[1]

    def spectral_density(self):
        """Im tr polarizability / pi per frequency (zero without damping)."""
        if self.result is None:
            raise RuntimeError("spectral_density: needs a finished solve()")
        return np.imag(np.trace(self.result["polarizability"], axis1=1, axis2=2)) / np.pi
