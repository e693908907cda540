"""Left EOM-CCSD eigenvectors, transition densities and strengths on the MI355X engine.

``EOM_CCSD_Transitions(no, n_excit).solve(f_dressed, dict_or_DressedDeviceIntegrals, t2, t1, lam=None)`` solves, on ONE hoisted
sigma handle (csrc/eom.cpp, ``EomSigma``), the right problem ``A r_k = w_k r_k``, the Lambda equations ``A^T lambda + eta = 0``
(unless ``lam`` is given) and the left problem ``A^T l_k = w_k l_k``, normalises ``<l_j, r_k> = delta_jk`` with the inverse of
the k x k overlap matrix, and assembles the two transition densities of every root on the device (``pymes_tdm1``; definitions
and written-out formulas in include/pymes_amd.h):

  gammaL_k = d/df ( <l1_k, R1(f)> + <l2_k, R2(f)> ),   gammaR_k = d/df <0|(1 + Lambda) f~ (r0_k + R_k)|0>,   r0_k = -<lambda, r_k>,
  S_k(O) = (sum gammaL_k O) (sum gammaR_k O),   oscillator strength (2/3) w_k sum_x S_k(mu_x).

Both eigenproblems run through one block Davidson on flat vectors [x1 | zero pad | x2] (the layout and the subspace tools of
``EOM_CCSD``): sigma of the NEW vectors of a pass in one stacked library call (``pymes_eom_sigma_apply`` /
``pymes_eom_sigma_apply_left``), the corrections ``(s - w x) / (w - d + shift)`` of all roots and their residual norms from one
launch and one synchronisation (``pymes_eom_correction``, d from ``pymes_eom_diagonals``), collapse to the Ritz vectors at
``max_dim``.  The right run starts from unit vectors on the smallest singles diagonals and takes the lowest roots; the left run
starts from the right vectors, takes the Ritz pair nearest each w_k and measures its residual with w_k itself.  Nothing is assumed
hermitian; a root whose Ritz value keeps an imaginary part (complex pairs of strongly non-hermitian integrals) is refused by name.
"""
import ctypes as C
import time

import numpy as np

from pymes_amd import _lib
from pymes_amd.device import DeviceArray, PymesError
from pymes_amd.log import print_logging_info, print_title
from pymes_amd.mixer.diis import _single_threaded_blas
from pymes_amd.solver import lambda_ccsd
from pymes_amd.solver.eom_ccsd import EOM_CCSD

LDS_BYTES = 64 * 1024


def check_context(ctx, no):
    """The refusals that need no allocation: integral sharding, a launch graph being recorded, an o too large for the LDS tile
    of the left assembly (o (o + 1) + 256 doubles)."""
    if getattr(ctx, "shard", None) is not None:
        raise PymesError("EOM_CCSD_Transitions: not available with integral sharding (shard=%s): the left sigma reads the whole "
                         "V_abcd" % (ctx.shard,))
    if getattr(ctx, "recording", False):
        raise PymesError("EOM_CCSD_Transitions: the context is recording a launch graph")
    check_occupied(no)


def check_occupied(no):
    if 8 * (no * (no + 1) + 256) > LDS_BYTES:
        raise PymesError("EOM_CCSD_Transitions: nocc = %d is too large for the LDS tile of lambda_assemble (o (o + 1) + 256 doubles "
                         "in 64 KB)" % no)


def device_tdm1(ctx, t1, t2, lam1, lam2, l1s, l2s, r1s, r2s):
    """(gammaL [k,n,n], gammaR [k,n,n], r0 [k]) as host arrays (``pymes_tdm1``); every input a device array of ctx."""
    k, n = len(l1s), ctx.n
    gl, gr, r0 = np.zeros((k, n, n)), np.zeros((k, n, n)), np.zeros(k)
    ctx.lib.call("pymes_tdm1", ctx.handle, C.c_void_p(t1.ptr), C.c_void_p(t2.ptr), C.c_void_p(lam1.ptr), C.c_void_p(lam2.ptr), k,
                 _lib.ptr_array([x.ptr for x in l1s]), _lib.ptr_array([x.ptr for x in l2s]), _lib.ptr_array([x.ptr for x in r1s]),
                 _lib.ptr_array([x.ptr for x in r2s]), _lib.host_ptr(gl), _lib.host_ptr(gr), _lib.host_ptr(r0))
    return gl, gr, r0


class EOM_CCSD_Transitions(EOM_CCSD):
    BLOCKS = lambda_ccsd.Lambda_CCSD.BLOCKS

    def __init__(self, no, n_excit=3, r_epsilon=1.e-8, max_iter=200, device=0):
        self.algo_name = "EOM-CCSD transitions"
        self.no = no
        self.n_excit = int(n_excit)
        self.r_epsilon = float(r_epsilon)
        self.max_iter = int(max_iter)
        self.device = device
        self.max_dim = 8 * self.n_excit
        self.shift = 1.e-5
        self.lambda_r_epsilon = None                  # (default: r_epsilon)
        self.result = None
        self.lambda_solver = None

    # ---- one block Davidson for both sides --------------------------------------------------------------------------------------
    def _davidson(self, ctx, lay, apply_flat, d, start, targets, side):
        """(w [k], Ritz vectors, relative residuals [k], passes).  ``targets`` None: the k lowest roots, residuals with the Ritz
        values; else the Ritz pair nearest each target, residuals and corrections with the target itself."""
        nr, nflat = self.n_excit, lay[2]
        fresh = lambda: ctx.empty((nflat,))
        us, ws, B, new = [], [], np.zeros((0, 0)), list(start)
        rel, rz, w, complex_passes = np.full(nr, np.inf), [], np.zeros(nr), 0
        for it in range(self.max_iter):
            new = self._orthonormalise_block(ctx, us, new, lay) if new else []
            if new:
                wn = apply_flat(new)                                        # sigma of the new vectors only, one stacked call
                d0 = len(us)
                us, ws = us + new, ws + wn
                Bn = np.zeros((len(us), len(us)))
                Bn[:d0, :d0] = B
                Bn[:, d0:] = ctx.gram(us, wn)
                if d0:
                    Bn[d0:, :d0] = ctx.gram(new, ws[:d0])
                B = Bn
            elif it > 0:
                break                                                       # (the subspace is invariant)
            with _single_threaded_blas():
                lam, vec = np.linalg.eig(B)
            if targets is None:
                pick = np.argsort(lam.real, kind="stable")[:nr]
            else:
                pick, left = [], list(range(len(lam)))
                for t in targets:                                           # nearest Ritz value, each taken once
                    p = min(left, key=lambda q: abs(lam[q] - t))
                    pick.append(p)
                    left.remove(p)
                pick = np.array(pick)
            theta, imag = np.real(lam[pick]), np.imag(lam[pick])
            complex_passes = complex_passes + 1 if np.abs(imag).max() > self.r_epsilon else 0
            if complex_passes >= 3:
                bad = int(np.argmax(np.abs(imag)))
                raise PymesError("EOM_CCSD_Transitions: root %d of the %s problem has a complex Ritz value (%.6f %+.3ej): a "
                                 "complex-conjugate pair has no real eigenvector" % (bad, side, theta[bad], imag[bad]))
            v = np.real(vec[:, pick])
            v = v / np.linalg.norm(v, axis=0)[None, :]
            w = theta if targets is None else np.asarray(targets, dtype=np.float64)
            rz, sz, qs = [fresh() for _ in range(nr)], [fresh() for _ in range(nr)], [fresh() for _ in range(nr)]
            ctx.lincomb_multi(rz, us, v)
            ctx.lincomb_multi(sz, ws, v)
            res, nrm = self._correction(ctx, lay, sz, rz, w, d, qs)
            rel = np.sqrt(res / nrm)
            print_logging_info("%s pass %d" % (side, it), level=1)
            for r in range(nr):
                print_logging_info("Root {:d} energy = {:.12f}  |residual| / |x| = {:.3e}".format(r, theta[r], rel[r]), level=2)
            if np.all(rel < self.r_epsilon) and complex_passes == 0:
                return theta if targets is None else w, rz, rel, it + 1
            todo = [n for n in range(nr) if not rel[n] < self.r_epsilon]
            if len(us) + len(todo) > self.max_dim:                          # collapse to the Ritz vectors
                us, ws = self._orthonormalise_block(ctx, [], rz, lay, shadows=sz)
                B = ctx.gram(us, ws)
            new = [qs[n] for n in todo]
        return (w if targets is not None else theta), rz, rel, self.max_iter

    def _correction(self, ctx, lay, ss, rs, w, d, qs):
        n = len(rs)
        ww = np.ascontiguousarray(w, dtype=np.float64)
        out = np.zeros(2 * max(n, 1))
        ctx.lib.call("pymes_eom_correction", ctx.handle, n, _lib.ptr_array([x.ptr for x in ss]), _lib.ptr_array([x.ptr for x in rs]),
                     _lib.host_ptr(ww), C.c_void_p(d.ptr), float(self.shift), _lib.ptr_array([x.ptr for x in qs]), lay[1], lay[2],
                     _lib.host_ptr(out))
        return out[0:2 * n:2].copy(), out[1:2 * n:2].copy()

    # ---- the solve ------------------------------------------------------------------------------------------------------------------
    def solve(self, f_dressed, V_dressed, t2, t1, lam=None, eps=None, level_shift=0.0):
        """Call forms as ``EOM_CCSD.solve``: (dressed Fock matrix, dictionary of dressed host blocks, host T2) — a context is
        built and dies with the call — or the device hand-over of a CCSD solve (``DressedDeviceIntegrals``, T2 a host array
        or a DeviceArray of that context).  ``t1`` [v,o]: the converged singles (the densities undo the T1 dressing);
        ``lam = (lambda1, lambda2)``: a Lambda solution the caller has (else solved here; ``eps`` / ``level_shift`` as
        ``Lambda_CCSD.solve``).  Returns the result dictionary (host arrays): "e" [k], "r1", "r2", "l1", "l2" (lists),
        "r0" [k], "tdm left", "tdm right" [k,n,n], "right residual", "left residual" [k], "biorthogonality", "iterations",
        "converged" (and "lambda1", "lambda2")."""
        print_title("EOM-CCSD transition solver", )
        t_start = time.time()
        from pymes_amd.integral.device import DressedDeviceIntegrals
        from pymes_amd.solver.ccd import quiet_collector
        if isinstance(V_dressed, DressedDeviceIntegrals):
            check_context(V_dressed.ctx, self.no)
        else:
            check_occupied(self.no)
        opener = lambda_ccsd.Lambda_CCSD(self.no, device=self.device)
        opener.algo_name = self.algo_name
        f, ctx, sig, own = opener._open(f_dressed, V_dressed, t2)
        collector = quiet_collector().__enter__()
        nr, no, nv = self.n_excit, self.no, ctx.nv
        try:
            if nr < 1 or nr > no * nv:
                raise ValueError("EOM_CCSD_Transitions: 1 <= n_excit <= %d (the number of singles)" % (no * nv))
            lay = self._layout(no, nv)
            n1, off2, nflat = lay
            part1 = lambda x: self._u1(ctx, x, lay)
            part2 = lambda x: self._u2(ctx, x, lay)

            def flat_apply(fn):
                def run(vecs):
                    outs = [self._zero_pad(ctx, ctx.empty((nflat,)), lay) for _ in vecs]
                    fn([part1(u) for u in vecs], [part2(u) for u in vecs], [True] * len(vecs),
                       out1=[part1(x) for x in outs], out2=[part2(x) for x in outs])
                    return outs
                return run
            right, left = flat_apply(sig.apply_many), flat_apply(sig.apply_left_many)
            d = ctx.zeros((nflat,))
            ctx.lib.call("pymes_eom_diagonals", ctx.handle, _lib.host_ptr(np.ascontiguousarray(f)), C.c_void_p(sig.T.ptr),
                         int(sig.dressed), C.c_void_p(d.ptr), C.c_void_p(d.ptr + 8 * off2))
            d1 = part1(d).get().ravel()
            start = []
            for p in np.argsort(d1, kind="stable")[:nr]:
                vec = ctx.zeros((nflat,))
                one = np.zeros(n1)
                one[p] = 1.0
                part1(vec).set(one.reshape(nv, no))
                start.append(vec)
            # ---- right vectors, unit norm, ascending ---------------------------------------------------------------------------
            w, rz, _, it_r = self._davidson(ctx, lay, right, d, start, None, "right")
            order = np.argsort(w, kind="stable")
            w, rz = w[order], [rz[n] for n in order]
            nrm = np.sqrt(np.diag(ctx.gram(rz, rz)))
            for n in range(nr):
                ctx.lincomb_multi([rz[n]], [], np.zeros((0, 1)), beta=[1.0 / nrm[n]])
            # ---- Lambda, on the same handle ---------------------------------------------------------------------------------------
            if lam is None:
                solver = lambda_ccsd.Lambda_CCSD(no, r_epsilon=self.lambda_r_epsilon or self.r_epsilon, device=self.device)
                out = solver.solve(f, V_dressed, t2, eps=eps, level_shift=level_shift, handle=(ctx, sig))
                solver.t2 = None
                self.lambda_solver = solver
                lam, lam_ok = (out["lambda1"], out["lambda2"]), bool(out["converged"])
            else:
                lam, lam_ok = (np.asarray(lam[0], dtype=np.float64), np.asarray(lam[1], dtype=np.float64)), True
            # ---- left vectors: from the right ones, the Ritz pair nearest each w_k ----------------------------------------------
            start = [ctx.empty((nflat,)).copy_from(x) for x in rz]
            _, lz, _, it_l = self._davidson(ctx, lay, left, d, start, w, "left")
            G = ctx.gram(lz, rz)                                            # G_jk = <l_j, r_k>
            with _single_threaded_blas():
                Gi = np.linalg.inv(G)
            ln = [ctx.empty((nflat,)) for _ in range(nr)]
            ctx.lincomb_multi(ln, lz, Gi.T)                                 # l_j <- sum_m (G^-1)_jm l_m
            lz = ln
            # ---- certificates from one fresh stacked build per side -----------------------------------------------------------------
            scratch = [ctx.empty((nflat,)) for _ in range(nr)]
            res_r, nrm_r = self._correction(ctx, lay, right(rz), rz, w, d, scratch)
            res_l, nrm_l = self._correction(ctx, lay, left(lz), lz, w, d, scratch)
            rel_r, rel_l = np.sqrt(res_r / nrm_r), np.sqrt(res_l / nrm_l)
            bio = float(np.abs(ctx.gram(lz, rz) - np.eye(nr)).max())
            # ---- densities -------------------------------------------------------------------------------------------------------------
            t1d = t1 if isinstance(t1, DeviceArray) and t1.ctx is ctx else ctx.array(
                np.ascontiguousarray(t1.get() if isinstance(t1, DeviceArray) else t1, dtype=np.float64))
            gl, gr, r0 = device_tdm1(ctx, t1d, sig.T, ctx.array(lam[0]), ctx.array(lam[1]), [part1(x) for x in lz],
                                     [part2(x) for x in lz], [part1(x) for x in rz], [part2(x) for x in rz])
            self.result = {"e": w.copy(), "r1": [part1(x).get() for x in rz], "r2": [part2(x).get() for x in rz],
                           "l1": [part1(x).get() for x in lz], "l2": [part2(x).get() for x in lz], "r0": r0,
                           "tdm left": gl, "tdm right": gr, "right residual": rel_r, "left residual": rel_l,
                           "biorthogonality": bio, "iterations": {"right": it_r, "left": it_l},
                           "converged": bool(lam_ok and np.all(rel_r < self.r_epsilon) and np.all(rel_l < self.r_epsilon)),
                           "lambda1": lam[0], "lambda2": lam[1]}
            print_logging_info("EOM-CCSD transitions finished in {:.3f} seconds".format(time.time() - t_start), level=1)
            return self.result
        finally:
            collector.__exit__()
            sig.close()
            if own:
                ctx.close()
            elif ctx.handle is not None:
                ctx.trim()

    # ---- D3 -----------------------------------------------------------------------------------------------------------------------------
    def strengths(self, O):
        """S_k(O) = (sum gammaL_k O) (sum gammaR_k O) of the last solve for a one-body operator O [n,n] (the basis of f)."""
        if self.result is None:
            raise RuntimeError("strengths: needs a finished solve()")
        O = np.asarray(O, dtype=np.float64)
        gl, gr = self.result["tdm left"], self.result["tdm right"]
        if O.shape != gl.shape[1:]:
            raise ValueError("strengths: O must be [n, n] = %s" % (gl.shape[1:],))
        return np.einsum("kpq,pq->k", gl, O) * np.einsum("kpq,pq->k", gr, O)

    def oscillator_strengths(self, mu):
        """(2/3) w_k sum_x S_k(mu_x) for the three dipole components mu [3,n,n]."""
        mu = np.asarray(mu, dtype=np.float64)
        if mu.ndim != 3 or mu.shape[0] != 3:
            raise ValueError("oscillator_strengths: mu must be [3, n, n]")
        return (2.0 / 3.0) * self.result["e"] * sum(self.strengths(mu[x]) for x in range(3))
