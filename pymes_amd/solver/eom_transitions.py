"""Left EOM-CCSD eigenvectors, transition densities and strengths on the MI355X engine.

``EOM_CCSD_Transitions(no, n_excit).solve(f_dressed, dict_or_DressedDeviceIntegrals, t2, t1, lam=None)`` solves, on ONE hoisted
sigma handle (csrc/eom.cpp, ``EomSigma``), the right problem ``A r_k = w_k r_k``, the Lambda equations ``A^T lambda + eta = 0``
(unless ``lam`` is given) and the left problem ``A^T l_k = w_k l_k``, normalises ``<l_j, r_k> = delta_jk`` with the inverse of
the k x k overlap matrix, and assembles the two transition densities of every root on the device (``pymes_tdm1``; definitions
and written-out formulas in include/pymes_amd.h):

  gammaL_k = d/df ( <l1_k, R1(f)> + <l2_k, R2(f)> ),   gammaR_k = d/df <0|(1 + Lambda) f~ (r0_k + R_k)|0>,   r0_k = -<lambda, r_k>,
  S_k(O) = (sum gammaL_k O) (sum gammaR_k O),   oscillator strength (2/3) w_k sum_x S_k(mu_x).

Both eigenproblems run through the block Davidson of ``subspace.py`` on flat vectors [x1 | zero pad | x2] (``FlatLayout``):
sigma of the NEW vectors of a pass in one stacked library call (``pymes_eom_sigma_apply`` /
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
from pymes_amd.solver import lambda_ccsd, subspace

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
    lambda_ccsd.check_occupied(no, "EOM_CCSD_Transitions")


def device_tdm1(ctx, t1, t2, lam1, lam2, l1s, l2s, r1s, r2s):
    """(gammaL [k,n,n], gammaR [k,n,n], r0 [k]) as host arrays (``pymes_tdm1``); every input a device array of ctx."""
    k, n = len(l1s), ctx.n
    gl, gr, r0 = np.zeros((k, n, n)), np.zeros((k, n, n)), np.zeros(k)
    ctx.lib.call("pymes_tdm1", ctx.handle, C.c_void_p(t1.ptr), C.c_void_p(t2.ptr), C.c_void_p(lam1.ptr), C.c_void_p(lam2.ptr), k,
                 _lib.ptr_array([x.ptr for x in l1s]), _lib.ptr_array([x.ptr for x in l2s]), _lib.ptr_array([x.ptr for x in r1s]),
                 _lib.ptr_array([x.ptr for x in r2s]), _lib.host_ptr(gl), _lib.host_ptr(gr), _lib.host_ptr(r0))
    return gl, gr, r0


class EOM_CCSD_Transitions:
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
        f, ctx, sig, own = subspace.open_handle(self.no, self.device, f_dressed, V_dressed, t2, self.BLOCKS, lambda_ccsd.LeftSigma,
                                                self.algo_name)
        collector = quiet_collector().__enter__()
        nr, no, nv = self.n_excit, self.no, ctx.nv
        try:
            if nr < 1 or nr > no * nv:
                raise ValueError("EOM_CCSD_Transitions: 1 <= n_excit <= %d (the number of singles)" % (no * nv))
            lay = subspace.FlatLayout(ctx, (nv, no), (nv, nv, no, no))
            part1, part2, off2 = lay.part1, lay.part2, lay.off2
            right = lambda vecs: subspace.apply_flat(lay, sig.apply_many, vecs, [True] * len(vecs))
            left = lambda vecs: subspace.apply_flat(lay, sig.apply_left_many, vecs, [True] * len(vecs))
            d = ctx.zeros((lay.nflat,))
            ctx.lib.call("pymes_eom_diagonals", ctx.handle, _lib.host_ptr(np.ascontiguousarray(f)), C.c_void_p(sig.T.ptr),
                         int(sig.dressed), C.c_void_p(d.ptr), C.c_void_p(d.ptr + 8 * off2))
            d1 = part1(d).get().ravel()
            start = [lay.unit(p) for p in np.argsort(d1, kind="stable")[:nr]]

            def correction(ss, rs, w, d, shift, qs):
                return subspace.correction(ctx.lib, "pymes_eom_correction", ctx.handle, lay, ss, rs, w, d, shift, qs)

            def davidson(apply, start, targets, side):
                """(w, Ritz vectors, passes): a root whose Ritz value keeps an imaginary part is refused by name.  (As before the
                move, a run that ends without converging — no new direction left included — reports max_iter passes.)"""
                dav = subspace.block_davidson(ctx, lay, apply, correction, d, start, nr, self.max_dim, self.max_iter, self.r_epsilon,
                                              self.shift, targets=targets, label=side,
                                              refuse_complex="EOM_CCSD_Transitions: root %d of the " + side + " problem")
                return dav.w, dav.rz, dav.passes if dav.converged else self.max_iter
            # ---- right vectors, unit norm, ascending ---------------------------------------------------------------------------
            w, rz, it_r = davidson(right, start, None, "right")
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
            start = [lay.empty().copy_from(x) for x in rz]
            _, lz, it_l = davidson(left, start, w, "left")
            G = ctx.gram(lz, rz)                                            # G_jk = <l_j, r_k>
            with _single_threaded_blas():
                Gi = np.linalg.inv(G)
            ln = [lay.empty() for _ in range(nr)]
            ctx.lincomb_multi(ln, lz, Gi.T)                                 # l_j <- sum_m (G^-1)_jm l_m
            lz = ln
            # ---- certificates from one fresh stacked build per side -----------------------------------------------------------------
            scratch = [lay.empty() for _ in range(nr)]
            res_r, nrm_r = correction(right(rz), rz, w, d, self.shift, scratch)
            res_l, nrm_l = correction(left(lz), lz, w, d, self.shift, scratch)
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
