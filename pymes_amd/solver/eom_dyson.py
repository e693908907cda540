"""Left IP / EA-EOM-CCSD eigenvectors, Dyson amplitudes and pole strengths on the MI355X engine.

``IP_EOM_CCSD_Dyson(no, n_roots).solve(f_dressed, dict_or_DressedDeviceIntegrals, t2, t1, lam=None)`` (``EA_EOM_CCSD_Dyson``
likewise) solves, on ONE hoisted sigma handle (csrc/eom.cpp, ``IpEaSigma``), the right problem ``H r_k = w_k r_k`` and the left
problem ``H^T l_k = w_k l_k`` of the IP / EA operator, normalises ``<l_j, r_k> = delta_jk`` with the inverse of the k x k overlap
matrix, and assembles the Dyson amplitudes of every root on the device (``pymes_ipea_dyson``; definitions and written-out formulas
in include/pymes_amd.h):

  psiL_k(p) = <l_k, b_p>,  psiR_k(q) = <e_q, r_k>,  residue Z_k[q,p] = psiR_k(q) psiL_k(p),  pole strength P_k = sum_p psiR_k(p) psiL_k(p),
  A_pq(w) = (1/pi) sum_k Z_k[p,q] eta / ((w - eps_k)^2 + eta^2),  eps_k = -w_k (IP), +w_k (EA).

The right amplitudes need the solution of the Lambda equations: ``lam = (lambda1, lambda2)`` if the caller has it, else it is solved
here on an EE sigma handle of the same context (``Lambda_CCSD``; the context then also needs the ten blocks of that build).  Both
eigenproblems run through the block Davidson of ``subspace.py`` on flat vectors [x1 | zero pad | x2]: the right run starts from unit
vectors on the smallest singles diagonals and takes the lowest roots; the left run starts from the right vectors, takes the Ritz pair
nearest each w_k and measures its residual with w_k itself.  Nothing is assumed hermitian; a root whose Ritz value keeps an imaginary
part is refused by name.
"""
import time

import numpy as np

from pymes_amd.device import DeviceArray, PymesError
from pymes_amd.log import print_logging_info, print_title
from pymes_amd.mixer.diis import _single_threaded_blas
from pymes_amd.solver import lambda_ccsd, subspace
from pymes_amd.solver.eom_ip_ea import KIND_EA, KIND_IP, IPEASigma


def residues(psi_left, psi_right):
    """Z_k[q,p] = psiR_k(q) psiL_k(p), [k,n,n]."""
    return np.einsum("kq,kp->kqp", np.asarray(psi_right, dtype=np.float64), np.asarray(psi_left, dtype=np.float64))


def pole_strengths(psi_left, psi_right):
    return (np.asarray(psi_left, dtype=np.float64) * np.asarray(psi_right, dtype=np.float64)).sum(axis=1)


class _IPEA_Dyson:
    KIND = None
    NAME = None

    def __init__(self, no, n_roots=3, r_epsilon=1.e-8, max_iter=200, device=0):
        self.algo_name = self.NAME
        self.no = no
        self.n_roots = int(n_roots)
        self.r_epsilon = float(r_epsilon)
        self.max_iter = int(max_iter)
        self.device = device
        self.max_dim = 8 * self.n_roots
        self.shift = 1.e-5
        self.lambda_r_epsilon = None                  # (default: r_epsilon)
        self.result = None
        self.lambda_solver = None

    # the dressed blocks the solve reads: those of the sigma build, and those of the Lambda solve when no ``lam`` is given
    BLOCKS = None

    @classmethod
    def blocks(cls, with_lambda):
        if not with_lambda:
            return cls.BLOCKS
        return cls.BLOCKS + tuple(b for b in lambda_ccsd.Lambda_CCSD.BLOCKS if b not in cls.BLOCKS)

    def check_context(self, ctx, have_lambda):
        """The refusals that need no allocation: integral sharding (EA always: the operator reads the whole V_abcd; IP without
        ``lam``: the Lambda equations do), a launch graph being recorded."""
        if getattr(ctx, "shard", None) is not None:
            if self.KIND == KIND_EA:
                raise PymesError("%s: not available with integral sharding (shard=%s): the operator reads the whole V_abcd"
                                 % (self.NAME, ctx.shard))
            if not have_lambda:
                raise PymesError("%s: with integral sharding (shard=%s) pass lam=(lambda1, lambda2): the Lambda equations read "
                                 "the whole V_abcd" % (self.NAME, ctx.shard))
        if getattr(ctx, "recording", False):
            raise PymesError("%s: the context is recording a launch graph" % self.NAME)

    def solve(self, f_dressed, V_dressed, t2, t1, lam=None, eps=None, level_shift=0.0):
        """Call forms as ``IP_EOM_CCSD.solve``: (dressed Fock matrix, dictionary of dressed host blocks, host T2) — a context is
        built and dies with the call — or the device hand-over of a CCSD solve (``DressedDeviceIntegrals``, T2 a host array or
        a DeviceArray of that context).  ``t1`` [v,o]: the converged singles (the amplitudes undo the T1 dressing);
        ``lam = (lambda1, lambda2)``: a Lambda solution the caller has (else solved here; ``eps`` / ``level_shift`` as
        ``Lambda_CCSD.solve``).  Returns the result dictionary (host arrays): "e" [k], "r1", "r2", "l1", "l2" (lists),
        "dyson left", "dyson right" [k,n], "pole strengths" [k], "right residual", "left residual" [k], "biorthogonality",
        "iterations", "converged" (and "lambda1", "lambda2")."""
        print_title(self.NAME + " solver", )
        t_start = time.time()
        from pymes_amd.integral.device import DressedDeviceIntegrals
        from pymes_amd.solver.ccd import quiet_collector
        if lam is None:                        # Lambda is solved here: its cap on nocc, before a context or a handle exists
            lambda_ccsd.check_occupied(self.no, self.NAME)
        if isinstance(V_dressed, DressedDeviceIntegrals):
            self.check_context(V_dressed.ctx, lam is not None)
        make = lambda ctx, f, t2, dressed: IPEASigma(ctx, self.KIND, f, t2, dressed)
        f, ctx, sig, own = subspace.open_handle(self.no, self.device, f_dressed, V_dressed, t2, self.blocks(lam is None), make,
                                                self.NAME)
        collector = quiet_collector().__enter__()
        nr = self.n_roots
        ee = None
        try:
            if nr < 1 or nr > sig.n1:
                raise ValueError("%s: 1 <= n_roots <= %d (the number of singles)" % (self.NAME, sig.n1))
            lay = sig.layout
            part1, part2 = lay.part1, lay.part2
            right = lambda vecs: subspace.apply_flat(lay, sig.apply_many, vecs)
            left = lambda vecs: subspace.apply_flat(lay, sig.apply_left_many, vecs)
            d = sig.diagonals()
            d1 = part1(d).get().ravel()
            start = [lay.unit(p) for p in np.argsort(d1, kind="stable")[:nr]]

            def davidson(apply, start, targets, side):
                dav = subspace.block_davidson(ctx, lay, apply, sig.correction, d, start, nr, self.max_dim, self.max_iter,
                                              self.r_epsilon, self.shift, targets=targets, label=self.NAME + " " + side,
                                              refuse_complex=self.NAME + ": root %d of the " + side + " problem",
                                              on_null=subspace.DROP_NULL)
                return dav.w, dav.rz, dav.passes
            # ---- right vectors, unit norm, ascending ---------------------------------------------------------------------------
            w, rz, it_r = davidson(right, start, None, "right")
            order = np.argsort(w, kind="stable")
            w, rz = w[order], [rz[n] for n in order]
            nrm = np.sqrt(np.diag(ctx.gram(rz, rz)))
            for n in range(nr):
                ctx.lincomb_multi([rz[n]], [], np.zeros((0, 1)), beta=[1.0 / nrm[n]])
            # ---- Lambda, on an EE handle of the same context ---------------------------------------------------------------------
            if lam is None:
                ee = lambda_ccsd.LeftSigma(ctx, f, sig.T, sig.dressed)
                solver = lambda_ccsd.Lambda_CCSD(self.no, r_epsilon=self.lambda_r_epsilon or self.r_epsilon, device=self.device)
                out = solver.solve(f, V_dressed, t2, eps=eps, level_shift=level_shift, handle=(ctx, ee))
                solver.t2 = None
                self.lambda_solver = solver
                ee.close()
                ee = None
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
            res_r, nrm_r = sig.correction(right(rz), rz, w, d, self.shift, scratch)
            res_l, nrm_l = sig.correction(left(lz), lz, w, d, self.shift, scratch)
            rel_r, rel_l = np.sqrt(res_r / nrm_r), np.sqrt(res_l / nrm_l)
            bio = float(np.abs(ctx.gram(lz, rz) - np.eye(nr)).max())
            # ---- amplitudes ------------------------------------------------------------------------------------------------------------
            t1d = t1 if isinstance(t1, DeviceArray) and t1.ctx is ctx else ctx.array(
                np.ascontiguousarray(t1.get() if isinstance(t1, DeviceArray) else t1, dtype=np.float64))
            pl, pr = sig.dyson(t1d, ctx.array(np.ascontiguousarray(lam[0])), ctx.array(np.ascontiguousarray(lam[1])),
                               [part1(x) for x in lz], [part2(x) for x in lz], [part1(x) for x in rz], [part2(x) for x in rz])
            self.result = {"e": w.copy(), "r1": [part1(x).get() for x in rz], "r2": [part2(x).get() for x in rz],
                           "l1": [part1(x).get() for x in lz], "l2": [part2(x).get() for x in lz],
                           "dyson left": pl, "dyson right": pr, "pole strengths": pole_strengths(pl, pr),
                           "right residual": rel_r, "left residual": rel_l, "biorthogonality": bio,
                           "iterations": {"right": it_r, "left": it_l},
                           "converged": bool(lam_ok and np.all(rel_r < self.r_epsilon) and np.all(rel_l < self.r_epsilon)),
                           "lambda1": lam[0], "lambda2": lam[1]}
            print_logging_info("{} finished in {:.3f} seconds".format(self.NAME, time.time() - t_start), level=1)
            return self.result
        finally:
            collector.__exit__()
            if ee is not None:
                ee.close()
            sig.close()
            if own:
                ctx.close()
            elif ctx.handle is not None:
                ctx.trim()

    # ---- D3: host numpy on the [k,n] arrays ------------------------------------------------------------------------------------------
    def _amplitudes(self, who):
        if self.result is None:
            raise RuntimeError("%s: needs a finished solve()" % who)
        return self.result["dyson left"], self.result["dyson right"]

    def residues(self):
        """Z_k[q,p] = psiR_k(q) psiL_k(p) of the last solve, [k,n,n]."""
        return residues(*self._amplitudes("residues"))

    def spectral_function(self, omegas, eta):
        """A_pq(w) = (1/pi) sum_k Z_k[p,q] eta / ((w - eps_k)^2 + eta^2) over the roots of the last solve, [len(omegas),n,n];
        eps_k = -w_k for ionisation, +w_k for attachment."""
        Z = residues(*self._amplitudes("spectral_function"))
        om = np.asarray(omegas, dtype=np.float64).ravel()
        eta = float(eta)
        if not eta > 0.0:
            raise ValueError("spectral_function: eta must be positive")
        eps = -self.result["e"] if self.KIND == KIND_IP else self.result["e"]
        lor = eta / ((om[:, None] - eps[None, :]) ** 2 + eta ** 2) / np.pi
        return np.einsum("wk,kpq->wpq", lor, Z)


class IP_EOM_CCSD_Dyson(_IPEA_Dyson):
    """Ionisation: l1[i], l2[i,j,b]; poles at -w_k."""
    KIND, NAME = KIND_IP, "IP-EOM-CCSD Dyson"
    BLOCKS = IPEASigma.BLOCKS[KIND_IP]


class EA_EOM_CCSD_Dyson(_IPEA_Dyson):
    """Attachment: l1[a], l2[a,b,j]; poles at +w_k."""
    KIND, NAME = KIND_EA, "EA-EOM-CCSD Dyson"
    BLOCKS = IPEASigma.BLOCKS[KIND_EA]
