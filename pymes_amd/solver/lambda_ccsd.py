"""CCSD Lambda equations and the one-particle response density on the MI355X engine.

``Lambda_CCSD(no).solve(f_dressed, dict_or_DressedDeviceIntegrals, t2)`` solves ``A^T lambda + eta = 0`` for the left-hand
ground state of a converged CCSD solution: ``A`` is the EE-EOM-CCSD sigma (eom_ccsd.py:268-385), ``A^T`` its adjoint under the
plain inner product on the exchange-symmetric vectors, ``eta1[a,i] = 2 f~_ov[i,a]``, ``eta2[a,b,i,j] = 2 V_ijab[i,j,a,b] -
V_ijab[i,j,b,a]`` (formulas and caveats: include/pymes_amd.h, ``pymes_lambda_step``).  The adjoint build runs in
the engine on the handle of the sigma build (csrc/eom.cpp, ``EomSigma::apply_left``): the same hoisted V.T intermediates read
through transposed views.  The iteration is ``lambda <- lambda - (eta + A^T lambda) / d`` with the orbital-energy denominators
of the CCSD update and the device DIIS; one library call and one synchronisation (the residual norm) per iteration.

``rdm1(t1)`` is the one-particle response density ``gamma_pq = dL/df_pq`` of the CCSD Lagrangian plus 2 on the occupied diagonal
(its trace is the electron count), ``expectation(O)`` the correlation part ``sum gamma_pq O_pq`` of a one-body expectation value.
Nothing is assumed hermitian: for transcorrelated integrals the left state is not the transpose of the right one.

``rdm2(t1)`` is the two-particle response density ``Gamma_pqrs = (dL/dV_pqrs + dL/dV_qpsr) / 2`` block by block and
``expectation2(W)`` the two-body expectation value ``sum Gamma W`` — ``L(f, V) = sum gamma f + sum Gamma V`` for every V with
V_pqrs = V_qpsr (gamma: ``rdm1`` without the 2 on the occupied diagonal; no factor 1/2; formulas: include/pymes_amd.h,
``pymes_rdm2``).  ``full_rdm2`` assembles the spin-summed two-particle density matrix from them.
"""
import ctypes as C
import time

import numpy as np

from pymes_amd import _lib
from pymes_amd.device import Context, DeviceArray, PymesError
from pymes_amd.log import print_logging_info, print_title
from pymes_amd.mixer.diis import DIIS
from pymes_amd.solver.eom_ccsd import _Sigma
from pymes_amd.solver.subspace import open_handle


# The DIIS error vector is ERR_SCALE x the update: the mixer tests linear dependence of its subspace with an ABSOLUTE 1e-12 on the
# overlaps (the reference's bookkeeping, mixer/diis.py), which plain updates pass below a residual of 1e-6 — the extrapolation
# then degenerates and the iteration creeps.  A fixed factor leaves the coefficients unchanged and moves that point to 1e-11.
ERR_SCALE = 1.0e5


NOCC_MAX = 88          # PYMES_NOCC_MAX_LAMBDA (include/pymes_amd.h): o (o + 1) + 256 doubles of LDS in 64 KB


def check_occupied(no, name="Lambda_CCSD"):
    """The left assembly stages an o x (o + 1) tile and 256 partial sums in LDS: refused here, before a context, a handle or a
    vector exists (the library refuses the same shapes at the head of ``pymes_eom_sigma_apply_left`` / ``pymes_lambda_step``)."""
    if no > NOCC_MAX:
        raise PymesError("%s: nocc = %d is too large for the LDS tile of lambda_assemble (o (o + 1) + 256 doubles in 64 KB: "
                         "nocc <= %d)" % (name, no, NOCC_MAX))


def check_context(ctx):
    """The adjoint build reads the whole V_abcd: a context that shards its integrals is refused, by the name of the mode."""
    if getattr(ctx, "shard", None) is not None:
        raise PymesError("Lambda_CCSD: not available with integral sharding (shard=%s): the left sigma reads the whole V_abcd"
                         % (ctx.shard,))


class LeftSigma(_Sigma):
    """The handle of the sigma build with its adjoint (``pymes_eom_sigma_apply_left``) and the Lambda step on it."""

    def apply_left_many(self, l1s, l2s, syms=None, out1=None, out2=None):
        """[(A^T l)_1, (A^T l)_2] for the left vectors (l1s[z], l2s[z]), device arrays; l2 must be exchange-symmetric."""
        return self._apply("pymes_eom_sigma_apply_left", l1s, l2s, syms, out1, out2)

    def apply_left(self, l1, l2, l2_sym=None):
        return self.apply_left_many([l1], [l2], None if l2_sym is None else [l2_sym])[0]

    def lambda_step(self, lam, eps_o, eps_v, shift, out, err, start=False, sym=False, err_scale=1.0):
        """One iteration (``pymes_lambda_step``): out = lam - (eta + A^T lam) / d, err = err_scale (out - lam); returns
        |eta + A^T lam|."""
        eo = np.ascontiguousarray(eps_o, dtype=np.float64)
        ev = np.ascontiguousarray(eps_v, dtype=np.float64)
        if eo.shape != (self.no,) or ev.shape != (self.nv,):
            raise ValueError("lambda_step: eps_o / eps_v must be [no] / [nv]")
        norm = np.zeros(1)
        l1, l2 = (None, None) if start else (C.c_void_p(lam[0].ptr), C.c_void_p(lam[1].ptr))
        self.ctx.lib.call("pymes_lambda_step", self._handle(), l1, l2, _lib.host_ptr(eo), _lib.host_ptr(ev), float(shift),
                          float(err_scale), int(bool(start)), int(bool(sym)), C.c_void_p(out[0].ptr), C.c_void_p(out[1].ptr),
                          C.c_void_p(err[0].ptr), C.c_void_p(err[1].ptr), _lib.host_ptr(norm))
        return float(norm[0])


def device_rdm1(ctx, t1, t2, lam1, lam2, ref=2.0):
    """gamma + ref on the occupied diagonal as a host [n,n] array (``pymes_rdm1``); all four inputs device arrays of ctx."""
    out = np.zeros((ctx.n, ctx.n))
    ctx.lib.call("pymes_rdm1", ctx.handle, C.c_void_p(t1.ptr), C.c_void_p(t2.ptr), C.c_void_p(lam1.ptr), C.c_void_p(lam2.ptr),
                 float(ref), _lib.host_ptr(out))
    return out


# ---- the two-particle density (include/pymes_amd.h, pymes_rdm2) ------------------------------------------------------
RDM2_NAMES = ("klij", "ijka", "ijak", "ijab", "iajk", "iajb", "iabj", "iabc", "aijk", "aijb", "aibj", "aibc", "abij", "abic", "abci",
              "abcd")                                  # by pattern number: 8 p + 4 q + 2 r + s, 1 for a virtual position
# A block and its image under (pq,rs) -> (qp,sr) hold the same numbers: the library stores one of each pair
RDM2_IMAGE = {"ijak": "ijka", "aijk": "iajk", "aibj": "iajb", "aijb": "iabj", "aibc": "iabc", "abci": "abic"}
RDM2_STORED = tuple(nm for nm in RDM2_NAMES if nm not in RDM2_IMAGE)


def _rdm2_names(blocks):
    """The block names of a request, checked; default: all blocks except abcd."""
    names = tuple(nm for nm in RDM2_NAMES if nm != "abcd") if blocks is None else tuple(blocks)
    for nm in names:
        if nm not in RDM2_NAMES:
            raise ValueError("rdm2: unknown block %r (the sixteen names of split_blocks: %s)" % (nm, ", ".join(RDM2_NAMES)))
    if not names:
        raise ValueError("rdm2: no block requested")
    return names


def device_rdm2(ctx, t1, t2, lam1, lam2, blocks=None, out=None):
    """The blocks of Gamma as device arrays (``pymes_rdm2``): a dictionary over the STORED names among ``blocks`` (default: all
    but abcd) and the stored images of the others (RDM2_IMAGE: Gamma_aibc[a,i,b,c] = Gamma_iabc[i,a,c,b], ...).  All four inputs
    device arrays of ctx; ``out``: a dictionary of device arrays to write into (default: new ones)."""
    check_occupied(ctx.no, "rdm2")
    stored = []
    for nm in _rdm2_names(blocks):
        nm = RDM2_IMAGE.get(nm, nm)
        if nm not in stored:
            stored.append(nm)
    res = {nm: (out[nm] if out is not None and nm in out else ctx.empty(ctx.block_shape(nm))) for nm in stored}
    ptrs = (C.c_void_p * 16)()
    mask = 0
    for nm, arr in res.items():
        if tuple(arr.shape) != ctx.block_shape(nm):
            raise ValueError("rdm2: the output for block %r must have shape %s" % (nm, ctx.block_shape(nm)))
        k = RDM2_NAMES.index(nm)
        ptrs[k] = arr.ptr
        mask |= 1 << k
    ctx.lib.call("pymes_rdm2", ctx.handle, C.c_void_p(t1.ptr), C.c_void_p(t2.ptr), C.c_void_p(lam1.ptr), C.c_void_p(lam2.ptr),
                 mask, ptrs)
    return res


def device_expectation2(ctx, t1, t2, lam1, lam2):
    """sum Gamma_pqrs W_pqrs for the operator W held as the undressed blocks of ctx (``pymes_rdm2_expectation``); the abcd
    density is never built."""
    check_occupied(ctx.no, "expectation2")
    val = np.zeros(1)
    ctx.lib.call("pymes_rdm2_expectation", ctx.handle, C.c_void_p(t1.ptr), C.c_void_p(t2.ptr), C.c_void_p(lam1.ptr),
                 C.c_void_p(lam2.ptr), _lib.host_ptr(val))
    return float(val[0])


def full_rdm2(no, gamma, Gamma_blocks):
    """The spin-summed two-particle density matrix [n,n,n,n] of E = sum h D1 + 1/2 sum V D with f = h + sum_i (2 V_piqi - V_piiq):
    D = D_HF + 2 (gamma_pr n_qs + n_pr gamma_qs) - (gamma_ps n_qr + n_ps gamma_qr) + 2 Gamma, D_HF = 4 n_pr n_qs - 2 n_ps n_qr, n
    the unit matrix on the occupied block.  ``gamma``: the response density [n,n] WITHOUT the reference term (``rdm1`` minus 2
    on the occupied diagonal); ``Gamma_blocks``: a complete dictionary of the sixteen blocks (``rdm2`` with every name)."""
    g = np.asarray(gamma, dtype=np.float64)
    m = g.shape[0]
    missing = [nm for nm in RDM2_NAMES if nm not in Gamma_blocks]
    if missing:
        raise ValueError("full_rdm2: needs all sixteen blocks; missing %s" % ", ".join(missing))
    nocc = np.zeros((m, m))
    nocc[np.arange(no), np.arange(no)] = 1.0
    D = 4.0 * np.einsum("pr,qs->pqrs", nocc, nocc) - 2.0 * np.einsum("ps,qr->pqrs", nocc, nocc)
    D += 2.0 * (np.einsum("pr,qs->pqrs", g, nocc) + np.einsum("pr,qs->pqrs", nocc, g))
    D -= np.einsum("ps,qr->pqrs", g, nocc) + np.einsum("ps,qr->pqrs", nocc, g)
    sl = {"o": slice(0, no), "v": slice(no, None)}
    for nm in RDM2_NAMES:
        D[tuple(sl["v" if ch in "abcd" else "o"] for ch in nm)] += 2.0 * np.asarray(Gamma_blocks[nm])
    return D


class Lambda_CCSD:
    BLOCKS = _Sigma.BLOCKS

    def __init__(self, no, r_epsilon=1.e-8, max_iter=100, device=0, diis_dim=6):
        self.algo_name = "Lambda-CCSD"
        self.no = no
        self.r_epsilon = float(r_epsilon)
        self.max_iter = int(max_iter)
        self.device = device
        self.diis_dim = int(diis_dim)
        self.lambda1 = self.lambda2 = self.t2 = None
        self.residual_norm, self.iterations, self.converged, self.history = np.inf, 0, False, []

    def apply_left(self, f_dressed, V_dressed, t2, l1, l2):
        """One adjoint build for host arrays: ((A^T l)_1, (A^T l)_2)."""
        check_occupied(self.no)
        _, ctx, sig, own = open_handle(self.no, self.device, f_dressed, V_dressed, t2, self.BLOCKS, LeftSigma, self.algo_name,
                                       check_context)
        try:
            o1, o2 = sig.apply_left(ctx.array(np.asarray(l1, dtype=np.float64)), ctx.array(np.asarray(l2, dtype=np.float64)))
            return o1.get(), o2.get()
        finally:
            sig.close()
            if own:
                ctx.close()

    def solve(self, f_dressed, V_dressed, t2, eps=None, level_shift=0.0, handle=None):
        """Solve the Lambda equations.  Call forms as ``EOM_CCSD.solve``: (dressed Fock matrix, dictionary of dressed host
        blocks, host T2) — a context is built and dies with the call — or the device-resident hand-over of a CCSD solve
        (``DressedDeviceIntegrals``, T2 a host array or a DeviceArray of the same context).  ``eps = (eps_o, eps_v)`` and
        ``level_shift`` are the orbital energies and the shift of the denominators (default: the diagonal of the dressed
        Fock matrix, no shift; ``CCSD.solve(density=True)`` passes those of its own update).  Returns a dictionary with
        "lambda1" [v,o], "lambda2" [v,v,o,o] (host), "residual norm" (|eta + A^T lambda|), "iterations", "converged".
        ``handle = (ctx, LeftSigma)``: iterate on a handle the caller has hoisted from the same (f, V, t2) and keeps (the
        transition solver: one hoist for the right, the Lambda and the left solve); it is not closed here."""
        check_occupied(self.no)
        print_title("Lambda-CCSD Solver", )
        t_init = time.time()
        if handle is None:
            f, ctx, sig, own = open_handle(self.no, self.device, f_dressed, V_dressed, t2, self.BLOCKS, LeftSigma, self.algo_name,
                                           check_context)
        else:
            f, (ctx, sig), own = np.asarray(f_dressed, dtype=np.float64), handle, False
        no, nv = self.no, ctx.nv
        eps_o, eps_v = (f.diagonal()[:no].copy(), f.diagonal()[no:].copy()) if eps is None else eps
        mixer = DIIS(dim_space=self.diis_dim)
        s1, s2 = (nv, no), (nv, nv, no, no)
        new = lambda: (ctx.pool_get(s1), ctx.pool_get(s2))
        self.history, self.converged = [], False
        held = []
        try:
            lam, err = new(), new()
            sig.lambda_step(None, eps_o, eps_v, level_shift, lam, err, start=True)          # lambda = -eta / d
            for arr in err:
                ctx.pool_put(arr)
            norm, it = np.inf, 0
            for it in range(1, self.max_iter + 1):
                out, err = new(), new()
                norm = sig.lambda_step(lam, eps_o, eps_v, level_shift, out, err, sym=True, err_scale=ERR_SCALE)
                self.history.append(norm)
                print_logging_info("Iteration = ", it, level=1)
                print_logging_info("Norm Residual = {:.6e}".format(norm), level=2)
                if not np.isfinite(norm):
                    raise np.linalg.LinAlgError("Lambda-CCSD: the residual norm is not finite")
                self.converged = norm < self.r_epsilon
                if self.converged or it == self.max_iter:
                    # the norm is that of `lam`, which therefore is what is returned — converged or not
                    for arr in out + err:
                        ctx.pool_put(arr)
                    break
                if len(mixer.error_list) == mixer.dim_space:
                    # a full subspace is dropped, not shifted: the mixer reproduces the reference's bookkeeping, whose shifted
                    # copy of the overlap matrix leaves out the second-newest vector (mixer/diis.py) and stalls this iteration
                    mixer.restart(release=ctx.pool_put)
                mixed = mixer.mix(list(err), list(out), release=ctx.pool_put, on_device=True)
                for arr in lam:                          # (the history keeps `out` and `err`, never the extrapolated vector)
                    ctx.pool_put(arr)
                lam = tuple(mixed)
            self.iterations, self.residual_norm = it, norm
            self.lambda1, self.lambda2 = lam[0].get(), lam[1].get()
            held = list(lam)
            self.t2 = sig.T.get() if own else sig.T
            if not self.converged:
                print_logging_info("A converged solution is not found!", level=1)
            print_logging_info("{:.3f} seconds spent on Lambda-CCSD".format(time.time() - t_init), level=1)
            return {"lambda1": self.lambda1, "lambda2": self.lambda2, "residual norm": norm, "iterations": it,
                    "converged": self.converged}
        finally:
            alive = not own and ctx.handle is not None
            mixer.restart(release=ctx.pool_put if alive else None)
            if handle is None:
                sig.close()
            if own:
                ctx.close()
            elif alive:
                for arr in held:
                    ctx.pool_put(arr)

    def rdm1(self, t1, ctx=None):
        """The one-particle density [n,n] (occupied orbitals first) of the last solve: the response density plus 2 on the
        occupied diagonal.  Not symmetric, and not symmetrised.  ``ctx``: a live context to run on (default: a small one of
        its own; the density reads no integrals)."""
        if self.lambda1 is None:
            raise RuntimeError("rdm1: needs a finished solve()")
        if self.t2 is None:
            raise RuntimeError("rdm1: the amplitudes of the solve are no longer held (CCSD.solve(density=True) returns \"rdm1\")")
        if ctx is None and isinstance(self.t2, DeviceArray) and self.t2.ctx.handle is not None:
            ctx = self.t2.ctx
        own = ctx is None
        if own:
            ctx = Context(self.no, self.lambda1.shape[0], device=self.device)

        def on_ctx(x):
            if isinstance(x, DeviceArray):
                return x if x.ctx is ctx else ctx.array(x.get())
            return ctx.array(np.ascontiguousarray(x, dtype=np.float64))
        try:
            g = device_rdm1(ctx, on_ctx(t1), on_ctx(self.t2), on_ctx(self.lambda1), on_ctx(self.lambda2))
        finally:
            if own:
                ctx.close()
        self.gamma = g
        return g

    def _on_context(self, what, ctx):
        """(ctx, own, on_ctx): the context a density call runs on and the function that brings an operand onto it."""
        if self.lambda1 is None:
            raise RuntimeError("%s: needs a finished solve()" % what)
        if self.t2 is None:
            raise RuntimeError("%s: the amplitudes of the solve are no longer held (CCSD.solve(density=True, rdm2=True) returns "
                               "\"rdm2 blocks\")" % what)
        if ctx is None and isinstance(self.t2, DeviceArray) and self.t2.ctx.handle is not None:
            ctx = self.t2.ctx
        own = ctx is None
        if own:
            ctx = Context(self.no, self.lambda1.shape[0], device=self.device)

        def on_ctx(x):
            if isinstance(x, DeviceArray):
                return x if x.ctx is ctx else ctx.array(x.get())
            return ctx.array(np.ascontiguousarray(x, dtype=np.float64))
        return ctx, own, on_ctx

    def rdm2(self, t1, blocks=None, ctx=None):
        """The blocks of the two-particle response density Gamma of the last solve as a dictionary of host arrays, names and
        shapes as ``split_blocks``.  ``blocks``: the names wanted (default: all except abcd, which is v^4 and returned only when
        named).  Not hermitian, and not symmetrised.  ``ctx``: a live context to run on (default: a small one of its own; the
        density reads no integrals)."""
        names = _rdm2_names(blocks)
        check_occupied(self.no, "rdm2")
        ctx, own, on_ctx = self._on_context("rdm2", ctx)
        try:
            dev = device_rdm2(ctx, on_ctx(t1), on_ctx(self.t2), on_ctx(self.lambda1), on_ctx(self.lambda2), names)
            host = {nm: arr.get() for nm, arr in dev.items()}
            for arr in dev.values():
                arr.free()
        finally:
            if own:
                ctx.close()
        return {nm: (np.ascontiguousarray(host[RDM2_IMAGE[nm]].transpose(1, 0, 3, 2)) if nm in RDM2_IMAGE else host[nm])
                for nm in names}

    def expectation2(self, W, O=None, t1=None):
        """sum Gamma_pqrs W_pqrs (+ sum gamma_pq O_pq): the correlation part of the expectation value of the two-body operator W
        (and the one-body operator O) in the orbital basis of the solve.  ``W``: a host [n,n,n,n] array, a dictionary of its
        sixteen blocks or a ``DeviceIntegrals`` of the same shape; it must have W_pqrs = W_qpsr (tested once, refused by name
        otherwise).  The contraction runs on the device, block by block; the abcd density is never built.  ``t1``: the singles of
        the solve (needed unless ``rdm1(t1)`` / ``rdm2(t1)`` / a call with ``t1`` went before)."""
        from pymes_amd.integral.device import DeviceIntegrals
        if t1 is not None:
            self.t1 = t1
        if getattr(self, "t1", None) is None:
            raise RuntimeError("expectation2: pass t1 (the singles amplitudes of the solve)")
        check_occupied(self.no, "expectation2")
        nv = self.lambda1.shape[0] if self.lambda1 is not None else 0
        m = self.no + nv
        own = not isinstance(W, DeviceIntegrals)
        if own:
            if self.lambda1 is None:
                raise RuntimeError("expectation2: needs a finished solve()")
            wctx = Context(self.no, nv, device=self.device)
        else:
            wctx = W.ctx
        try:
            if not own:
                if tuple(W.shape) != (m,) * 4:
                    raise ValueError("expectation2: W must have shape %s" % ((m,) * 4,))
            elif isinstance(W, dict):
                missing = [nm for nm in RDM2_NAMES if nm not in W]
                if missing:
                    raise ValueError("expectation2: W needs all sixteen blocks; missing %s" % ", ".join(missing))
                for nm in RDM2_NAMES:
                    wctx.set_V_block(nm, np.ascontiguousarray(W[nm], dtype=np.float64))
            else:
                W = np.asarray(W, dtype=np.float64)
                if W.shape != (m,) * 4:
                    raise ValueError("expectation2: W must have shape %s" % ((m,) * 4,))
                wctx.set_V_pqrs(W)
            if not wctx.V_exchange_symmetric():
                raise PymesError("expectation2: the operator does not have the symmetry W_pqrs = W_qpsr (max |W_pqrs - W_qpsr| = "
                                 "%.3e)" % wctx.V_exchange_asymmetry()[0])
            _, _, on_ctx = self._on_context("expectation2", wctx)
            val = device_expectation2(wctx, on_ctx(self.t1), on_ctx(self.t2), on_ctx(self.lambda1), on_ctx(self.lambda2))
        finally:
            if own:
                wctx.close()
        if O is not None:
            val += self.expectation(O, t1=self.t1)
        return val

    def expectation(self, O, t1=None):
        """sum gamma_pq O_pq: the correlation part of the expectation value of the one-body operator O (orbital basis of f).
        Uses the density of the last ``rdm1`` call (``t1`` given: computes it first)."""
        if t1 is not None:
            self.rdm1(t1)
        if getattr(self, "gamma", None) is None:
            raise RuntimeError("expectation: call rdm1(t1) first")
        g = self.gamma.copy()
        g[np.arange(self.no), np.arange(self.no)] -= 2.0
        return float((g * np.asarray(O, dtype=np.float64)).sum())


def natural_occupations(rdm1):
    """Eigenvalues of the symmetrised density, descending."""
    return np.linalg.eigvalsh(0.5 * (rdm1 + rdm1.T))[::-1].copy()
