"""What the EOM drivers share on the host side: the flat device vector [x1 | zero pad | x2], the orthonormalisers of a trial
space, the growth of the subspace matrix, ONE block Davidson, and the lifetime / opening of a library handle bound to a context.

The vectors live on the device; the host sees only overlaps (``ctx.gram``) and coefficients (``ctx.lincomb_multi``).  The EE driver
(``EOM_CCSD.solve``) keeps its own loop — it is pinned pass by pass to the reference's schedule and expands without a residual
kernel — and uses the layout, the orthonormalisers and ``extend_subspace``; the IP / EA driver and the transition solver run
``block_davidson``.
"""
import ctypes as C
import time
from types import SimpleNamespace

import numpy as np

from pymes_amd import _lib
from pymes_amd.device import Context, DeviceArray, PymesError
from pymes_amd.integral.device import DressedDeviceIntegrals
from pymes_amd.log import print_logging_info
from pymes_amd.mixer.diis import _single_threaded_blas

ORTH_TOL = 1e-13       # max |U^T U - 1| accepted for the trial space (numpy's Householder QR: ~1e-15)

# what the sequential orthonormaliser does with a vector that vanishes against the others, and below which relative norm it does
REPLACE_NULL, DROP_NULL = "replace", "drop"
_NULL_NORM = {REPLACE_NULL: 1e-12, DROP_NULL: 1e-10}


def view(ctx, vec, offset, shape):
    """A non-owning device array of ``shape``, ``offset`` doubles into ``vec``."""
    return DeviceArray(ctx, vec.ptr + 8 * offset, shape, owned=False, keepalive=vec)


class FlatLayout:
    """Flat subspace vectors [x1 (shape1) | zero pad | x2 (shape2)], the doubles part on a 256-byte boundary.  (A combination of
    vectors with a zero pad has a zero pad; a sigma vector gets its parts written one by one, so its pad is zeroed: ``padded``.)"""

    def __init__(self, ctx, shape1, shape2):
        self.ctx, self.shape1, self.shape2 = ctx, tuple(shape1), tuple(shape2)
        self.n1, self.n2 = int(np.prod(self.shape1)), int(np.prod(self.shape2))
        self.off2 = -(-self.n1 // 32) * 32
        self.nflat = self.off2 + self.n2

    def part1(self, vec):
        return view(self.ctx, vec, 0, self.shape1)

    def part2(self, vec):
        return view(self.ctx, vec, self.off2, self.shape2)

    def zero_pad(self, vec):
        if self.off2 > self.n1:
            view(self.ctx, vec, self.n1, (self.off2 - self.n1,)).zero_()
        return vec

    def empty(self):
        return self.ctx.empty((self.nflat,))

    def padded(self):
        return self.zero_pad(self.empty())

    def unit(self, p):
        """The zero vector with singles element ``p`` set to 1."""
        vec = self.ctx.zeros((self.nflat,))
        one = np.zeros(self.n1)
        one[p] = 1.0
        self.part1(vec).set(one.reshape(self.shape1))
        return vec


# ---- orthonormalisation ----------------------------------------------------------------------------------------------------------
def orthonormalise_block(ctx, layout, us, ys, shadows=None, on_null=REPLACE_NULL):
    """EOM_CCSD.QR (eom_ccsd.py:512-541) for a trial space [us | ys] whose leading vectors ``us`` are orthonormal already
    (Householder QR leaves those as they are, up to a sign the Rayleigh-Ritz step does not see): the block ``ys`` is
    projected against ``us`` and orthonormalised in itself by rounds of block Gram-Schmidt in its Pythagorean form
    — ONE Gram product [us | ys]^T ys (every vector read once), the Cholesky factor of ys^T ys - P^T P on the host, ONE
    multi-output combination (ys - us P) R^-1 — so a round costs two passes over the subspace instead of a dot product
    and an update per pair of vectors; a round is repeated only when the check of the result asks for it.  Returns the
    new orthonormal block; with ``shadows`` (vectors that any linear map of ``ys`` must follow, e.g. their sigma vectors;
    only for an empty ``us``) returns (block, mapped shadows).  ``on_null``: see ``orthonormalise_sequential``."""
    assert shadows is None or not us
    k, d = len(ys), len(us)
    eye = np.vstack([np.zeros((d, k)), np.eye(k)])
    for rnd in range(4):
        G = ctx.gram(us + ys, ys)
        # a-posteriori check = the Gram product the next round needs anyway: expansion vectors are residuals, orthogonal
        # to the basis up to rounding (U^T (W v - e U v) = B v - e v), and one round brings them to the unit matrix
        if rnd > 0 and np.abs(G - eye).max() <= ORTH_TOL:
            break
        P, S = G[:d], G[d:] - G[:d].T @ G[:d]
        S = 0.5 * (S + S.T)
        scale = np.sqrt(np.abs(np.diag(S)))
        ok = bool(np.all(np.isfinite(scale)) and np.all(scale > 0.0) and np.all(np.diag(S) > 0.0))
        if ok:
            try:
                with _single_threaded_blas():
                    Lc = np.linalg.cholesky(S / np.outer(scale, scale))          # equilibrated: S = D L L^T D
                    ok = bool(np.diag(Lc).min() > 1e-7)                          # (condition number of ys below ~1e7)
                    Rinv = np.linalg.inv(Lc.T * scale[None, :]) if ok else None  # R = L^T D, ys_new = ys' R^-1
            except np.linalg.LinAlgError:
                ok = False
        if not ok or rnd == 3:       # (numerically) dependent new vectors: vector by vector
            return orthonormalise_sequential(ctx, layout, us, ys, shadows, on_null)
        coef = np.vstack([-P @ Rinv, Rinv])
        out = [layout.empty() for _ in range(k)]
        ctx.lincomb_multi(out, us + ys, coef)
        if shadows is not None:
            sh = [layout.empty() for _ in range(k)]
            ctx.lincomb_multi(sh, shadows, Rinv)
            shadows = sh
        ys = out
    return ys if shadows is None else (ys, shadows)


def orthonormalise_sequential(ctx, layout, us, ys, shadows=None, on_null=REPLACE_NULL):
    """The fall-back of ``orthonormalise_block``: modified Gram-Schmidt with re-orthogonalisation, one vector at a time
    (one Gram product and one combination per sweep).  A vector that vanishes against the others — the reference's
    Householder QR would return an arbitrary unit vector orthogonal to them — is, by ``on_null``, replaced by a seeded random,
    exchange-symmetric direction (``REPLACE_NULL``, below 1e-12 of its norm; for doubles [a,b,i,j]: the EE driver and the
    transition solver) or dropped (``DROP_NULL``, below 1e-10: IP / EA, where nothing new in a direction ends the search in
    it).  With ``shadows`` a null vector is an error; under ``DROP_NULL`` so is the fall-back itself."""
    if shadows is not None and on_null == DROP_NULL:
        raise np.linalg.LinAlgError("linearly dependent Ritz vectors in the Davidson collapse")
    done, sh_done = list(us), []
    rng = np.random.default_rng(len(us) + 1000 * len(ys))
    for z, y in enumerate(ys):
        q = layout.empty().copy_from(y)
        sh = None if shadows is None else layout.empty().copy_from(shadows[z])
        for attempt in range(3):
            nrm0 = np.sqrt(ctx.gram([q], [q])[0, 0])
            for _ in range(2):
                if done:
                    proj = ctx.gram(done, [q])[:, 0]
                    ctx.lincomb_multi([q], done, -proj[:, None], beta=[1.0])
                    if sh is not None:
                        ctx.lincomb_multi([sh], sh_done, -proj[len(us):, None], beta=[1.0])
            nrm = np.sqrt(ctx.gram([q], [q])[0, 0])
            if np.isfinite(nrm) and nrm > _NULL_NORM[on_null] * max(nrm0, 1e-300) and nrm > 0.0:
                break
            if shadows is not None:
                raise np.linalg.LinAlgError("linearly dependent Ritz vectors in the Davidson collapse")
            if on_null == DROP_NULL:
                q = None                                       # nothing new in this direction
                break
            r1 = rng.standard_normal(layout.shape1)
            r2 = rng.standard_normal(layout.shape2)
            q.zero_()
            layout.part1(q).set(r1)
            layout.part2(q).set(r2 + r2.transpose(1, 0, 3, 2))
        if q is None:
            continue
        ctx.lincomb_multi([q], [], np.zeros((0, 1)), beta=[1.0 / nrm])
        if sh is not None:
            ctx.lincomb_multi([sh], [], np.zeros((0, 1)), beta=[1.0 / nrm])
            sh_done.append(sh)
        done.append(q)
    block = done[len(us):]
    return block if shadows is None else (block, sh_done)


# ---- the subspace matrix and the block Davidson ----------------------------------------------------------------------------------
def extend_subspace(ctx, us, ws, B, new, wn):
    """(us + new, ws + wn, B grown by the rows and columns of the new vectors) for B = U^T W, wn = sigma(new)."""
    d0 = len(us)
    us, ws = us + new, ws + wn
    Bn = np.zeros((len(us), len(us)))
    Bn[:d0, :d0] = B
    Bn[:, d0:] = ctx.gram(us, wn)
    if d0:
        Bn[d0:, :d0] = ctx.gram(new, ws[:d0])
    return us, ws, Bn


def block_davidson(ctx, layout, apply_flat, correction, d, start, n_roots, max_dim, max_iter, r_epsilon, shift=1.e-5,
                   targets=None, refuse_complex=None, label="Davidson", on_null=REPLACE_NULL):
    """Block Davidson for ``n_roots`` eigenpairs of a real, not necessarily symmetric operator on flat vectors.

    ``apply_flat(vecs)``: sigma of flat vectors as new flat vectors; ``correction(ss, rs, w, d, shift, qs)``: q_n = (s_n - w_n
    r_n) / (w_n - d + shift) into qs, returns (|s_n - w_n r_n|^2, |r_n|^2); ``d``: the flat diagonal; ``start``: the start vectors.
    Per pass: the new vectors are orthonormalised against the basis, sigma is built for the NEW vectors only, the subspace matrix
    grows by their rows and columns, the Ritz vectors and their sigma vectors are one combination each, residual norms and
    preconditioned corrections come from one launch; converged when every root has |s - w r| / |r| < r_epsilon; collapse to the
    Ritz vectors when the corrections would not fit in ``max_dim``.  Complex Ritz pairs: the real parts are taken.

    ``targets`` None: the lowest roots by real part, residuals with the Ritz values; else the Ritz pair nearest each target, each
    taken once, residuals and corrections with the target itself.  ``refuse_complex``: a format "... root %d ..." for the root's
    index — three consecutive passes with an imaginary part above r_epsilon among the chosen Ritz values raise ``PymesError``,
    and convergence is not accepted while such a pass is being counted; None: imaginary parts are only logged.

    Returns a namespace: ``theta`` (Ritz values), ``w`` (theta, or the targets), ``rz`` / ``sz`` (Ritz vectors and their sigma
    vectors), ``rel``, ``res``, ``nrm`` (|s - w r| / |r|, |s - w r|^2, |r|^2) of the last pass, ``passes``, ``converged``,
    ``history`` (theta of every pass), ``max_basis`` (the largest subspace dimension)."""
    nr = n_roots
    us, ws, B, new = [], [], np.zeros((0, 0)), list(start)
    out = SimpleNamespace(theta=np.zeros(nr), w=np.zeros(nr), rz=[], sz=[], rel=np.full(nr, np.inf), res=np.full(nr, np.inf),
                          nrm=np.ones(nr), passes=0, converged=False, history=[], max_basis=0)
    complex_passes = 0
    for it in range(max_iter):
        t_it = time.time()
        new = orthonormalise_block(ctx, layout, us, new, on_null=on_null) if new else []
        if new:
            us, ws, B = extend_subspace(ctx, us, ws, B, new, apply_flat(new))     # sigma of the new vectors only, one stacked call
            out.max_basis = max(out.max_basis, len(us))
        elif it > 0:
            # (kept as it was: the IP / EA driver's log line for this exit, not an error and not ``converged``; ``passes`` counts the
            # passes done, and the transition solver goes on reporting max_iter for it)
            print_logging_info("No new direction left: the subspace is invariant.", level=1)
            break
        with _single_threaded_blas():
            lam, vec = np.linalg.eig(B)
        if targets is None:
            pick = np.argsort(lam.real, kind="stable")[:nr]
        else:
            pick, left = [], list(range(len(lam)))
            for t in targets:                                               # nearest Ritz value, each taken once
                p = min(left, key=lambda q: abs(lam[q] - t))
                pick.append(p)
                left.remove(p)
            pick = np.array(pick)
        theta, imag = np.real(lam[pick]), np.imag(lam[pick])
        if refuse_complex is not None:
            complex_passes = complex_passes + 1 if np.abs(imag).max() > r_epsilon else 0
            if complex_passes >= 3:
                bad = int(np.argmax(np.abs(imag)))
                raise PymesError((refuse_complex % bad) + " has a complex Ritz value (%.6f %+.3ej): a complex-conjugate pair has "
                                 "no real eigenvector" % (theta[bad], imag[bad]))
        v = np.real(vec[:, pick])
        v = v / np.linalg.norm(v, axis=0)[None, :]
        w = theta if targets is None else np.asarray(targets, dtype=np.float64)
        rz, sz, qs = ([layout.empty() for _ in range(nr)] for _ in range(3))
        ctx.lincomb_multi(rz, us, v)
        ctx.lincomb_multi(sz, ws, v)
        res, nrm = correction(sz, rz, w, d, shift, qs)
        rel = np.sqrt(res / nrm)
        out.theta, out.w, out.rz, out.sz, out.rel, out.res, out.nrm, out.passes = theta, w, rz, sz, rel, res, nrm, it + 1
        out.history.append(np.array(theta))
        print_logging_info("%s pass %d" % (label, it), level=1)
        for r in range(nr):
            print_logging_info("Root {:d} energy = {:.12f}  |residual| / |x| = {:.3e}".format(r, theta[r], rel[r]), level=2)
        if np.abs(imag).max() > 0.0:
            print_logging_info("Ritz values imaginary part = ", imag, level=2)
        print_logging_info("Took {:.3f} seconds ".format(time.time() - t_it), level=2)
        if np.all(rel < r_epsilon) and complex_passes == 0:
            out.converged = True
            print_logging_info("Iterative solver converged.", level=1)
            break
        todo = [n for n in range(nr) if not rel[n] < r_epsilon]
        if len(us) + len(todo) > max_dim:                                   # collapse to the Ritz vectors
            us, ws = orthonormalise_block(ctx, layout, [], rz, shadows=sz, on_null=on_null)
            B = ctx.gram(us, ws)
        new = [qs[n] for n in todo]
    return out


# ---- library handles -------------------------------------------------------------------------------------------------------------
class LibraryHandle:
    """A handle of the engine bound to a context ``self.ctx``: it dies before its context does.  A subclass names the entry that
    destroys it and the noun of the error message, and hands the prepared handle to ``_bind``."""
    DESTROY = NOUN = _h = None

    def _bind(self, h):
        self._h = h
        self.ctx.on_close(self._ctx_closing)

    def _handle(self):
        if self._h is None:
            raise PymesError("the %s handle has been destroyed (its context was closed)" % self.NOUN)
        return self._h

    def close(self):
        h, self._h = self._h, None
        if h is not None:        # (also after the context has gone: the library invalidated the handle then, this frees its shell)
            self.ctx.lib.call(self.DESTROY, h)

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


def apply_flat(layout, apply_many, vecs, *args):
    """sigma of flat vectors as new flat vectors (zero pad), through a handle's ``apply_many(x1s, x2s, *args, out1=, out2=)``."""
    outs = [layout.padded() for _ in vecs]
    apply_many([layout.part1(u) for u in vecs], [layout.part2(u) for u in vecs], *args,
               out1=[layout.part1(w) for w in outs], out2=[layout.part2(w) for w in outs])
    return outs


def correction(lib, entry, handle, layout, ss, rs, w, d, shift, qs):
    """q_n = (s_n - w_n r_n) / (w_n - d + shift) into qs for all roots in one launch (``pymes_eom_correction`` on a context,
    ``pymes_ipea_sigma_correction`` on a sigma handle); returns (|s_n - w_n r_n|^2, |r_n|^2) per root (one synchronisation)."""
    n = len(rs)
    ww = np.ascontiguousarray(w, dtype=np.float64)
    out = np.zeros(2 * max(n, 1))
    lib.call(entry, handle, n, _lib.ptr_array([x.ptr for x in ss]), _lib.ptr_array([x.ptr for x in rs]), _lib.host_ptr(ww),
             C.c_void_p(d.ptr), float(shift), _lib.ptr_array([x.ptr for x in qs]), layout.off2, layout.nflat, _lib.host_ptr(out))
    return out[0:2 * n:2].copy(), out[1:2 * n:2].copy()


def open_handle(no, device, f, V, t2, blocks, make, name, check=None):
    """(f as a host array, ctx, make(ctx, f, t2 on the device, dressed), owns the context) for the two call forms of
    ``EOM_CCSD.solve``: the device hand-over of a CCSD solve (``DressedDeviceIntegrals`` that hold ``blocks``; ``check(ctx)`` may
    refuse their context) or a dictionary of dressed host blocks, for which a context is built that the caller closes."""
    if isinstance(f, DeviceArray):
        f = f.get()
    f = np.asarray(f, dtype=np.float64)
    nv = f.shape[0] - no
    if isinstance(V, DressedDeviceIntegrals):
        ctx = V.ctx
        if check is not None:
            check(ctx)
        if ctx.no != no or ctx.nv != nv:
            raise ValueError("the integrals' context does not match (no, nv) of the Fock matrix")
        if isinstance(t2, DeviceArray) and t2.ctx is not ctx:
            raise ValueError("t2 lives in another context than the dressed integrals")
        V.require(blocks)
        t2d = t2 if isinstance(t2, DeviceArray) else ctx.array(np.asarray(t2, dtype=np.float64))
        return f, ctx, make(ctx, f, t2d, True), False
    ctx = Context(no, nv, device=device)
    try:
        for blk_name in blocks:
            blk = V.get(blk_name)
            if blk is None:
                raise KeyError("%s: the dressed block '%s' is missing from the dictionary" % (name, blk_name))
            ctx.set_V_block(blk_name, np.ascontiguousarray(blk, dtype=np.float64))
        return f, ctx, make(ctx, f, ctx.array(np.asarray(t2, dtype=np.float64)), False), True
    except Exception:
        ctx.close()
        raise
