"""Frozen natural orbitals (FNO) and frozen core for CCSD(T) on the MI355X engine (include/pymes_amd.h, pymes_fno_density,
pymes_derive_context).

Definitions (closed shell, canonical Fock matrix, Hermitian integrals):

* Orbital window: the ``n_frozen`` lowest occupied orbitals are dropped; the active occupied orbitals are [n_frozen, no),
  no' = no - n_frozen.
* Amplitudes over the active occupied orbitals and all virtuals, in the project's T[a,b,i,j] convention:
  t[a,b,i,j] = V_ijab / (eps_i + eps_j - eps_a - eps_b),  E_MP2 = sum (2 t_abij - t_baij) V_ijab.
* Density: the spin-summed virtual block of the unrelaxed MP2 density,
  D_ab = 2 sum_{c,i,j} (2 t[a,c,i,j] - t[c,a,i,j]) t[b,c,i,j]; symmetric, eigenvalues (natural occupations) in [0, 2].
* Truncation: eigenvectors sorted by occupation, descending, each with its largest-magnitude component positive; kept are
  those with occupation >= ``occ_threshold`` or the first ``nv_keep`` (at most one of the two).  With neither only the core
  is frozen: C is the identity and the MP2 correction is exactly 0.
* Semicanonicalisation: N (v x v') the kept natural orbitals, N^T f_vv N = W diag(eps') W^T with eps' ascending; the new
  virtuals are C = N W (same sign rule).  Occupied orbitals are not rotated.
* dMP2 = E_MP2(active occupied, all virtuals) - E_MP2(active occupied, kept semicanonical virtuals).

The density and the transformed integrals are built on the device; only the v x v and v' x v' eigenproblems run on the
host.  ``truncate`` returns the Fock matrix and the ``DeviceIntegrals`` of the correlated space, which ``CCSD.solve``
takes like any other source.
"""
import ctypes as C

import numpy as np

from pymes_amd import _lib
from pymes_amd import dist as pdist
from pymes_amd.device import Context
from pymes_amd.integral.device import DeviceIntegrals
from pymes_amd.solver import ccsd_t


class FNOResult:
    """What ``truncate`` returns.  ``fock``: U^T f U (n' x n', host), ``ints``: DeviceIntegrals of the new space (owned by
    the result: ``close()`` releases them), ``no`` / ``nv``: the correlated space, ``n_frozen``, ``occupations``: all v
    natural occupations (descending), ``C``: the new virtuals in the old ones (v x v'), ``eps_v``: their orbital energies,
    ``e_mp2_full``, ``e_mp2_kept``, ``de_mp2`` = e_mp2_full - e_mp2_kept."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def close(self):
        if self.ints is not None:
            self.ints.ctx.close()


def sign_fix(M):
    """Columns of M with their largest-magnitude component made positive (the first one of equal magnitude)."""
    M = np.array(M, dtype=np.float64, copy=True)
    if M.size:
        idx = np.argmax(np.abs(M), axis=0)
        s = np.where(M[idx, np.arange(M.shape[1])] < 0.0, -1.0, 1.0)
        M *= s
    return M


def natural_orbitals(D):
    """(occupations descending, eigenvectors as columns with the sign rule) of the symmetric density D."""
    occ, vec = np.linalg.eigh(np.asarray(D, dtype=np.float64))
    order = np.argsort(-occ, kind="stable")
    return occ[order], sign_fix(vec[:, order])


def check_options(no, nv, n_frozen=0, occ_threshold=None, nv_keep=None):
    """ValueError naming the condition unless 0 <= n_frozen < no, at most one of occ_threshold / nv_keep is given and
    nv_keep lies in [1, nv]."""
    if int(n_frozen) != n_frozen or not 0 <= int(n_frozen) < int(no):
        raise ValueError("n_frozen = %r must lie in [0, no) = [0, %d): at least one occupied orbital stays active"
                         % (n_frozen, no))
    if occ_threshold is not None and nv_keep is not None:
        raise ValueError("give at most one of occ_threshold and nv_keep")
    if nv_keep is not None and (int(nv_keep) != nv_keep or not 1 <= int(nv_keep) <= int(nv)):
        raise ValueError("nv_keep = %r must lie in [1, nv] = [1, %d]" % (nv_keep, nv))
    if occ_threshold is not None and not np.isfinite(float(occ_threshold)):
        raise ValueError("occ_threshold must be a finite number")


def n_kept(occ, occ_threshold=None, nv_keep=None):
    """How many of the natural orbitals (occupations descending) are kept: those with occupation >= occ_threshold, or
    the first nv_keep; all of them with neither.  ValueError if the threshold keeps none."""
    occ = np.asarray(occ)
    if nv_keep is not None:
        return int(nv_keep)
    if occ_threshold is None:
        return occ.size
    k = int(np.count_nonzero(occ >= float(occ_threshold)))
    if k < 1:
        raise ValueError("occ_threshold = %g keeps no virtual orbital (largest occupation %.3e)"
                         % (occ_threshold, occ.max(initial=0.0)))
    return k


def semicanonical(N, f_vv):
    """(C = N W, eps' ascending) with N^T f_vv N = W diag(eps') W^T, columns of C with the sign rule."""
    F = N.T @ np.asarray(f_vv, dtype=np.float64) @ N
    F = 0.5 * (F + F.T)
    e, W = np.linalg.eigh(F)
    return sign_fix(N @ W), e


def density(ctx, n_frozen, v_ijab=None):
    """pymes_fno_density: (D [v,v] host, E_MP2) of the window [n_frozen, no) of ``ctx`` (its orbital energies set);
    ``v_ijab``: a DeviceArray [no,no,v,v] of ``ctx``, None = the context's own block."""
    D = np.empty((ctx.nv, ctx.nv))
    e = C.c_double()
    ctx.lib.call("pymes_fno_density", ctx.handle, C.c_void_p(v_ijab.ptr if v_ijab is not None else None), int(n_frozen),
                 _lib.host_ptr(D), C.byref(e))
    return D, float(e.value)


def derive_context(ints, n_frozen, Cmat):
    """pymes_derive_context: DeviceIntegrals of occupied [n_frozen, no) and virtuals rotated by Cmat [v, v'] (a new
    context on the same device)."""
    src = ints.ctx
    Cmat = np.ascontiguousarray(Cmat, dtype=np.float64)
    if Cmat.ndim != 2 or Cmat.shape[0] != src.nv:
        raise ValueError("C has the shape %s, expected (%d, nv')" % (Cmat.shape, src.nv))
    dst = Context(src.no - int(n_frozen), Cmat.shape[1], device=src.device, lib=src.lib)
    try:
        src.lib.call("pymes_derive_context", src.handle, dst.handle, int(n_frozen), _lib.host_ptr(Cmat), Cmat.shape[1])
    except BaseException:
        dst.close()
        raise
    return DeviceIntegrals(dst)


def _from_rank0(vec):
    """Rank 0's float64 vector on every rank (replicated torch.distributed path), else ``vec`` itself."""
    vec = np.asarray(vec, dtype=np.float64)
    if not pdist.sharded() or pdist.stubbed():
        return vec
    rank, _, _ = pdist.world()
    return pdist.allreduce_sum(vec if rank == 0 else np.zeros_like(vec))


def _factor_source(source, n):
    B = np.ascontiguousarray(source[1], dtype=np.float64)
    if B.ndim != 3 or B.shape[1:] != (n, n):
        raise ValueError("factors: B must be [naux, n, n] with n = %d, got %s" % (n, B.shape))
    asym = float(np.abs(B - B.transpose(0, 2, 1)).max(initial=0.0))
    if not asym <= 1e-10 * max(float(np.abs(B).max(initial=0.0)), 1e-300):
        raise ValueError("frozen natural orbitals need Hermitian integrals: the factors B[Q,p,r] are not symmetric in (p,r) "
                         "(max |B - B^T| = %.3e); transcorrelated integrals are not supported" % asym)
    return B


def truncate(no, t_fock_pq, source, *, n_frozen=0, occ_threshold=None, nv_keep=None, shard=None, direct=None, device=0,
             lib=None):
    """Frozen core and frozen natural orbitals (definitions in the module docstring).

    ``source``: a host V_pqrs, a full-space replicated ``DeviceIntegrals`` (left as it is, apart from its orbital
    energies), or ``("factors", B)`` with V[p,q,r,s] = sum_Q B[Q,p,r] B[Q,q,s] (no full-space v^4 block is ever formed;
    ``shard=(rank, world)`` then builds the new space's integrals with that integral shard, ``direct=True | bytes`` as a
    factor-direct context without any V_abcd, pymes_set_integral_direct).  ``device`` / ``lib``: where
    the contexts of a host source live.  With torch.distributed running one process per GPU, rank 0's choice of the
    space (C, eps') and its energies are used on every rank.  Returns an ``FNOResult``."""
    f = ccsd_t.check_canonical(no, t_fock_pq)
    n = f.shape[0]
    if f.shape != (n, n) or not 0 < no < n:
        raise ValueError("the Fock matrix is %s with no = %d" % (f.shape, no))
    nv = n - no
    check_options(no, nv, n_frozen, occ_threshold, nv_keep)
    nf = int(n_frozen)
    truncating = occ_threshold is not None or nv_keep is not None
    eps_o, eps_v = f.diagonal()[:no].copy(), f.diagonal()[no:].copy()
    factors = isinstance(source, tuple) and len(source) == 2 and isinstance(source[0], str)
    if factors and source[0] != "factors":
        raise ValueError("a tuple source must be ('factors', B)")
    if not factors and shard is not None:
        raise ValueError("shard= is supported with the ('factors', B) source only: a new space is not derived as a sharded "
                         "context from a replicated one")
    if not factors and direct:
        raise ValueError("direct= is supported with the ('factors', B) source only: a factor-direct context is built from "
                         "factors, not derived from stored integrals")
    owned = []          # contexts made here and closed before returning
    result = None
    try:
        if factors:
            B = _factor_source(source, n)
            ctx = Context(no, nv, device=device, lib=lib)
            owned.append(ctx)
            Bov = ctx.array(B[:, :no, no:])
            Vijab = ctx.contract("Qia,Qjb->ijab", Bov, Bov)
            Bov.free()
            ints = None
        else:
            if isinstance(source, DeviceIntegrals):
                ints = source
                if ints.shard is not None or ints.ctx.shard is not None:
                    raise ValueError("the source DeviceIntegrals are a sharded context (shard %s): frozen natural orbitals "
                                     "are derived from a replicated source" % (ints.ctx.shard,))
                if getattr(ints, "direct", False):
                    raise ValueError("the source DeviceIntegrals are a factor-direct context (direct=True): frozen natural "
                                     "orbitals are derived from a stored source, or from ('factors', B)")
                if (ints.no, ints.nv) != (no, nv):
                    raise ValueError("the integrals are for (no, nv) = (%d, %d), the Fock matrix for (%d, %d)"
                                     % (ints.no, ints.nv, no, nv))
            else:
                V = np.asarray(source)
                if np.iscomplexobj(V):
                    raise NotImplementedError("complex integrals are not supported by the fp64 HIP path")
                if V.shape != (n,) * 4:
                    raise ValueError("V_pqrs has the shape %s, expected %s" % (V.shape, (n,) * 4))
                ints = DeviceIntegrals.from_V_pqrs(no, V, device=device, lib=lib)
                owned.append(ints.ctx)
            ctx, Vijab = ints.ctx, None
        ctx.set_orbital_energies(eps_o, eps_v)
        D, e_full = density(ctx, nf, Vijab)
        if Vijab is not None:
            Vijab.free()
        occ, N = natural_orbitals(D)
        if truncating:
            k = n_kept(occ, occ_threshold, nv_keep)
            k = int(_from_rank0([k])[0])
            Cm, eps_new = semicanonical(N[:, :k], f[no:, no:])
        else:
            k, Cm, eps_new = nv, np.eye(nv), eps_v.copy()
        payload = _from_rank0(np.concatenate([Cm.ravel(), eps_new, occ, [e_full]]))
        Cm, eps_new = payload[:nv * k].reshape(nv, k).copy(), payload[nv * k:nv * k + k].copy()
        occ, e_full = payload[nv * k + k:nv * k + k + nv].copy(), float(payload[-1])
        # the new space: occupied [nf, no) unrotated, virtuals C
        U = np.zeros((n, no - nf + k))
        U[nf:no, :no - nf] = np.eye(no - nf)
        U[no:, no - nf:] = Cm
        fock = U.T @ f @ U
        if factors:
            Bd = ctx.array(B)
            Ud = ctx.array(U)
            half = ctx.contract("Qpq,qy->Qpy", Bd, Ud)
            Bd.free()
            Bn = ctx.contract("px,Qpy->Qxy", Ud, half, batch="Q")
            half.free()
            Ud.free()
            Bh = Bn.get()
            Bn.free()
            new = DeviceIntegrals.from_factors(no - nf, Bh, shard=shard, direct=direct, device=ctx.device, lib=ctx.lib)
        else:
            new = derive_context(ints, nf, Cm)
        result = FNOResult(fock=fock, ints=new, no=no - nf, nv=k, n_frozen=nf, occupations=occ, C=Cm, eps_v=eps_new,
                           e_mp2_full=e_full, e_mp2_kept=e_full, de_mp2=0.0)
        if truncating:
            new.ctx.set_orbital_energies(eps_o[nf:], eps_new)
            e_kept = float(_from_rank0([density(new.ctx, 0)[1]])[0])
            result.e_mp2_kept, result.de_mp2 = e_kept, e_full - e_kept
        return result
    except BaseException:
        if result is not None:
            result.close()
        raise
    finally:
        for c in owned:
            c.close()
