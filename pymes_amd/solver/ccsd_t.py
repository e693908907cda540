"""The perturbative triples correction (T) of CCSD(T) on the MI355X engine (include/pymes_amd.h, pymes_ccsd_t).

Closed shell, canonical orbitals: the energy is a sum over the o(o+1)(o+2)/6 unique occupied triples i >= j >= k of
m_ijk S_ijk, each formed from the undressed integral blocks and the amplitudes in HBM (W_ijk by fp64 MFMA products, the
energy of a batch of triples by one kernel).  With ``torch.distributed`` initialised (one process per GPU) every rank sums
a contiguous chunk of the triples and one double is all-reduced.

``get_lambda_triples_energy`` is Lambda-CCSD(T) (pymes_ccsd_t_lambda): the same sum with Lambda as the left state, the
triples correction that is defined for transcorrelated (non-Hermitian) integrals, which (T) refuses."""
import ctypes as C

import numpy as np

from pymes_amd import _lib
from pymes_amd import dist as pdist
from pymes_amd.device import DeviceArray
from pymes_amd.integral.device import DeviceIntegrals


def n_triples(no):
    """Number of unique occupied triples i >= j >= k."""
    no = int(no)
    return no * (no + 1) * (no + 2) // 6


def rank_range(no, rank, world):
    """The contiguous chunk of the triples (library order) that rank ``rank`` of ``world`` sums."""
    n = n_triples(no)
    c = -(-n // int(world))
    lo = min(int(rank) * c, n)
    return lo, min(lo + c, n)


def check_canonical(no, t_fock_pq, canonical_tol=1e-6):
    """ValueError unless the off-diagonal oo, vv and ov entries of f are at most ``canonical_tol``."""
    f = np.asarray(t_fock_pq, dtype=np.float64)
    off = f - np.diag(np.diag(f))
    for name, blk in (("oo", off[:no, :no]), ("vv", off[no:, no:]), ("ov", off[:no, no:]), ("vo", off[no:, :no])):
        worst = float(np.abs(blk).max(initial=0.0))
        if worst > canonical_tol:
            raise ValueError("(T) needs canonical orbitals: the largest off-diagonal %s entry of the Fock matrix is %.3e "
                             "(canonical_tol = %.1e)" % (name, worst, canonical_tol))
    return f


def _on_device(ctx, x, shape, what):
    if isinstance(x, DeviceArray):
        if x.ctx is not ctx:
            raise ValueError("%s is a DeviceArray of another context than the integrals'" % what)
        if x.size != int(np.prod(shape)):
            raise ValueError("%s has %d elements, expected the shape %s" % (what, x.size, shape))
        return x, None
    h = np.ascontiguousarray(x, dtype=np.float64)
    if h.shape != tuple(shape):
        raise ValueError("%s has the shape %s, expected %s" % (what, h.shape, tuple(shape)))
    d = ctx.array(h)
    return d, d


def triples_energy(ctx, eps, t1, t2, t_begin, t_end, per_triple=False):
    """pymes_ccsd_t on a context: (sum over [t_begin, t_end), per-triple values as a host array or None).  t1 / t2 are
    DeviceArrays of ``ctx`` (t1 may be None)."""
    eps = np.ascontiguousarray(eps, dtype=np.float64)
    assert eps.shape == (ctx.n,)
    out = ctx.empty((max(t_end - t_begin, 1),)) if per_triple else None
    e = C.c_double()
    try:
        ctx.lib.call("pymes_ccsd_t", ctx.handle, _lib.host_ptr(eps), C.c_void_p(t1.ptr if t1 is not None else None),
                     C.c_void_p(t2.ptr), int(t_begin), int(t_end), C.c_void_p(out.ptr if out is not None else None),
                     C.byref(e))
        vec = out.get()[:t_end - t_begin] if out is not None else None
    finally:
        if out is not None:
            out.free()
    return float(e.value), vec


def lambda_triples_energy(ctx, eps, t2, lam1, lam2, t_begin, t_end, per_triple=False):
    """pymes_ccsd_t_lambda on a context, as ``triples_energy``.  t2 / lam1 / lam2 are DeviceArrays of ``ctx`` (lam1 may be
    None); lam1, lam2 in the library's normalisation (``Lambda_CCSD.solve``)."""
    eps = np.ascontiguousarray(eps, dtype=np.float64)
    assert eps.shape == (ctx.n,)
    out = ctx.empty((max(t_end - t_begin, 1),)) if per_triple else None
    e = C.c_double()
    try:
        ctx.lib.call("pymes_ccsd_t_lambda", ctx.handle, _lib.host_ptr(eps), C.c_void_p(t2.ptr),
                     C.c_void_p(lam1.ptr if lam1 is not None else None), C.c_void_p(lam2.ptr), int(t_begin), int(t_end),
                     C.c_void_p(out.ptr if out is not None else None), C.byref(e))
        vec = out.get()[:t_end - t_begin] if out is not None else None
    finally:
        if out is not None:
            out.free()
    return float(e.value), vec


def _triple_chunk(no, triple_range):
    """(begin, end, all-reduce afterwards?) of a call: the given range, or this rank's chunk of all triples."""
    reduce = triple_range is None and pdist.sharded() and not pdist.stubbed()
    if triple_range is None:
        rank, world, _ = pdist.world()
        lo, hi = rank_range(no, rank, world) if reduce else (0, n_triples(no))
    else:
        lo, hi = int(triple_range[0]), int(triple_range[1])
    return lo, hi, reduce


def get_triples_energy(no, t_fock_pq, ints_or_V_pqrs, t1, t2, device=0, triple_range=None, per_triple=False,
                       canonical_tol=1e-6):
    """E(T) for the amplitudes (t1 [v,o] or None for CCD amplitudes, t2 [v,v,o,o] with T_abij = T_baji) and canonical
    f = t_fock_pq.  ``ints_or_V_pqrs``: a dense host V_pqrs or ``DeviceIntegrals`` (then t1 / t2 may be DeviceArrays of
    its context, e.g. from ``CCSD.solve(..., device_amplitudes=True)``).  ``triple_range=(begin, end)``: only those
    triples (library order, include/pymes_amd.h), no collective; otherwise all of them — split over the ranks and
    all-reduced when ``torch.distributed`` runs one process per GPU.  Returns the energy, or (energy, per-triple
    m_ijk S_ijk of the range as a host array) with ``per_triple=True``."""
    f = check_canonical(no, t_fock_pq, canonical_tol)
    own = not isinstance(ints_or_V_pqrs, DeviceIntegrals)
    ints = DeviceIntegrals.from_V_pqrs(no, ints_or_V_pqrs, device=device) if own else ints_or_V_pqrs
    ctx = ints.ctx
    temps = []
    try:
        if f.shape != (ctx.n, ctx.n) or ctx.no != no:
            raise ValueError("the Fock matrix is %s, the integrals are for %d occupied of %d orbitals" % (f.shape, ctx.no, ctx.n))
        nv = ctx.nv
        d1 = None
        if t1 is not None:
            d1, tmp = _on_device(ctx, t1, (nv, no), "t1")
            temps.append(tmp)
        d2, tmp = _on_device(ctx, t2, (nv, nv, no, no), "t2")
        temps.append(tmp)
        lo, hi, reduce = _triple_chunk(no, triple_range)
        e, vec = triples_energy(ctx, np.diag(f), d1, d2, lo, hi, per_triple)
        if reduce:
            e = float(pdist.allreduce_sum([e])[0])
        return (e, vec) if per_triple else e
    finally:
        for t in temps:
            if t is not None:
                t.free()
        if own:
            ctx.close()


def get_lambda_triples_energy(no, t_fock_pq, ints_or_V_pqrs, t2, lam1, lam2, device=0, triple_range=None, per_triple=False,
                              canonical_tol=1e-6):
    """E_Lambda(T) of Lambda-CCSD(T) for the amplitudes t2 [v,v,o,o], the library's Lambda (lam1 [v,o] or None, lam2
    [v,v,o,o]: ``Lambda_CCSD.solve`` / ``CCSD.solve(density=True)``) and canonical f = t_fock_pq.  t1 does not enter.  The
    integrals need V_pqrs = V_qpsr only: transcorrelated ones are served.  Arguments, ranges, ranks and the return value as
    ``get_triples_energy``."""
    f = check_canonical(no, t_fock_pq, canonical_tol)
    own = not isinstance(ints_or_V_pqrs, DeviceIntegrals)
    ints = DeviceIntegrals.from_V_pqrs(no, ints_or_V_pqrs, device=device) if own else ints_or_V_pqrs
    ctx = ints.ctx
    temps = []
    try:
        if f.shape != (ctx.n, ctx.n) or ctx.no != no:
            raise ValueError("the Fock matrix is %s, the integrals are for %d occupied of %d orbitals" % (f.shape, ctx.no, ctx.n))
        nv = ctx.nv
        dev = []
        for x, shape, what in ((t2, (nv, nv, no, no), "t2"), (lam1, (nv, no), "lam1"), (lam2, (nv, nv, no, no), "lam2")):
            if x is None and what == "lam1":
                dev.append(None)
                continue
            d, tmp = _on_device(ctx, x, shape, what)
            dev.append(d)
            temps.append(tmp)
        lo, hi, reduce = _triple_chunk(no, triple_range)
        e, vec = lambda_triples_energy(ctx, np.diag(f), dev[0], dev[1], dev[2], lo, hi, per_triple)
        if reduce:
            e = float(pdist.allreduce_sum([e])[0])
        return (e, vec) if per_triple else e
    finally:
        for t in temps:
            if t is not None:
                t.free()
        if own:
            ctx.close()
