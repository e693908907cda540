"""CPU: the (T) correction (include/pymes_amd.h, pymes_ccsd_t; pymes_amd/solver/ccsd_t.py).  The numpy loop over the unique
triples (tests/_triples_reference.py, the GPU tests' oracle) against the textbook spin-orbital form, for 8-fold and for
plane-wave-like 4-fold integrals; the C interface and its bindings; the host simulator's refusal; the Python refusals."""
import contextlib
import io
import itertools
import os
import re

import numpy as np
import pytest

from oracle.cases import synthetic_case
from pymes_amd import _lib
from pymes_amd.device import Context
from tests import _triples_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(no, nv, kind, seed=1):
    f, V, _, eps = synthetic_case(no, nv, seed=seed)
    if kind == "4fold":
        V = R.four_fold_V(no + nv, seed + 2)
    t1, t2 = R.random_amplitudes(no, nv, seed + 4, amp=0.1)
    return f, V, eps, t1, t2


@pytest.mark.parametrize("kind", ["8fold", "4fold"])
@pytest.mark.parametrize("no,nv", [(2, 5), (3, 4), (4, 5), (2, 3)])
def test_loop_form_matches_spin_orbital_form(no, nv, kind):
    f, V, eps, t1, t2 = _inputs(no, nv, kind)
    e_loop = R.energy(no, V, eps, t1, t2)
    e_so = R.spin_orbital_energy(no, V, eps, t1, t2)
    assert abs(e_so) > 1e-6
    assert abs(e_loop - e_so) <= 1e-14 * abs(e_so), (e_loop, e_so)
    # CCD amplitudes (t1 = None): the connected part alone
    e_loop = R.energy(no, V, eps, None, t2)
    e_so = R.spin_orbital_energy(no, V, eps, None, t2)
    assert abs(e_loop - e_so) <= 1e-14 * abs(e_so), (e_loop, e_so)


@pytest.mark.parametrize("kind", ["8fold", "4fold"])
@pytest.mark.parametrize("nv", [3, 5])
def test_one_occupied_orbital_gives_zero(nv, kind):
    f, V, eps, t1, t2 = _inputs(1, nv, kind)
    assert abs(R.energy(1, V, eps, t1, t2)) <= 1e-15
    assert abs(R.spin_orbital_energy(1, V, eps, t1, t2)) <= 1e-15


@pytest.mark.parametrize("kind", ["8fold", "4fold"])
def test_S_is_permutation_invariant(kind):
    no, nv = 3, 4
    f, V, eps, t1, t2 = _inputs(no, nv, kind, seed=7)
    for tri in ((2, 1, 0), (2, 2, 0), (1, 0, 0)):
        ref = R.S_ijk(no, V, eps, t1, t2, *tri)
        assert abs(ref) > 1e-8
        for p in itertools.permutations(tri):
            assert abs(R.S_ijk(no, V, eps, t1, t2, *p) - ref) <= 1e-14 * abs(ref), (tri, p)


def test_triple_numbering():
    for no in (1, 2, 5):
        tri = R.triples(no)
        assert len(tri) == R.n_triples(no) == no * (no + 1) * (no + 2) // 6
        for t, (i, j, k) in enumerate(tri):
            assert t == i * (i + 1) * (i + 2) // 6 + j * (j + 1) // 2 + k
    from pymes_amd.solver import ccsd_t
    for no, world in ((5, 3), (2, 4), (7, 1)):
        chunks = [ccsd_t.rank_range(no, r, world) for r in range(world)]
        assert chunks[0][0] == 0 and chunks[-1][1] == ccsd_t.n_triples(no)
        assert all(chunks[r][1] == chunks[r + 1][0] for r in range(world - 1))


def test_c_interface_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "pymes_amd.h")).read()
    for name in ("pymes_ccsd_t_triples", "pymes_ccsd_t"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    lib = _lib.Library()                      # libpymes_amd.so (HIP); raises if missing
    for name in ("pymes_ccsd_t_triples", "pymes_ccsd_t"):
        assert hasattr(lib.dll, name), name


@pytest.mark.parametrize("no,nv", [(2, 4), (6, 3)])
def test_host_simulator_has_no_triples_kernel(hostsim_lib, no, nv):
    """The host side runs to the kernel (the Hermiticity check included, also with more occupied than virtual orbitals)."""
    import ctypes as C
    f, V, eps, t1, t2 = _inputs(no, nv, "8fold")
    ctx = Context(no, nv, lib=hostsim_lib)
    try:
        ctx.set_V_pqrs(V)
        n = C.c_int64()
        hostsim_lib.call("pymes_ccsd_t_triples", ctx.handle, C.byref(n))
        assert n.value == R.n_triples(no)
        from pymes_amd.solver.ccsd_t import triples_energy
        with pytest.raises(_lib.PymesError, match="not available in this backend"):
            triples_energy(ctx, eps, ctx.array(t1), ctx.array(t2), 0, n.value)
    finally:
        ctx.close()


def test_python_refusals():
    from pymes_amd.solver.ccsd import CCSD
    from pymes_amd.solver.ccsd_t import get_triples_energy
    no, nv = 2, 4
    f, V, eps, t1, t2 = _inputs(no, nv, "8fold")
    bad = f.copy()
    bad[0, no + 1] = bad[no + 1, 0] = 1e-4
    with pytest.raises(ValueError, match="canonical"):
        get_triples_energy(no, bad, V, t1, t2)
    bad = f.copy()
    bad[no, no + 2] = bad[no + 2, no] = 2e-6
    with pytest.raises(ValueError, match="canonical"):
        get_triples_energy(no, bad, V, t1, t2)
    with pytest.raises(ValueError, match="canonical"):
        get_triples_energy(no, bad, V, t1, t2, canonical_tol=1e-6)
    with pytest.raises(ValueError, match="DCSD"):
        with contextlib.redirect_stdout(io.StringIO()):
            CCSD(no, is_dcsd=True).solve(f, V, triples=True)
    with pytest.raises(ValueError, match="canonical"):
        with contextlib.redirect_stdout(io.StringIO()):
            CCSD(no).solve(bad, V, triples=True)
