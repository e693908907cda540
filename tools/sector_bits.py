#!/usr/bin/env python3
"""The bits of the momentum-sector path (pymes_amd/solver/ueg_cc.py): one JSON line {case, quantity, sha256} per
quantity, the hash taken over the bytes of the fp64 values.  Two runs of one checkout that differ in a line say that the
quantity is not reproducible; two checkouts whose reproducible lines agree compute the same bits.

  solver cases   N = 14 at cutoff 2 and 5, N = 54 at cutoff 5 (k_cutoff = 1.0) and the twisted basis of
                 tests/golden/ueg_twist.npz; Coulomb integrals and the transcorrelated only_2b + effect_2b (trunc); CCD and DCD:
                 SectorCCD.get_residual and SectorLambda.get_residual on seeded symmetric vectors; a
                 SectorCCD.solve(max_iter=3, lambda_max_iter=3, density=True, lambda_triples=...) with every scalar result,
                 "t2 amp", "lambda2", "n(k)", the structure factor, the density arena, gamma, stored_transfer() and
                 pair_transfer()
  kernel cases   pymes_sector_triples and pymes_sector_triples_lambda on the seeded operands of tests/test_gpu_sector_triples.py
                 and tests/test_gpu_sector_lambda.py: per-triple values and the sum at (14,2), (14,8), the twisted support, and
                 at (14,5) with a workspace of 1, 5 and all triples; Lambda-(T) with both sides equal ("lambda L=T": the (T) bits
                 if the two entries share their energy kernel)
  ipea cases     the sector IP / EA-EOM-CCD at the solver cases, Coulomb and transcorrelated, the lowest and the
                 highest admissible target of either kind: sigma of 3 seeded stacked vectors, the flat diagonal, and the roots,
                 singles weights and residuals of a one-root solve of 6 passes.  Printed after the 292 lines of the other cases, and only by a
                 checkout that has pymes_amd/solver/ueg_eom.py
  gf cases       the sector spectral functions at the same cases and targets: the Hessenberg matrix of a 20-step device
                 Arnoldi run (pymes_sector_arnoldi_step), G at 9 frequencies and its residuals, for a fixed n(k).  Printed after
                 the 404 lines of the other cases, and only by a checkout whose ueg_eom has SectorSpectralFunction

    python3 tools/sector_bits.py [--out FILE]
It uses the package and the test helpers of the checkout it lies in; the first 292 lines need only names that older checkouts
of the sector path have too: copy it into one to compare."""
import argparse
import functools
import hashlib
import json
import operator
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from pymes_amd.device import Context  # noqa: E402
from pymes_amd.solver.ueg_cc import SectorCCD, SectorLambda  # noqa: E402
from tests import _triples_reference as R  # noqa: E402
from tests.test_gpu_sector_cc import model, quiet  # noqa: E402
from tests.test_gpu_sector_lambda import run_lambda_kernel, symmetric, two_sided_operands  # noqa: E402
from tests.test_gpu_sector_triples import random_operands, run_kernel, support, twisted_model  # noqa: E402

SOLVER_CASES = [(14, 2), (14, 5), (54, 5), "twist"]
SCALARS = ("ccd e", "dE", "lambda residual", "density e", "lambda (t) e", "ccd(t)_lambda e")


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()


def solver_lines(ctx, case, emit):
    m = twisted_model() if case == "twist" else model(*case, k_cutoff=1.0)
    tab = m.sector_tables()
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    T, lam = symmetric(tab, 11, 0.1), symmetric(tab, 12)
    for kind in ("coulomb", "tc"):
        terms = [{}] if kind == "coulomb" else [dict(correlator=m.trunc, is_only_2b=True),
                                                dict(correlator=m.trunc, is_effect_2b=True)]
        ints, tints = (functools.reduce(operator.add, [quiet(f, tab, ctx=ctx, **t, **kw) for t in terms])
                       for f, kw in ((m.eval_2b_sectors, {}), (m.eval_2b_triples, dict(both_sides=True))))
        eps = ints.hf_orbital_energies(kin)
        for is_dcd in (False, True):
            name = "%s %s %s" % (case, kind, "dcd" if is_dcd else "ccd")
            emit(name, "residual", SectorCCD(tab.no, is_dcd=is_dcd).get_residual(eps, ints, T))
            emit(name, "lambda residual vector", SectorLambda(tab.no, is_dcd=is_dcd).get_residual(eps, ints, T, lam))
            res = quiet(SectorCCD(tab.no, is_dcd=is_dcd).solve, eps, ints, max_iter=3, lambda_max_iter=3, density=True,
                        lambda_triples=tints)
            for key in SCALARS:
                emit(name, key, res[key])
            emit(name, "t2 amp", res["t2 amp"].get())
            emit(name, "lambda2", res["lambda2"].get())
            emit(name, "n(k)", res["n(k)"])
            emit(name, "structure factor", res["structure factor"])
            dens = res["density"]
            emit(name, "density arena", dens.arena.get())
            emit(name, "gamma", dens.gamma.get())
            emit(name, "stored_transfer", dens.stored_transfer().get())
            emit(name, "pair_transfer", dens.pair_transfer().get())


def kernel_lines(ctx, emit):
    for case, sizes in (((14, 2), [None]), ((14, 8), [None]), ("twist", [None]), ((14, 5), [1, 5, None])):
        tab, tt = support(case)
        n = R.n_triples(tt.no)
        eps, Tc, Vv, Vo = random_operands(tt, 31)
        two = two_sided_operands(tt)
        for k in sizes:
            name = "kernel %s ws=%s" % (case, "all" if k is None else k)
            e, p = run_kernel(ctx, tt, eps, Tc, Vv, Vo, 0, n, triples_in_ws=k)
            emit(name, "triples per triple", p)
            emit(name, "triples sum", e)
            e, p = run_lambda_kernel(ctx, tt, *two, 0, n, triples_in_ws=k)
            emit(name, "lambda per triple", p)
            emit(name, "lambda sum", e)
            e, p = run_lambda_kernel(ctx, tt, eps, Tc, Tc, Vv, Vo, Vv, Vo, 0, n, triples_in_ws=k)
            emit(name, "lambda L=T per triple", p)
            emit(name, "lambda L=T sum", e)


def ipea_lines(ctx, case, emit):
    from pymes_amd.solver.sectors import TriplesTables
    from pymes_amd.solver.ueg_eom import SectorEA_EOM_CCD, SectorIP_EOM_CCD, SectorIPEASigma
    m = twisted_model() if case == "twist" else model(*case, k_cutoff=1.0)
    tab = m.sector_tables()
    tt = TriplesTables(tab)
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    T = symmetric(tab, 11, 0.1)
    for kind in ("coulomb", "tc"):
        terms = [{}] if kind == "coulomb" else [dict(correlator=m.trunc, is_only_2b=True),
                                                dict(correlator=m.trunc, is_effect_2b=True)]
        total = lambda f, *a, **kw: functools.reduce(operator.add, [quiet(f, *a, ctx=ctx, **t, **kw) for t in terms])
        ints, tints = total(m.eval_2b_sectors, tab), total(m.eval_2b_triples, tt, both_sides=True)
        eps = ints.hf_orbital_energies(kin)
        for op, cls, targets in (("ip", SectorIP_EOM_CCD, [0, tab.no - 1]), ("ea", SectorEA_EOM_CCD, [tab.no, tab.n - 1])):
            ladders = total(m.eval_2b_ladder, tt, targets) if op == "ea" else None
            sig = SectorIPEASigma(op, eps, ints, tints, T, ladders=ladders)
            rng = np.random.default_rng(5)
            for p in targets:
                name, qt = "%s %s %s target %d" % (case, kind, op, p), sig.tables_of(p)
                r1, R = rng.standard_normal(3), rng.standard_normal((3,) + qt.shape) * qt.inside.reshape(qt.shape)
                s1, S = sig.get_sigma(p, r1, R)
                emit(name, "sigma", np.concatenate([s1, S.ravel()]))
                emit(name, "diagonals", sig.diagonals(p).get())
            sig.close()
            res = quiet(cls(tab.no, n_roots=1, max_iter=6).solve, eps, ints, tints, T,
                        targets, ladders=ladders)
            for key in (op + " e", "singles weight", "residuals"):
                emit("%s %s %s" % (case, kind, op), key, res[key])


def gf_lines(ctx, case, emit):
    from pymes_amd.solver.sectors import TriplesTables
    from pymes_amd.solver.ueg_eom import SectorSpectralFunction
    m = twisted_model() if case == "twist" else model(*case, k_cutoff=1.0)
    tab = m.sector_tables()
    tt = TriplesTables(tab)
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    T, nk = symmetric(tab, 11, 0.1), np.linspace(1.9, 0.1, tab.n)
    for kind in ("coulomb", "tc"):
        terms = [{}] if kind == "coulomb" else [dict(correlator=m.trunc, is_only_2b=True),
                                                dict(correlator=m.trunc, is_effect_2b=True)]
        total = lambda f, *a, **kw: functools.reduce(operator.add, [quiet(f, *a, ctx=ctx, **t, **kw) for t in terms])
        ints, tints = total(m.eval_2b_sectors, tab), total(m.eval_2b_triples, tt, both_sides=True)
        eps = ints.hf_orbital_energies(kin)
        for op, targets in (("ip", [0, tab.no - 1]), ("ea", [tab.no, tab.n - 1])):
            ladders = total(m.eval_2b_ladder, tt, targets) if op == "ea" else None
            res = quiet(SectorSpectralFunction(tab.no, max_dim=20, r_epsilon=0.0).solve, eps, ints, tints, T, nk,
                        np.linspace(-3.0, 3.0, 9), 0.1, keep_basis=True, ladders=ladders, **{op: targets})
            for n, p in enumerate(targets):
                name = "%s %s %s target %d" % (case, kind, op, p)
                emit(name, "gf hessenberg", res[op + " basis"].hessenberg(p))
                emit(name, "gf G", np.concatenate([res[op + " G"][n].real, res[op + " G"][n].imag]))
                emit(name, "gf residuals", res[op + " residuals"][n])
            res[op + " basis"].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(case, quantity, value):
        line = json.dumps({"case": case, "quantity": quantity, "sha256": digest(value)})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
    ctx = Context(1, 1, device=0)
    try:
        kernel_lines(ctx, emit)
        for case in SOLVER_CASES:
            solver_lines(ctx, case, emit)
        if os.path.exists(os.path.join(ROOT, "pymes_amd", "solver", "ueg_eom.py")):
            for case in SOLVER_CASES:
                ipea_lines(ctx, case, emit)
            from pymes_amd.solver import ueg_eom
            if hasattr(ueg_eom, "SectorSpectralFunction"):
                for case in SOLVER_CASES:
                    gf_lines(ctx, case, emit)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
