#!/usr/bin/env python3
"""GPU probe of Lambda and Lambda-(T) on the momentum sectors (pymes_amd/solver/ueg_cc.py, SectorLambda and
sector_lambda_triples_energy).  Prints JSON lines and appends them to profiles/sector_lambda/probe_sector_lambda.txt,
one line per --nel at --cutoff (default 60: 1 935 plane waves), all from one run on Coulomb integrals unless said otherwise:
  iteration  ms per Lambda iteration next to ms per amplitude iteration of the same class (CCD and DCD), each the difference
             of a long and a short solve after a warm-up solve, smallest of three (host clock around solves that end in a
             synchronisation); the library calls per iteration of both;
  ladder     the adjoint ladder launch (V_abcd^T lam, the TRANS_A read of the same blocks) next to the forward one: median of
             --reps windows each, alternating, a window being as many back-to-back launches as fill 0.3 s with one
             synchronisation at the end (host-timed launches, not kernel times); bytes of V_abcd over that time;
  triples    whole sector_lambda_triples_energy calls next to whole sector_triples_energy calls, windows of the same kind;
  tc         the transcorrelated Hamiltonian only_2b + effect_2b (trunc correlator, default k_cutoff): DCD, Lambda and the
             DCD(T)_Lambda energy by SectorCCD.solve(lambda_triples=), with the bytes held.
    python3 tools/probe_sector_lambda.py [--nel 14,54] [--cutoff 60] [--iters 50] [--reps 3] [--part iteration,ladder,triples,tc]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from pymes_amd.device import Context  # noqa: E402
from pymes_amd.model.ueg import UEG  # noqa: E402
from pymes_amd.solver.sectors import TriplesTables  # noqa: E402
from pymes_amd.solver.ueg_cc import (SectorCCD, SectorLambda, lambda_triple_bytes, sector_lambda_triples_energy,  # noqa: E402
                                     sector_triples_energy)

HBM_BYTES_PER_S = 6.3e12


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def per_iteration(solve, iters):
    """ms per iteration: (time of 1 + iters passes) - (time of 1 pass), after one untimed solve; smallest of three each."""
    def run(cap):
        t0 = time.perf_counter()
        quiet(solve, cap)
        return time.perf_counter() - t0
    run(1)
    short, long_ = min(run(1) for _ in range(3)), min(run(1 + iters) for _ in range(3))
    return 1e3 * (long_ - short) / iters


def count_calls(ctx, solve, iters):
    calls, lib_call = {"n": 0}, ctx.lib.call

    def counting(name, *a):
        calls["n"] += 1
        return lib_call(name, *a)
    ctx.lib.call = counting
    try:
        quiet(solve, 1)
        short = calls["n"]
        calls["n"] = 0
        quiet(solve, 1 + iters)
        return (calls["n"] - short) / iters
    finally:
        del ctx.lib.call


WINDOW_S = 0.3


def alternating(fa, fb, ctx, reps):
    """(seconds per call of fa, of fb, calls per window): --reps windows each, alternating; a window is as many back-to-back
    calls as fill WINDOW_S (sized by one timed call after the warm-up), one synchronisation at its end, host clock around it.
    Launch and synchronisation overhead is inside the window: these are host-timed calls, not kernel times."""
    def window(f, n):
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        ctx.sync()
        return (time.perf_counter() - t0) / n
    fa(), fb()
    ctx.sync()
    inner = max(1, int(np.ceil(WINDOW_S / max(window(fa, 1), window(fb, 1)))))
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(fa, inner))
        tb.append(window(fb, inner))
    return ta, tb, inner


def run(ctx, nel, cutoff, iters, reps, parts):
    m = UEG(nel, nel // 2, nel // 2, 1.0)
    m.init_single_basis(cutoff)
    tab = m.sector_tables()
    tt = TriplesTables(tab)
    no = tab.no
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    out = {"nel": nel, "cutoff": cutoff, "plane_waves": tab.n, "no": no, "nv": tab.nv, "nnz": tab.nnz}
    ints = quiet(m.eval_2b_sectors, tab, ctx=ctx)
    eps = ints.hf_orbital_energies(kin)
    res = quiet(SectorCCD(no, is_dcd=True, delta_e=1e-7).solve, eps, ints)
    T = res["t2 amp"]
    if "iteration" in parts:
        for name, is_dcd in (("ccd", False), ("dcd", True)):
            amp = lambda cap: SectorCCD(no, is_dcd=is_dcd, delta_e=0.0).solve(eps, ints, max_iter=cap)
            lam = lambda cap: SectorLambda(no, 0.0, is_dcd=is_dcd).solve(eps, ints, T, max_iter=cap)
            a, b = per_iteration(amp, iters), per_iteration(lam, iters)
            out[name] = {"amplitude_ms_per_iteration": round(a, 4), "lambda_ms_per_iteration": round(b, 4),
                         "ratio": round(b / a, 3), "amplitude_calls_per_iteration": count_calls(ctx, amp, iters),
                         "lambda_calls_per_iteration": count_calls(ctx, lam, iters)}
    if "ladder" in parts:
        dt = ints.device_tables()
        at = dt.adjoint()
        x, y = ctx.array(np.random.default_rng(0).standard_normal(tab.nnz)), ctx.zeros((tab.nnz,))
        tf, ta, inner = alternating(lambda: dt.ladder.run(ints["abcd"], x, y), lambda: at.ladder_t.run(ints["abcd"], x, y), ctx, reps)
        nbytes = 8 * ints.sizes["abcd"]
        out["ladder"] = {"abcd_bytes": nbytes, "tiles": dt.ladder.tiles, "launches_per_window": inner,
                         "forward_ms": round(1e3 * statistics.median(tf), 4), "adjoint_ms": round(1e3 * statistics.median(ta), 4),
                         "forward_bytes_per_s": nbytes / statistics.median(tf), "adjoint_bytes_per_s": nbytes / statistics.median(ta),
                         "forward_fraction_of_hbm": round(nbytes / statistics.median(tf) / HBM_BYTES_PER_S, 4),
                         "adjoint_fraction_of_hbm": round(nbytes / statistics.median(ta) / HBM_BYTES_PER_S, 4),
                         "forward_ms_all": [round(1e3 * t, 4) for t in tf], "adjoint_ms_all": [round(1e3 * t, 4) for t in ta]}
    if "triples" in parts:
        tints = quiet(m.eval_2b_triples, tt, ctx=ctx, both_sides=True)
        lam = quiet(SectorLambda(no, 1e-7, is_dcd=True).solve, eps, ints, T)["lambda2"]
        got = {}

        def plain():
            got["t"] = sector_triples_energy(eps, ints, tints, T)

        def left():
            got["l"] = sector_lambda_triples_energy(eps, ints, tints, T, lam)
        tp, tl, inner = alternating(plain, left, ctx, reps)
        out["triples"] = {"t_s": round(statistics.median(tp), 4), "lambda_t_s": round(statistics.median(tl), 4),
                          "ratio": round(statistics.median(tl) / statistics.median(tp), 3), "t_s_all": [round(t, 4) for t in tp],
                          "lambda_t_s_all": [round(t, 4) for t in tl], "e_t": got["t"], "e_lambda_t": got["l"], "calls_per_window": inner,
                          "triples_per_batch": (1 << 30) // lambda_triple_bytes(tab.nv), "triples_integral_bytes": tints.nbytes,
                          "note": "Coulomb integrals, DCD amplitudes and their Lambda: E_Lambda(T) differs from E(T) because "
                                  "lambda2 of DCD is not 2 T - T^x"}
        for arr in (tints.Vv, tints.Vo, tints.VvR, tints.VoR):
            arr.free()
    ints.arena.free()
    if "tc" in parts:
        t0 = time.perf_counter()
        v2 = quiet(m.eval_2b_sectors, tab, correlator=m.trunc, is_only_2b=True, ctx=ctx)
        eps = v2.hf_orbital_energies(kin) + quiet(m.double_contractions_in_3_body)
        eff = quiet(m.eval_2b_sectors, tab, correlator=m.trunc, is_effect_2b=True, ctx=ctx)
        tc = v2 + eff
        v2.arena.free(), eff.arena.free()
        a = quiet(m.eval_2b_triples, tt, correlator=m.trunc, is_only_2b=True, ctx=ctx, both_sides=True)
        b = quiet(m.eval_2b_triples, tt, correlator=m.trunc, is_effect_2b=True, ctx=ctx, both_sides=True)
        tints = a + b
        ctx.sync()
        t_build = time.perf_counter() - t0
        t0 = time.perf_counter()
        solver = SectorCCD(no, is_dcd=True, delta_e=1e-9)
        res = quiet(solver.solve, eps, tc, lambda_triples=tints, max_iter=100, lambda_threshold=1e-8)
        t_solve = time.perf_counter() - t0
        lam = SectorLambda(no, 1e-8, is_dcd=True)
        left = quiet(lam.solve, eps, tc, res["t2 amp"], lam=res["lambda2"])
        out["tc"] = {"k_cutoff": m.k_cutoff, "integral_build_s": round(t_build, 3), "sector_integral_bytes": tc.nbytes,
                     "triples_integral_bytes": tints.nbytes, "largest_other_array_bytes": 8 * max(tab.nnz, tc.device_tables().nsq),
                     "dcd_energy": res["ccd e"], "dcd_iterations": solver.iterations, "lambda_residual": left["lambda residual"],
                     "lambda_t_energy": res["lambda (t) e"], "dcd_t_lambda_energy": res["ccd(t)_lambda e"],
                     "solve_lambda_and_triples_s": round(t_solve, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="iteration,ladder,triples,tc")
    ap.add_argument("--nel", default="14,54")
    ap.add_argument("--cutoff", type=int, default=60)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sector_lambda", "probe_sector_lambda.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for nel in (int(x) for x in args.nel.split(",")):
        ctx = Context(1, 1, device=0)
        try:
            line = json.dumps(run(ctx, nel, args.cutoff, args.iters, args.reps, args.part.split(",")))
        finally:
            ctx.close()
        print(line, flush=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
