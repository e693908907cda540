#!/usr/bin/env python3
"""GPU probe of the sector spectral functions (pymes_amd/solver/ueg_eom.py, SectorSpectralFunction).  Prints JSON
lines and appends them to profiles/sector_gf/probe_sector_gf.txt, one line per --nel at --cutoff (default 60: 1 935 plane waves),
Coulomb integrals, DCD amplitudes and their Lambda; the targets are the k_F orbitals (the highest occupied for IP, the lowest
virtual for EA) and the k = 0 hole:
  timing   on the Krylov basis of a real run, at j = 50 and j = 200 where the block is that large: one apply alone, the fused step
           (pymes_sector_arnoldi_step) alone and with its apply, the step's time against its mandatory traffic 2 (j + 1) len
           doubles at 6.3 TB/s, and the host route on the same basis (ctx.gram + lincomb_multi twice, norm, scale) -- medians of
           --reps windows of 0.3 s of back-to-back calls with one synchronisation, the fused step and the host route alternating,
           everything else alternating with one SectorCCD.residual (host clocks: launch overhead is inside every figure);
  physics  A(k, w) at k = 0 and k_F, Z_kF from both sides next to the jump of n(k) / 2 at k_F, the occupied band width from the
           peak of A(0, w), and m, eta and the largest residual of each run.
    python3 tools/probe_sector_gf.py [--nel 14,54] [--cutoff 60] [--reps 3] [--part timing,physics] [--eta 0.02] [--max-dim 256]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from probe_sector_ipea import alternating, hamiltonian, quiet  # noqa: E402
from pymes_amd.device import Context  # noqa: E402
from pymes_amd.model.ueg import UEG  # noqa: E402
from pymes_amd.solver import subspace  # noqa: E402
from pymes_amd.solver.sectors import TriplesTables  # noqa: E402
from pymes_amd.solver.ueg_cc import SectorCCD  # noqa: E402
from pymes_amd.solver.ueg_eom import (SectorIPEASigma, SectorSpectralFunction, arnoldi_step,  # noqa: E402
                                      arnoldi_workspace)

HBM_BYTES_PER_S = 6.3e12


def host_route(ctx, rows, w):
    """CGS2 of w against the rows through the host: two Gram products and two combinations, the norm, the scaling."""
    for _ in range(2):
        h = ctx.gram(rows, [w])
        ctx.lincomb_multi([w], rows, -h, beta=[1.0])
    nrm = np.sqrt(ctx.gram([w], [w])[0, 0])
    ctx.lincomb_multi([w], [], np.zeros((0, 1)), beta=[1.0 / max(nrm, 1e-300)])


def timing(ctx, sig, kind, p, kept, yard, reps):
    lay, out = sig.layout(p), {}
    rows = kept.rows(p)
    k = len(rows) - 1
    t = kept._targets[p]
    length, pitch = lay.nflat, t.pitch
    out["dimension"], out["vector_length"], out["krylov_dim"] = sig.tables_of(p).dim, length, k
    for j in (50, 200):
        if j + 1 > k:
            continue
        # a copy of the rows 0..j+1, so that the kept basis stays what the run left
        basis = ctx.empty(((j + 2) * pitch,))
        subspace.view(ctx, basis, 0, ((j + 2) * pitch,)).copy_from(subspace.view(ctx, t.basis, 0, ((j + 2) * pitch,)))
        mine = [subspace.view(ctx, basis, i * pitch, (length,)) for i in range(j + 2)]
        hess, flag = ctx.zeros(((j + 2) * (j + 1),)), ctx.zeros((1,))
        ws = ctx.empty((arnoldi_workspace(ctx, length, j),))
        src, dst = mine[j], mine[j + 1]
        apply = lambda: sig.apply_many(p, [lay.part1(src)], [lay.part2(src)], out1=[lay.part1(dst)], out2=[lay.part2(dst)])
        step = lambda: arnoldi_step(ctx, basis, pitch, length, j, hess, j + 1, 1e-10, ws, flag)
        both = lambda: (apply(), step())
        host = lambda: host_route(ctx, mine[:j + 1], dst)
        rec = out["j=%d" % j] = {"apply": alternating(apply, yard, ctx, reps), "step": alternating(step, yard, ctx, reps),
                                 "apply+step": alternating(both, yard, ctx, reps)}
        ab = alternating(step, host, ctx, reps)                      # the fused step against the host route, alternating
        rec["fused_ms"], rec["host_route_ms"] = ab["ms"], ab["yardstick_ms"]
        traffic = 16.0 * (j + 1) * length
        rec["mandatory_bytes"], rec["mandatory_us_at_6.3TB/s"] = traffic, round(1e6 * traffic / HBM_BYTES_PER_S, 3)
        rec["step_over_mandatory"] = round(1e-3 * rec["step"]["ms"] / (traffic / HBM_BYTES_PER_S), 1)
        for arr in (basis, hess, flag, ws):
            arr.free()
    return out


def run(ctx, nel, cutoff, reps, parts, eta, max_dim):
    m = UEG(nel, nel // 2, nel // 2, 1.0)
    m.init_single_basis(cutoff)
    tab = m.sector_tables()
    tt = TriplesTables(tab)
    no = tab.no
    zero = int(np.flatnonzero((tab.k_int == 0).all(axis=1))[0])
    homo, lumo = no - 1, no
    out = {"nel": nel, "cutoff": cutoff, "plane_waves": tab.n, "no": no, "nv": tab.nv, "eta": eta, "max_dim": max_dim,
           "targets": {"k0": zero, "homo": homo, "lumo": lumo}}
    eps, ints, tints, lad = hamiltonian(m, tab, tt, ctx, "coulomb", [lumo])
    solver = SectorCCD(no, is_dcd=True, delta_e=1e-9)
    res = quiet(solver.solve, eps, ints, max_iter=100, density=True)
    amps, dens, nk = res["t2 amp"], res["density"], res["n(k)"]
    out["n(k)/2"] = {"k0": 0.5 * nk[zero], "homo": 0.5 * nk[homo], "lumo": 0.5 * nk[lumo], "jump": 0.5 * (nk[homo] - nk[lumo])}
    if "physics" in parts:
        lo, hi = eps[zero] - 1.0, eps[lumo] + 1.0
        omegas = np.linspace(lo, hi, 801)
        sf = SectorSpectralFunction(no, max_dim=max_dim, r_epsilon=1e-6, check_every=32)
        got = quiet(sf.solve, eps, ints, tints, amps, dens, omegas, eta, ip=[homo, zero], ea=[lumo], ladders=lad)
        phys = out["physics"] = {"omega_lo": lo, "omega_hi": hi, "points": len(omegas)}
        for K, n, name in (("ip", 0, "homo"), ("ip", 1, "k0"), ("ea", 0, "lumo")):
            A = got[K + " A"][n]
            strong = np.argsort(-np.abs(got[K + " pole strengths"][n]))[:4]
            phys[name] = {"krylov_dim": int(got[K + " krylov dim"][n]), "breakdown": bool(got[K + " breakdown"][n]),
                          "converged": bool(got[K + " converged"][n]), "largest_residual": float(got[K + " residuals"][n].max()),
                          "norm": float(got[K + " norm"][n]), "qp_e": float(got[K + " qp e"][n]), "qp_z": float(got[K + " qp z"][n]),
                          "peak_omega": float(omegas[np.argmax(A)]), "peak_A": float(A.max()),
                          "integral_of_A": float(np.sum(0.5 * (A[1:] + A[:-1]) * np.diff(omegas))),
                          "strongest_poles": [[round(float(got[K + " poles"][n][s].real), 6),
                                               round(float(got[K + " pole strengths"][n][s].real), 6),
                                               float("%.1e" % got[K + " pole residuals"][n][s])] for s in strong],
                          "A": [round(float(a), 5) for a in A[::4]]}
        phys["Z_kF"] = {"hole_side": phys["homo"]["qp_z"], "particle_side": phys["lumo"]["qp_z"], "jump_of_n(k)/2": out["n(k)/2"]["jump"]}
        phys["band_width_from_peak_of_A(0,w)"] = phys["homo"]["peak_omega"] - phys["k0"]["peak_omega"]
        phys["hf_band_width"] = float(eps[homo] - eps[zero])
    if "timing" in parts:
        T, R = amps.vector, ctx.empty((tab.nnz,))
        ccd = SectorCCD(no, is_dcd=True)
        ws, eps_dev = ccd.workspace(ints), ctx.array(eps)
        yard = lambda: ccd.residual(ints, eps_dev, T, R, ws)
        tim = out["timing"] = {}
        for kind, p, ladders in (("ip", homo, None), ("ip", zero, None), ("ea", lumo, lad)):
            run_ = quiet(SectorSpectralFunction(no, max_dim=208, r_epsilon=0.0).solve, eps, ints, tints, amps, dens, [0.0], eta,
                         keep_basis=True, ladders=ladders, **{kind: [p]})
            kept = run_[kind + " basis"]
            sig = SectorIPEASigma(kind, eps, ints, tints, amps, ladders=ladders)
            try:
                tim["%s target %d" % (kind, p)] = timing(ctx, sig, kind, p, kept, yard, reps)
            finally:
                sig.close()
                kept.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="timing,physics")
    ap.add_argument("--nel", default="14,54")
    ap.add_argument("--cutoff", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eta", type=float, default=0.02)
    ap.add_argument("--max-dim", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sector_gf", "probe_sector_gf.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for nel in (int(x) for x in args.nel.split(",")):
        ctx = Context(1, 1, device=0)
        try:
            line = json.dumps(run(ctx, nel, args.cutoff, args.reps, args.part.split(","), args.eta, args.max_dim))
        finally:
            ctx.close()
        print(line, flush=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
