#!/usr/bin/env python3
"""GPU probe of the sector IP- / EA-EOM-CCD (pymes_amd/solver/ueg_eom.py).  Prints JSON lines and appends them to
profiles/sector_ipea/probe_sector_ipea.txt, one line per --nel at --cutoff (default 60: 1 935 plane waves), DCD amplitudes, the
targets of the k_F shells (the highest occupied and the lowest virtual orbital) and the k = 0 orbital:
  timing   (Coulomb) the hoist (a SectorIPEAHoist constructor, shared by both kinds), the per-target prepare, one IP and one EA
           apply at k = 1 and k = 4, the EA ladder launch alone as bytes of V_abcd read per second, a one-root solve per kind -- each a median of
           --reps windows, alternating with one SectorCCD.residual on the same integrals (the yardstick); a window is as many
           back-to-back calls as fill 0.3 s with one synchronisation at the end: host clocks around synchronised work, so launch
           overhead is inside every figure;
  physics  Coulomb and transcorrelated (only_2b + effect_2b, trunc): the quasi-particle gap at k_F, the occupied band width from
           the root of the k = 0 block with the largest singles weight (a one-root and a three-root solve), and the singles weights.
    python3 tools/probe_sector_ipea.py [--nel 14,54] [--cutoff 60] [--reps 3] [--part timing,physics] [--modes coulomb,tc]"""
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
from pymes_amd.solver.ueg_cc import SectorCCD  # noqa: E402
from pymes_amd.solver.ueg_eom import SectorEA_EOM_CCD, SectorIP_EOM_CCD, SectorIPEAHoist, SectorIPEASigma  # noqa: E402

WINDOW_S = 0.3


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def alternating(f, yard, ctx, reps):
    """(median ms per call of f, of the yardstick, all windows of f): --reps windows each, alternating."""
    def window(g, n):
        t0 = time.perf_counter()
        for _ in range(n):
            g()
        ctx.sync()
        return (time.perf_counter() - t0) / n
    f(), yard()
    ctx.sync()
    nf, ny = (max(1, int(np.ceil(WINDOW_S / max(window(g, 1), 1e-6)))) for g in (f, yard))
    tf, ty = [], []
    for _ in range(reps):
        tf.append(window(f, nf))
        ty.append(window(yard, ny))
    return {"ms": round(1e3 * statistics.median(tf), 4), "yardstick_ms": round(1e3 * statistics.median(ty), 4),
            "ms_all": [round(1e3 * t, 4) for t in tf], "calls_per_window": nf}


def hamiltonian(m, tab, tt, ctx, mode, ea_targets):
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    if mode == "coulomb":
        ints = quiet(m.eval_2b_sectors, tab, ctx=ctx)
        eps = ints.hf_orbital_energies(kin)
        tints = quiet(m.eval_2b_triples, tt, ctx=ctx, both_sides=True)
        lad = quiet(m.eval_2b_ladder, tt, ea_targets, ctx=ctx)
        return eps, ints, tints, lad
    parts = [dict(correlator=m.trunc, is_only_2b=True), dict(correlator=m.trunc, is_effect_2b=True)]
    v2, eff = (quiet(m.eval_2b_sectors, tab, ctx=ctx, **p) for p in parts)
    eps = v2.hf_orbital_energies(kin) + quiet(m.double_contractions_in_3_body)
    ints = v2 + eff
    v2.arena.free(), eff.arena.free()
    a, b = (quiet(m.eval_2b_triples, tt, ctx=ctx, both_sides=True, **p) for p in parts)
    la, lb = (quiet(m.eval_2b_ladder, tt, ea_targets, ctx=ctx, **p) for p in parts)
    return eps, ints, a + b, la + lb


def physics(no, eps, ints, tints, lad, amps, homo, lumo, zero):
    ip = quiet(SectorIP_EOM_CCD(no, n_roots=1, r_epsilon=1e-7).solve, eps, ints, tints, amps, [homo])
    ea = quiet(SectorEA_EOM_CCD(no, n_roots=1, r_epsilon=1e-7).solve, eps, ints, tints, amps, [lumo], ladders=lad)
    # the deep hole lies in the 2h1p continuum.  One root: the lowest of the Krylov space of the singles vector alone, which
    # states without singles weight cannot enter.  Three roots: the start vectors on the smallest d2 bring such states in (they
    # are the lowest of the block); if the Ritz vectors of a collapse come out dependent, only the one-root solve is reported.
    one = quiet(SectorIP_EOM_CCD(no, n_roots=1, r_epsilon=1e-7, max_iter=200, max_dim=60).solve, eps, ints, tints, amps, [zero])
    try:
        deep = quiet(SectorIP_EOM_CCD(no, n_roots=3, r_epsilon=1e-7, max_iter=200, max_dim=60).solve, eps, ints, tints, amps, [zero])
    except np.linalg.LinAlgError:
        deep = one
    if one["singles weight"][0].max() >= deep["singles weight"][0].max():
        best_e, best_w = float(one["ip e"][0, 0]), float(one["singles weight"][0, 0])
    else:
        qp = int(np.argmax(deep["singles weight"][0]))
        best_e, best_w = float(deep["ip e"][0, qp]), float(deep["singles weight"][0, qp])
    return {"ip_kF": float(ip["ip e"][0, 0]), "ea_kF": float(ea["ea e"][0, 0]), "qp_gap": float(ip["ip e"][0, 0] + ea["ea e"][0, 0]),
            "hf_gap": float(eps[lumo] - eps[homo]), "ip_kF_singles_weight": float(ip["singles weight"][0, 0]),
            "ea_kF_singles_weight": float(ea["singles weight"][0, 0]), "ip_k0_roots": [float(x) for x in deep["ip e"][0]],
            "ip_k0_singles_weights": [float(x) for x in deep["singles weight"][0]], "ip_k0_converged": bool(deep["converged"][0]),
            "ip_k0_one_root": float(one["ip e"][0, 0]),
            "ip_k0_one_root_singles_weight": float(one["singles weight"][0, 0]), "ip_k0_one_root_converged": bool(one["converged"][0]),
            "ip_k0_one_root_passes": int(one["passes"][0]), "band_width": best_e - float(ip["ip e"][0, 0]),
            "band_width_root_singles_weight": best_w, "hf_band_width": float(eps[homo] - eps[zero]),
            "passes": [int(ip["passes"][0]), int(ea["passes"][0]), int(deep["passes"][0])]}


def run(ctx, nel, cutoff, reps, parts, modes=("coulomb", "tc")):
    m = UEG(nel, nel // 2, nel // 2, 1.0)
    m.init_single_basis(cutoff)
    tab = m.sector_tables()
    tt = TriplesTables(tab)
    no = tab.no
    zero = int(np.flatnonzero((tab.k_int == 0).all(axis=1))[0])
    homo, lumo = no - 1, no
    out = {"nel": nel, "cutoff": cutoff, "plane_waves": tab.n, "no": no, "nv": tab.nv, "nnz": tab.nnz,
           "targets": {"k0": zero, "homo": homo, "lumo": lumo}}
    for mode in modes:
        if mode == "tc" and "physics" not in parts:
            continue
        t0 = time.perf_counter()
        eps, ints, tints, lad = hamiltonian(m, tab, tt, ctx, mode, [lumo])
        ctx.sync()
        rec = out[mode] = {"integral_build_s": round(time.perf_counter() - t0, 2), "sector_integral_bytes": ints.nbytes,
                           "triples_integral_bytes": tints.nbytes, "ladder_integral_bytes": lad.nbytes}
        solver = SectorCCD(no, is_dcd=True, delta_e=1e-9)
        amps = quiet(solver.solve, eps, ints, max_iter=100)["t2 amp"]
        rec["dcd_iterations"] = solver.iterations
        if "physics" in parts:
            rec["physics"] = physics(no, eps, ints, tints, lad, amps, homo, lumo, zero)
        if "timing" in parts and mode == "coulomb":
            T, R = amps.vector, ctx.empty((tab.nnz,))
            ccd = SectorCCD(no, is_dcd=True)
            ws, eps_dev = ccd.workspace(ints), ctx.array(eps)
            yard = lambda: ccd.residual(ints, eps_dev, T, R, ws)
            tim = rec["timing"] = {}

            def hoist():
                SectorIPEAHoist(eps, ints, tints, amps).close()
            tim["hoist"] = alternating(hoist, yard, ctx, reps)
            for kind, p, ladders in (("ip", homo, None), ("ea", lumo, lad)):
                sig = SectorIPEASigma(kind, eps, ints, tints, amps, ladders=ladders)

                def prepare():
                    sig.forget(p)
                    sig.tables_of(p)
                tim[kind + " prepare"] = alternating(prepare, yard, ctx, reps)
                qt, lay = sig.tables_of(p), sig.layout(p)
                tim[kind + " dimension"] = qt.dim
                rng = np.random.default_rng(0)
                for k in (1, 4):
                    vecs = []
                    for _ in range(k):
                        v = ctx.zeros((lay.nflat,))
                        lay.part1(v).set(rng.standard_normal(1))
                        lay.part2(v).set(rng.standard_normal(qt.shape) * qt.inside.reshape(qt.shape))
                        vecs.append(v)
                    outs = [lay.padded() for _ in vecs]
                    a1, a2, o1, o2 = ([f(x) for x in xs] for xs, f in ((vecs, lay.part1), (vecs, lay.part2), (outs, lay.part1),
                                                                       (outs, lay.part2)))
                    apply = lambda: sig.apply_many(p, a1, a2, out1=o1, out2=o2)
                    tim["%s apply k=%d" % (kind, k)] = alternating(apply, yard, ctx, reps)
                    if kind == "ea" and k == 1:
                        tg = sig._target(p)
                        tasks = sig._work(tg, 1)[0]
                        x, y = ctx.zeros((max(qt.count, 1),)), ctx.zeros((max(qt.count, 1),))
                        stored = 8 * int((qt.pair_len[qt.pair_sec >= 0] ** 2).sum())
                        extra = 8 * qt.extra_size
                        if stored:
                            t = alternating(lambda: tasks["ladder"].run(ints["abcd"], x, y), yard, ctx, reps)
                            t.update(bytes=stored, bytes_per_s=stored / (1e-3 * t["ms"]), tiles=tasks["ladder"].tiles)
                            tim["ea ladder stored sectors"] = t
                        if extra:
                            t = alternating(lambda: tasks["ladder_extra"].run(tg.extra, x, y), yard, ctx, reps)
                            t.update(bytes=extra, bytes_per_s=extra / (1e-3 * t["ms"]), tiles=tasks["ladder_extra"].tiles)
                            tim["ea ladder extra family"] = t
                cls = SectorIP_EOM_CCD if kind == "ip" else SectorEA_EOM_CCD
                solve = lambda: quiet(cls(no, n_roots=1).solve, eps, ints, tints, amps, [p], ladders=ladders)
                tim[kind + " solve"] = alternating(solve, yard, ctx, reps)
                tim[kind + " solve"]["passes"] = int(solve()["passes"][0])
                sig.close()
        ints.arena.free()
        for arr in (tints.Vv, tints.Vo, tints.VvR, tints.VoR):
            arr.free()
        for arr in lad.arenas.values():
            arr.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="timing,physics")
    ap.add_argument("--nel", default="14,54")
    ap.add_argument("--cutoff", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="coulomb,tc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sector_ipea", "probe_sector_ipea.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for nel in (int(x) for x in args.nel.split(",")):
        ctx = Context(1, 1, device=0)
        try:
            line = json.dumps(run(ctx, nel, args.cutoff, args.reps, args.part.split(","), args.modes.split(",")))
        finally:
            ctx.close()
        print(line, flush=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
