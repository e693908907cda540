#!/usr/bin/env python3
"""GPU probe of the momentum-blocked (T) (pymes_amd/solver/ueg_cc.py, sector_triples_energy).  Prints JSON lines
and appends them to profiles/sector_triples/probe_sector_triples.txt:
  small   N = 14 at cutoff 8 (93 plane waves): the sector (T) next to the dense ``get_triples_energy`` on the same converged
          DCD amplitudes (host clock around calls that end in a synchronisation, median of --reps);
  big     a basis no dense (T) can hold (--nel 14 and 54 at --cutoff 60: 1 935 plane waves): table and integral build
          times, bytes held, the time of the whole (T) call, and the traffic its two kernels must move at the least --
          per triple the distinct Vv slabs read, Wt written once and read once -- over that time, against the 6.3 TB/s this
          project uses for HBM;
  trace   the workload only (one batch of triples, three times), for a kernel trace of its own:
          rocprofv3 --kernel-trace --stats -- python3 tools/probe_sector_triples.py --part trace --nel 54
    python3 tools/probe_sector_triples.py [--part small,big] [--nel 14,54] [--cutoff 60] [--reps 3]"""
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
from pymes_amd.solver import ccsd_t  # noqa: E402
from pymes_amd.solver.sectors import TriplesTables  # noqa: E402
from pymes_amd.solver.ueg_cc import SectorCCD, sector_triples_energy, triple_bytes  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    out = fn(*a, **k)
    return out, time.perf_counter() - t0


def problem(ctx, nel, cutoff):
    m = UEG(nel, nel // 2, nel // 2, 1.0)
    m.init_single_basis(cutoff)
    tab, t_tab = timed(m.sector_tables)
    tt, t_tt = timed(TriplesTables, tab)
    ints = quiet(m.eval_2b_sectors, tab, ctx=ctx)
    ctx.sync()
    t0 = time.perf_counter()
    tints = quiet(m.eval_2b_triples, tt, ctx=ctx)
    ctx.sync()
    t_int = time.perf_counter() - t0
    kin = np.array([b.kinetic for b in m.basis_fns[::2]])
    return m, tab, tt, ints, tints, ints.hf_orbital_energies(kin), {"sector_tables_s": round(t_tab, 3),
                                                                    "triples_tables_s": round(t_tt, 3),
                                                                    "triples_integral_build_s": round(t_int, 3)}


def least_bytes(no, nv, lo, hi):
    """What the W and energy kernels must move for the triples [lo, hi): the distinct Vv slabs of (i,j,k), Wt out and in."""
    total = 0
    t = 0
    for i in range(no):
        for j in range(i + 1):
            for k in range(j + 1):
                if lo <= t < hi:
                    total += (len({i, j, k}) + 2) * 8 * nv * nv
                t += 1
    return total


def part_small(ctx, reps):
    m, tab, tt, ints, tints, eps, times = problem(ctx, 14, 8)
    res = quiet(SectorCCD(7, is_dcd=True, delta_e=1e-9).solve, eps, ints)
    amps = res["t2 amp"]
    V = quiet(m.eval_2b_integrals)
    t2 = amps.to_dense()
    sector_triples_energy(eps, ints, tints, amps)
    ccsd_t.get_triples_energy(7, np.diag(eps), V, None, t2)
    ts, td = [], []
    for _ in range(reps):
        (e_s, dt) = timed(sector_triples_energy, eps, ints, tints, amps)
        ts.append(dt)
        (e_d, dt) = timed(ccsd_t.get_triples_energy, 7, np.diag(eps), V, None, t2)
        td.append(dt)
    return [dict(times, part="small", nel=14, cutoff=8, plane_waves=tab.n, triples=ccsd_t.n_triples(7),
                 sector_t_ms=round(1e3 * statistics.median(ts), 3), dense_t_ms=round(1e3 * statistics.median(td), 3),
                 e_t_sector=e_s, e_t_dense=e_d, triples_integral_bytes=tints.nbytes, dense_V_bytes=8 * tab.n ** 4,
                 note="whole calls: the sector one uploads eps and the amplitudes and checks V_klcd = V_cdkl on the host; the "
                      "dense one uploads the [n]^4 integrals (0.6 GB) and the dense amplitudes")]


def part_big(ctx, nel, cutoff, reps):
    m, tab, tt, ints, tints, eps, times = problem(ctx, nel, cutoff)
    no, nv = tab.no, tab.nv
    res = quiet(SectorCCD(no, is_dcd=True, delta_e=1e-7).solve, eps, ints)
    amps = res["t2 amp"]
    n = ccsd_t.n_triples(no)
    sector_triples_energy(eps, ints, tints, amps, triple_range=(0, min(n, 4)))            # warm-up: code objects, tables
    ts = []
    for _ in range(reps):
        (e_t, dt) = timed(sector_triples_energy, eps, ints, tints, amps)
        ts.append(dt)
    t = statistics.median(ts)
    need = least_bytes(no, nv, 0, n)
    return [dict(times, part="big", nel=nel, cutoff=cutoff, plane_waves=tab.n, no=no, nv=nv, triples=n,
                 triples_integral_bytes=tints.nbytes, sector_integral_bytes=ints.nbytes, workspace_bytes=1 << 30,
                 triples_per_batch=(1 << 30) // triple_bytes(nv), dense_V_bytes=8 * tab.n ** 4, dcd_energy=res["ccd e"],
                 e_t=e_t, dcd_t_energy=res["ccd e"] + e_t, t_call_s=round(t, 4), t_call_s_all=[round(x, 4) for x in ts],
                 least_bytes=need, least_s_at_hbm=round(need / HBM_BYTES_PER_S, 5),
                 fraction_of_hbm_yardstick=round(need / HBM_BYTES_PER_S / t, 4))]


def part_trace(ctx, nel, cutoff):
    m, tab, tt, ints, tints, eps, _ = problem(ctx, nel, cutoff)
    rng = np.random.default_rng(0)
    T = rng.standard_normal(tab.nnz) * 0.01
    T = 0.5 * (T + T[tab.pp_swap])
    n = min(ccsd_t.n_triples(tab.no), (1 << 30) // triple_bytes(tab.nv))
    lo = ccsd_t.n_triples(tab.no) - n                                                      # the last batch: i > j > k mostly
    for _ in range(3):
        e = sector_triples_energy(eps, ints, tints, T, triple_range=(lo, lo + n))
    return [{"part": "trace", "nel": nel, "cutoff": cutoff, "nv": tab.nv, "triples_in_the_batch": n, "first_triple": lo,
             "least_bytes": least_bytes(tab.no, tab.nv, lo, lo + n), "e": e}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="small,big")
    ap.add_argument("--nel", default="14,54")
    ap.add_argument("--cutoff", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sector_triples", "probe_sector_triples.txt"))
    args = ap.parse_args()
    ctx = Context(1, 1, device=0)
    lines = []
    try:
        if "small" in args.part:
            lines += part_small(ctx, args.reps)
        for nel in (int(x) for x in args.nel.split(",")):
            if "big" in args.part:
                lines += part_big(ctx, nel, args.cutoff, args.reps)
            if "trace" in args.part:
                lines += part_trace(ctx, nel, args.cutoff)
    finally:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as fh:
            for ln in lines:
                print(json.dumps(ln))
                fh.write(json.dumps(ln) + "\n")
        ctx.close()


if __name__ == "__main__":
    main()
