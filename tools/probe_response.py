"""EOM-CCSD linear response on the synthetic factors (pymes_amd/model/synthetic.py): CCSD with device amplitudes, then on ONE
handle of the sigma build
  * one sweep of 12 complex systems (three operators, two frequencies, +z and -z; 24 stacked vectors) against the stacked
    ``apply_many`` of the same 24 vectors alone — same vectors, same handle, same process, so the ratio is that of one visit to one
    device — with the HBM bound of the sweep's own passes next to it,
  * ``pymes_response_vectors`` for the three operators,
  * a dipole-like solve (three operators, one static and one damped frequency) and its sweep count.
Times are host wall clock around a device synchronisation, best of --repeat.
Usage: python tools/probe_response.py [--sizes 30x120,50x200] [--out profiles/response/probe_response.txt]"""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymes_amd import _lib  # noqa: E402
from pymes_amd.integral.device import DeviceIntegrals  # noqa: E402
from pymes_amd.model import synthetic  # noqa: E402
from pymes_amd.solver import response as M  # noqa: E402
from pymes_amd.solver import subspace  # noqa: E402
from pymes_amd.solver.ccsd import CCSD  # noqa: E402
from pymes_amd.solver.lambda_ccsd import LeftSigma  # noqa: E402

HBM_BYTES_PER_S = 6.3e12      # the HBM rate a streaming copy reaches on one MI355X (8 TB/s peak): what the bound is computed with


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return time.perf_counter() - t0


def probe(no, nv, repeat, history, r_epsilon, emit):
    import ctypes as C
    B, eps = synthetic.factors(no, nv, seed=0)
    f = np.diag(eps)
    gap = float(eps[no] - eps[no - 1])
    ints = DeviceIntegrals.from_factors(no, B)
    ctx = ints.ctx
    try:
        cc = CCSD(no, delta_e=1e-8)
        res = quiet(cc.solve, f, ints, device_amplitudes=True)
        fd = quiet(cc.get_T1_dressed_fock, f, res["t1"], ints)
        dressed = quiet(cc.get_T1_dressed_V, res["t1"], ints, M.EOM_CCSD_Response.BLOCKS)
        emit("(%d,%d): E_CCSD = %.10f, HF gap %.4f" % (no, nv, res["ccsd e"], gap))
        n = no + nv
        rng = np.random.default_rng(1)
        ops = rng.standard_normal((3, n, n))
        ops = ops + ops.transpose(0, 2, 1)
        lam2 = 0.01 * rng.standard_normal((nv, nv, no, no))
        lam = (ctx.array(0.01 * rng.standard_normal((nv, no))), ctx.array(lam2 + lam2.transpose(1, 0, 3, 2)))
        # ---- the property vectors ------------------------------------------------------------------------------------------------
        lay = subspace.FlatLayout(ctx, (nv, no), (nv, nv, no, no))
        xi, eta = [lay.padded() for _ in range(3)], [lay.padded() for _ in range(3)]
        out = ([lay.part1(x) for x in xi], [lay.part2(x) for x in xi], [lay.part1(x) for x in eta], [lay.part2(x) for x in eta])
        vectors = lambda: M.device_response_vectors(ctx, res["t1"], res["t2"], lam[0], lam[1], ops, out=out)
        vectors()
        emit("  property vectors of 3 operators (pymes_response_vectors): %.3f ms" % (
            1e3 * min(timed(ctx, vectors) for _ in range(repeat))))
        # ---- one sweep of 12 complex systems against the stacked apply of its 24 vectors -----------------------------------------
        sig = LeftSigma(ctx, fd, res["t2"], dressed=True)
        d = ctx.zeros((lay.nflat,))
        ctx.lib.call("pymes_eom_diagonals", ctx.handle, _lib.host_ptr(np.ascontiguousarray(fd)), C.c_void_p(sig.T.ptr), 1,
                     C.c_void_p(d.ptr), C.c_void_p(d.ptr + 8 * lay.off2))
        s = M.EOM_CCSD_Response(no, r_epsilon=0.0)          # (never converged: every timed sweep steps all twelve systems)
        s.history = history
        for nh in (0, history):
            systems = []
            for w in (0.2 * gap, 0.5 * gap):
                for o in range(3):
                    for sign in (1.0, -1.0):
                        sy = M._System(o, sign * complex(w, 0.05), True)
                        sy.x = (ctx.zeros((lay.nflat,)), ctx.zeros((lay.nflat,)))
                        sy.r = (lay.empty().copy_from(xi[o]), ctx.zeros((lay.nflat,)))
                        sy.pn = (lay.empty(), lay.empty())
                        systems.append(sy)
            for sy, nrm in zip(systems, s._update(ctx, lay, d, systems, False)):
                sy.norm0 = sy.norm = float(np.sqrt(nrm))
            for _ in range(nh):                      # fill the stored directions
                s._sweep(ctx, lay, sig, d, systems)
            flat = [v for sy in systems for v in sy.pn]
            outs = [lay.padded() for _ in flat]
            parts = ([lay.part1(u) for u in flat], [lay.part2(u) for u in flat], [lay.part1(u) for u in outs],
                     [lay.part2(u) for u in outs])
            apply = lambda: sig.apply_many(parts[0], parts[1], [True] * len(flat), out1=parts[2], out2=parts[3])
            apply()
            t_apply = min(timed(ctx, apply) for _ in range(repeat))
            t_sweep = min(timed(ctx, lambda: s._sweep(ctx, lay, sig, d, systems)) for _ in range(repeat))
            # (the timed sweeps add a direction each, up to `history`: the bound counts the passes of the first one)
            # per system and part (re, im): the dots read p, A p, r and nh hq; the update reads those, x and nh hp and writes x, r, ph, qh, pn
            vectors_moved = len(flat) * ((3 + nh) + (4 + 2 * nh) + 5)
            bound = vectors_moved * 8.0 * lay.nflat / HBM_BYTES_PER_S
            emit("  sweep of 12 complex systems starting from %d stored directions: %.3f ms; stacked apply of its 24 vectors alone: %.3f ms; "
                 "ratio %.3f; overhead %.3f ms against an HBM bound of %.3f ms (%d vector passes at %.1f TB/s): %.2f x the bound" % (
                     nh, 1e3 * t_sweep, 1e3 * t_apply, t_sweep / t_apply, 1e3 * (t_sweep - t_apply), 1e3 * bound,
                     vectors_moved, HBM_BYTES_PER_S / 1e12, (t_sweep - t_apply) / bound))
            del systems, flat, outs, parts
            ctx.trim()
        sig.close()
        del sig, d, xi, eta, out
        ctx.trim()
        # ---- a dipole-like solve ---------------------------------------------------------------------------------------------------
        solver = M.EOM_CCSD_Response(no, r_epsilon=r_epsilon)
        solver.history = history
        ctx.sync()
        t0 = time.perf_counter()
        lam_host = (lam[0].get(), lam[1].get())
        sol = quiet(solver.solve, fd, dressed, res["t2"], res["t1"], ops, [0.0, 0.5 * gap], gamma=0.05, lam=lam_host)
        ctx.sync()
        emit("  solve, 3 operators x (0, 0.5 gap) + 0.05i, r_epsilon %g, history %d: %.3f s, %d sweeps, iterations %s, converged %s, "
             "max residual %.2e" % (r_epsilon, history, time.perf_counter() - t0, sol["sweeps"], sol["iterations"].ravel(),
                                    sol["converged"], sol["residuals"].max()))
        emit("  isotropic polarizability %s" % np.array2string(solver.isotropic(), precision=8))
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="30x120,50x200")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--history", type=int, default=4)
    ap.add_argument("--r-epsilon", type=float, default=1e-6)
    ap.add_argument("--out", default="profiles/response/probe_response.txt")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("probe_response: synthetic.factors(seed=0), CCSD delta_e = 1e-8, random Lambda (it enters eta alone)")
    for size in a.sizes.split(","):
        no, nv = (int(x) for x in size.split("x"))
        probe(no, nv, a.repeat, a.history, a.r_epsilon, emit)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
