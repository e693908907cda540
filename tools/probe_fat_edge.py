#!/usr/bin/env python3
"""GPU probe: what a fat tile of the LDS-DMA GEMM costs, and which plan suits the fat tiling of a ring product.

  (1) tile time: 512 whole tiles (two per CU, one round) without an edge, (4096, 2048), against 512 tiles of which the last
      tile row is fat in M, (4112, 2048), fat in N, (4096, 2064), and today's tiling of those (528 / 544 tiles);
  (2) the (50,200) ring product 10000^3: today's tiling and the fat tiling under their own plans and under forced ones.

    python3 tools/probe_fat_edge.py [K of part 1] [n of part 2, default 10000]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pymes_amd.device import Context


def main():
    K1 = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    n2 = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    ctx = Context(4, 4, workspace_bytes=1 << 28)
    ctx.prof_enable(True)
    rng = np.random.default_rng(0)

    def product(M, N, K):
        A = ctx.array(rng.standard_normal((M, K)))
        B = ctx.array(rng.standard_normal((K, N)))
        Cm = ctx.zeros((M, N))

        def run(fat, plan=None, reps=4):
            os.environ["PYMES_GEMM_FAT"] = fat
            if plan is None:
                os.environ.pop("PYMES_GEMM_PLAN", None)
            else:
                os.environ["PYMES_GEMM_PLAN"] = plan
            ctx.dgemm(M, N, K, 1.0, A, K, 1, B, N, 1, 0.0, Cm, N)
            ctx.sync()
            ctx.prof_reset()
            for _ in range(reps):
                ctx.dgemm(M, N, K, 1.0, A, K, 1, B, N, 1, 0.0, Cm, N)
            ctx.sync()
            return ctx.prof_query()["ms"] / reps * 1e3

        def free():
            for x in (A, B, Cm):
                x.free()
        return run, free

    print(f"# (1) one round of 512 tiles, K = {K1}: us")
    for M, N in ((4096, 2048), (4112, 2048), (4096, 2064), (4112, 2064)):
        run, free = product(M, N, K1)
        run("0", reps=8)          # clock ramp-up
        t_plain_whole = run("0", plan="%d,1" % (((M + 127) // 128) * ((N + 127) // 128)))
        t_plain = run("0")
        t_fat_whole = run("1", plan="512,1")
        t_fat = run("1")
        print(f"M={M} N={N}: today's tiling whole {t_plain_whole:.0f}, planned {t_plain:.0f}; fat 512 whole {t_fat_whole:.0f}, "
              f"planned {t_fat:.0f}", flush=True)
        free()

    print(f"# (2) {n2}^3: us")
    run, free = product(n2, n2, n2)
    run("0", reps=4)
    tp = ((n2 + 127) // 128) ** 2
    fm = n2 // 128 if 1 <= n2 % 128 <= 16 else (n2 + 127) // 128
    tf = fm * fm
    print(f"today's tiling ({tp} tiles): planned {run('0'):.0f}, whole {run('0', plan='%d,1' % tp):.0f}", flush=True)
    print(f"fat tiling ({tf} tiles): planned {run('1'):.0f}, whole {run('1', plan='%d,1' % tf):.0f}", flush=True)
    for w in sorted({(tf // 256) * 256, (tf // 256) * 256 - 256, (tf // 512) * 512, ((tf - 64) // 8) * 8, ((tf - 128) // 8) * 8}, reverse=True):
        res = []
        for s in (2, 3, 4, 5, 6, 8, 10, 12, 16):
            if (tf - w) * s > 1500:
                continue
            res.append(f"/{s}:{run('1', plan='%d,%d' % (w, s)):.0f}")
        print(f"fat {w}+{tf - w}  " + "  ".join(res), flush=True)
    print(f"today's tiling again: planned {run('0'):.0f}; fat planned {run('1'):.0f}", flush=True)
    free()
    ctx.close()


if __name__ == "__main__":
    main()
