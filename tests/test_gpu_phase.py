"""GPU: phase launches (include/pymes_amd.h) — the small operations of the library recorded with their address
ranges and launched level by level of their hazard graph, one union grid per level.  The whole parity suite runs with them
on (the default); here: the same solve with phases on, off and serialised (one task per level) agrees; the environment
switches do what INTEGRATION.md 4 says; hand-made hazards — column slices of one pitched array, accumulation chains that are
fused, a chain that must NOT be fused because somebody reads the array in between — against numpy."""
import contextlib
import io
import os

import numpy as np
import pytest

from oracle.cases import synthetic_case
from pymes_amd import _lib
from pymes_amd.device import Context

pytestmark = pytest.mark.gpu


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@contextlib.contextmanager
def phase_env(ctx, **env):
    """Environment switches are read when the phase machinery is (re)armed: pymes_phase_enable(-1)."""
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    ctx.phase_enable(-1)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        ctx.phase_enable(-1)


def solve(lib, monkeypatch, no, nv, dcsd=False):
    from pymes_amd.solver.ccsd import CCSD
    monkeypatch.setattr(_lib, "_default", lib)
    f, V, _, _ = synthetic_case(no, nv, seed=0, scale=0.3)
    s = CCSD(no, delta_e=1e-10, is_dcsd=dcsd)
    r = quiet(s.solve, f, V)
    return r["ccsd e"], s.iterations, r["t2"]


def test_on_off_serial_agree(gpu_lib, monkeypatch):
    ctx = Context(2, 3, lib=gpu_lib)
    try:
        res = {}
        for mode, env in (("on", {"PYMES_PHASE": None}), ("off", {"PYMES_PHASE": "0"}), ("serial", {"PYMES_PHASE": "serial"}),
                          ("nofuse", {"PYMES_PHASE_FUSE_MB": "0"}), ("big", {"PYMES_PHASE_MAX_US": "100000", "PYMES_PHASE_FUSE_MB": "64"})):
            with phase_env(ctx, **env):
                before = ctx.phase_stats()
                res[mode] = solve(gpu_lib, monkeypatch, 8, 32) + (ctx.phase_stats()["tasks"] - before["tasks"],
                                                                   ctx.phase_stats()["launches"] - before["launches"])
        e, it, t2 = res["on"][:3]
        assert res["on"][3] > 100 and res["on"][4] < res["on"][3]              # recorded, and fewer grids than tasks
        assert res["off"][3] == 0                                             # PYMES_PHASE=0: nothing is recorded
        assert res["serial"][4] >= res["serial"][3] > 0                       # one grid per task
        for mode in ("off", "serial", "nofuse", "big"):
            assert abs(res[mode][0] - e) < 1e-12 and res[mode][1] == it, (mode, res[mode][:2], e, it)
            assert np.abs(res[mode][2] - t2).max() < 1e-11
        # serialised and unfused differ from immediate launches only in WHERE the launches are cut: bit-identical
        assert res["serial"][0] == res["off"][0] and np.array_equal(res["serial"][2], res["off"][2])
    finally:
        ctx.close()


def test_switches(gpu_lib, monkeypatch, capfd):
    ctx = Context(2, 3, lib=gpu_lib)
    try:
        with phase_env(ctx, PYMES_PHASE_MAX_US="0"):                          # nothing is "small": nothing recorded
            before = ctx.phase_stats()["tasks"]
            e0 = solve(gpu_lib, monkeypatch, 4, 12)[0]
            # (only the unconditional tasks of the reductions' last stages are left)
            assert ctx.phase_stats()["tasks"] - before < 200
        capfd.readouterr()
        with phase_env(ctx, PYMES_PHASE_LOG="1"):
            e1 = solve(gpu_lib, monkeypatch, 4, 12)[0]
        err = capfd.readouterr().err
        assert "[phase] flush" in err and " gemm:" in err and "L0" in err
        assert abs(e0 - e1) < 1e-12
    finally:
        ctx.close()


def test_hand_made_hazards(gpu_lib):
    """Operations of several calls in ONE held phase (pymes_phase_hold): what the hazard analysis may run side by side and
    what it must keep apart."""
    ctx = Context(2, 3, lib=gpu_lib, workspace_bytes=1 << 28)
    rng = np.random.default_rng(5)
    try:
        M, K, N1, N2 = 150, 70, 40, 24
        A, B1, B2 = rng.standard_normal((M, K)), rng.standard_normal((K, N1)), rng.standard_normal((K, N2))
        dA, dB1, dB2 = ctx.array(A), ctx.array(B1), ctx.array(B2)
        # (1) two products into disjoint column slices of the same rows (one pitched array): independent — one level
        C = ctx.zeros((M, N1 + N2))
        from pymes_amd.device import DeviceArray
        right = DeviceArray(ctx, C.ptr + 8 * N1, (M, N2), owned=False, keepalive=C)
        before = ctx.phase_stats()
        with ctx.phase_hold():
            ctx.dgemm(M, N1, K, 1.0, dA, K, 1, dB1, N1, 1, 0.0, C, N1 + N2)
            ctx.dgemm(M, N2, K, 1.0, dA, K, 1, dB2, N2, 1, 0.0, right, N1 + N2)
        after = ctx.phase_stats()
        assert after["tasks"] - before["tasks"] == 2 and after["levels"] - before["levels"] == 1
        assert np.abs(C.get() - np.hstack([A @ B1, A @ B2])).max() < 1e-12
        # (2) an accumulation chain into a small contiguous array: fused — the members side by side, one combining task
        X = [rng.standard_normal((M, K)) for _ in range(5)]
        Y = [rng.standard_normal((K, N1)) for _ in range(5)]
        dX, dY = [ctx.array(x) for x in X], [ctx.array(y) for y in Y]
        R0 = rng.standard_normal((M, N1))
        R = ctx.array(R0)
        before = ctx.phase_stats()
        with ctx.phase_hold():
            for x, y in zip(dX, dY):
                ctx.dgemm(M, N1, K, 0.5, x, K, 1, y, N1, 1, 1.0, R, N1)
        after = ctx.phase_stats()
        assert after["levels"] - before["levels"] == 2 and after["launches"] - before["launches"] == 2
        want = R0 + 0.5 * sum(x @ y for x, y in zip(X, Y))
        assert np.abs(R.get() - want).max() < 1e-12
        # (3) ... but not across a reader of the array: R2 = R @ Z must see R after the first two members only
        R = ctx.array(R0)
        Z = rng.standard_normal((N1, 30))
        dZ, R2 = ctx.array(Z), ctx.zeros((M, 30))
        with ctx.phase_hold():
            ctx.dgemm(M, N1, K, 1.0, dX[0], K, 1, dY[0], N1, 1, 1.0, R, N1)
            ctx.dgemm(M, N1, K, 1.0, dX[1], K, 1, dY[1], N1, 1, 1.0, R, N1)
            ctx.dgemm(M, 30, N1, 1.0, R, N1, 1, dZ, 30, 1, 0.0, R2, 30)
            ctx.dgemm(M, N1, K, 1.0, dX[2], K, 1, dY[2], N1, 1, 1.0, R, N1)
        mid = R0 + X[0] @ Y[0] + X[1] @ Y[1]
        assert np.abs(R2.get() - mid @ Z).max() < 1e-11
        assert np.abs(R.get() - (mid + X[2] @ Y[2])).max() < 1e-12
        # (4) a temporary that is overwritten while an earlier reader is still only recorded (write-after-read)
        T = ctx.array(A)
        out1, out2 = ctx.zeros((M, N1)), ctx.zeros((M, N1))
        with ctx.phase_hold():
            ctx.dgemm(M, N1, K, 1.0, T, K, 1, dB1, N1, 1, 0.0, out1, N1)
            T.copy_from(dX[3])                                   # (a copy is not recorded: the phase is launched first)
            ctx.dgemm(M, N1, K, 1.0, T, K, 1, dB1, N1, 1, 0.0, out2, N1)
        assert np.abs(out1.get() - A @ B1).max() < 1e-12 and np.abs(out2.get() - X[3] @ B1).max() < 1e-12
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", list(range(8)))
def test_random_overlapping_views(gpu_lib, seed):
    """Forty products C <- alpha A B + beta C in ONE held phase on random pitched 2-D views of one buffer that overlap each
    other at random (row slices, column slices of the same rows, partial overlaps; A or B may be the transposed reading of
    a view) against the same sequence in numpy, one after the other: every read-after-write, write-after-read and write-
    after-write pair the generator happens to produce must be found by the range analysis (pitch-aware boxes, accumulation
    fusion included: beta = 1 chains into contiguous outputs occur)."""
    from pymes_amd.device import DeviceArray
    ctx = Context(2, 3, lib=gpu_lib, workspace_bytes=1 << 28)
    rng = np.random.default_rng(100 + seed)
    try:
        total = 1 << 16
        host = rng.standard_normal(total)
        buf = ctx.array(host.copy())

        def view(rows, cols):
            """(offset, pitch) of a rows x cols box somewhere in the buffer; pitch == cols now and then (contiguous)."""
            pitch = cols if rng.random() < 0.4 else cols + int(rng.integers(1, 40))
            span = (rows - 1) * pitch + cols
            # a handful of anchor offsets, so that boxes collide often
            off = int(rng.choice([0, 64, 1000, 1024, 5000, 5003, 20000, 20016])) + int(rng.integers(0, 8)) * 2
            assert off + span <= total
            return off, pitch

        def np_box(off, rows, cols, pitch):
            idx = off + np.arange(rows)[:, None] * pitch + np.arange(cols)[None, :]
            return idx

        def dev(off):
            return DeviceArray(ctx, buf.ptr + 8 * off, (1,), owned=False, keepalive=buf)

        def disjoint(i1, i2):
            return not np.intersect1d(i1.ravel(), i2.ravel()).size

        ops, done = [], 0
        before = ctx.phase_stats()
        with ctx.phase_hold():
            while done < 40:
                M, N, K = int(rng.integers(3, 70)), int(rng.integers(3, 70)), int(rng.integers(3, 50))
                ta, tb = rng.random() < 0.3, rng.random() < 0.3
                (oa, pa), (ob, pb), (oc, pc) = view(*((K, M) if ta else (M, K))), view(*((N, K) if tb else (K, N))), view(M, N)
                ia = np_box(oa, *((K, M) if ta else (M, K)), pa)
                ib = np_box(ob, *((N, K) if tb else (K, N)), pb)
                ic = np_box(oc, M, N, pc)
                if not (disjoint(ia, ic) and disjoint(ib, ic)):
                    continue                                # an output aliasing its own operands is undefined in any BLAS
                A = host[ia].T if ta else host[ia]
                B = host[ib].T if tb else host[ib]
                # (scaled by the operands' size in the host model, so that forty chained products stay O(1))
                alpha = float(rng.choice([-1.0, 0.5, 1.0])) / (np.sqrt(K) * max(1.0, np.abs(A).max()) * max(1.0, np.abs(B).max()))
                beta = float(rng.choice([0.0, 1.0, 1.0, 0.5]))
                ctx.dgemm(M, N, K, alpha, dev(oa), *((1, pa) if ta else (pa, 1)), dev(ob), *((1, pb) if tb else (pb, 1)),
                          beta, dev(oc), pc)
                host[ic] = alpha * (A @ B) + beta * host[ic]
                done += 1
        after = ctx.phase_stats()
        assert after["tasks"] - before["tasks"] >= 40 and after["levels"] - before["levels"] >= 2
        got = buf.get()
        assert np.isfinite(host).all() and np.abs(got - host).max() < 1e-11 * max(1.0, np.abs(host).max()), np.abs(got - host).max()
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", list(range(6)))
def test_random_mixed_operations(gpu_lib, seed):
    """The other recorded kinds next to the products: index permutations of 3- and 4-index arrays (both permutation kernels),
    binary contractions that end in matrix-vector kernels, linear combinations, and overlaps read back in between —
    fifty operations on contiguous arrays that overlap at random inside one buffer, in ONE held phase (an overlap read-back
    launches what is recorded and the phase goes on), against the same sequence in numpy."""
    from pymes_amd.device import DeviceArray
    ctx = Context(3, 5, lib=gpu_lib, workspace_bytes=1 << 28)
    rng = np.random.default_rng(500 + seed)
    try:
        total = 1 << 15
        host = rng.standard_normal(total)
        buf = ctx.array(host.copy())
        anchors = [0, 96, 2000, 2048, 9000, 9008, 16000]

        def place(n):
            off = int(rng.choice(anchors)) + 2 * int(rng.integers(0, 6))
            assert off + n <= total
            return off

        def dev(off, shape):
            return DeviceArray(ctx, buf.ptr + 8 * off, tuple(shape), owned=False, keepalive=buf)

        def hv(off, shape):
            n = int(np.prod(shape))
            return host[off:off + n].reshape(shape)

        def apart(o1, n1, o2, n2):
            return o1 + n1 <= o2 or o2 + n2 <= o1

        done, dots_seen = 0, 0
        with ctx.phase_hold():
            while done < 50:
                kind = rng.choice(["perm3", "perm4", "gemv", "lincomb", "dots", "gemm"])
                if kind in ("perm3", "perm4"):
                    nd = 3 if kind == "perm3" else 4
                    shape = [int(rng.integers(2, 13)) for _ in range(nd)]
                    perm = list(rng.permutation(nd))
                    n = int(np.prod(shape))
                    oi, oo = place(n), place(n)
                    if not apart(oi, n, oo, n):
                        continue
                    li = "abcd"[:nd]
                    lo = "".join(li[p] for p in perm)
                    alpha, beta = float(rng.choice([1.0, -0.5])), float(rng.choice([0.0, 1.0]))
                    out_shape = [shape[p] for p in perm]
                    res = alpha * hv(oi, shape).transpose(perm) + beta * hv(oo, out_shape)
                    ctx.permute(f"{li}->{lo}", dev(oi, shape), out=dev(oo, out_shape), alpha=alpha, beta=beta)
                    host[oo:oo + n] = res.ravel()
                elif kind == "gemv":
                    M, K = int(rng.integers(4, 120)), int(rng.integers(4, 120))
                    oa, ox, oy = place(M * K), place(K), place(M)
                    if not (apart(oa, M * K, oy, M) and apart(ox, K, oy, M)):
                        continue
                    s = 1.0 / (np.sqrt(K) * max(1.0, np.abs(hv(oa, (M, K))).max()))
                    res = s * (hv(oa, (M, K)) @ hv(ox, (K,)))
                    ctx.contract("mk,k->m", dev(oa, (M, K)), dev(ox, (K,)), out=dev(oy, (M,)), alpha=s, beta=0.0)
                    host[oy:oy + M] = res
                elif kind == "lincomb":
                    n, m = int(rng.integers(10, 1500)), int(rng.integers(1, 5))
                    oo = place(n)
                    offs = [place(n) for _ in range(m)]
                    if not all(apart(o, n, oo, n) for o in offs):
                        continue
                    cs = [float(c) for c in rng.uniform(-0.7, 0.7, m)]
                    res = sum(c * hv(o, (n,)) for c, o in zip(cs, offs))
                    ctx.lincomb(dev(oo, (n,)), [dev(o, (n,)) for o in offs], cs)
                    host[oo:oo + n] = res
                elif kind == "dots":
                    n = int(rng.integers(10, 3000))
                    ox, oy = place(n), place(n)
                    got = ctx.dots([dev(ox, (n,))], [dev(oy, (n,))])[0]
                    want = float(hv(ox, (n,)) @ hv(oy, (n,)))
                    assert abs(got - want) < 1e-10 * max(1.0, abs(want)), (done, got, want)
                    dots_seen += 1
                else:
                    M, N, K = int(rng.integers(3, 60)), int(rng.integers(3, 60)), int(rng.integers(3, 40))
                    oa, ob, oc = place(M * K), place(K * N), place(M * N)
                    if not (apart(oa, M * K, oc, M * N) and apart(ob, K * N, oc, M * N)):
                        continue
                    A, B = hv(oa, (M, K)), hv(ob, (K, N))
                    alpha = 1.0 / (np.sqrt(K) * max(1.0, np.abs(A).max()) * max(1.0, np.abs(B).max()))
                    beta = float(rng.choice([0.0, 1.0]))
                    res = alpha * (A @ B) + beta * hv(oc, (M, N))
                    ctx.dgemm(M, N, K, alpha, dev(oa, (1,)), K, 1, dev(ob, (1,)), N, 1, beta, dev(oc, (1,)), N)
                    host[oc:oc + M * N] = res.ravel()
                done += 1
        got = buf.get()
        assert np.isfinite(host).all() and np.abs(got - host).max() < 1e-11 * max(1.0, np.abs(host).max()), np.abs(got - host).max()
    finally:
        ctx.close()


# ---- split-K workspace reuse inside one held phase (the fusion-room rule) --------------------------------------
WS_DOUBLES = 32 << 20           # the engine's split-K workspace (engine.cpp): 256 MiB


def splitk_slice(M, N, K):
    """Doubles of the split-K workspace that phase_gemm (kernels.hip) takes for ONE recorded product M x N x K (batch 1):
    64 x 64 tiles (64 x 32 / 32 x 64 when a side is at most 32), BK = 16; with ktiles = ceil(K / 16) >= 16 the last,
    partially filled round of tiles (rem = tiles % 1024, all of them for a small output) is split over k in `sp` pieces,
    2 <= sp <= min(512, max(8, 2048 // rem), ktiles // 8, capacity // rem), the one that minimises
    ceil(rem sp / 1024) / sp + 1e-5 sp if that is below 0.8.  0: no k-split (no slice)."""
    BM, BN = 64, 64
    if N <= 32:
        BN = 32
    elif M <= 32:
        BM = 32
    tiles = -(-M // BM) * -(-N // BN)
    ktiles = -(-K // 16)
    rem = tiles % 1024
    if ktiles < 16 or rem == 0:
        return 0
    smax = min(512, max(8, 2048 // rem), ktiles // 8, (WS_DOUBLES // (BM * BN)) // rem)
    best, best_cost = 1, 1.0
    for sp in range(2, smax + 1):
        c = -(-(rem * sp) // 1024) / sp + 1e-5 * sp
        if c < best_cost - 1e-9:
            best, best_cost = sp, c
    if best < 2 or best_cost >= 0.8:
        return 0
    kt_per = -(-ktiles // best)
    nsplit = -(-ktiles // kt_per)
    return (rem * nsplit * BM * BN + 15) // 16 * 16


def test_fusion_after_workspace_wrap(gpu_lib, capfd):
    """A fused accumulation chain whose private buffers would land on the slice of a split-K product recorded inside the
    chain.  In one held phase: R = A0 B0 (beta 0: opens the fusion group), R += A1 B1 (a member), nine products
    Q_j = X_j Y of M = 64, N = 6400, K = 2560, then R += A2 B2 (a member).  Each Q_j is recorded (M <= 64 keeps it off the
    LDS-DMA kernel; PYMES_PHASE_MAX_US lifts its ~86-us estimate under the cap) with a k-split: 100 tiles of 64 x 64,
    ktiles = 160, sp = 10 (splitk_slice), a slice of 100 * 10 * 4096 = 4,096,000 doubles.  Eight slices fill 32.8 M of the
    33.55 M doubles, the ninth wraps to 0 and leaves the cursor at 4,096,000 — the start of Q_2's slice.  Fusion hands out
    its buffers at flush time from that cursor: member 1's buffer would be overwritten by Q_2's partial tiles before the
    combining task reads it.  The rule (kernels.hip, phase_fuse_accumulations): no fusion once the workspace has wrapped."""
    M, N, K, nq = 64, 6400, 2560, 9
    slice_ = splitk_slice(M, N, K)
    assert slice_ == 4096000 and (nq - 1) * slice_ <= WS_DOUBLES < nq * slice_      # (precondition: exactly one wrap)
    ctx = Context(2, 3, lib=gpu_lib, workspace_bytes=1 << 28)
    rng = np.random.default_rng(11)
    try:
        m, n, k = 64, 64, 32
        # R between two arrays nobody reads: an operand's range has one double of slack at its top (pbox), and an operand
        # right below R would "touch" it — the group would close before the last member and nothing would be at stake
        guard = [ctx.zeros((64,))]
        R = ctx.array(rng.standard_normal((m, n)))
        guard.append(ctx.zeros((64,)))
        As = [rng.standard_normal((m, k)) for _ in range(3)]
        Bs = [rng.standard_normal((k, n)) for _ in range(3)]
        Xs = [rng.standard_normal((M, K)) / np.sqrt(K) for _ in range(nq)]
        Y = rng.standard_normal((K, N))
        dA, dB, dX, dY = [ctx.array(a) for a in As], [ctx.array(b) for b in Bs], [ctx.array(x) for x in Xs], ctx.array(Y)
        Q = [ctx.array(np.full((M, N), np.nan)) for _ in range(nq)]
        ctx.sync()
        capfd.readouterr()
        with phase_env(ctx, PYMES_PHASE_MAX_US="1000", PYMES_PHASE_LOG="1"):
            before = ctx.phase_stats()
            with ctx.phase_hold():
                ctx.dgemm(m, n, k, 1.0, dA[0], k, 1, dB[0], n, 1, 0.0, R, n)
                ctx.dgemm(m, n, k, 1.0, dA[1], k, 1, dB[1], n, 1, 1.0, R, n)
                for x, q in zip(dX, Q):
                    ctx.dgemm(M, N, K, 1.0, x, K, 1, dY, N, 1, 0.0, q, N)
                ctx.dgemm(m, n, k, 1.0, dA[2], k, 1, dB[2], n, 1, 1.0, R, n)
            after = ctx.phase_stats()
        err = capfd.readouterr().err
        # everything recorded, in one phase: 3 small products + a (tiles, reduction) pair per split product
        assert after["tasks"] - before["tasks"] == 3 + 2 * nq and after["flushes"] - before["flushes"] == 1
        for j, (x, q) in enumerate(zip(Xs, Q)):
            want = x @ Y
            assert np.abs(q.get() - want).max() < 1e-12 * np.abs(want).max(), j
        want = sum(a @ b for a, b in zip(As, Bs))
        assert np.abs(R.get() - want).max() < 1e-12 * np.abs(want).max()
        assert err.count("[phase] workspace wrap") == 1, err[-2000:]
        assert "[phase] fusion declined: 2 members" in err, err[-2000:]
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", list(range(3)))
def test_random_workspace_wraps(gpu_lib, seed, capfd):
    """Fifty-six recorded operations in ONE held phase whose split-K slices wrap the workspace two times or more: k-split
    products (splitk_slice) into large outputs, beta = 1 accumulation chains into small contiguous arrays (fusion
    candidates; some members k-split themselves), matrix-vector contractions whose row-chunk partials take workspace slices
    too (the column-sum path of gemv_dispatch), and now and then a product that reads an accumulation target in the middle
    of its chain — against the same sequence in numpy."""
    ctx = Context(2, 3, lib=gpu_lib, workspace_bytes=1 << 28)
    rng = np.random.default_rng(900 + seed)
    try:
        LD, KMAX = 6400, 4096
        big_shapes = [(64, 6400, 2560), (64, 3200, 2560), (48, 6400, 4096), (32, 6400, 2560), (64, 6400, 2048)]
        host = {"Y": rng.standard_normal((KMAX, LD))}
        host.update({f"X{i}": rng.standard_normal((64, KMAX)) for i in range(3)})
        host.update({f"O{i}": rng.standard_normal((64, LD)) for i in range(4)})            # large outputs
        host.update({f"T{i}": rng.standard_normal((40, 48)) for i in range(3)})            # accumulation targets
        host.update({f"W{i}": rng.standard_normal((40, 20)) for i in range(2)})            # readers' outputs
        host.update({f"v{i}": rng.standard_normal((1, LD)) for i in range(2)})             # matrix-vector outputs
        host.update({f"x{i}": rng.standard_normal((1, KMAX)) for i in range(2)})
        host.update({f"A{k}": rng.standard_normal((40, k)) for k in (16, 32, 320)})
        host.update({f"B{k}": rng.standard_normal((k, 48)) for k in (16, 32, 320)})
        host["Z"] = rng.standard_normal((48, 20))
        dev = {name: ctx.array(a) for name, a in host.items()}
        ctx.sync()
        slices = 0
        capfd.readouterr()
        with phase_env(ctx, PYMES_PHASE_MAX_US="100000", PYMES_PHASE_LOG="1"):
            before = ctx.phase_stats()
            with ctx.phase_hold():
                for _ in range(56):
                    kind = rng.choice(["big", "big", "big", "big", "acc", "acc", "acc", "gemv", "read"])
                    beta = float(rng.choice([0.0, 1.0, 1.0]))
                    if kind == "big":
                        M, N, K = big_shapes[int(rng.integers(len(big_shapes)))]
                        x, o = f"X{int(rng.integers(3))}", f"O{int(rng.integers(4))}"
                        alpha = 1.0 / np.sqrt(K)
                        ctx.dgemm(M, N, K, alpha, dev[x], KMAX, 1, dev["Y"], LD, 1, beta, dev[o], LD)
                        host[o][:M, :N] = alpha * (host[x][:M, :K] @ host["Y"][:K, :N]) + beta * host[o][:M, :N]
                        slices += splitk_slice(M, N, K)
                    elif kind == "acc":
                        k, t = int(rng.choice([16, 32, 320])), f"T{int(rng.integers(3))}"
                        alpha = float(rng.choice([0.5, -1.0])) / np.sqrt(k)
                        ctx.dgemm(40, 48, k, alpha, dev[f"A{k}"], k, 1, dev[f"B{k}"], 48, 1, beta, dev[t], 48)
                        host[t] = alpha * (host[f"A{k}"] @ host[f"B{k}"]) + beta * host[t]
                        slices += splitk_slice(40, 48, k)
                    elif kind == "gemv":
                        K, v, x = int(rng.choice([2560, 4096])), f"v{int(rng.integers(2))}", f"x{int(rng.integers(2))}"
                        alpha = 1.0 / np.sqrt(K)
                        ctx.dgemm(1, LD, K, alpha, dev[x], KMAX, 1, dev["Y"], LD, 1, beta, dev[v], LD)
                        host[v] = alpha * (host[x][:, :K] @ host["Y"][:K]) + beta * host[v]
                    else:
                        t, w = f"T{int(rng.integers(3))}", f"W{int(rng.integers(2))}"
                        ctx.dgemm(40, 20, 48, 0.2, dev[t], 48, 1, dev["Z"], 20, 1, 0.0, dev[w], 20)
                        host[w] = 0.2 * (host[t] @ host["Z"])
            after = ctx.phase_stats()
        err = capfd.readouterr().err
        assert after["flushes"] - before["flushes"] == 1 and after["tasks"] - before["tasks"] >= 50
        for name, want in host.items():
            got = dev[name].get()
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (name, np.abs(got - want).max())
        # (the precondition: the workspace wrapped twice or more — the products' slices, splitk_slice, and the matrix-vector
        # partials, 80 row chunks x 6400 each)
        assert slices > WS_DOUBLES and err.count("[phase] workspace wrap") >= 2, (slices, err.count("[phase] workspace wrap"))
    finally:
        ctx.close()


def _residual_passes(lib, calls, workspace_bytes=0, marks=()):
    """`calls` whole-step CCSD residuals (pymes_ccsd_residuals) on ONE (8, 32) context, phases on: r1, r2 and the
    workspace high-water mark after the calls listed in `marks`."""
    no, nv = 8, 32
    f, V, _, _ = synthetic_case(no, nv, seed=1, scale=0.3)
    rng = np.random.default_rng(2)
    t1h = 0.05 * rng.standard_normal((nv, no))
    x = 0.05 * rng.standard_normal((nv, nv, no, no))
    ctx = Context(no, nv, lib=lib, workspace_bytes=workspace_bytes)
    try:
        with phase_env(ctx, PYMES_PHASE=None):
            ctx.set_V_pqrs(V)
            ctx.set_orbital_energies(f.diagonal()[:no].copy(), f.diagonal()[no:].copy())
            fd, t1, t2 = ctx.array(f), ctx.array(t1h), ctx.array(x + x.transpose(1, 0, 3, 2))
            r1, r2 = ctx.empty(t1.shape), ctx.empty(t2.shape)
            high = {}
            for i in range(1, calls + 1):
                ctx.ccsd_residuals(fd, t1, t2, r1, r2)
                if i in marks:
                    high[i] = ctx.workspace()[1]
            assert ctx.phase_stats()["tasks"] > 0
            return r1.get(), r2.get(), high
    finally:
        ctx.close()


def test_arena_reuse_across_sibling_scopes(gpu_lib):
    """pymes_ccsd_residuals runs its dressings, the doubles slab, the singles and the finish as sibling arena scopes with no
    enclosing one; a release deferred for the open phase (engine.h, Arena) must come back to the next sibling.  The
    high-water mark is the same after 2 and after 20 passes, and a workspace only 1.25 x that mark serves 20 passes with
    results bit-identical to those of a generous workspace (phases on in both: the same fusion, the same order of sums)."""
    r1, r2, high = _residual_passes(gpu_lib, 20, marks=(2, 20))
    assert high[2] > 0 and high[20] == high[2], high
    t1, t2, _ = _residual_passes(gpu_lib, 20, workspace_bytes=int(1.25 * high[2]))
    assert np.array_equal(t1, r1) and np.array_equal(t2, r2)
