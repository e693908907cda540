"""Strided, offset, padded and broadcast views for the C-ABI entry points that take element strides (pymes_contract,
pymes_permute, pymes_set_V_pqrs, pymes_set_V_block of include/pymes_amd.h), and the checks built on them.  Shared by
tests/test_strided_abi.py (CPU stand-in: the host planner) and tests/test_gpu_strided_abi.py (the kernels).

Every view lives in a one-dimensional base array that is uploaded whole.  What is outside an input view is NaN; with
beta == 0 the elements of the output view are NaN before the call; after the call the whole output base is downloaded,
compared with numpy inside the view and bit for bit with what was uploaded outside it.  No view ends flush with its base:
one more double follows its last element (the one-element over-read the header allows a product).

Bounds, as in the rest of the suite: products err / max(1, |ref|max) < 1e-13 sqrt(K) + 1e-14 (tests/test_gpu_fuzz.py),
permutations bit-exact for alpha = 1, beta = 0 and < 1e-14 absolute otherwise (tests/test_host_engine.py, test_permute)."""
import contextlib
import ctypes as C

import numpy as np
from numpy.lib.stride_tricks import as_strided

from pymes_amd._lib import PymesError, i64_array
from pymes_amd.device import Context

STEPS = (1, 1, 2, 3)
LETTERS = "abcdefghijklmnop"


# ---------------------------------------------------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------------------------------------------------
def element_indices(offset, dims, strides):
    """Index into the base of every element of a view, as an int64 array of the view's shape."""
    idx = np.full(tuple(dims), int(offset), dtype=np.int64)
    for ax, (n, s) in enumerate(zip(dims, strides)):
        shape = [1] * len(dims)
        shape[ax] = n
        idx = idx + (np.arange(n, dtype=np.int64) * int(s)).reshape(shape)
    return idx


def strided_view(rng, dims, offset, strides, size, values=None):
    """(base, view): a NaN-filled base of ``size`` + 1 doubles and the read-only view of it with these extents, element
    offset and element strides, holding random numbers (or ``values``)."""
    base = np.full(size + 1, np.nan)                      # + 1: the view is never flush with the end of its base
    assert offset >= 0 and all(s >= 0 for s in strides) and offset + sum((n - 1) * s for n, s in zip(dims, strides)) < size
    held = tuple(n if s != 0 else 1 for n, s in zip(dims, strides))          # (a stride-0 axis holds one element)
    w = as_strided(base[offset:], shape=held, strides=tuple(8 * s for s in strides))
    w[...] = rng.standard_normal(held) if values is None else np.asarray(values).reshape(held)
    view = as_strided(base[offset:], shape=tuple(dims), strides=tuple(8 * s for s in strides), writeable=False)
    return base, view


def make_view(rng, dims, allow_broadcast, order=None, tight=(), unit=()):
    """(base, view): a NaN-filled 1-D base and a read-only view of it with the logical extents ``dims`` and random values.
    The axes lie in memory in a random order (``order``: outer -> inner, if given); each has a slice step from {1, 1, 2, 3}, a
    leading offset of 0..2 and a trailing pad of 0..2 of its own pitch; with ``allow_broadcast`` an axis now and then has
    stride 0.  Axes in ``tight`` have step 1 and no pads, axes in ``unit`` step 1 (pads allowed); neither is broadcast."""
    dims = [int(d) for d in dims]
    r = len(dims)
    order = [int(a) for a in (rng.permutation(r) if order is None else order)]
    strides, offset, run = [0] * r, 0, 1
    for ax in reversed(order):
        step, lead, trail = int(rng.choice(STEPS)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
        bcast = rng.random() < 0.12
        if ax in tight:
            step, lead, trail, bcast = 1, 0, 0, False
        elif ax in unit:
            step, bcast = 1, False
        if bcast and allow_broadcast:
            continue                                       # stride 0: the axis takes no room in the base
        strides[ax] = step * run
        offset += lead * run
        run *= lead + (dims[ax] - 1) * step + 1 + trail
    return strided_view(rng, dims, offset, strides, run)


def padded_view(rng, labels, extents, memory, pads, lead=0, broadcast="", values=None):
    """(base, view) by construction: logical axes ``labels`` with ``extents[label]``, laid out in memory in the order of the
    string ``memory`` (outer -> inner) with ``pads[label]`` unused elements after each axis (default 0) and ``lead`` elements
    before the first; the labels in ``broadcast`` get stride 0.  ``values``: the elements, instead of random ones."""
    st, run = {}, 1
    for ch in reversed(memory):
        if ch in broadcast:
            st[ch] = 0
            continue
        st[ch] = run
        run *= extents[ch] + pads.get(ch, 0)
    return strided_view(rng, [extents[ch] for ch in labels], lead, [st[ch] for ch in labels], run + lead, values)


def view_layout(base, view):
    """(element offset of the view's first element in its base, element strides of the view)."""
    off = view.__array_interface__["data"][0] - base.__array_interface__["data"][0]
    assert off % 8 == 0 and all(s % 8 == 0 for s in view.strides)
    return off // 8, [s // 8 for s in view.strides]


def output_base(rng, base, view, beta):
    """The base of an output view as it is uploaded: random numbers outside the view, NaN inside for beta == 0 (the output
    must be written, not scaled) and random numbers inside otherwise.  Returns (uploaded base, index array of the view)."""
    off, st = view_layout(base, view)
    idx = element_indices(off, view.shape, st)
    assert np.unique(idx).size == idx.size                 # an output never overlaps itself
    up = np.random.default_rng(int(rng.integers(1 << 30))).standard_normal(base.size)
    if beta == 0.0:
        up[idx.ravel()] = np.nan
    return up, idx


def check_output(got, up, idx, ref, bound, what):
    """Inside the view against ``ref`` (``bound`` None: bit-exact), outside bit-identical to the uploaded base.  Returns
    err / bound (0 for an exact comparison)."""
    mask = np.zeros(up.size, dtype=bool)
    mask[idx.ravel()] = True
    assert np.array_equal(got.view(np.uint64)[~mask], up.view(np.uint64)[~mask]), ("written outside the view", what)
    inside = got[idx]
    if bound is None:
        assert np.array_equal(inside, ref), what
        return 0.0
    err = np.abs(inside - ref).max(initial=0.0)
    assert err < bound, (what, err, bound)                 # (a NaN that leaked in fails here too)
    return err / bound


def _dev_ptr(darr, offset):
    return C.c_void_p(darr.ptr + 8 * int(offset))


def call_contract(ctx, alpha, dA, A, la, dB, B, lb, beta, dC, Cv, lc, batch=""):
    """pymes_contract on three (device base, (offset, strides), dims) operands."""
    (oa, sa, da), (ob, sb, db), (oc, sc, dc) = A, B, Cv
    ctx.lib.call("pymes_contract", ctx.handle, float(alpha),
                 _dev_ptr(dA, oa), la.encode(), i64_array(da), i64_array(sa),
                 _dev_ptr(dB, ob), lb.encode(), i64_array(db), i64_array(sb),
                 float(beta), _dev_ptr(dC, oc), lc.encode(), i64_array(dc), i64_array(sc), batch.encode())


def call_permute(ctx, alpha, dI, I, li, beta, dO, O, lo):
    (oi, si, di), (oo, so, _) = I, O
    ctx.lib.call("pymes_permute", ctx.handle, float(alpha), _dev_ptr(dI, oi), li.encode(), i64_array(di), i64_array(si),
                 float(beta), _dev_ptr(dO, oo), lo.encode(), i64_array(so))


def _layout(base, view):
    off, st = view_layout(base, view)
    return off, st, list(view.shape)


@contextlib.contextmanager
def launch_mode(ctx, mode):
    """'env': phase launches as the environment says; 'nophase' and 'group': off (the caller opens the groups)."""
    ctx.phase_enable(-1 if mode == "env" else 0)
    try:
        yield
    finally:
        ctx.phase_enable(-1)


# ---------------------------------------------------------------------------------------------------------------------
# the planner's choice of copies, mirrored (Engine::contract, csrc/engine.cpp): which operands go through a temporary
# ---------------------------------------------------------------------------------------------------------------------
def _merge_group(dims, strides, pos):
    size, stride, have = 1, 0, False
    for p in reversed(pos):
        n, s = dims[p], strides[p]
        if n == 1:
            continue
        if not have:
            size, stride, have = n, s, True
        elif s != size * stride:
            return None
        else:
            size *= n
    return size, stride


def plan_copies(la, lb, lc, batch, A, B, Cv, beta):
    """(copyA, copyB, copyC) as Engine::contract chooses them for operands (dims, strides) that are not kept integral
    blocks: the cheapest of the eight M / N / K orderings, the first one on a tie."""
    kind = {}
    for ch in dict.fromkeys(la + lb + lc):
        a, b, c = ch in la, ch in lb, ch in lc
        forced = ch in batch
        if a and b and c:
            kind[ch] = "Z"
        elif a and c:
            kind[ch] = "Z" if forced else "M"
        elif b and c:
            kind[ch] = "Z" if forced else "N"
        else:
            kind[ch] = "K"

    def ordered(k, s):
        return [ch for ch in s if kind[ch] == k]
    M_cand, N_cand = (ordered("M", lc), ordered("M", la)), (ordered("N", lc), ordered("N", lb))
    K_cand = (ordered("K", la), ordered("K", lb))

    def direct(X, s, g1, g2):
        dims, st = X
        m1 = _merge_group(dims, st, [s.index(ch) for ch in g1])
        m2 = _merge_group(dims, st, [s.index(ch) for ch in g2]) if m1 else None
        if not m1 or not m2:
            return False
        return m1[1] == 1 or m2[1] == 1 or m1[0] == 1 or m2[0] == 1
    size = lambda X: float(np.prod(X[0], dtype=np.float64)) if len(X[0]) else 1.0
    bA, bB, bC = 8.0 * size(A), 8.0 * size(B), 8.0 * size(Cv)
    best, best_cost = (True, True, True), 1e300
    for im in range(2):
        for in_ in range(2):
            for ik in range(2):
                cA = not direct(A, la, M_cand[im], K_cand[ik])
                cB = not direct(B, lb, K_cand[ik], N_cand[in_])
                cC = not direct(Cv, lc, M_cand[im], N_cand[in_])
                cost = (2 * bA if cA else 0) + (2 * bB if cB else 0) + ((3 if beta != 0.0 else 2) * bC if cC else 0)
                if cost < best_cost:
                    best, best_cost = (cA, cB, cC), cost
    return best


# ---------------------------------------------------------------------------------------------------------------------
# contraction fuzz
# ---------------------------------------------------------------------------------------------------------------------
EXTENTS = [1, 2, 3, 5, 8, 13, 17, 31, 32, 33]
MAX_ELEMENTS = 200_000           # per tensor (logical elements); the base of a view may be at most 16 times that
MAX_WORK = 20_000_000            # product of all label extents: keeps numpy's einsum and the CPU stand-in at a few ms a case
MINIMUM = 10                     # cases of every category per seed
CATEGORIES = ("outer_loop", "copied_operand", "copied_C_beta", "odd_offset", "stride0", "rank56")


def _friendly(labels, groups, zlabels):
    """Memory order and step constraints under which ``labels`` is a matrix on ``groups`` = (outer, inner) without a copy:
    batch labels outermost, each group together, inner labels of a group tight, unit steps where a merge or the unit stride
    needs them."""
    outer, inner = groups
    memory = [ch for ch in zlabels if ch in labels] + list(outer) + list(inner)
    tight, unit = [], []
    for g, is_inner in ((outer, False), (inner, True)):
        if len(g) == 1 and is_inner:
            unit.append(g[0])
        elif len(g) > 1:
            unit.append(g[0])
            tight.extend(g[1:])
    ax = lambda chs: [labels.index(ch) for ch in chs]
    return dict(order=ax(memory), tight=ax(tight), unit=ax(unit))


def gen_contraction(rng):
    """One random case (None: rejected for its size or ranks).  0..3 labels shared by A, B and C, 0..2 each of kind M, N and
    K; a shared label is now and then dropped from A or from B (a free label forced into ``batch``: the other operand is
    shared across the batch), M and N labels are now and then forced into ``batch``."""
    nz, nm, nn, nk = int(rng.integers(0, 4)), int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
    labs = list(LETTERS[: nz + nm + nn + nk])
    rng.shuffle(labs)
    Z, M, N, K = labs[:nz], labs[nz:nz + nm], labs[nz + nm:nz + nm + nn], labs[nz + nm + nn:]
    inA, inB, inC, batch = Z + M + K, Z + N + K, Z + M + N, []
    for ch in Z:
        u = rng.random()
        if u < 0.15:
            inA.remove(ch); batch.append(ch)
        elif u < 0.30:
            inB.remove(ch); batch.append(ch)
    for ch in M + N:
        if rng.random() < 0.15:
            batch.append(ch)
    small = rng.random() < 0.5           # half of the cases lean to small extents: the ones that reach ranks 5 and 6
    dims = {ch: int(rng.choice(EXTENTS[:6] if small else EXTENTS)) for ch in labs}
    for s in (inA, inB, inC):
        rng.shuffle(s)
    la, lb, lc = "".join(inA), "".join(inB), "".join(inC)
    alpha, beta = float(rng.choice([1.0, -1.0, 0.5])), float(rng.choice([0.0, 0.0, 1.0, -0.5]))
    profile = rng.random()
    if not all(1 <= len(s) <= 6 for s in (la, lb, lc)):
        return None
    if any(np.prod([dims[ch] for ch in s]) > MAX_ELEMENTS for s in (la, lb, lc)):
        return None
    if np.prod([float(dims[ch]) for ch in labs]) > MAX_WORK:
        return None
    zs = [ch for ch in lc if ch in batch or (ch in la and ch in lb)]
    kw = {"A": {}, "B": {}, "C": {}}
    if profile < 0.8:                    # inputs that are matrices as they lie (M and K by A's order, N by B's)
        mA = [c for c in la if c in M and c not in batch]
        kA = [c for c in la if c in K]
        nB = [c for c in lb if c in N and c not in batch]
        flip = rng.random() < 0.5
        kw["A"] = _friendly(la, (kA, mA) if flip else (mA, kA), zs)
        kw["B"] = _friendly(lb, (nB, kA) if rng.random() < 0.5 else (kA, nB), zs)
        if profile < 0.15:               # ... and an output that is one too
            kw["C"] = _friendly(lc, (mA, nB), zs)
    views = {}
    for name, s in (("A", la), ("B", lb), ("C", lc)):
        base, view = make_view(rng, [dims[ch] for ch in s], allow_broadcast=name != "C", **kw[name])
        if base.size > 16 * MAX_ELEMENTS:
            return None
        views[name] = (base, view)
    return dict(la=la, lb=lb, lc=lc, batch="".join(batch), alpha=alpha, beta=beta, dims=dims, views=views,
                K=int(np.prod([dims[ch] for ch in la if ch in lb and ch not in lc])))


def check_strided_contractions(lib, seed, n_cases, mode="env"):
    """``n_cases`` accepted random contractions through strided views in one launch mode: 'env' (phase launches as the
    environment says), 'nophase', or 'group' (phases off, as in tests/test_subspace.py: an open phase takes a small product
    before the group does).  Ten cases at a time are generated and uploaded, then issued — in 'group' mode inside one
    ``ctx.gemm_group()`` that holds nothing but the pymes_contract calls, the cases that need no copy first (a product that
    went through a temporary ends the queue) — and checked after the block.  Asserts the bound of every case, the minimum
    count of every category and, on the device, that the products of a group shared launches; returns (counts, worst)."""
    rng = np.random.default_rng(seed)
    ctx = Context(2, 2, workspace_bytes=1 << 26, lib=lib)
    counts = dict.fromkeys(CATEGORIES, 0)
    worst, done = 0.0, 0
    grouped = dict(blocks=0, products=0, launches=0)
    try:
        with launch_mode(ctx, mode):
            while done < n_cases:
                block = []
                while len(block) < 10 and done + len(block) < n_cases:
                    case = gen_contraction(rng)
                    if case is None:
                        continue                     # (a rejection never counts)
                    (bA, vA), (bB, vB), (bC, vC) = (case["views"][k] for k in "ABC")
                    A, B, Cv = _layout(bA, vA), _layout(bB, vB), _layout(bC, vC)
                    up, idx = output_base(rng, bC, vC, case["beta"])
                    spec = f"{case['la']},{case['lb']}->{case['lc']}"
                    ref = case["alpha"] * np.einsum(spec, vA, vB)
                    if case["beta"] != 0.0:
                        ref = ref + case["beta"] * up[idx]
                    copies = plan_copies(case["la"], case["lb"], case["lc"], case["batch"], (A[2], A[1]), (B[2], B[1]),
                                         (Cv[2], Cv[1]), case["beta"])
                    what = dict(seed=seed, case=done + len(block), spec=spec, batch=case["batch"], dims=case["dims"],
                                alpha=case["alpha"], beta=case["beta"], A=A[:2], B=B[:2], C=Cv[:2], mode=mode)
                    counts["odd_offset"] += bool(A[0] & 1 or B[0] & 1)
                    counts["stride0"] += any(s == 0 and n > 1 for X in (A, B) for s, n in zip(X[1], X[2]))
                    counts["rank56"] += max(len(case["la"]), len(case["lb"]), len(case["lc"])) >= 5
                    block.append(dict(case=case, A=A, B=B, C=Cv, up=up, idx=idx, ref=ref, copies=copies, what=what,
                                      dev=(ctx.array(bA), ctx.array(bB), ctx.array(up))))

                def issue(c):
                    case, (dA, dB, dC) = c["case"], c["dev"]
                    call_contract(ctx, case["alpha"], dA, c["A"], case["la"], dB, c["B"], case["lb"], case["beta"], dC, c["C"],
                                  case["lc"], case["batch"])
                if mode == "group":
                    order = sorted(block, key=lambda c: any(c["copies"]))          # (stable: the direct cases first)
                    direct = sum(not any(c["copies"]) for c in block)
                    with ctx.gemm_group() as grp:              # (nothing but products in here: any other entry ends the queue)
                        for c in order:
                            issue(c)
                    for c in block:
                        counts["copied_operand"] += any(c["copies"])
                        counts["copied_C_beta"] += c["copies"] == (False, False, True) and c["case"]["beta"] != 0.0
                    if lib.backend != "hostsim" and direct >= 2:              # (the CPU stand-in does not count groups)
                        assert grp.products >= 2 and grp.launches < grp.products, (seed, done, direct, grp.products, grp.launches)
                        grouped["blocks"] += 1
                    grouped["products"] += grp.products
                    grouped["launches"] += grp.launches
                else:
                    for c in block:
                        ctx.stats(reset=True)
                        issue(c)
                        st = ctx.stats(reset=True)
                        assert st["permute_calls"] <= 3, (c["what"], st)
                        counts["outer_loop"] += st["gemm_calls"] > 1
                        counts["copied_operand"] += st["permute_calls"] > 0
                        # (which operand was copied is not in the counters: the mirror of the planner's choice says)
                        counts["copied_C_beta"] += (st["permute_calls"] > 0 and c["copies"] == (False, False, True)
                                                    and c["case"]["beta"] != 0.0)
                for c in block:                                   # (the bases stay alive until here)
                    got = c["dev"][2].get()
                    ref, K = c["ref"], c["case"]["K"]
                    scale = max(1.0, np.abs(ref).max(initial=0.0))
                    worst = max(worst, check_output(got, c["up"], c["idx"], ref, (1e-13 * max(1, K) ** 0.5 + 1e-14) * scale,
                                                    c["what"]))
                    for x in c["dev"]:
                        x.free()
                done += len(block)
    finally:
        ctx.close()
    print(f"strided contractions seed {seed} mode {mode}: {counts} worst err/bound {worst:.3g}"
          + (f" grouped {grouped}" if mode == "group" else ""))
    for cat in CATEGORIES:
        if cat == "outer_loop" and mode == "group":
            continue
        assert counts[cat] >= MINIMUM * n_cases // 120, (cat, counts)
    if mode == "group" and lib.backend != "hostsim":
        assert grouped["blocks"] >= n_cases // 20, grouped          # most blocks of ten hold two cases without a copy
    return counts, worst


def run_contraction(ctx, rng, spec, vA, vB, vC, alpha, beta, batch="", ref0=None, what=None):
    """One pymes_contract between three (base, view) pairs, checked at once; ``ref0``: the product without alpha and beta, if
    the caller has it already.  Returns err / bound."""
    ins, lc = spec.split("->")
    la, lb = ins.split(",")
    (bA, xA), (bB, xB), (bC, xC) = vA, vB, vC
    A, B, Cv = _layout(bA, xA), _layout(bB, xB), _layout(bC, xC)
    up, idx = output_base(rng, bC, xC, beta)
    ref = alpha * (np.einsum(spec, xA, xB, optimize=True) if ref0 is None else ref0)
    if beta != 0.0:
        ref = ref + beta * up[idx]
    K = int(np.prod([n for ch, n in zip(la, xA.shape) if ch in lb and ch not in lc]))
    dA, dB, dC = ctx.array(bA), ctx.array(bB), ctx.array(up)
    call_contract(ctx, alpha, dA, A, la, dB, B, lb, beta, dC, Cv, lc, batch)
    got = dC.get()
    scale = max(1.0, np.abs(ref).max(initial=0.0))
    r = check_output(got, up, idx, ref, (1e-13 * max(1, K) ** 0.5 + 1e-14) * scale, what or spec)
    for x in (dA, dB, dC):
        x.free()
    return r


# ---------------------------------------------------------------------------------------------------------------------
# permutation fuzz
# ---------------------------------------------------------------------------------------------------------------------
PERM_EXTENTS = [1, 2, 3, 7, 8, 9, 31, 32, 33, 65]


def run_permutation(ctx, rng, li, lo, vin, vout, alpha, beta, what):
    """One pymes_permute between two (base, view) pairs; returns err / bound (0: the exact comparison)."""
    (bi, vi), (bo, vo) = vin, vout
    I, O = _layout(bi, vi), _layout(bo, vo)
    up, idx = output_base(rng, bo, vo, beta)
    ref = alpha * vi.transpose([li.index(ch) for ch in lo])
    if beta != 0.0:
        ref = ref + beta * up[idx]
    dI, dO = ctx.array(bi), ctx.array(up)
    call_permute(ctx, alpha, dI, I, li, beta, dO, O, lo)
    got = dO.get()
    exact = alpha == 1.0 and beta == 0.0
    r = check_output(got, up, idx, ref, None if exact else 1e-14, what)
    dI.free()
    dO.free()
    return r


def fixed_permutations(rng):
    """(name, li, lo, input view, output view, alpha, beta), each built for one path of dev::permute (csrc/kernels.hip)."""
    cases = []
    # tiled kernel, rank-6 canonical form [a, b, c, d, Q, L]: four rest dims that odd pitches keep unmerged on both sides,
    # Q = 33 (unit stride of the input) and L = 65 (unit stride of the output), neither a multiple of the 32-wide tile
    e = dict(a=2, b=3, c=2, d=3, q=33, l=65)
    cases.append(("tiled rank 6", "abcdql", "qdlbac",
                  padded_view(rng, "abcdql", e, "dcbalq", dict(q=2, l=2, a=1, b=1, c=1, d=1), lead=1),
                  padded_view(rng, "qdlbac", e, "abcdql", dict(l=2, q=2, d=1, c=1, b=1, a=1), lead=3), 1.0, 0.0))
    # tiled at its threshold Q = 8, L = 8 ...
    e = dict(r=3, q=8, l=8)
    cases.append(("tiled 8 x 8", "rql", "rql", padded_view(rng, "rql", e, "rlq", dict(q=1, l=1)),
                  padded_view(rng, "rql", e, "rql", dict(q=1, l=1)), -1.0, 0.0))
    # ... and Q = 7, which falls to the direct kernel
    e = dict(r=3, q=7, l=8)
    cases.append(("direct 7 x 8", "rql", "rql", padded_view(rng, "rql", e, "rlq", dict(q=1, l=1)),
                  padded_view(rng, "rql", e, "rql", dict(q=1, l=1)), 1.0, 0.0))
    # direct kernel over more than one trip of its grid-stride loop (more than 8192 x 256 elements): four odd extents that
    # pads keep unmerged on both sides, the same unit-stride axis in and out (so not the tiled kernel), accumulating
    e = dict(a=13, b=41, c=61, d=71)
    cases.append(("direct 2.3e6", "abcd", "cabd", padded_view(rng, "abcd", e, "bcad", dict(a=1, b=1, c=1, d=1), lead=1),
                  padded_view(rng, "cabd", e, "cabd", dict(a=1, b=1, c=1, d=1)), 0.5, -1.0))
    # the same element count with an extent-1 dim in the middle and a stride-0 input axis
    e = dict(a=13, b=41, x=1, c=61, d=71)
    cases.append(("direct 2.3e6 extent 1 stride 0", "abxcd", "cxabd",
                  padded_view(rng, "abxcd", e, "xbcad", dict(b=1, c=1, d=1, x=2), broadcast="a"),
                  padded_view(rng, "cxabd", e, "caxbd", dict(a=1, b=1, c=1, d=1, x=1), lead=1), 1.0, 0.0))
    # the identity permutation between two differently pitched views (Engine::axpby's route)
    e = dict(a=9, b=31, c=33)
    cases.append(("identity pitched", "abc", "abc", padded_view(rng, "abc", e, "abc", dict(b=1, c=3), lead=1),
                  padded_view(rng, "abc", e, "abc", dict(b=2, c=1)), 0.5, 1.0))
    return cases


def check_strided_permutations(lib, seed, mode="env", n_cases=150, fixed=True):
    """``n_cases`` random permutations of rank 1..6 between strided views (stride 0 on the input allowed), then the fixed
    cases.  Returns the worst err / bound."""
    rng = np.random.default_rng(1000 + seed)
    ctx = Context(2, 2, workspace_bytes=1 << 24, lib=lib)
    worst, done = 0.0, 0
    try:
        with launch_mode(ctx, mode):
            while done < n_cases:
                r = int(rng.integers(1, 7))
                dims = [int(rng.choice(PERM_EXTENTS)) for _ in range(r)]
                if np.prod(dims) > MAX_ELEMENTS:
                    continue
                li = LETTERS[:r]
                lo = "".join(rng.permutation(list(li)))
                vin = make_view(rng, dims, True)
                vout = make_view(rng, [dims[li.index(ch)] for ch in lo], False)
                if vin[0].size > 16 * MAX_ELEMENTS or vout[0].size > 16 * MAX_ELEMENTS:
                    continue
                alpha, beta = float(rng.choice([1.0, -1.0, 0.5])), float(rng.choice([0.0, 0.0, 1.0, -0.5]))
                what = dict(seed=seed, case=done, spec=f"{li}->{lo}", dims=dims, alpha=alpha, beta=beta, mode=mode,
                            strides_in=view_layout(*vin), strides_out=view_layout(*vout))
                worst = max(worst, run_permutation(ctx, rng, li, lo, vin, vout, alpha, beta, what))
                done += 1
            if fixed:
                for name, li, lo, vin, vout, alpha, beta in fixed_permutations(rng):
                    worst = max(worst, run_permutation(ctx, rng, li, lo, vin, vout, alpha, beta, dict(fixed=name, mode=mode)))
    finally:
        ctx.close()
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# integrals from strided device views
# ---------------------------------------------------------------------------------------------------------------------
BLOCK_NAMES = ["klij", "ijka", "ijak", "ijab", "iajk", "iajb", "iabj", "iabc",
               "aijk", "aijb", "aibj", "aibc", "abij", "abic", "abci", "abcd"]


def _block_of(V, name, no):
    return V[tuple(slice(no, None) if ch in "abcd" else slice(0, no) for ch in name)]


def _device_views_of_V(rng, n):
    """Two device layouts of one V[n,n,n,n]: a slice of a [n+1, n+2, n, n+3] base, and a base that holds it transposed."""
    e = dict(p=n, q=n, r=n, s=n)
    yield "sliced", padded_view(rng, "pqrs", e, "pqrs", dict(p=1, q=2, s=3), lead=(n + 3) * n + 2)
    yield "transposed", padded_view(rng, "pqrs", e, "srqp", dict(r=1), lead=1)


def check_strided_integrals(lib, no=3, nv=5):
    rng = np.random.default_rng(5)
    n = no + nv
    ctx = Context(no, nv, lib=lib)
    try:
        for how, (base, V) in _device_views_of_V(rng, n):
            off, st = view_layout(base, V)
            d = ctx.array(base)
            ctx.lib.call("pymes_set_V_pqrs", ctx.handle, _dev_ptr(d, off), 1, i64_array(st))
            for name in BLOCK_NAMES:
                assert np.array_equal(ctx.V_block(name).get(), _block_of(V, name, no)), (how, name)
            d.free()
        for name in ("iabc", "abcd"):
            shape = ctx.block_shape(name)
            e = dict(zip("pqrs", shape))
            base, X = padded_view(rng, "pqrs", e, "rpsq", dict(p=1, q=2, s=1), lead=3)
            off, st = view_layout(base, X)
            d = ctx.array(base)
            ctx.lib.call("pymes_set_V_block", ctx.handle, name.encode(), _dev_ptr(d, off), X.size, 1, i64_array(st))
            assert np.array_equal(ctx.V_block(name).get(), X), name
            d.free()
    finally:
        ctx.close()
    # an integral-sharded context (rank 1 of 2): the stored rows of V_abcd from a strided device view equal those of the
    # contiguous host upload
    rows = []
    (_, (base, V)), _ = _device_views_of_V(rng, n)
    for strided in (False, True):
        ctx = Context(no, nv, lib=lib, shard=(1, 2))
        try:
            if strided:
                off, st = view_layout(base, V)
                d = ctx.array(base)
                ctx.lib.call("pymes_set_V_pqrs", ctx.handle, _dev_ptr(d, off), 1, i64_array(st))
            else:
                ctx.set_V_pqrs(np.ascontiguousarray(V))
            rows.append(ctx.shard_rows())
            assert np.array_equal(ctx.V_block("iabc").get(), _block_of(V, "iabc", no))
        finally:
            ctx.close()
    (p0, m0, a0, a1), (p1, m1, b0, b1) = rows
    assert (a0, a1) == (b0, b1) and a1 > a0
    assert np.array_equal(p0, p1) and np.array_equal(m0, m1)
    assert np.isfinite(p0).all() and np.isfinite(m0).all()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def live_allocations(lib):
    n = C.c_int64()
    lib.call("pymes_live_allocations", C.byref(n))
    return n.value


def refused(fn, message):
    try:
        fn()
    except PymesError as e:
        assert message in str(e), (message, str(e))
        return
    raise AssertionError(f"not refused: expected '{message}'")
