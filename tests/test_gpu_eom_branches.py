"""GPU: the EE-EOM sigma build (csrc/eom.cpp, EomSigma) on every symmetry branch, right and left.

The constructor tests V_abcd, T and B2 = V_klij + V_klcd T on the device and every step of doubles(), stack(), general_ladders(),
apply() and apply_left() forks on the flags it sets.  The sibling modules reach two corners of that lattice (everything
symmetric; nothing symmetric) and the left build on a symmetric T only.  Here the seven states of tests/_eom_branch_cases.STATES
are reached by noise on single inputs, ASSERTED through pymes_eom_sigma_flags against numpy, and run
  a. right, k = 3 symmetric / general / mixed vectors, declared and detected, at (3,5) and (7,6) (no > nv, odd no); (3,5)
     with phase launches on, off and serial (every mode against the oracle; whether the modes agree to the bit is printed)
  b. left, k = 1 and 3, the same states, shapes and modes: left_build with t_sym or hole_sym false
  c. the batch boundaries at (3,4): k = 17, flushes of the deferred ladders at eight vectors, a mixed batch
  d. stacked builds with o^2 = 289 > 256 at (17,4), and o^2 = 256 at (16,3)
  e. extents of one and two
  f. a handle on T1-dressed blocks
against oracle/eom_oracle.py (right) and tests/_lambda_reference.left_sigma (left) at the bounds the sibling modules assert for
these builds: right 1e-11 max(1, max |sigma2|) up to ov = 15 and 1e-10 above, left 1e-10 max(|r1|, |r2|).  Outputs go into
NaN-filled arrays of the caller and every vector is also built alone.  The right cases of a. and c. run on the CPU stand-in in
tests/test_eom.py::test_sigma_branch_lattice_host_logic, where test_sigma_branch_cases_can_fail shows with the oracle alone that
symmetrising any broken input moves sigma2 by more than 1e-4 of its size.  Recorded errors: profiles/eom_branches/."""
import numpy as np
import pytest

from oracle import cc_oracle as oc
from pymes_amd.device import Context
from pymes_amd.integral.partition import BLOCK_NAMES
from tests import _eom_branch_cases as BC
from tests.test_gpu_sym_tail import env
from tests.test_gpu_transitions import _live

pytestmark = pytest.mark.gpu
MODES = (("on", None), ("off", "0"), ("serial", "serial"))
LATTICE_SHAPES = [(3, 5), (7, 6)]
SEED = 7


def bools(want):
    return tuple(bool(x) for x in want)


class built:
    """``with built(gpu_lib, case) as (ctx, sig):`` — a context with the blocks of the case, a LeftSigma handle on them whose
    flags are what numpy says; nothing is left allocated afterwards."""

    def __init__(self, lib, case, want=None):
        self.lib, self.case, self.want = lib, case, want

    def __enter__(self):
        from pymes_amd.solver.lambda_ccsd import LeftSigma
        case = self.case
        self.before = _live()
        self.ctx = Context(case.no, case.nv, lib=self.lib, workspace_bytes=1 << 24)
        try:
            case.upload(self.ctx, LeftSigma.BLOCKS)
            self.sig = self.handle()
        except BaseException:
            self.ctx.close()
            raise
        return self.ctx, self.sig

    def handle(self):
        from pymes_amd.solver.lambda_ccsd import LeftSigma
        sig = LeftSigma(self.ctx, self.case.f, self.ctx.array(self.case.t2))
        got = BC.handle_flags(sig)
        assert got == self.case.flags, (got, self.case.flags, self.case.break_)
        if self.want is not None:
            assert got == bools(self.want), (got, self.want)
        assert sig.fused_ok
        return sig

    def __exit__(self, *exc):
        self.ctx.close()
        self.sig = self.ctx = None
        if exc[0] is None:
            assert _live() == self.before
        return False


def in_modes(ctx, shape, run):
    """``run(label)`` -> (worst error over the bound, the outputs) under every phase mode at (3,5), under the default elsewhere.
    Phases on must have recorded tasks and phases off none, or the mode was not the one that ran."""
    modes = MODES if shape == (3, 5) else MODES[:1]
    kept = {}
    for name, value in modes:
        with env(ctx, PYMES_PHASE=value, PYMES_PHASE_MAX_US=None):
            before = ctx.phase_stats()["tasks"]
            worst, kept[name] = run(name)
            ctx.sync()
            recorded = ctx.phase_stats()["tasks"] - before
        assert (recorded > 0) == (name != "off"), (name, recorded)
        assert worst <= 1.0
    if len(kept) == 3:
        print("   bit-identical: on/off %s, on/serial %s" % (BC.same_bits(kept["on"], kept["off"]), BC.same_bits(kept["on"], kept["serial"])))


# ---- a. the lattice, right -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", BC.STATES, ids=BC.STATE_IDS)
@pytest.mark.parametrize("shape", LATTICE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_lattice_right(gpu_lib, shape, state):
    want, brk = state
    case = BC.Case(shape[0], shape[1], SEED, brk)
    b = built(gpu_lib, case, want)
    with b as (ctx, _):
        def run(mode):
            sig = b.handle()                        # (hoisted under the mode as well)
            keep = []
            worst = BC.lattice_right(ctx, sig, case, keep, "(%d,%d) %s %s" % (shape + ("+".join(brk) or "none", mode)))
            sig.close()
            return worst, keep
        in_modes(ctx, shape, run)


# ---- b. the lattice, left ------------------------------------------------------------------------------------------------------------
def lattice_left(ctx, sig, case, keep, label):
    worst = 0.0
    for k in (1, 3):
        l1s, l2s = BC.vectors(case.no, case.nv, 20 * case.seed + k, (True,) * k)
        for syms in ([True] * k, None):
            worst = max(worst, BC.check_left(ctx, sig, case, l1s, l2s, syms, BC.LEFT_TOL, keep, label) / BC.LEFT_TOL)
    return worst


@pytest.mark.parametrize("state", BC.STATES, ids=BC.STATE_IDS)
@pytest.mark.parametrize("shape", LATTICE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_lattice_left(gpu_lib, shape, state):
    """left_build, as a stack of one and of three, on a handle whose flags are not all set: a wrong number here is a finding in
    csrc/eom.cpp."""
    want, brk = state
    case = BC.Case(shape[0], shape[1], SEED, brk)
    b = built(gpu_lib, case, want)
    with b as (ctx, _):
        def run(mode):
            sig = b.handle()
            keep = []
            worst = lattice_left(ctx, sig, case, keep, "(%d,%d) %s %s" % (shape + ("+".join(brk) or "none", mode)))
            sig.close()
            return worst, keep
        in_modes(ctx, shape, run)


# ---- c. the batch boundaries (the outputs are tested, not the split: stack_limit() depends on the free device memory) ------------------
@pytest.mark.parametrize("k,sy,brk", BC.BOUNDARY_RIGHT, ids=["k17-sym", "k9-general", "k17-general", "k9-general-klij", "k5-mixed"])
def test_batch_boundaries_right(gpu_lib, k, sy, brk):
    no, nv = 3, 4
    case = BC.Case(no, nv, SEED, brk)
    with built(gpu_lib, case, (1, 1, 0) if brk else (1, 1, 1)) as (ctx, sig):
        u1s, u2s = BC.vectors(no, nv, 100 + k, sy)
        tol = BC.right_tol(no, nv)
        assert BC.check_right(ctx, sig, case, u1s, u2s, list(sy), tol, label="(3,4) %s" % ("+".join(brk) or "none")) <= tol


def test_batch_boundaries_left(gpu_lib):
    no, nv, k = 3, 4, 17
    case = BC.Case(no, nv, SEED)
    with built(gpu_lib, case, (1, 1, 1)) as (ctx, sig):
        l1s, l2s = BC.vectors(no, nv, 100 + k, (True,) * k)
        assert BC.check_left(ctx, sig, case, l1s, l2s, [True] * k, BC.LEFT_TOL, label="(3,4) none") <= BC.LEFT_TOL


# ---- d. o^2 > 256: the second trip of the e += 256 loops of the k-vector t2_layouts, hole_ladder_packed_multi, residual_assemble,
# lambda_assemble; exchange_split, a batched ladder_sym_multi of six and sgn_ij_add for general vectors ------------------------------------
PAST_ONE_TRIP = [
    ((17, 4), (1, 1, 1), (), "right", (True, True, True)),
    ((17, 4), (1, 1, 1), (), "left", (True, True, True)),
    ((17, 4), (1, 1, 0), ("klij",), "right", (True, True, True)),
    ((17, 4), (1, 0, 0), ("t2",), "right", (True, True)),
    ((17, 4), (1, 0, 0), ("t2",), "left", (True, True)),
    ((17, 4), (1, 1, 1), (), "right", (False, False, False)),
    ((16, 3), (1, 1, 1), (), "right", (True, True, True)),
    ((16, 3), (1, 1, 1), (), "left", (True, True, True)),
]


@pytest.mark.parametrize("shape,want,brk,side,sy", PAST_ONE_TRIP,
                         ids=["%dx%d-%s-%s-%s" % (c[0] + ("+".join(c[2]) or "none", c[3], "".join(str(int(s)) for s in c[4])))
                              for c in PAST_ONE_TRIP])
def test_stacked_past_one_trip(gpu_lib, shape, want, brk, side, sy):
    no, nv = shape
    case = BC.Case(no, nv, SEED, brk)
    with built(gpu_lib, case, want) as (ctx, sig):
        x1s, x2s = BC.vectors(no, nv, 300 + len(sy), sy)
        label = "(%d,%d) %s" % (no, nv, "+".join(brk) or "none")
        if side == "right":
            tol = BC.right_tol(no, nv)
            assert BC.check_right(ctx, sig, case, x1s, x2s, list(sy), tol, label=label) <= tol
        else:
            assert BC.check_left(ctx, sig, case, x1s, x2s, list(sy), BC.LEFT_TOL, label=label) <= BC.LEFT_TOL


# ---- e. extents of one and two: La and the packed antisymmetric rows are empty at no = 1 or nv = 1 ------------------------------------
@pytest.mark.parametrize("brk", [(), ("klij", "ijab"), BC.BREAKS], ids=["none", "klij+ijab", "all"])
@pytest.mark.parametrize("shape", [(1, 3), (3, 1), (2, 2), (1, 1), (2, 1)], ids=lambda s: "%dx%d" % s)
def test_degenerate_extents(gpu_lib, shape, brk):
    """The flags are what numpy finds on the inputs: a block with an extent of one keeps its symmetry whatever is added to it."""
    no, nv = shape
    case = BC.Case(no, nv, SEED, brk)
    v_, t_, h_ = case.flags
    if not brk or (no, nv) == (1, 1):
        assert (v_, t_, h_) == (True, True, True)
    else:
        assert v_ == ("abcd" not in brk or nv == 1) and t_ == ("t2" not in brk) and not h_
    with built(gpu_lib, case) as (ctx, sig):
        tol, label = BC.right_tol(no, nv), "(%d,%d) %s" % (no, nv, "+".join(brk) or "none")
        for sy in ((True, True), (False, False)):
            u1s, u2s = BC.vectors(no, nv, 400 + sy[0], sy)
            for syms in (list(sy), None):
                assert BC.check_right(ctx, sig, case, u1s, u2s, syms, tol, label=label) <= tol
        l1s, l2s = BC.vectors(no, nv, 402, (True, True))
        assert BC.check_left(ctx, sig, case, l1s, l2s, [True, True], BC.LEFT_TOL, label=label) <= BC.LEFT_TOL


# ---- f. a handle on the context's T1-dressed blocks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("want,brk", [((1, 1, 1), ()), ((0, 0, 0), ("abcd", "t2"))], ids=["v1t1h1", "v0t0h0"])
def test_dressed_handle(gpu_lib, want, brk):
    """All sixteen blocks uploaded as they are, the blocks the build reads dressed on the device; the oracle reads
    cc_oracle.dressed_V of the same blocks, and the flags are those of the DRESSED blocks."""
    from pymes_amd.solver.eom_ccsd import _Sigma
    no, nv = 3, 5
    f, Vb, t2 = BC.branch_case(no, nv, SEED, brk)
    t1 = 0.1 * np.random.default_rng(SEED + 2).standard_normal((nv, no))
    Vd = oc.dressed_V(t1, Vb, _Sigma.BLOCKS)
    case = BC.Case(no, nv, SEED, brk, problem=(oc.dressed_fock(no, f, t1, Vb), Vd, t2))
    assert max(np.abs(Vd[k] - Vb[k]).max() for k in ("abcd", "klij", "iabc")) > 1e-3
    assert case.flags == bools(want)
    before = _live()
    ctx = Context(no, nv, lib=gpu_lib, workspace_bytes=1 << 24)
    try:
        for name in BLOCK_NAMES:
            ctx.set_V_block(name, np.ascontiguousarray(Vb[name]))
        ctx.dress_V(ctx.array(t1), _Sigma.BLOCKS)
        sig = _Sigma(ctx, case.f, ctx.array(t2), dressed=True)
        assert BC.handle_flags(sig) == bools(want)
        tol = BC.right_tol(no, nv)
        for sy in ((True, True), (False, False), (True, False)):
            u1s, u2s = BC.vectors(no, nv, 500 + sum(sy), sy)
            assert BC.check_right(ctx, sig, case, u1s, u2s, list(sy), tol, label="(3,5) dressed %s" % ("+".join(brk) or "none")) <= tol
    finally:
        ctx.close()
    assert _live() == before
