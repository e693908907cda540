"""The EE-EOM sigma build (csrc/eom.cpp, EomSigma) on every symmetry branch: inputs, expected flags and checks shared by
tests/test_eom.py (host simulator), tests/test_gpu_eom_branches.py and tests/test_gpu_nocc_cap.py.  TEST INFRASTRUCTURE ONLY.

The constructor tests its inputs on the device and every step of the build forks on the outcome:
  v_sym     V_abcd = V_badc
  t_sym     T_abij = T_baji
  hole_sym  t_sym, and B2 = V_klij + V_klcd T_cdij and V_ijab have the exchange symmetry
``branch_case`` starts from integrals and amplitudes that have all of them and adds noise WITHOUT the symmetry to the named inputs;
the device and the oracle read the same blocks, so a perturbed block is as valid an input as any other.
"""
import ctypes as C

import numpy as np

from oracle import cc_oracle as oc
from oracle import eom_oracle as eo
from oracle.cases import random_case
from tests import _lambda_reference as R

BREAKS = ("abcd", "klij", "ijab", "t2")
NOISE = 0.05
# (v_sym, t_sym, hole_sym) the noise is meant to give, and the inputs it goes to; the tests assert ``expected_flags``, not this column
STATES = (
    ((1, 1, 1), ()),
    ((1, 1, 0), ("klij",)),
    ((1, 1, 0), ("ijab",)),
    ((1, 0, 0), ("t2",)),
    ((0, 1, 1), ("abcd",)),
    ((0, 1, 0), ("abcd", "klij")),
    ((0, 0, 0), ("abcd", "t2")),
)
STATE_IDS = ["v%dt%dh%d-%s" % (s + ("+".join(b) or "none",)) for s, b in STATES]


def tr(x):
    return x.transpose(1, 0, 3, 2)


def branch_case(no, nv, seed, break_=()):
    """(f, Vb, t2): ``random_case(symmetric=True)`` split into blocks, 0.05 N(0,1) added to every input named in ``break_``
    ("abcd", "klij", "ijab": that block of V; "t2": the amplitudes), and a Fock matrix that is not symmetric."""
    for name in break_:
        if name not in BREAKS:
            raise ValueError("branch_case: unknown input %r" % (name,))
    f, V, _, t2 = random_case(no, nv, seed, symmetric=True)
    Vb = {k: np.array(b) for k, b in oc.split_blocks(no, V).items()}
    f = f + 0.02 * np.random.default_rng(seed + 1).standard_normal(f.shape)
    for k, name in enumerate(BREAKS):              # (one generator per input: what one input gets does not depend on the others)
        if name not in break_:
            continue
        rng = np.random.default_rng(1000 * seed + 17 + k)
        if name == "t2":
            t2 = t2 + NOISE * rng.standard_normal(t2.shape)
        else:
            Vb[name] = Vb[name] + NOISE * rng.standard_normal(Vb[name].shape)
    return f, Vb, np.ascontiguousarray(t2)


def _symmetric(x):
    """The device's criterion (EomSigma::exchange_symmetric): max |x - P x| <= 1e-13 max(1, max |x|)."""
    return bool(np.abs(x - tr(x)).max() <= 1e-13 * max(1.0, np.abs(x).max()))


def expected_flags(no, Vb, t2):
    """(v_sym, t_sym, hole_sym) by the definitions in the constructor.  A block with an extent of one cannot lose the symmetry,
    whatever was added to it."""
    B2 = Vb["klij"] + np.einsum("klcd,cdij->klij", Vb["ijab"], t2, optimize=True)
    t_sym = _symmetric(t2)
    return _symmetric(Vb["abcd"]), t_sym, bool(t_sym and _symmetric(B2) and _symmetric(Vb["ijab"]))


def handle_flags(sig):
    """What the handle itself says (pymes_eom_sigma_flags), asked again."""
    fl = C.c_int()
    sig.ctx.lib.call("pymes_eom_sigma_flags", sig._h, C.byref(fl))
    fl = fl.value
    assert (bool(fl & 1), bool(fl & 2), bool(fl & 4), bool(fl & 8), bool(fl & 16)) == (sig.v_sym, sig.t_sym, sig.hole_sym, sig.fused_ok,
                                                                                  sig.many_ok)
    assert sig.many_ok == (sig.v_sym and sig.t_sym and sig.hole_sym and sig.fused_ok)
    return sig.v_sym, sig.t_sym, sig.hole_sym


class Case:
    """One problem with the oracle's results for its vectors, computed once per vector however many builds are compared."""

    def __init__(self, no, nv, seed, break_=(), problem=None):
        self.no, self.nv, self.seed, self.break_ = no, nv, seed, tuple(break_)
        self.f, self.Vb, self.t2 = problem if problem is not None else branch_case(no, nv, seed, break_)
        self._right, self._left = {}, {}

    @property
    def flags(self):
        return expected_flags(self.no, self.Vb, self.t2)

    def right(self, u1, u2):
        key = (u1.tobytes(), u2.tobytes())
        if key not in self._right:
            self._right[key] = (eo.sigma_singles(self.no, self.f, self.Vb, u1, u2, self.t2),
                                eo.sigma_doubles(self.no, self.f, self.Vb, u1, u2, self.t2))
        return self._right[key]

    def left(self, l1, l2):
        key = (l1.tobytes(), l2.tobytes())
        if key not in self._left:
            self._left[key] = R.left_sigma(self.no, self.f, self.Vb, l1, l2, self.t2)
        return self._left[key]

    def upload(self, ctx, names):
        for name in names:
            ctx.set_V_block(name, np.ascontiguousarray(self.Vb[name]))


def vectors(no, nv, seed, syms):
    """(u1s, u2s): u2_z exchange-symmetric bit for bit where syms[z], without any symmetry elsewhere."""
    rng = np.random.default_rng(seed)
    u1s = [rng.standard_normal((nv, no)) for _ in syms]
    u2s = [rng.standard_normal((nv, nv, no, no)) for _ in syms]
    return u1s, [np.ascontiguousarray(u + tr(u)) if s else u for u, s in zip(u2s, syms)]


def _nan_outputs(ctx, k):
    no, nv = ctx.no, ctx.nv
    return ([ctx.array(np.full((nv, no), np.nan)) for _ in range(k)],
            [ctx.array(np.full((nv, nv, no, no), np.nan)) for _ in range(k)])


def check_right(ctx, sig, case, u1s, u2s, syms, tol, keep=None, label=""):
    """One ``apply_many`` of the k vectors into caller arrays filled with NaN; every vector against the oracle and against the
    build of that vector alone, each at ``tol`` x max(1, max |sigma2 of the oracle|).  ``syms``: declared per vector, or None
    (detected on the device).  Returns the worst error against the oracle in units of that scale; ``keep``: a list that
    receives the 2 k host arrays (to compare runs bit for bit)."""
    k = len(u1s)
    d1, d2 = [ctx.array(u) for u in u1s], [ctx.array(u) for u in u2s]
    o1, o2 = _nan_outputs(ctx, k)
    res = sig.apply_many(d1, d2, syms=syms, out1=o1, out2=o2)
    worst = single = 0.0
    for z in range(k):
        assert res[z][0] is o1[z] and res[z][1] is o2[z]
        g1, g2 = o1[z].get(), o2[z].get()
        assert np.all(np.isfinite(g1)) and np.all(np.isfinite(g2)), (label, z, "an element was not written")
        r1, r2 = case.right(u1s[z], u2s[z])
        sc = max(1.0, np.abs(r2).max())
        err = max(np.abs(g1 - r1).max(), np.abs(g2 - r2).max()) / sc
        s1, s2 = sig.apply(d1[z], d2[z], None if syms is None else bool(syms[z]))
        one = max(np.abs(g1 - s1.get()).max(), np.abs(g2 - s2.get()).max()) / sc
        worst, single = max(worst, err), max(single, one)
        assert err <= tol, (label, z, "against the oracle", err, tol)
        assert one <= tol, (label, z, "stacked against single", one, tol)
        if keep is not None:
            keep += [g1, g2]
    print("right %s k=%d syms=%s: oracle %.2e = %.2e of the bound, stacked - single %.2e" % (label, k, _short(syms), worst, worst / tol,
                                                                                           single))
    return worst


def check_left(ctx, sig, case, l1s, l2s, syms, tol, keep=None, label=""):
    """``apply_left_many`` of k left vectors (l2 exchange-symmetric) into NaN-filled caller arrays against
    tests/_lambda_reference.left_sigma and against the build of each vector alone, at ``tol`` x max(|r1|, |r2|); the doubles
    of the result lie on the symmetric subspace exactly.  Returns the worst error in units of that scale."""
    k = len(l1s)
    d1, d2 = [ctx.array(u) for u in l1s], [ctx.array(u) for u in l2s]
    o1, o2 = _nan_outputs(ctx, k)
    res = sig.apply_left_many(d1, d2, syms=syms, out1=o1, out2=o2)
    worst = single = 0.0
    for z in range(k):
        assert res[z][0] is o1[z] and res[z][1] is o2[z]
        g1, g2 = o1[z].get(), o2[z].get()
        assert np.all(np.isfinite(g1)) and np.all(np.isfinite(g2)), (label, z, "an element was not written")
        r1, r2 = case.left(l1s[z], l2s[z])
        sc = max(np.abs(r1).max(), np.abs(r2).max())
        err = max(np.abs(g1 - r1).max(), np.abs(g2 - r2).max()) / sc
        s1, s2 = sig.apply_left(d1[z], d2[z], None if syms is None else bool(syms[z]))
        one = max(np.abs(g1 - s1.get()).max(), np.abs(g2 - s2.get()).max()) / sc
        worst, single = max(worst, err), max(single, one)
        assert err <= tol, (label, z, "against left_sigma", err, tol)
        assert one <= tol, (label, z, "stacked against single", one, tol)
        assert np.array_equal(g2, tr(g2)), (label, z)
        if keep is not None:
            keep += [g1, g2]
    print("left  %s k=%d syms=%s: reference %.2e = %.2e of the bound, stacked - single %.2e" % (label, k, _short(syms), worst,
                                                                                             worst / tol, single))
    return worst


def _short(syms):
    return "detected" if syms is None else "".join(str(int(bool(s))) for s in syms)


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def right_tol(no, nv):
    """The bounds tests/test_eom.py::check_apply_many asserts for this build: 1e-11 up to ov = 15, 1e-10 above."""
    return 1e-11 if no * nv <= 15 else 1e-10


LEFT_TOL = 1e-10          # tests/test_gpu_lambda.py::test_left_apply_against_the_reference


def sensitivity(case, u1, u2):
    """The oracle alone: for every input named in ``case.break_`` the sigma2 of the same problem with that input symmetrised,
    (x + P x) / 2, differs from the true one by more than 1e-4 max |sigma2| — a build that took the symmetric branch on this case
    could not pass.  Returns {name: difference / max |sigma2|}."""
    ref = case.right(u1, u2)[1]
    out = {}
    for name in case.break_:
        Vb, t2 = dict(case.Vb), case.t2
        if name == "t2":
            t2 = 0.5 * (t2 + tr(t2))
        else:
            Vb[name] = 0.5 * (Vb[name] + tr(Vb[name]))
        out[name] = np.abs(eo.sigma_doubles(case.no, case.f, Vb, u1, u2, t2) - ref).max() / np.abs(ref).max()
        assert out[name] > 1e-4, (case.no, case.nv, name, out[name])
    return out


# ---- the cases of the right build that the host simulator and the kernels both run (tests/test_eom.py, test_gpu_eom_branches.py) ------
VECTOR_SETS = ((True, True, True), (False, False, False), (True, False, True))      # the last: the deferred ladder when v_sym holds


def lattice_right(ctx, sig, case, keep=None, label=""):
    """k = 3, all symmetric / none / mixed, declared and detected.  Returns the worst error over the bound."""
    tol = right_tol(case.no, case.nv)
    worst = 0.0
    for n, sy in enumerate(VECTOR_SETS):
        u1s, u2s = vectors(case.no, case.nv, 10 * case.seed + n, sy)
        for syms in (list(sy), None):
            worst = max(worst, check_right(ctx, sig, case, u1s, u2s, syms, tol, keep, label) / tol)
    return worst


# (k, symmetry of each vector, state) at (3,4): the tails and flushes of the batch loops
BOUNDARY_RIGHT = (
    (17, (True,) * 17, ()),                  # stacks of up to 16 and a tail of one
    (9, (False,) * 9, ()),                   # deferred ladders: a flush at eight, then one
    (17, (False,) * 17, ()),                 # 8 + 8 + 1
    (9, (False,) * 9, ("klij",)),
    (5, (True, False, True, False, False), ()),
)
