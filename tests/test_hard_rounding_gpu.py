"""The device's elementary operations against the constructed hard-to-round cases of tests/hard_rounding.py.

MATH_XACT, the default arithmetic policy (csrc/pmaf_device.hpp), claims the correctly rounded IEEE bits for operands
whose exponents lie within +-250: every constructed case is compared for bit equality, sign of zero included -- the
quotients through ops 6 and 11, a / sqrt(b) through ops 9 and 12, the roots through ops 5 and 13 (pmaf_debug_math,
include/pmaf.h). The compiler's own sequences (ops 0, 1, 10) get the same cases in a test of their own: a mismatch there
is a finding about the expectation or the toolchain, not about the policy. (These cases found the policy's division
1 ulp low for the divisor mantissas 2^53 - 5, - 11, - 13, its refined reciprocal being the neighbour of RN(1 / b) there;
rcp_refined has taken a third Newton step since. The compiler's division still returns those three: NOTES.md 1.)

MATH_FAST, the opt-in policy, claims an error bound instead: tests/hp_reference.py's per-operation EPS_FAST. Ops 14-17
are held to the bound hp_reference.Arith("fast") carries for the same expression on exact inputs, on the constructed
cases and on 10^6 random operands, and the largest error seen is printed in ulp."""
from fractions import Fraction

import numpy as np
import pytest

import hard_rounding as H
import hp_reference as R

pytestmark = pytest.mark.gpu

# the three quotients the modelled sequence gets 1 ulp low when rcp_refined lands beside RN(1 / b) (divisors 2^53 - k,
# k = 1, 5, 11; tests/test_hard_rounding.py prints for which modelled seeds): (a, b, RN(a / b))
MODEL_FAILURES = (("0x1p-1", "0x1.fffffffffffffp-1", "0x1.0000000000001p-1"),
                  ("0x1.6666666666663p-1", "0x1.ffffffffffffbp-1", "0x1.6666666666667p-1"),
                  ("0x1.5d1745d1745cap-1", "0x1.ffffffffffff5p-1", "0x1.5d1745d1745d2p-1"))


def _np(arr):
    return np.frombuffer(arr, dtype=np.float64 if arr.typecode == "d" else np.int32)


@pytest.fixture(scope="module")
def sent():
    """every family, generated once: the arrays go to the device whole"""
    return H.sent_to_gpu()


def _same_bits(got, want):
    return got.view(np.uint64) == want.view(np.uint64)


def _mismatches(F, op, got, want, operands):
    """'' when every result has the expected bits, else the report: the count, the divisors / residues hit, and the
    first cases with operands, result and expectation in hex"""
    bad = np.flatnonzero(~_same_bits(got, want))
    if bad.size == 0:
        return ""
    lines = ["op %d, %s: %d of %d cases differ from the correctly rounded result" % (op, F.family, bad.size, len(F))]
    if hasattr(F, "k"):
        ks, n = np.unique(_np(F.k)[bad], return_counts=True)
        lines.append("  by k (+k: divisor mantissa 2^52 + k, -k: 2^53 - k, 0: other): " + ", ".join("%d: %d" % kn for kn in list(zip(ks, n))[:40]))
    for i in bad[:25]:
        lines.append("  %s | sent %s | got %s, expected %s" % (F.describe(int(i)), ", ".join(float(x[i]).hex() for x in operands),
                                                               float(got[i]).hex(), float(want[i]).hex()))
    return "\n".join(lines)


def _check(pmaf, F, op, a, b, want):
    got = pmaf.debug_math(op, a, b)
    assert got.shape == want.shape
    return _mismatches(F, op, got, want, (a, b))


def _division_operands(F, positive_divisor):
    a, b, q = _np(F.a), _np(F.b), _np(F.q)
    if positive_divisor:                      # the fixup-free variants take a positive divisor: a / |b| = q sign(b), exactly
        return a, np.abs(b), q * np.sign(b)
    return a, b, q


@pytest.mark.parametrize("op", [6, 11])
def test_xact_division_returns_the_correctly_rounded_quotient(pmaf, sent, op):
    reports = []
    n = 0
    for F in sent["div"] + sent["zero"]:
        a, b, q = _division_operands(F, op == 11)
        reports.append(_check(pmaf, F, op, a, b, q))
        n += len(F)
    # the hardware's answer to the seed-dependence question: the divisors 2^53 - k, odd k < 64
    P = sent["div"][1]
    k = _np(P.k)
    sel = (k < 0) & (k > -64)
    a, b, q = _division_operands(P, op == 11)
    got = pmaf.debug_math(op, a[sel], b[sel])
    wrong = ~_same_bits(got, q[sel])
    print("op %d: %d constructed quotients compared; divisors (2^53 - k) 2^-53, odd k < 64: %d of %d wrong%s" % (
        op, n, wrong.sum(), sel.sum(), "" if not wrong.any() else " (k: %s)" % sorted(set((-k[sel][wrong]).tolist()))))
    ex = np.array([[float.fromhex(x) for x in row] for row in MODEL_FAILURES])
    got = pmaf.debug_math(op, ex[:, 0].copy(), ex[:, 1].copy())
    for row, g in zip(MODEL_FAILURES, got):
        print("op %d: %s / %s = %s (correctly rounded: %s)" % (op, row[0], row[1], float(g).hex(), row[2]))
    reports.append("" if _same_bits(got, ex[:, 2].copy()).all() else "op %d: the modelled failures fail on the device too" % op)
    assert not any(reports), "\n".join(r for r in reports if r)


@pytest.mark.parametrize("op", [9, 12])
def test_xact_division_by_a_root_returns_the_correctly_rounded_quotient(pmaf, sent, op):
    (F,) = sent["asqrt"]
    a, b, q, s = _np(F.a), _np(F.b), _np(F.q), _np(F.s)
    # the construction's premise on the device: the root the quotient is formed with is s
    assert _same_bits(pmaf.debug_math(5, b), s).all()
    report = _check(pmaf, F, op, a, b, q)
    print("op %d: %d constructed a / sqrt(b) compared" % (op, len(F)))
    assert not report, report


@pytest.mark.parametrize("op", [5, 13])
def test_xact_square_root_returns_the_correctly_rounded_root(pmaf, sent, op):
    reports = []
    for F in sent["sqrt"]:
        z, g = _np(F.z), _np(F.g)
        reports.append(_check(pmaf, F, op, z, z, g))
        print("op %d: %d %s cases compared" % (op, len(F), F.family))
    assert not any(reports), "\n".join(r for r in reports if r)


def _compiler_report(pmaf, F, op, a, b, want, exact):
    """the compiler's sequence on one family: its mismatches are printed (the finding), each one's EXPECTATION is held to
    exact rational arithmetic (`exact(i)`: it is then the toolchain's result that is not correctly rounded, not the
    expectation), and the result must still be the expectation's neighbour. Returns the number of mismatches."""
    got = pmaf.debug_math(op, a, b)
    report = _mismatches(F, op, got, want, (a, b))
    if report:
        print("FINDING (toolchain) -- " + report)
    bad = np.flatnonzero(~_same_bits(got, want))
    for i in bad:
        assert exact(int(i)) == float(want[i]), "the expectation is wrong: " + F.describe(int(i))
        assert got[i] in (np.nextafter(want[i], np.inf), np.nextafter(want[i], -np.inf)), report
    return bad.size


def test_compiler_sequences_on_the_same_cases(pmaf, sent):
    """ops 0, 1, 10: the compiler's own expansions of a / b, sqrt and a / sqrt(b) (MATH_IEEE; every division outside the
    tuned rollout kernels) on the same cases. A mismatch is a finding about the expectation or the toolchain, not about
    the default policy: it is reported here, apart from the policy's tests, the expectation of every mismatching case is
    re-derived in exact rational arithmetic, and the sequence is held to faithful rounding (the neighbour at worst).

    Measured (MI355X, ROCm 7.2): the division expansion (v_rcp_f64, two Newton steps, one
    residual step in v_div_fmas) returns the quotient 1 ulp low for 3 of the 2 532 307 division cases -- divisor
    mantissas 2^53 - 5, 2^53 - 11, 2^53 - 13 with the residue -1, e.g. 0x1.6666666666663p-1 / 0x1.ffffffffffffbp-1 --
    and for the 3 cases of a / sqrt(b) with those roots; 0 of the 339 348 roots differ. The reciprocal its two Newton
    steps leave for these divisors is the neighbour of RN(1 / b) (csrc/pmaf_device.hpp, rcp_refined)."""
    n_div = n_sqrt = n_asqrt = 0
    for F in sent["div"] + sent["zero"]:
        a, b = _np(F.a), _np(F.b)
        n_div += _compiler_report(pmaf, F, 0, a, b, _np(F.q), lambda i: H.rn_fraction(H.to_fraction(F.a[i]) / H.to_fraction(F.b[i])))
    for F in sent["sqrt"]:
        n_sqrt += _compiler_report(pmaf, F, 1, _np(F.z), _np(F.z), _np(F.g), lambda i: H.rn_sqrt(F.z[i]))
    (F,) = sent["asqrt"]
    n_asqrt = _compiler_report(pmaf, F, 10, _np(F.a), _np(F.b), _np(F.q),
                               lambda i: H.rn_fraction(H.to_fraction(F.a[i]) / H.to_fraction(H.rn_sqrt(F.b[i]))))
    print("compiler sequences: %d quotients, %d roots, %d a / sqrt(b) not correctly rounded" % (n_div, n_sqrt, n_asqrt))
    # the root's expansion (v_rsq_f64 + Goldschmidt with a final correction) has no such class: bit equality
    assert n_sqrt == 0


# ---- MATH_FAST: error against the exact value, within hp_reference's bound ---------------------------------------------
# Every element's error is measured twice. (1) All of them, vectorised: the residual of the defining equation (got b - a,
# got^2 - z, got^2 b - a^2) in double-double arithmetic -- Dekker's exact product, one Sterbenz-exact subtraction -- which
# gives the relative error to about 2^-50 of itself; it is compared with the least relative bound Arith("fast") carries
# for the expression over a spread of operands, shrunk by 2^-40 to cover the estimate's own rounding (the bound of these
# expressions is a multiple of |value|: hp_reference._round). (2) The elements with the largest errors, exactly: Fraction
# for a quotient, hp_reference's 113-bit value for a root, against the .e Arith("fast") carries for that very element.
_SPLITTER = 134217729.0        # 2^27 + 1 (Veltkamp)
N_EXACT = 300                   # elements per op and set held to Arith's own .e
N_RANDOM = 1_000_000


def _two_prod(x, y):
    p = x * y
    t = _SPLITTER * x
    xh = t - (t - x)
    xl = x - xh
    t = _SPLITTER * y
    yh = t - (t - y)
    yl = y - yh
    return p, ((xh * yh - p) + xh * yl + xl * yh) + xl * yl


def _rel_err_div(got, a, b):
    p, e = _two_prod(got, b)
    return np.abs((p - a) + e) / np.abs(a)


def _rel_err_sqrt(got, z):
    p, e = _two_prod(got, got)
    return np.abs((p - z) + e) / (2.0 * z)                         # (g^2 - z) / (g + sqrt z) / sqrt z


def _rel_err_div_root(got, a, b):
    p1, e1 = _two_prod(got, got)
    p2, e2 = _two_prod(p1, b)
    p3, e3 = _two_prod(a, a)
    return np.abs((p2 - p3) + ((e2 + e1 * b) - e3)) / (2.0 * p3)   # (w^2 b - a^2) / (2 a^2)


def _expr(A, kind, a, b):
    if kind == "div":
        return A.div(A.c(a), A.c(b))
    if kind == "sqrt":
        return A.sqrt(A.c(a))
    return A.div(A.c(a), A.sqrt(A.c(b)))


def _least_relative_bound(kind):
    A = R.Arith("fast")
    rng = np.random.default_rng(5)
    rel = []
    for e in range(-240, 241, 8):
        a, b = np.ldexp(rng.uniform(1.0, 2.0), e), np.ldexp(rng.uniform(1.0, 2.0), int(rng.integers(-240, 241)))
        q = _expr(A, kind, a, b)
        rel.append(q.e / abs(float(q.v)))
    # the premise of the vectorised check: the bound of these expressions is one multiple of |value| at every scale
    # (the samples differ only by the rounding of the bound arithmetic itself, which hp_reference inflates for)
    assert max(rel) - min(rel) <= 2.0 ** -44 * min(rel), (kind, min(rel), max(rel))
    return min(rel) * (1.0 - 2.0 ** -40)


def _exact_check(kind, got, a, b, idx):
    A = R.Arith("fast")
    worst = 0.0
    for i in idx:
        q = _expr(A, kind, float(a[i]), float(b[i]))
        if kind == "div":
            err = abs(Fraction(float(got[i])) - Fraction(float(a[i])) / Fraction(float(b[i])))
            assert err <= Fraction(q.e), (kind, float(a[i]).hex(), float(b[i]).hex(), float(got[i]).hex(), float(err), q.e)
        else:
            err = abs(R.MPF(float(got[i])) - q.v)
            assert err <= q.e, (kind, float(a[i]).hex(), float(b[i]).hex(), float(got[i]).hex(), float(err), q.e)
        worst = max(worst, float(err) / float(np.spacing(abs(got[i]))))
    return worst


def _fast_sets(sent):
    """(name, a, b) per operation kind: the constructed cases, then random operands in the planner's range (half within
    its lengths / speeds / gains, half across the validated 2^-100 .. 2^100)"""
    rng = np.random.default_rng(17)
    n = N_RANDOM // 2

    def rnd():
        return np.concatenate([rng.uniform(1e-6, 4.0, n), np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-100, 100, n))])
    sign = rng.choice([-1.0, 1.0], 2 * n)
    div = [(F.family, _np(F.a), _np(F.b)) for F in sent["div"]] + [("random", rnd() * sign, rnd() * sign[::-1])]
    sq = [(F.family, _np(F.z), _np(F.z)) for F in sent["sqrt"]] + [("random", rnd(), rnd())]
    (F,) = sent["asqrt"]
    dr = [(F.family, _np(F.a), _np(F.b)), ("random", rnd() * sign, rnd())]
    return div, sq, dr


@pytest.mark.parametrize("op,kind", [(14, "div"), (15, "sqrt"), (16, "rsqrt"), (17, "div_root")])
def test_fast_policy_stays_within_the_reference_bound(pmaf, sent, op, kind):
    div, sq, dr = _fast_sets(sent)
    sets = {"div": div, "sqrt": sq, "rsqrt": sq, "div_root": dr}[kind]
    ekind = "div_root" if kind == "rsqrt" else kind
    bound = _least_relative_bound(ekind)
    worst_ulp, worst_rel = 0.0, 0.0
    for name, a, b in sets:
        if kind == "rsqrt":                                            # y ~ 1 / sqrt(b): the expression div(c(1), sqrt(c(b)))
            a = np.ones_like(b)
        got = pmaf.debug_math(op, a, b)
        assert np.isfinite(got).all()
        rel = {"div": _rel_err_div, "div_root": _rel_err_div_root}[ekind](got, a, b) if ekind != "sqrt" else _rel_err_sqrt(got, a)
        worst = np.argsort(rel)[-N_EXACT:]
        spread = np.random.default_rng(op).choice(rel.size, N_EXACT // 3, replace=False)
        ulp = _exact_check(ekind, got, a, b, np.concatenate([worst, spread]))
        print("op %d, %-13s %8d operands: largest error %.3f ulp (relative %.3g = %.3f of the reference's bound %.3g)" % (
            op, name + ":", rel.size, ulp, rel.max(), rel.max() / bound, bound))
        worst_ulp, worst_rel = max(worst_ulp, ulp), max(worst_rel, rel.max())
        assert rel.max() <= bound, (op, name, float(a[worst[-1]]).hex(), float(b[worst[-1]]).hex(), float(got[worst[-1]]).hex())
    print("op %d (%s): largest error over all sets %.3f ulp, %.3f of the reference's bound" % (op, kind, worst_ulp, worst_rel / bound))
