"""The constructed hard-to-round cases of tests/hard_rounding.py, checked on the CPU: the closed-form expectations against
exact rational arithmetic, the construction's properties and counts, and -- with a small model of the default policy's
sequences (Mth<MATH_XACT>, csrc/pmaf_device.hpp) -- that the case sets catch the mistakes that matter where random
operands do not. The model shows what the cases can detect; it is no reference: the hardware's own answer is
tests/test_hard_rounding_gpu.py's, which sends every case generated here."""
import ast
import math
import os
import random
import struct

import hard_rounding as H

HERE = os.path.dirname(os.path.abspath(__file__))
N_SAMPLE = 2500                       # cases per family held to Fraction / isqrt (the families are generated in full)
SEEDS = (0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 2.0 ** -26, -2.0 ** -26, 2.0 ** -28, -2.0 ** -28,
         2.0 ** -30, -2.0 ** -30)       # modelled relative errors of the v_rcp_f64 / v_rsq_f64 seeds (documented: 2^-24)


def _sample(n, count, seed):
    return random.Random(seed).sample(range(n), min(count, n))


# ---- the module itself ----------------------------------------------------------------------------------------------
def test_module_is_standard_library_only():
    tree = ast.parse(open(os.path.join(HERE, "hard_rounding.py")).read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            assert node.level == 0
            mods.add(node.module.split(".")[0])
    assert mods <= {"math", "random", "array", "fractions", "functools"}, mods


def test_counts_meet_the_floors():
    counts, per_k = H.kept_counts()
    for fam, (kept, draws) in sorted(counts.items()):
        print("%-14s kept %8d of %8d draws" % (fam, kept, draws))
    for fam in ("div_random", "div_pow2", "div_all_ones", "sqrt_midpoint", "sqrt_twin", "a_over_sqrt"):
        assert counts[fam][0] >= H.FAMILY_FLOOR, (fam, counts[fam])
    ks = [k for k in range(1, H.POW2_KMAX, 2)]
    assert sorted(per_k) == sorted([-k for k in ks] + ks)
    print("near-power-of-two divisors: %d, kept per divisor %d .. %d" % (len(per_k), min(per_k.values()), max(per_k.values())))
    assert min(per_k.values()) >= H.POW2_FLOOR
    A = H.asqrt()
    near_one = sum(1 for k in A.k if k < 0)
    print("a / sqrt(b): %d roots rejected (RN(sqrt(RN(s^2))) != s), %d cases with a root within 64 ulp below 1" % (A.rejected_s, near_one))
    assert near_one >= 32 * 100


def test_closed_form_expectations_against_exact_arithmetic():
    for F in H.division_families() + (H.div_zero_numerators(),):
        for i in _sample(len(F), N_SAMPLE, 11):
            a, b, q = F.a[i], F.b[i], F.q[i]
            want = H.rn_fraction(H.to_fraction(a) / H.to_fraction(b))
            if a == 0.0:
                want = math.copysign(0.0, a) * math.copysign(1.0, b)
            assert want == q and math.copysign(1.0, want) == math.copysign(1.0, q), F.describe(i)
    for F in H.sqrt_families():
        for i in _sample(len(F), N_SAMPLE, 12):
            assert H.rn_sqrt(F.z[i]) == F.g[i], F.describe(i)
    F = H.asqrt()
    for i in _sample(len(F), N_SAMPLE, 13):
        s = H.rn_sqrt(F.b[i])
        assert s == F.s[i], F.describe(i)
        assert H.rn_fraction(H.to_fraction(F.a[i]) / H.to_fraction(s)) == F.q[i], F.describe(i)


def _exponent(x):
    return math.frexp(x)[1] - 1


def test_construction_properties():
    two = H.to_fraction(2.0)
    for F in H.division_families() + (H.asqrt(),):
        assert min(F.r) < 0 < max(F.r)                                  # both sides of the midpoint
        ea = [_exponent(x) for x in F.a]
        eb = [_exponent(x) for x in F.b]
        assert -H.EXP_RANGE <= min(ea) <= -H.EXP_RANGE + 5 and H.EXP_RANGE - 5 <= max(ea) <= H.EXP_RANGE, (F.family, min(ea), max(ea))
        assert -H.EXP_RANGE <= min(eb) and max(eb) <= H.EXP_RANGE
        if F.family in ("div_random", "div_pow2"):
            assert min(eb) <= -H.EXP_RANGE + 5 and max(eb) >= H.EXP_RANGE - 5
        if F.family != "a_over_sqrt":
            assert min(F.a) < 0 < max(F.a) and min(F.b) < 0 < max(F.b)  # both signs of both operands
        div = F.s if F.family == "a_over_sqrt" else F.b
        for i in _sample(len(F), N_SAMPLE, 21):
            v = H.to_fraction(F.a[i]) / H.to_fraction(div[i])
            q = H.to_fraction(F.q[i])
            side = 1 if F.r[i] > 0 else -1                              # r > 0: the quotient lies below the midpoint
            if v < 0:
                v, q = -v, -q
            # half the spacing of the doubles around the midpoint (q is the midpoint's neighbour on the quotient's side)
            m, e = math.frexp(abs(F.q[i]))
            if m == 0.5 and side < 0:
                e -= 1
            half = two ** (e - 54)
            mid = q + side * half
            dist_ulp = abs(mid - v) / (2 * half)
            assert 0 < (mid - v) * side and dist_ulp <= abs(F.r[i]) * two ** -52, F.describe(i)
    mid, twin = H.sqrt_families()
    for F, moduli in ((mid, (54, 55)), (twin, (52, 53))):
        assert min(F.r) < 0 < max(F.r)
        assert set(F.m) == set(moduli)                                  # both exponent parities of the construction
        ez = [_exponent(x) for x in F.z]
        assert {e & 1 for e in ez} == {0, 1}
        assert -H.EXP_RANGE - 1 <= min(ez) <= -H.EXP_RANGE + 5 and H.EXP_RANGE - 5 <= max(ez) <= H.EXP_RANGE
        for i in _sample(len(F), N_SAMPLE, 22):
            z, g = H.to_fraction(F.z[i]), H.to_fraction(F.g[i])
            m, e = math.frexp(F.g[i])
            ulp = two ** (e - 53)
            if F is mid:
                side = 1 if F.r[i] > 0 else -1                          # r > 0: the root lies below the midpoint
                if m == 0.5 and side < 0:
                    ulp /= 2
                t = g + side * ulp / 2                                  # the midpoint
                bound = abs(F.r[i]) * two ** -54
            else:
                side = 1 if F.r[i] > 0 else -1                          # r > 0: the root lies below the double
                t = g
                bound = abs(F.r[i]) * two ** -52
            # |sqrt(z) - t| = |z - t^2| / (sqrt(z) + t) < |z - t^2| / t   (t within an ulp of the root)
            assert (t * t - z) * side > 0 and abs(z - t * t) / t / ulp <= bound, F.describe(i)


# ---- a model of the MATH_XACT sequences: exact fused multiply-add, an explicit seed ------------------------------------
def _split(x):
    m, e = math.frexp(x)
    return int(math.ldexp(m, 53)), e - 53


def fma(a, b, c):
    """RN(a b + c) with IEEE's signs of zero; int / int and float(int) are correctly rounded in CPython"""
    (ma, ea), (mb, eb), (mc, ec) = _split(a), _split(b), _split(c)
    p, ep = ma * mb, ea + eb
    if p == 0 and mc == 0:
        neg = math.copysign(1.0, a) * math.copysign(1.0, b) < 0 and math.copysign(1.0, c) < 0
        return -0.0 if neg else 0.0
    if p == 0:
        return c
    e = min(ep, ec) if mc else ep
    n = (p << (ep - e)) + ((mc << (ec - e)) if mc else 0)
    if n == 0:
        return 0.0
    return n / (1 << -e) if e < 0 else float(n << e)


def rcp_refined(b, delta, steps=3, ones_select=True):
    """as written: three Newton steps and the select for a divisor whose mantissa is all ones (the odd one of the
    step's two fixed points). steps=2, ones_select=False is the sequence this project shipped before, which the
    hardware fails for the divisors (2^53 - k) 2^-53, k = 5, 11, 13 (tests/test_hard_rounding_gpu.py)"""
    r = (1.0 / b) * (1.0 + delta)             # v_rcp_f64, modelled
    for _ in range(steps):
        e = fma(-b, r, 1.0)
        r = fma(r, e, r)
    if ones_select and abs(math.frexp(b)[0]) == 1.0 - 2.0 ** -53:
        r = struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", r))[0] | 1))[0]
    return r


def rcp_two_steps(b, delta):
    return rcp_refined(b, delta, steps=2, ones_select=False)


def _fixup(q, b, a):                          # v_div_fixup for finite non-zero b: only a zero numerator differs from q
    return math.copysign(0.0, a) * math.copysign(1.0, b) if a == 0.0 else q


def div_r(a, b, r, residual=True):
    q = a * r
    if residual:
        e = fma(-b, q, a)
        q = fma(e, r, q)
    return _fixup(q, b, a)


def div_r_pos(a, b, r, as_written=True):
    q = a * r
    if as_written:
        e = fma(b, q, -a)
        return fma(-e, r, q)
    e = fma(-b, q, a)                         # the mutant: (+0) + (-0) = +0 loses the sign of a zero numerator
    return fma(e, r, q)


def sqrt_xact(z, delta, last=True):
    y = (1.0 / math.sqrt(z)) * (1.0 + delta)  # v_rsq_f64, modelled
    g, h = z * y, 0.5 * y
    r = fma(-h, g, 0.5)
    g = fma(g, r, g)
    h = fma(h, r, h)
    d = fma(-g, g, z)
    g = fma(d, h, g)
    if last:
        d = fma(-g, g, z)
        g = fma(d, h, g)
    return g, h


def rcp_from_sqrt(s, h):
    """the historical bug (csrc/pmaf_device.hpp, norm_rcp): the reciprocal of the root taken from the iteration's h"""
    rs = h + h
    e = fma(-s, rs, 1.0)
    return fma(rs, e, rs)


def _ulp_up(x, n):
    for _ in range(abs(n)):
        x = math.nextafter(x, math.copysign(math.inf, x) if n > 0 else 0.0)
    return x


DIV_MUTANTS = {
    "as written": lambda a, b, d: div_r(a, b, rcp_refined(b, d)),
    "one Newton step in the reciprocal": lambda a, b, d: div_r(a, b, rcp_refined(b, d, steps=1, ones_select=False)),
    "two Newton steps (before the fix)": lambda a, b, d: div_r(a, b, rcp_two_steps(b, d)),
    "no select for an all-ones divisor": lambda a, b, d: div_r(a, b, rcp_refined(b, d, ones_select=False)),
    "reciprocal 1 ulp high": lambda a, b, d: div_r(a, b, _ulp_up(rcp_refined(b, d), 1)),
    "reciprocal 1 ulp low": lambda a, b, d: div_r(a, b, _ulp_up(rcp_refined(b, d), -1)),
    "no residual step": lambda a, b, d: div_r(a, b, rcp_refined(b, d), residual=False),
}


def _random_pairs(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        a = math.ldexp(rng.getrandbits(52) | (1 << 52), rng.randrange(-250, 251) - 52)
        b = math.ldexp(rng.getrandbits(52) | (1 << 52), rng.randrange(-250, 251) - 52)
        out.append((a, b, H.rn_fraction(H.to_fraction(a) / H.to_fraction(b))))
    return out


def _constructed_division(n):
    R, P, A = H.div_random(), H.div_pow2(), H.div_all_ones()
    out = [(R.a[i], R.b[i], R.q[i]) for i in range(n // 2)]
    out += [(P.a[i], P.b[i], P.q[i]) for i in _sample(len(P), n // 4, 31)]
    out += [(A.a[i], A.b[i], A.q[i]) for i in _sample(len(A), n - n // 2 - n // 4, 32)]
    return out


def _wrong(fn, cases, seeds=(0.0, 2.0 ** -24, -2.0 ** -24)):
    """cases that some modelled seed gets wrong"""
    n = 0
    for a, b, want in cases:
        for d in seeds:
            got = fn(a, b, d)
            if got != want or math.copysign(1.0, got) != math.copysign(1.0, want):
                n += 1
                break
    return n


def test_the_cases_catch_the_division_mutants():
    n = 3000
    constructed, rnd = _constructed_division(n), _random_pairs(n, 41)
    print()
    # the block of divisors 2^53 - k, k < 64, whole: where a reciprocal beside RN(1 / b) shows (a handful of cases)
    P = H.div_pow2()
    near_one = [(P.a[i], P.b[i], P.q[i]) for i in range(len(P)) if -64 < P.k[i] < 0]
    for name, fn in DIV_MUTANTS.items():
        wc, wr = _wrong(fn, constructed), _wrong(fn, rnd)
        print("div, %-36s wrong on %4d of %d constructed cases, %4d of %d random pairs" % (name + ":", wc, n, wr, n))
        if "before the fix" in name or "all-ones" in name:
            wc = _wrong(fn, near_one)
            print("div, %-36s wrong on %4d of the %d cases of the divisors 2^53 - k, k < 64" % ("", wc, len(near_one)))
        if name != "as written":
            assert wc >= 1, name
        else:
            assert wc == 0 and _wrong(fn, near_one, SEEDS) == 0     # every seed of the band on the block beside 1
    # the first two are the ones random operands cannot see
    assert _wrong(DIV_MUTANTS["as written"], rnd) == 0
    # the sign of a zero numerator through the fixup-free division
    Z = H.div_zero_numerators()
    zc = [(Z.a[i], abs(Z.b[i]), Z.q[i] * math.copysign(1.0, Z.b[i])) for i in range(len(Z))]
    ok = _wrong(lambda a, b, d: div_r_pos(a, b, rcp_refined(b, d)), zc)
    bad = _wrong(lambda a, b, d: div_r_pos(a, b, rcp_refined(b, d), as_written=False), zc)
    rz = [(a, abs(b), q * math.copysign(1.0, b)) for a, b, q in rnd[:len(zc)]]
    bad_r = _wrong(lambda a, b, d: div_r_pos(a, b, rcp_refined(b, d), as_written=False), rz)
    print("div_r_pos, residual as a - b q:             wrong on %4d of %d zero numerators (as written: %d), %d of %d random pairs"
          % (bad, len(zc), ok, bad_r, len(rz)))
    assert ok == 0 and bad >= 1


def test_the_cases_catch_the_square_root_mutants():
    mid, twin = H.sqrt_families()
    n = 3000
    cases = [(mid.z[i], mid.g[i]) for i in _sample(len(mid), n // 2, 51)] + [(twin.z[i], twin.g[i]) for i in _sample(len(twin), n // 2, 52)]
    rng = random.Random(53)
    rnd = []
    for _ in range(n):
        z = math.ldexp(rng.getrandbits(52) | (1 << 52), rng.randrange(-250, 251) - 52)
        rnd.append((z, H.rn_sqrt(z)))
    print()
    for name, last in (("as written", True), ("without its last correction", False)):
        wc = sum(1 for z, g in cases if any(sqrt_xact(z, d, last)[0] != g for d in SEEDS[:3]))
        wr = sum(1 for z, g in rnd if any(sqrt_xact(z, d, last)[0] != g for d in SEEDS[:3]))
        print("sqrt, %-35s wrong on %4d of %d constructed cases, %4d of %d random arguments" % (name + ":", wc, n, wr, n))
        assert wc >= 1 if not last else wc == 0
    # a / sqrt(b) with the reciprocal taken from the root's iteration instead of rcp_refined(root)
    A = H.asqrt()
    near = [i for i in range(len(A)) if A.k[i] < 0]
    idx = near[::max(1, len(near) // (n // 2))][:n // 2]
    idx += _sample(len(A), n - len(idx), 54)

    def a_over_sqrt(a, b, d, historical):
        s, h = sqrt_xact(b, d)
        return div_r(a, s, rcp_from_sqrt(s, h) if historical else rcp_refined(s, d))
    ac = [(A.a[i], A.b[i], A.q[i]) for i in idx]
    ar = []
    for a, b, _ in _random_pairs(n, 55):
        b = abs(b)
        ar.append((a, b, H.rn_fraction(H.to_fraction(a) / H.to_fraction(H.rn_sqrt(b)))))
    for name, hist in (("as written", False), ("reciprocal from the sqrt iteration", True)):
        wc = _wrong(lambda a, b, d: a_over_sqrt(a, b, d, hist), ac)
        wr = _wrong(lambda a, b, d: a_over_sqrt(a, b, d, hist), ar)
        print("a / sqrt(b), %-28s wrong on %4d of %d constructed cases, %4d of %d random pairs" % (name + ":", wc, n, wr, n))
        assert wc >= 1 if hist else wc == 0


def test_seed_dependence_below_a_power_of_two():
    """For which divisors 2^53 - k do two Newton steps (the sequence before the fix) land beside RN(1 / b), for which
    modelled seeds, and which constructed quotients come out wrong then. Whether the hardware's v_rcp_f64 does was the
    GPU test's to answer -- it does, for k = 5, 11, 13 -- and every case the model fails here is one of those it sends
    (H.sent_to_gpu). The sequence as written gets every such case right for every seed of the band, and returns
    RN(1 / b) for every one of these divisors and for the all-ones ones."""
    P = H.div_pow2()
    assert any(F is P for F in H.sent_to_gpu()["div"])
    start = {}
    for i, k in enumerate(P.k):
        if k not in start:
            start[k] = i
    order = sorted(start.items(), key=lambda kv: kv[1])
    span = {k: (s, order[j + 1][1] if j + 1 < len(order) else len(P)) for j, (k, s) in enumerate(order)}
    print()
    n_div, n_cases, failed_k = 0, 0, set()
    for k in range(1, H.POW2_KMAX, 2):
        b = math.ldexp(float(H.M53 - k), -53)
        want = H.rn_fraction(1 / H.to_fraction(b))
        assert all(rcp_refined(b, d) == want for d in SEEDS), k          # as written: RN(1 / b), every seed
        off = [d for d in SEEDS if rcp_two_steps(b, d) != want]
        if not off:
            continue
        n_div += 1
        s, e = span[-k]
        failing = set()
        for i in range(s, e):
            for d in off:
                if div_r(P.a[i], P.b[i], rcp_two_steps(P.b[i], d)) != P.q[i]:
                    failing.add(i)
                    break
            # ... and as written, for every seed of the band, through both divisions
            for d in SEEDS:
                r = rcp_refined(P.b[i], d)
                assert div_r(P.a[i], P.b[i], r) == P.q[i], (P.describe(i), d)
                assert div_r_pos(P.a[i], abs(P.b[i]), abs(r)) == math.copysign(P.q[i], P.a[i]), (P.describe(i), d)
        assert all(s <= i < e <= len(P) and P.k[i] == -k for i in failing)
        n_cases += len(failing)
        if failing:
            failed_k.add(k)
        if k < 64 or failing:
            print("b = (2^53 - %4d) 2^-53: two Newton steps land beside RN(1/b) for seed errors %s; %d of %d constructed quotients wrong"
                  % (k, ", ".join("%+.0f*2^-30" % (d * 2.0 ** 30) for d in off), len(failing), e - s))
    print("%d of %d divisors 2^53 - k have a modelled seed that leaves two Newton steps beside RN(1 / b); %d constructed cases "
          "fail in the model (k: %s)" % (n_div, H.POW2_KMAX // 2, n_cases, sorted(failed_k)))
    # the hardware's failures (k = 5, 11, 13) are among the model's
    assert {5, 11, 13} <= failed_k
    # the all-ones divisors: as written every seed gives RN(1 / b); without the select the step's other fixed point stays
    stuck = 0
    for B, eb in H.ALL_ONES:
        b = math.ldexp(float(B), eb)
        want = H.rn_fraction(1 / H.to_fraction(b))
        assert all(rcp_refined(b, d) == want and rcp_refined(-b, d) == -want for d in SEEDS), b.hex()
        stuck += sum(1 for d in SEEDS if rcp_refined(b, d, ones_select=False) != want)
    print("all-ones divisors: %d (divisor, seed) pairs stay on the wrong fixed point without the select" % stuck)
    assert stuck >= 1
