"""The default policy's refined reciprocal as it is written now (Mth<MATH_XACT>::rcp_refined, csrc/pmaf_device.hpp): one
cubic step biased upwards by 2^-54 relative, then one exact Newton step -- no select on the divisor's mantissa. A model
of that sequence on the exact fused multiply-add of tests/test_hard_rounding.py, held to RN(1 / b) from Fraction for
every modelled seed error of v_rcp_f64, and the mutants that show why the bias has to be what it is.

The model in tests/test_hard_rounding.py (three plain Newton steps and the all-ones select) describes the sequence
this one replaced. It stays there as the historical model: its tests show what the constructed cases catch, and this
file does not change what they assert. As there, the model is no reference for the hardware -- the device's own answer
is tests/test_rcp_bias_gpu.py's (ops 18 - 20) and tests/test_hard_rounding_gpu.py's (the divisions built on it).

The second half models the reciprocal of a root taken from the root's own iteration (sqrt_seed / rcp_seeded): the
seed y (1 + r) of the Goldschmidt iteration, the biased step and the exact last step, without v_rcp_f64 -- the same
hard mantissas taken as roots, both neighbours of their squares, and the constructed a / sqrt(b) family. It is the
`2h + one Newton step` shortcut whose failure tests/test_hard_rounding.py keeps as a mutant, made right; taking its
last step away again is a mutant here.

What is held, and what is smaller than the divisors' own sets (the model is pure Python: an exact fma costs microseconds,
and the device's answer on the full sets is the GPU test's): every mantissa 2^53 - k and 2^52 + k, odd k < 4096, at five
exponents, both signs, the all-ones divisors, the powers of two, 20 000 random and 4 010 family divisors, for all eleven
seeds of the band; the mutants against every such mantissa at exponent 0 for all eleven seeds (the model is exactly
invariant under scaling by a power of two, which the five exponents of the first test show) and against 20 000 random
divisors for the seven seeds within the documented 2^-24. As roots: every such mantissa at three root exponents
(the radicand's exponent is twice the root's and stays within +-250), both neighbours of each radicand and 10 000
random radicands for seven seeds (the documented band, 4x beyond it and the two odd ones); the 4 000 sampled cases of the
a / sqrt(b) family and the division through them for 0 and +-2^-24."""
import math
import random

import hard_rounding as H
from test_hard_rounding import div_r, div_r_pos, fma

BIAS = 2.0 ** -54
# modelled relative errors of the v_rcp_f64 seed: the documented 2^-24 and inside it, 4x beyond it, two odd ones
SEEDS = (0.0, 2.0 ** -30, -2.0 ** -30, 2.0 ** -25, -2.0 ** -25, 2.0 ** -24, -2.0 ** -24, 2.0 ** -22, -2.0 ** -22, 3e-8, -1.1e-8)
EXPONENTS = (0, -37, 101, 250, -250)
KMAX = H.POW2_KMAX


def rcp_biased(b, delta, bias=BIAS, cubic=True, last=True):
    """as written. bias / cubic / last: the mutants"""
    r = (1.0 / b) * (1.0 + delta)             # v_rcp_f64, modelled
    e = fma(-b, r, 1.0)
    e = fma(e, e, e + bias) if cubic else e + bias
    r = fma(r, e, r)
    if last:
        e = fma(-b, r, 1.0)
        r = fma(r, e, r)
    return r


MUTANTS = {
    # name: (keyword arguments, the k of the divisors 2^53 - k that must come out wrong)
    "no bias": (dict(bias=0.0), {1}),
    "bias 2^-52": (dict(bias=2.0 ** -52), {1, 3}),
    "bias 2^-51": (dict(bias=2.0 ** -51), {1, 3, 5}),
    "bias -2^-54": (dict(bias=-BIAS), {1}),
    "quadratic first step": (dict(cubic=False), set(range(1, 16, 2))),
}


def _mantissas():
    """(k, integer mantissa): -k for 2^53 - k, +k for 2^52 + k, odd k < 4096"""
    return [(-k, H.M53 - k) for k in range(1, KMAX, 2)] + [(k, (1 << 52) + k) for k in range(1, KMAX, 2)]


def _want(mant):
    """RN(1 / mant) for the integer mantissa, exactly; scaling by a power of two is exact within the range"""
    return H.rn_fraction(1 / H.to_fraction(float(mant)))


def _hard_divisors():
    """(k, b, RN(1 / b)) at every exponent of EXPONENTS"""
    out = []
    for k, mant in _mantissas():
        w = _want(mant)
        for e in EXPONENTS:
            out.append((k, math.ldexp(float(mant), e - 52), math.ldexp(w, 52 - e)))
    return out


def _random_divisors(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        b = math.ldexp(rng.getrandbits(52) | (1 << 52), rng.randrange(-250, 251) - 52)
        out.append((0, b, H.rn_fraction(1 / H.to_fraction(b))))
    return out


def _family_divisors(n):
    """divisors of the constructed division families (tests/hard_rounding.py), both signs as they come"""
    out = []
    for F, seed in zip(H.division_families(), (71, 72, 73)):
        seen = set()
        for i in random.Random(seed).sample(range(len(F)), min(len(F), 4 * n)):
            b = F.b[i]
            if b in seen:
                continue
            seen.add(b)
            out.append((F.k[i], b, H.rn_fraction(1 / H.to_fraction(b))))
            if len(seen) >= n // 3:
                break
    return out


def _wrong(cases, seeds=SEEDS, **kw):
    """the cases some modelled seed gets wrong"""
    return [(k, b) for k, b, want in cases if any(rcp_biased(b, d, **kw) != want for d in seeds)]


def test_every_hard_divisor_and_every_seed_gives_the_correctly_rounded_reciprocal():
    hard = _hard_divisors()
    assert len(hard) == 2 * (KMAX // 2) * len(EXPONENTS)
    bad = _wrong(hard)
    assert not bad, [(k, b.hex()) for k, b in bad[:10]]
    # both signs: the sequence is odd in b (the bias is relative: it enters through e, which does not see b's sign)
    neg = [(k, -b, -w) for k, b, w in hard]
    assert not _wrong(neg)
    # the five all-ones divisors and their neighbours of test_xact_sequences_match_ieee, both signs
    for B, eb in H.ALL_ONES:
        b = math.ldexp(float(B), eb)
        want = H.rn_fraction(1 / H.to_fraction(b))
        for d in SEEDS:
            assert rcp_biased(b, d) == want and rcp_biased(-b, d) == -want, (b.hex(), d)
    print("\n%d hard divisors x %d seeds, %d negated, %d all-ones: every reciprocal is RN(1 / b)" % (len(hard), len(SEEDS), len(neg), len(H.ALL_ONES)))


def test_powers_of_two_and_one_stay_exact():
    """norm_unit<true> divides by a selected 1.0 and relies on rcp_refined(1.0) == 1.0; v_rcp_f64 returns the exact
    reciprocal of a power of two or a neighbour, and the band's seeds are held too"""
    seeds = SEEDS + (2.0 ** -52, -2.0 ** -53, 2.0 ** -51, -2.0 ** -52)
    for d in seeds:
        assert rcp_biased(1.0, d) == 1.0 and rcp_biased(-1.0, d) == -1.0, d
    for e in range(-250, 251):
        b = math.ldexp(1.0, e)
        for d in seeds:
            assert rcp_biased(b, d) == math.ldexp(1.0, -e) and rcp_biased(-b, d) == -math.ldexp(1.0, -e), (e, d)


def test_random_and_family_divisors():
    rnd = _random_divisors(20000, 61)
    fam = _family_divisors(6000)
    # (the all-ones family has ten distinct divisors, the other two give 2000 each)
    assert len(fam) >= 4000 and min(b for _, b, _ in fam) < 0 < max(b for _, b, _ in fam)
    seeds = SEEDS
    assert not _wrong(rnd, seeds) and not _wrong(fam, seeds)
    print("\n%d random and %d family divisors x %d seeds: every reciprocal is RN(1 / b)" % (len(rnd), len(fam), len(seeds)))


def test_the_biased_step_arrives_where_the_last_step_needs_it():
    """the premise of the exact last step, in Fraction: behind the biased cubic step r lies within 1 ulp of 1 / b and
    never more than 1/4 ulp below it, and for an all-ones divisor it IS the odd one of the last step's two fixed points"""
    for k, mant in _mantissas()[:64] + _mantissas()[KMAX // 2:KMAX // 2 + 64]:
        b = math.ldexp(float(mant), -52)
        inv = 1 / H.to_fraction(b)
        ulp = H.to_fraction(math.ulp(_want(mant) * 2.0 ** 52))
        for d in SEEDS:
            r = H.to_fraction(rcp_biased(b, d, last=False))
            assert -ulp / 4 <= r - inv < ulp, (k, d)
    for B, eb in H.ALL_ONES:
        if B != H.M53 - 1:
            continue
        b = math.ldexp(float(B), eb)
        for d in SEEDS:
            r = rcp_biased(b, d, last=False)
            assert math.frexp(r)[0] == 0.5 + 2.0 ** -53, (b.hex(), d, r.hex())      # 2^-n (1 + 2^-52)


def test_the_constructed_divisors_catch_the_mutants_and_random_ones_do_not():
    hard = [(k, math.ldexp(float(mant), -52), _want(mant) * 2.0 ** 52) for k, mant in _mantissas()]   # every k, exponent 0
    rnd = _random_divisors(20000, 62)
    seeds = SEEDS[:7]                                # random divisors and the quotients below: 0, +-2^-30, +-2^-25, +-2^-24
    print()
    assert not _wrong(hard) and not _wrong(rnd, seeds)                               # as written
    for name, (kw, must) in MUTANTS.items():
        wc = _wrong(hard, SEEDS, **kw)
        ks = sorted({-k for k, _ in wc if k < 0})
        wr = _wrong(rnd, seeds, **kw)
        print("rcp, %-22s wrong for 2^53 - k, k in %s%s; %d of %d random divisors" % (
            name + ":", ks[:12], " ..." if len(ks) > 12 else "", len(wr), len(rnd)))
        assert must <= set(ks), (name, ks)
        if "bias" in name:
            assert not wr, name                                                       # random divisors see no bias mutant
    # ... and through the divisions built on the reciprocal: a quotient of the constructed family comes out wrong
    P = H.div_pow2()
    near = [i for i in range(len(P)) if -8 < P.k[i] < 0]
    for name in ("no bias", "bias 2^-52", "bias 2^-51", "bias -2^-54"):
        kw = MUTANTS[name][0]
        bad = sum(1 for i in near if any(div_r(P.a[i], P.b[i], rcp_biased(P.b[i], d, **kw)) != P.q[i] for d in seeds))
        good = sum(1 for i in near if any(div_r(P.a[i], P.b[i], rcp_biased(P.b[i], d)) != P.q[i] for d in seeds))
        print("div, %-22s %d of %d constructed quotients of the divisors 2^53 - k, k < 8 wrong (as written: %d)" % (name + ":", bad, len(near), good))
        assert bad >= 1 and good == 0, name


def test_divisions_on_the_biased_reciprocal_return_the_constructed_quotients():
    """div_r and div_r_pos (unchanged) on the new reciprocal, over a sample of every constructed division family and
    the whole block of divisors 2^53 - k, k < 64"""
    seeds = (0.0, 2.0 ** -24, -2.0 ** -24)
    P = H.div_pow2()
    idx = {id(P): [i for i in range(len(P)) if -64 < P.k[i] < 0]}
    for F, seed in zip(H.division_families(), (81, 82, 83)):
        for i in idx.get(id(F), []) + random.Random(seed).sample(range(len(F)), 1500):
            a, b, q = F.a[i], F.b[i], F.q[i]
            for d in seeds:
                r = rcp_biased(b, d)
                assert div_r(a, b, r) == q, (F.describe(i), d)
                assert div_r_pos(a, abs(b), abs(r)) == math.copysign(q, a), (F.describe(i), d)


# ---- the reciprocal of a root from the root's own iteration (sqrt_seed / rcp_seeded, csrc/pmaf_device.hpp) -------------
ROOT_EXPONENTS = (0, 101, -125)               # of the root: the radicand's stays within +-250


def sqrt_seed(z, delta):
    """the policy's root WITHOUT its zero / infinity select, and y2 = y (1 + r) ~ 1 / root out of the same iteration"""
    y = (1.0 / math.sqrt(z)) * (1.0 + delta)  # v_rsq_f64, modelled
    g, h = z * y, 0.5 * y
    r = fma(-h, g, 0.5)
    g = fma(g, r, g)
    y2 = fma(y, r, y)
    h = fma(h, r, h)
    d = fma(-g, g, z)
    g = fma(d, h, g)
    d = fma(-g, g, z)
    g = fma(d, h, g)
    return g, y2


def rcp_seeded(s, y2, bias=BIAS, last=True):
    e = fma(-s, y2, 1.0) + bias
    r = fma(y2, e, y2)
    if last:
        e = fma(-s, r, 1.0)
        r = fma(r, e, r)
    return r


def _radicands():
    """(k, z): RN(s^2) for every hard mantissa s taken as a root, and its two neighbours, at every exponent"""
    out = []
    for k, mant in _mantissas():
        sq = H.rn_fraction(H.to_fraction(float(mant)) ** 2)
        for e in ROOT_EXPONENTS:
            z = math.ldexp(sq, 2 * (e - 52))
            out += [(k, z), (k, math.nextafter(z, math.inf)), (k, math.nextafter(z, 0.0))]
    return out


def _root_failures(cases, seeds, **kw):
    bad = []
    for k, z in cases:
        want_s = H.rn_sqrt(z)
        want_r = H.rn_fraction(1 / H.to_fraction(want_s))
        for d in seeds:
            g, y2 = sqrt_seed(z, d)
            if g != want_s or rcp_seeded(g, y2, **kw) != want_r:
                bad.append((k, z))
                break
    return bad


def test_the_reciprocal_of_a_root_through_the_roots_seed():
    seeds = (0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -22, -2.0 ** -22, 3e-8, -1.1e-8)
    hard = _radicands()
    bad = _root_failures(hard, seeds)
    assert not bad, [(k, z.hex()) for k, z in bad[:10]]
    rng = random.Random(63)
    rnd = [(0, math.ldexp(rng.getrandbits(52) | (1 << 52), rng.randrange(-250, 251) - 52)) for _ in range(10000)]
    assert not _root_failures(rnd, seeds)
    A = H.asqrt()
    fam = [(A.k[i], A.b[i]) for i in random.Random(64).sample(range(len(A)), 4000)]
    assert not _root_failures(fam, seeds[:3])
    # a / sqrt(b) through the seeded reciprocal and the fixup-free division (op 20 on the device)
    for i in random.Random(65).sample(range(len(A)), 2000) + [i for i in range(len(A)) if A.k[i] < 0][::8]:
        for d in seeds[:3]:
            g, y2 = sqrt_seed(A.b[i], d)
            assert g == A.s[i] and div_r_pos(A.a[i], g, rcp_seeded(g, y2)) == A.q[i], (A.describe(i), d)
    # a selected divisor of 1.0 takes a selected seed of 1.0 and gives 1.0
    assert rcp_seeded(1.0, 1.0) == 1.0
    # the mutants: without the exact last step (the historical shortcut's flaw), and without the bias
    no_last = _root_failures(hard, seeds, last=False)
    no_bias = _root_failures(hard, seeds, bias=0.0)
    rnd_no_bias = _root_failures(rnd, seeds[:3], bias=0.0)
    print("\nroot-seed path: %d radicands, %d random, %d of a / sqrt(b); without the last step %d wrong, without the bias %d "
          "(roots 2^53 - k, k in %s; %d of the random ones)" % (len(hard), len(rnd), len(fam), len(no_last), len(no_bias),
                                                                 sorted({-k for k, _ in no_bias if k < 0})[:8], len(rnd_no_bias)))
    assert len(no_last) >= 1 and len(no_bias) >= 1 and not rnd_no_bias
