"""Constructed hard-to-round operands for a / b, sqrt(z) and a / sqrt(b), with exact expectations.

TEST INFRASTRUCTURE ONLY. Standard library only (Python ints, `fractions`, `math.isqrt`); like tests/hp_reference.py it
imports neither oracle/ nor the package's ctypes layer (tests/test_hard_rounding.py checks this with `ast`).

A Newton / residual sequence for a quotient or a root can only go wrong where the exact result lies within about
2^-53 ulp of the midpoint between two doubles; random operands come within about 1e-7 ulp of one and never get there.
Such operands can be written down in integer arithmetic, and the correctly rounded result with them -- no floating
point takes part in an expectation (math.ldexp of an integer below 2^54 that has at most 53 significant bits is exact).

Division. B odd, below 2^53; r a small odd residue of either sign; X = r B^-1 mod 2^54. Kept iff X lies in
[2^53, 2^54): X is odd, so X / 2^54 is the midpoint between two neighbouring doubles of [1/2, 1). Then
A = (B X - r) / 2^54 is an integer below 2^53 and A / B = X / 2^54 - r / (2^54 B): |r| / (2 B) ulp from the midpoint, on
the side r says. RN(A / B) = (X - 1) / 2^54 for r > 0, (X + 1) / 2^54 for r < 0.

Square root (Kahan). r = 1 (mod 8) of either sign; X^2 = r (mod 2^m) solved by Hensel lifting. For m = 54, 55 (the two
exponent parities), X odd in [2^53, 2^54) and Z = (X^2 - r) / 2^m in [2^52, 2^53): sqrt(Z 2^m) = sqrt(X^2 - r) lies
|r| / (4 X) ~ |r| 2^-55 ulp (an ulp is 2 here) from the midpoint X. RN = X - 1 for r > 0, X + 1 for r < 0. The even twins:
m = 52, 53 and X odd in [2^52, 2^53), where X itself is a double and the root lies |r| / (2 X) ulp beside it: RN = X.

a / sqrt(b) (the code rounds the root first). s odd below 2^53, b = RN(s^2), kept only where integer arithmetic
confirms RN(sqrt(b)) = s; the numerators are the division's hard numerators for the divisor s.

The only filtering is the construction's own range condition on X and Z. Every family is scaled by powers of two
(even ones under a root) and signs so that the operands' exponents cover +-250, the range the default arithmetic
policy documents (csrc/pmaf_device.hpp). Families are generated once per process and returned as arrays of doubles.
"""
import math
import random
from array import array
from fractions import Fraction
from functools import lru_cache

M53 = 1 << 53
M54 = 1 << 54
EXP_RANGE = 250                 # operand exponents (floor(log2 |x|)) are drawn from [-EXP_RANGE, EXP_RANGE]
POW2_KMAX = 4096                # divisors 2^53 - k and 2^52 + k for every odd k below this
POW2_RMAX = 1100                # their residues: every odd |r| below this, both signs (about half survive).
#                                 |r| = 1 must stay in the band (_odd_band starts at 1): a reciprocal 1 ulp off RN(1 / b)
#                                 shows on ONE numerator per divisor, the residue -1 one, 2^-54 ulp above its midpoint
#                                 (tests/test_hard_rounding.py pins it: k = 5, 11, 13 must fail in the model)
POW2_FLOOR = 500                # kept cases every such divisor must reach
FAMILY_FLOOR = 100_000          # kept cases every family must reach
# the five divisors of test_xact_sequences_match_ieee whose mantissa is all ones, and their neighbours, as
# (odd integer, exponent): 1 - 2^-53, 1 - 2^-52, 1 + 2^-52, 2 - 2^-52, 1/2 - 2^-54
ALL_ONES = ((M53 - 1, -53), ((1 << 52) - 1, -52), ((1 << 52) + 1, -52), (M53 - 1, -52), (M53 - 1, -54))
ALL_ONES_RMAX = 1 << 16


class DivCases:
    """a / b = q (q the correctly rounded quotient), structure of arrays; k: +k for the divisor mantissa 2^52 + k, -k
    for 2^53 - k, 0 elsewhere; r: the residue (its sign is the side of the midpoint the exact quotient lies on);
    draws: how many (divisor, residue) pairs were tried"""

    def __init__(self, family):
        self.family = family
        self.a, self.b, self.q = array("d"), array("d"), array("d")
        self.k, self.r = array("i"), array("i")
        self.draws = 0

    def __len__(self):
        return len(self.a)

    def describe(self, i):
        return "%s k=%d r=%d: %s / %s, expected %s" % (self.family, self.k[i], self.r[i], self.a[i].hex(), self.b[i].hex(),
                                                       self.q[i].hex())


class SqrtCases:
    """sqrt(z) = g (g the correctly rounded root); r: the residue; m: the modulus exponent of the construction (54 / 55:
    the root lies beside a midpoint; 52 / 53, the even twins: beside a double)"""

    def __init__(self, family):
        self.family = family
        self.z, self.g = array("d"), array("d")
        self.r, self.m = array("i"), array("i")
        self.draws = 0

    def __len__(self):
        return len(self.z)

    def describe(self, i):
        return "%s m=%d r=%d: sqrt(%s), expected %s" % (self.family, self.m[i], self.r[i], self.z[i].hex(), self.g[i].hex())


def _exp_and_signs(rng):
    """two operand exponents in [-EXP_RANGE, EXP_RANGE] and two signs out of one draw"""
    bits = rng.getrandbits(32)
    span = 2 * EXP_RANGE + 1
    return ((bits & 0x3fff) % span - EXP_RANGE, ((bits >> 14) & 0x3fff) % span - EXP_RANGE,
            -1.0 if bits & (1 << 30) else 1.0, -1.0 if bits & (1 << 31) else 1.0)


def _add_division(out, B, residues, rng, k=0, eb=None, b_exp_range=EXP_RANGE):
    """the hard numerators of the odd divisor mantissa B for the given residues; eb: a fixed exponent of the divisor
    (b = +-B 2^eb), else its exponent is drawn like the numerator's (clipped to +-b_exp_range)"""
    binv = pow(B, -1, M54)
    bl = B.bit_length() - 1
    ldexp = math.ldexp
    a_, b_, q_, k_, r_ = out.a, out.b, out.q, out.k, out.r
    for r in residues:
        out.draws += 1
        X = (r * binv) & (M54 - 1)
        if X < M53:
            continue
        A = (B * X - r) >> 54
        Xr = X - 1 if r > 0 else X + 1
        ta, tb, sa, sb = _exp_and_signs(rng)
        ea = ta - (A.bit_length() - 1)
        if eb is None:
            e = tb * b_exp_range // EXP_RANGE - bl
        else:
            e = eb
        a_.append(ldexp(sa * A, ea))
        b_.append(ldexp(sb * B, e))
        q_.append(ldexp(sa * sb * Xr, ea - e - 54))
        k_.append(k)
        r_.append(r)


def _odd_band(rmax):
    res = []
    for m in range(1, rmax, 2):
        res.append(m)
        res.append(-m)
    return res


@lru_cache(maxsize=None)
def div_random():
    """random odd 53-bit divisors, one small residue each"""
    rng = random.Random(0x5eed01)
    out = DivCases("div_random")
    for _ in range(230_000):
        B = rng.getrandbits(52) | (1 << 52) | 1
        r = (2 * rng.randrange(32) + 1) * (1 if rng.getrandbits(1) else -1)
        _add_division(out, B, (r,), rng)
    return out


@lru_cache(maxsize=None)
def div_pow2():
    """divisors beside a power of two -- norms beside 1: unit vectors, cross products of unit vectors"""
    rng = random.Random(0x5eed02)
    out = DivCases("div_pow2")
    band = _odd_band(POW2_RMAX)
    for k in range(1, POW2_KMAX, 2):
        _add_division(out, M53 - k, band, rng, k=-k)
        _add_division(out, (1 << 52) + k, band, rng, k=k)
    return out


@lru_cache(maxsize=None)
def div_all_ones():
    """the five all-ones divisors as they stand (either sign), numerators at every exponent"""
    rng = random.Random(0x5eed03)
    out = DivCases("div_all_ones")
    band = _odd_band(ALL_ONES_RMAX)
    for B, eb in ALL_ONES:
        _add_division(out, B, band, rng, eb=eb)
    return out


@lru_cache(maxsize=None)
def div_zero_numerators():
    """+-0 / b: the quotient is a zero whose sign is the operands' signs' product (the fixup-free division must keep it)"""
    rng = random.Random(0x5eed04)
    out = DivCases("div_zero")
    mant = [M53 - 1, M53 - 5, (1 << 52) + 1, 1 << 52] + [rng.getrandbits(52) | (1 << 52) for _ in range(252)]
    for B in mant:
        for sa in (1.0, -1.0):
            _, tb, _, sb = _exp_and_signs(rng)
            out.draws += 1
            out.a.append(sa * 0.0)
            out.b.append(math.ldexp(sb * B, tb - 52))
            out.q.append(sa * sb * 0.0)
            out.k.append(0)
            out.r.append(0)
    return out


def division_families():
    """every division family, in the order the GPU test sends them"""
    return (div_random(), div_pow2(), div_all_ones())


def sent_to_gpu():
    """what tests/test_hard_rounding_gpu.py sends, whole: {"div": families for a / b, "zero": zero numerators,
    "sqrt": families for sqrt(z), "asqrt": families for a / sqrt(b)}"""
    return {"div": division_families(), "zero": (div_zero_numerators(),), "sqrt": sqrt_families(), "asqrt": (asqrt(),)}


def sqrt_mod_pow2(r, m):
    """one x with x^2 = r (mod 2^m) for r = 1 (mod 8), m >= 3 (Hensel: x^2 = r mod 2^i holds on entry of step i, and
    (x + 2^(i-1))^2 = x^2 + 2^i mod 2^(i+1) for odd x and i >= 3). The others are -x and +-x + 2^(m-1)."""
    assert r % 8 == 1 and m >= 3
    x = 1
    for i in range(3, m):
        if ((x * x - r) >> i) & 1:
            x += 1 << (i - 1)
    return x


def _roots(x, m):
    mask = (1 << m) - 1
    h = 1 << (m - 1)
    return sorted({x & mask, -x & mask, (x + h) & mask, (h - x) & mask})


@lru_cache(maxsize=None)
def _sqrt_all():
    rng = random.Random(0x5eed05)
    mid, twin = SqrtCases("sqrt_midpoint"), SqrtCases("sqrt_twin")
    ldexp = math.ldexp
    for j in range(40_000):
        for r in (8 * j + 1, -(8 * j + 7)):
            x55 = sqrt_mod_pow2(r, 55)
            for m in (54, 55, 52, 53):
                out = mid if m >= 54 else twin
                lo = M53 if m >= 54 else 1 << 52         # X in [lo, 2 lo)
                for x in _roots(x55, m):
                    # every X of [lo, 2 lo) that solves the congruence (m < the bit length of X: several)
                    for X in range(x + ((lo - x + (1 << m) - 1) >> m << m), 2 * lo, 1 << m):
                        out.draws += 1
                        Z = (X * X - r) >> m
                        if not (1 << 52) <= Z < M53:
                            continue
                        G = X if m < 54 else (X - 1 if r > 0 else X + 1)
                        # z = Z 2^(m + 2 j2), exponent of z in +-EXP_RANGE; the root's is half of it
                        t, _, _, _ = _exp_and_signs(rng)
                        j2 = (t - 52 - m) >> 1
                        out.z.append(ldexp(float(Z), m + 2 * j2))
                        out.g.append(ldexp(float(G), j2))
                        out.r.append(r)
                        out.m.append(m)
    return mid, twin


def sqrt_midpoint():
    return _sqrt_all()[0]


def sqrt_twin():
    return _sqrt_all()[1]


def sqrt_families():
    return _sqrt_all()


def rn_square(s):
    """(Bz, shift): RN(s^2) = Bz 2^shift with Bz a 53-bit integer, for an odd s below 2^53 with s^2 >= 2^53 (never a tie:
    s^2 is odd), or None where RN(sqrt(RN(s^2))) is not s (decided in integers)"""
    sq = s * s
    shift = sq.bit_length() - 53
    Bz = (sq + (1 << (shift - 1))) >> shift
    n4 = (Bz << shift) * 4
    if not (2 * s - 1) ** 2 < n4 < (2 * s + 1) ** 2:
        return None
    return Bz, shift


class ASqrtCases(DivCases):
    """a / sqrt(b) = q, with s = RN(sqrt(b)) the divisor the code rounds to first"""

    def __init__(self, family):
        DivCases.__init__(self, family)
        self.s = array("d")
        self.rejected_s = 0

    def describe(self, i):
        return "%s k=%d r=%d: %s / sqrt(%s) [root %s], expected %s" % (
            self.family, self.k[i], self.r[i], self.a[i].hex(), self.b[i].hex(), self.s[i].hex(), self.q[i].hex())


@lru_cache(maxsize=None)
def asqrt():
    rng = random.Random(0x5eed06)
    out = ASqrtCases("a_over_sqrt")
    tmp = DivCases("tmp")

    def one(s, residues, k):
        sq = rn_square(s)
        if sq is None:
            out.rejected_s += 1
            return
        Bz, shift = sq
        del tmp.a[:], tmp.b[:], tmp.q[:], tmp.k[:], tmp.r[:]
        # the root's exponent within +-EXP_RANGE / 2 keeps b's within +-EXP_RANGE; b > 0
        _add_division(tmp, s, residues, rng, k=k, b_exp_range=EXP_RANGE // 2 - 2)
        out.draws += tmp.draws
        tmp.draws = 0
        for i in range(len(tmp)):
            sd = abs(tmp.b[i])
            j = math.frexp(sd)[1] - s.bit_length()          # sd = s 2^j
            out.a.append(tmp.a[i])
            out.s.append(sd)
            out.b.append(math.ldexp(float(Bz), shift + 2 * j))
            out.q.append(tmp.q[i] if tmp.b[i] > 0 else -tmp.q[i])
            out.k.append(k)
            out.r.append(tmp.r[i])

    band = _odd_band(POW2_RMAX)
    for k in range(1, 64, 2):                                # roots a few ulp below 1 (and above 1/2)
        one(M53 - k, band, -k)
        one((1 << 52) + k, band, k)
    for _ in range(150_000):
        s = rng.getrandbits(52) | (1 << 52) | 1
        r = (2 * rng.randrange(32) + 1) * (1 if rng.getrandbits(1) else -1)
        one(s, (r,), 0)
    return out


# ---- exact rounding, for the check of the closed-form expectations ---------------------------------------------------
def to_fraction(x):
    m, e = math.frexp(x)
    return Fraction(int(math.ldexp(m, 53))) * Fraction(2) ** (e - 53)


def rn_fraction(v):
    """the double nearest to the Fraction v (ties to even; results here are normal), in integers"""
    if v == 0:
        return 0.0
    sign = -1.0 if v < 0 else 1.0
    p, q = abs(v).numerator, abs(v).denominator
    e = p.bit_length() - q.bit_length() - 53       # p / q 2^-e in (2^52, 2^54)
    if e >= 0:
        q <<= e
    else:
        p <<= -e
    if p >= q << 53:
        q <<= 1
        e += 1
    n, rem = divmod(p, q)                           # n in [2^52, 2^53)
    assert (1 << 52) <= n < M53
    if 2 * rem > q or (2 * rem == q and n & 1):
        n += 1
    return sign * math.ldexp(float(n), e)


def rn_sqrt(z):
    """the double nearest to sqrt(z) for a positive double z, in integers (a root of a double is never a tie)"""
    m, e = math.frexp(z)
    M, e = int(math.ldexp(m, 53)), e - 53
    if e & 1:
        M, e = M << 1, e - 1
    N = M << 60                                     # sqrt(N) has 56 or 57 bits
    S = math.isqrt(N)
    sticky = S * S != N
    drop = S.bit_length() - 53
    n, rem = S >> drop, S & ((1 << drop) - 1)
    half = 1 << (drop - 1)
    if rem > half or (rem == half and (sticky or n & 1)):
        n += 1
    return math.ldexp(float(n), drop + e // 2 - 30)


def kept_counts():
    """{family: (kept, draws)} of every family, and the least kept count among the near-power-of-two divisors"""
    fams = division_families() + sqrt_families() + (asqrt(), div_zero_numerators())
    counts = {f.family: (len(f), f.draws) for f in fams}
    per_k = {}
    for k in div_pow2().k:
        per_k[k] = per_k.get(k, 0) + 1
    return counts, per_k
