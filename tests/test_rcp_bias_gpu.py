"""The default policy's refined reciprocal by itself on the device (pmaf_debug_math op 18: Mth<MATH_XACT>::rcp_refined,
csrc/pmaf_device.hpp) against RN(1 / b) from exact rational arithmetic: bit equality, no tolerance. The sequence
carries no select for an all-ones divisor any more -- a 2^-54 upward bias in its cubic step does that work
(tests/test_rcp_bias.py holds a model of it to every seed of a band) -- so the divisors where a last Newton step can
land beside RN(1 / b) are sent whole: every mantissa 2^53 - k and 2^52 + k for odd k < 4096 at three exponents, both
signs, the all-ones divisors, the powers of two of the validated range, 1.0, and random divisors. One launch.
The divisions built on the reciprocal are tests/test_hard_rounding_gpu.py's (ops 6, 9, 11, 12).

Ops 19 and 20: the reciprocal of a root taken from the root's own iteration (sqrt_seed / rcp_seeded behind norm_rcp_z
and norm_rcp_zpos: no v_rcp_f64), by itself and through the fixup-free division as a / sqrt(b) -- on the same
mantissas taken as ROOTS (radicand RN(s^2)), on both neighbours of those radicands, and on a sample of the constructed
a / sqrt(b) family of tests/hard_rounding.py. One launch per op, bit equality."""
import math
import random

import numpy as np
import pytest

import hard_rounding as H

pytestmark = pytest.mark.gpu

EXPONENTS = (-250, 0, 250)          # of the divisor's mantissa in [1, 2): both ends of the policy's range, and the unit
N_RANDOM = 20000


def _cases():
    """(b, RN(1 / b)) as two arrays; RN of a mantissa's reciprocal once, in Fraction -- the scaling by a power of two and
    the sign are exact"""
    b, w = [], []

    def add(x, want):
        b.extend((x, -x))
        w.extend((want, -want))
    for k in range(1, H.POW2_KMAX, 2):
        for mant in (H.M53 - k, (1 << 52) + k):
            r = H.rn_fraction(1 / H.to_fraction(float(mant)))
            for e in EXPONENTS:
                add(math.ldexp(float(mant), e - 52), math.ldexp(r, 52 - e))
    for B, eb in H.ALL_ONES:
        x = math.ldexp(float(B), eb)
        add(x, H.rn_fraction(1 / H.to_fraction(x)))
    for e in range(-250, 251):
        add(math.ldexp(1.0, e), math.ldexp(1.0, -e))
    rng = random.Random(0xb1a5)
    for _ in range(N_RANDOM):
        x = math.ldexp(rng.getrandbits(52) | (1 << 52), rng.randrange(-250, 251) - 52) * (1.0 if rng.getrandbits(1) else -1.0)
        b.append(x)
        w.append(H.rn_fraction(1 / H.to_fraction(x)))
    return np.array(b), np.array(w)


def test_refined_reciprocal_is_correctly_rounded(pmaf):
    b, want = _cases()
    assert b.size <= 100_000 and (b == 1.0).any() and (b < 0).any()
    got = pmaf.debug_math(18, b, b)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    print("\nop 18: %d divisors compared, %d differ from RN(1 / b)" % (b.size, bad.size))
    assert bad.size == 0, "\n".join("1 / %s: got %s, expected %s" % (float(b[i]).hex(), float(got[i]).hex(), float(want[i]).hex())
                                    for i in bad[:25])
    assert got[b == 1.0][0] == 1.0


ROOT_EXPONENTS = (-125, 0, 124)     # of the root: the radicand's exponent stays within +-250
N_ASQRT = 20000


@pytest.fixture(scope="module")
def root_cases():
    """(z, RN(sqrt z), RN(1 / RN(sqrt z))) -- radicands RN(s^2) of every hard mantissa s and their two neighbours, once"""
    z, sq, rc = [], [], []
    for k in range(1, H.POW2_KMAX, 2):
        for mant in (H.M53 - k, (1 << 52) + k):
            z0 = H.rn_fraction(H.to_fraction(float(mant)) ** 2)
            for zz in (z0, math.nextafter(z0, math.inf), math.nextafter(z0, 0.0)):
                s = H.rn_sqrt(zz)
                r = H.rn_fraction(1 / H.to_fraction(s))
                for e in ROOT_EXPONENTS:                     # exact scalings: z 2^(2 e'), s 2^e', r 2^-e'
                    z.append(math.ldexp(zz, 2 * (e - 52)))
                    sq.append(math.ldexp(s, e - 52))
                    rc.append(math.ldexp(r, 52 - e))
    return np.array(z), np.array(sq), np.array(rc)


def _differ(got, want):
    return np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))


def test_reciprocal_of_a_root_through_the_roots_seed(pmaf, root_cases):
    z, sq, rc = root_cases
    A = H.asqrt()
    idx = np.random.default_rng(19).choice(len(A), N_ASQRT, replace=False)
    b = np.frombuffer(A.b, dtype=np.float64)[idx]
    s = np.frombuffer(A.s, dtype=np.float64)[idx]
    want = np.concatenate([rc, np.array([H.rn_fraction(1 / H.to_fraction(float(x))) for x in s])])
    zz = np.concatenate([z, b])
    assert zz.size <= 100_000
    assert _differ(pmaf.debug_math(5, zz, zz), np.concatenate([sq, s])).size == 0       # the premise: the roots themselves
    got = pmaf.debug_math(19, zz, zz)
    bad = _differ(got, want)
    print("\nop 19: %d radicands compared, %d differ from RN(1 / RN(sqrt(b)))" % (zz.size, bad.size))
    assert bad.size == 0, "\n".join("1 / sqrt(%s): got %s, expected %s" % (float(zz[i]).hex(), float(got[i]).hex(), float(want[i]).hex())
                                    for i in bad[:25])


def test_division_by_a_root_through_the_roots_seed(pmaf, root_cases):
    z, sq, _ = root_cases
    rng = random.Random(20)
    a = np.array([math.ldexp(rng.getrandbits(52) | (1 << 52), rng.randrange(-100, 101) - 52) * (1.0 if rng.getrandbits(1) else -1.0)
                  for _ in range(z.size)])
    q = np.array([H.rn_fraction(H.to_fraction(float(x)) / H.to_fraction(float(y))) for x, y in zip(a, sq)])
    A = H.asqrt()
    idx = np.random.default_rng(20).choice(len(A), N_ASQRT, replace=False)
    aa = np.concatenate([a, np.frombuffer(A.a, dtype=np.float64)[idx]])
    bb = np.concatenate([z, np.frombuffer(A.b, dtype=np.float64)[idx]])
    want = np.concatenate([q, np.frombuffer(A.q, dtype=np.float64)[idx]])
    assert aa.size <= 100_000
    got = pmaf.debug_math(20, aa, bb)
    bad = _differ(got, want)
    print("\nop 20: %d a / sqrt(b) compared, %d differ from the correctly rounded quotient" % (aa.size, bad.size))
    assert bad.size == 0, "\n".join("%s / sqrt(%s): got %s, expected %s" % (float(aa[i]).hex(), float(bb[i]).hex(), float(got[i]).hex(),
                                                                            float(want[i]).hex()) for i in bad[:25])
