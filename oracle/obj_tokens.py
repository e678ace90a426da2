"""obj_tokens.py — TEST INFRASTRUCTURE: a seeded generator of OBJ number tokens and the curated and refused lists, aimed
at the boundary of the window in which the device decode (take_amd/csrc/tk_obj.h) converts a number itself: 15 / 16
significant digits, effective decimal exponent 22 / 23, zero runs across the 15th digit, uncounted trailing zeros,
signed zeros with absurd exponents, the ends of the double range.  Nothing here restates the device's conversion: a
token is SPELLED from a digit string, a layout and a target exponent; what it is worth is float()'s business.

It lives here, not under tests/, because tools/gen_obj_golden.py builds the reference-made `number_grammar` fixture from
it (a change to number_tokens() or CURATED changes that fixture, and the regeneration test says so); the tests reach it
through tests/obj_numbers.py.  Only tests/ and tools/ may import this module.
"""
import numpy as np

SIG_DIGITS = (1, 2, 7, 14, 15, 16, 17, 20)
# where `exponent - fraction digits + trailing zeros` lands: the value is (the significant digits as an integer) * 10^T
EFFECTIVE_EXPONENTS = (-24, -23, -22, -21, -1, 0, 1, 21, 22, 23, 24)

FIFTEEN = "123456789012345"

# accepted tokens worth naming
CURATED = [
    b"999999999999999e22", b"123456789012345e-22", b"9007199254740993", b"1e22", b"1e23", b"10e22",
    b"100000000000000000000000", (FIFTEEN + "000000000").encode(), (FIFTEEN + "000000000.").encode(),
    ("0." + FIFTEEN + "000000000").encode(), (FIFTEEN + ".000000000e-3").encode(),
    b"1200e20", b"1200e19", b"12e21", b"12e22", b".12e24", b".12e25", b"1.5e-22", b"1.5e-21", b"1.5e-23", b"15e-23", b"15e-24",
    b"999999999999999", b"9999999999999999", b"1000000000000000", b"10000000000000000", b"1000000000000001", b"10000000000000001",
    b"100000000000000e1", b"100000000000001e1", b"1000000000000010", b"12345678901234000000000000000000000005",
    b"0.1", b"0.30000000000000004", b".5", b"5.", b"+5.", b"-.5", b"+.5e1", b"005", b"000.500", b"1E+007", b"1e-007", b"1e+0", b"1E-0",
    b"0", b"+0", b"-0", b"0.", b"-0.", b".0", b"-.0", b"+.0", b"0.0", b"-0.0", b"-0.000e-5", b"0.000E+5", b"0e999999999999",
    b"-0E-999999999999", b"-0e999999999999", b"0e99999999999999999999", b"-0.0e-99999999999999999999", b"00000", b"-000.000",
    b"1.7976931348623157e308", b"-1.7976931348623157e308", b"2.2250738585072014e-308", b"-2.2250738585072014e-308",
    b"17976931348623157e292", b"0.00000000000000000000022250738585072014e-285",
]
# every spelling of a signed zero above, for the tests that look at np.signbit
NEGATIVE_ZEROS = [b"-0", b"-0.", b"-.0", b"-0.0", b"-0.000e-5", b"-0E-999999999999", b"-0e999999999999",
                  b"-0.0e-99999999999999999999", b"-000.000"]
POSITIVE_ZEROS = [b"0", b"+0", b"0.", b".0", b"+.0", b"0.0", b"0.000E+5", b"0e999999999999", b"0e99999999999999999999", b"00000"]

# non-zero tokens of the grammar clearly outside the range of a double (the reference's stream fails on them) ...
REFUSED_RANGE = [b"1e999", b"-1e999", b"1e-999", b"1e123456789012", b"-1e-123456789012", b"1e100000000", b"1e-100000001",
                 b"1e99999999999999999999", b"0.001e-99999999999999999999", b"123456789012345e295", b"1234567890123456e-400"]
# ... and tokens outside the grammar [+-]?(d+(.d*)?|.d+)([eE][+-]?d+)?
REFUSED_GRAMMAR = [b"nan", b"inf", b"-inf", b"1e", b"1e+", b"1e-", b".", b"+", b"-", b"+.", b"-.e1", b"e5", b".e5", b"1.2.3", b"0x10",
                   b"1f", b"1e5.0", b"1e+-5", b"--1", b"+-1", b"1,5", b"1d5", b"1_0", b"infinity", b"NAN"]
REFUSED = REFUSED_RANGE + REFUSED_GRAMMAR


def _digits(rng, nsig):
    """nsig significant digits: the first and the last are not zero; now and then an interior run of 1-7 zeros, and in
    numbers of 16 digits or more a run that covers the 15th digit"""
    d = rng.integers(1, 10, nsig) if rng.random() < 0.5 else rng.integers(0, 10, nsig)
    d[0] = rng.integers(1, 10)
    d[-1] = rng.integers(1, 10)
    if nsig >= 3 and rng.random() < 0.5:
        run = int(rng.integers(1, min(7, nsig - 2) + 1))
        if nsig >= 16 and rng.random() < 0.6:
            lo, hi = max(1, 14 - run + 1), min(14, nsig - 1 - run)  # the run [start, start + run) holds index 14
            start = int(rng.integers(lo, hi + 1))
        else:
            start = int(rng.integers(1, nsig - run))
        d[start:start + run] = 0
    return "".join(map(str, d.tolist()))


def number_token(rng):
    """one accepted token of the grammar, spelled from the choices the module docstring lists"""
    sig = _digits(rng, int(rng.choice(SIG_DIGITS)))
    tz = int(rng.integers(1, 25)) if rng.random() < 0.4 else 0  # trailing zeros behind the last significant digit
    layout = rng.integers(0, 5)
    lead = "0" * int(rng.choice((0, 0, 0, 1, 2, 5)))
    if layout == 0:  # ddd000 or ddd000.
        mant, nfrac = lead + sig + "0" * tz + ("." if rng.random() < 0.3 else ""), 0
    elif layout == 1:  # ddd00.000: the trailing zeros on both sides of the point
        k = int(rng.integers(0, tz + 1))
        mant, nfrac = lead + sig + "0" * k + "." + "0" * (tz - k), tz - k
    elif layout == 2 and len(sig) > 1:  # d.dd000
        k = int(rng.integers(1, len(sig)))
        mant, nfrac = lead + sig[:k] + "." + sig[k:] + "0" * tz, len(sig) - k + tz
    else:  # .000ddd000, 0.ddd, 00.0ddd
        lz = int(rng.choice((0, 0, 1, 3, 9)))
        mant, nfrac = str(rng.choice(("", "0", "00"))) + "." + "0" * lz + sig + "0" * tz, lz + len(sig) + tz
    tok = str(rng.choice(("", "+", "-"))) + mant
    if rng.random() < 0.75:
        ex = int(rng.choice(EFFECTIVE_EXPONENTS)) + nfrac - tz
        sign = "-" if ex < 0 else str(rng.choice(("", "+"))) if ex > 0 else str(rng.choice(("", "+", "-")))
        tok += str(rng.choice(("e", "E"))) + sign + "0" * int(rng.choice((0, 0, 1, 4))) + str(abs(ex))
    return tok.encode()


def number_tokens(n, seed=2025):
    rng = np.random.default_rng(seed)
    return [number_token(rng) for _ in range(n)]
