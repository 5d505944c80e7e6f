"""TEST INFRASTRUCTURE — float populations and exact references for tests/test_gpu_float_text.py. Nothing here reads a header of
etl_amd/csrc: shortest digits come from Python's repr (f64) and numpy's unique scientific form (f32), correctly rounded parsing from
exact rationals (fractions.Fraction) compared against the two floats that bracket them, the bits of a float from its fields.

Population A: finite bit patterns entered as their shortest text (every f32 exponent, every 8th f64 exponent and the ends of the range,
the powers of ten the layouts switch at with both neighbours, the integer edges, every shortest digit count, the subnormal / normal
boundary of both widths, signs, random fill).
Population B: the exact half-way points between a float and its successor as full decimal expansions, with the last digit bumped up and
down: texts only an exact parser settles.
Population C: float8[] / float4[] literals over population A's texts."""
import random
import struct
from fractions import Fraction

import numpy as np

# (mantissa bits, exponent bits)
F64, F32 = (52, 11), (23, 8)


def _fmt(is32):
    return F32 if is32 else F64


def bits_value(bits, is32):
    """The exact value of a non-negative bit pattern, from its fields. The pattern of +infinity counts as the next power of two: the
    value a tie against the largest finite float is measured with."""
    mb, eb = _fmt(is32)
    m, e = bits & ((1 << mb) - 1), (bits >> mb) & ((1 << eb) - 1)
    bias = (1 << (eb - 1)) - 1
    if e == 0:
        return Fraction(m) * Fraction(2) ** (1 - bias - mb)
    return Fraction((1 << mb) | m) * Fraction(2) ** (e - bias - mb)


def is_finite(bits, is32):
    mb, eb = _fmt(is32)
    return (bits >> mb) & ((1 << eb) - 1) != (1 << eb) - 1


def round_fraction(q, is32):
    """The bits of the float nearest to the rational q, ties to even (infinity's pattern on overflow): the two floats that bracket |q|
    are found (a first guess from the bit lengths, then moved until lo <= |q| < lo + 1 holds as exact comparisons) and the nearer wins."""
    mb, eb = _fmt(is32)
    sign = 1 << (mb + eb) if q < 0 else 0
    q = abs(q)
    inf = ((1 << eb) - 1) << mb
    if q == 0:
        return sign
    bias = (1 << (eb - 1)) - 1
    e = q.numerator.bit_length() - q.denominator.bit_length()              # 2^(e-1) < q < 2^(e+1)
    lo = min(inf, max(0, e - 1 + bias) << mb)                              # 2^(e-1), or zero below the normal range: not above q
    assert bits_value(lo, is32) <= q or lo == inf
    step = 1 << mb
    while step:                                                            # the largest pattern whose value is <= q
        while lo + step <= inf and bits_value(lo + step, is32) <= q:
            lo += step
        step >>= 1
    if lo >= inf:
        return sign | inf
    below, above = q - bits_value(lo, is32), bits_value(lo + 1, is32) - q
    assert below >= 0 and above > 0
    if below < above or (below == above and lo % 2 == 0):
        return sign | lo
    return sign | (lo + 1)


def to_float(bits, is32):
    return struct.unpack("<f", struct.pack("<I", bits))[0] if is32 else struct.unpack("<d", struct.pack("<Q", bits))[0]


def shortest_text(bits, is32):
    """The shortest decimal text that reads back as the pattern: repr for f64, numpy's unique scientific form for f32."""
    if is32:
        return np.format_float_scientific(np.float32(to_float(bits, True)), unique=True, trim="-")
    return repr(to_float(bits, False))


def shortest_digits(bits, is32):
    """The significant digits of shortest_text, without leading / trailing zeros."""
    t = shortest_text(bits & ~(1 << (31 if is32 else 63)), is32).lower()
    mant = t.split("e")[0].replace(".", "").strip("0")
    return mant or "0"


def exact_decimal(q):
    """The finite decimal expansion of a non-negative dyadic rational: numerator x 5^k, the point k places from the right."""
    assert q >= 0
    k = q.denominator.bit_length() - 1
    assert q.denominator == 1 << k
    s = str(q.numerator * 5 ** k)
    if k == 0:
        return s
    s = s.zfill(k + 1)
    return s[:-k] + "." + s[-k:]


def bump(text, delta):
    """`text` (digits with at most one point) with its last digit moved by delta, carries included."""
    ip, _, fp = text.partition(".")
    s = str(int(ip + fp) + delta).zfill(len(fp) + 1)
    return s[:len(s) - len(fp)] + "." + s[len(s) - len(fp):] if fp else s


# ---------------------------------------------------------------------------------------------------------------- population A
def _with_digit_count(rng, n, is32):
    """A pattern whose shortest text has exactly n significant digits."""
    for _ in range(10000):
        d = str(rng.randint(1, 9)) if n == 1 else str(rng.randint(1, 9)) + "".join(str(rng.randint(0, 9)) for _ in range(n - 2)) + str(rng.randint(1, 9))
        bits = round_fraction(Fraction(int(d)) * Fraction(10) ** rng.randint(-30, 20), is32)
        if len(shortest_digits(bits, is32)) == n:
            return bits
    raise AssertionError(n)


def population_a(is32, total, seed=20260):
    """`total` finite bit patterns of one width (a list, deterministic): the named classes first, random patterns up to the total."""
    mb, eb = _fmt(is32)
    rng = random.Random(seed + (32 if is32 else 64))
    ones, top = (1 << mb) - 1, 1 << (mb + eb)
    out = []
    if is32:
        exps = list(range(0, 255))
    else:
        exps = sorted(set(range(0, 2047, 8)) | {0, 1, 2} | set(range(1020, 1028)) | {2044, 2045, 2046})
    for e in exps:
        out += [(e << mb) | m for m in (0, 1, ones, rng.randint(2, ones - 1))]
    for k in range(-8, 24):                                                # the layouts' thresholds
        b = round_fraction(Fraction(10) ** k, is32)
        out += [b - 1, b, b + 1]
    p = 24 if is32 else 53
    out += [round_fraction(Fraction(2 ** p + d), is32) for d in (-1, 0, 1)] + [round_fraction(Fraction(2 ** p + 2), is32)]
    for n in range(1, (9 if is32 else 17) + 1):
        out += [_with_digit_count(rng, n, is32) for _ in range(3)]
    out += [1, ones, 1 << mb, (1 << mb) + 1, ones - 1]                     # the subnormal / normal boundary and its neighbours
    out = [b for b in out if b != 0]
    out = [0, top] + out + [b | top for b in out[::10]]                    # +-0, a negative copy of every tenth
    assert len(out) <= total, (len(out), total)
    while len(out) < total:
        b = rng.getrandbits(mb + eb + 1)
        if is_finite(b, is32):
            out.append(b)
    assert all(is_finite(b, is32) for b in out)
    return out


# ---------------------------------------------------------------------------------------------------------------- population B
def population_b(is32, n_base, seed=20261):
    """[(text, expected bits)]: for n_base patterns spread over every exponent (subnormals included) the exact half-way point to the
    successor, and that text with its last digit bumped down and up. Expected bits: round_fraction of the text's own value."""
    mb, eb = _fmt(is32)
    rng = random.Random(seed + (32 if is32 else 64))
    ones, emax = (1 << mb) - 1, (1 << eb) - 2
    out = []
    for i in range(n_base):
        e = 0 if i % 16 == 0 else (i * (emax + 1)) // n_base               # one in sixteen is subnormal, the rest walk the exponents
        m = rng.choice([0, 1, ones - 1, ones, rng.randint(0, ones)]) if i % 3 else rng.randint(0, ones)
        b = (e << mb) | m
        if b == 0:
            b = 1
        if not is_finite(b + 1, is32):
            b -= 1
        half = exact_decimal((bits_value(b, is32) + bits_value(b + 1, is32)) / 2)
        for t in (half, bump(half, -1), bump(half, 1)):
            out.append((t, round_fraction(Fraction(t), is32)))
    return out


# ---------------------------------------------------------------------------------------------------------------- population C
def population_c(n_rows, pats8, pats4, seed=20262):
    """[(float8[] literal, [bits | None], float4[] literal, [bits | None])]: 0..12 elements per literal drawn from the given patterns' shortest
    texts, every fifth element NULL, one element in four quoted."""
    rng = random.Random(seed)
    out = []
    for _ in range(n_rows):
        row = []
        for pats, is32 in ((pats8, False), (pats4, True)):
            want, parts = [], []
            for k in range(rng.randint(0, 12)):
                if k % 5 == 4:
                    want.append(None)
                    parts.append("NULL")
                    continue
                b = rng.choice(pats)
                want.append(b)
                t = shortest_text(b, is32)
                parts.append('"' + t + '"' if rng.random() < 0.25 else t)
            row += ["{" + ",".join(parts) + "}", want]
        out.append(tuple(row))
    return out
