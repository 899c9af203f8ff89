"""float32 searches and descriptors shared by the crafted-case suites (sbp_cases.py, bow_cases.py).  TEST INFRASTRUCTURE ONLY."""
from fractions import Fraction
import numpy as np

f32 = np.float32


def ordinal(v):
    """the float32 v as an integer that orders like the floats do"""
    i = int(np.array(v, f32).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def from_ordinal(o):
    i = o if o >= 0 else ((-o) | 0x80000000)
    return np.array(i & 0xFFFFFFFF, np.uint32).view(f32)[()]


def first_f32(pred, lo, hi):
    """smallest float32 in [lo, hi] with pred true (pred false at lo, true at hi, monotone)"""
    a, b = ordinal(lo), ordinal(hi)
    assert not pred(from_ordinal(a)) and pred(from_ordinal(b))
    while b - a > 1:
        m = (a + b) // 2
        if pred(from_ordinal(m)): b = m
        else: a = m
    return from_ordinal(b)


def below(v):
    return np.nextafter(f32(v), f32(-np.inf))


def above(v):
    return np.nextafter(f32(v), f32(np.inf))


def round_f32(fr):
    """the float32 nearest to a Fraction (ties to even)"""
    c = f32(float(fr))
    cands = sorted({float(below(c)), float(c), float(above(c))})
    best = min(cands, key=lambda v: (abs(Fraction(v) - fr), int(np.array(v, f32).view(np.uint32)) & 1))
    return f32(best)


def desc(bits):
    """a 256-bit descriptor with its first `bits` bits set: the Hamming distance of two of them is the difference of their bits"""
    a = np.zeros(256, np.uint8); a[:bits] = 1
    return np.packbits(a)
