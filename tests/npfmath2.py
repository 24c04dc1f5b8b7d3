"""Python ports of cice5_amd/csrc/evpk_fmath2.h (evpk_exp, evpk_log_hl, evpk_log, evpk_atan, evpk_pow_pos) and of the evpk_atan2 of
evpk_fmath.h that evpk_atan is -- operation for operation, so that they give the header's bits (tests/test_fmath2_host.py compares
them with the header compiled by the system C compiler).  Python floats are IEEE doubles and never contract; fma() is computed exactly
with rationals and rounded once, which is what a fused multiply-add is.
"""
from __future__ import annotations

import math
import struct
from fractions import Fraction

from .npridge import dev_exp

LN2_HI, LN2_LO = 0.6931471803691238, 1.9082149292705877e-10
LG = [0.6666666666666666, 0.4, 0.2857142857142857, 0.2222222222222222, 0.18181818181818182, 0.15384615384615385, 0.13333333333333333,
      0.11764705882352941, 0.10526315789473684, 0.09523809523809523]
PI_HI, PI_LO, PIO2_HI, PIO2_LO = 3.141592653589793, 1.2246467991473532e-16, 1.5707963267948966, 6.123233995736766e-17
ATAN_TAB = [0.0, 0.0, 0.06241880999595735, -1.5490756308295046e-18, 0.12435499454676144, -3.1253241424539383e-18,
            0.18534794999569476, 4.180692268843079e-18, 0.24497866312686414, 1.0698755618734451e-17, 0.3028848683749714, -1.1010827903001369e-17,
            0.35877067027057225, -2.4623815582638635e-17, 0.4124104415973873, -1.587652227770689e-17, 0.4636476090008061, 2.2698777452961687e-17,
            0.5123894603107377, -2.5462781472855804e-17, 0.5585993153435624, -5.4556305485916264e-18, 0.6022873461349642, 2.950430737228402e-17,
            0.6435011087932844, 1.5834785051444286e-17, 0.6823165548747481, 6.943223671560008e-18, 0.7188299996216245, -2.1478388444456983e-17,
            0.7531512809621944, -2.4256934659182068e-17, 0.7853981633974483, 3.061616997868383e-17]
A_SER = [-0.3333333333333333, 0.2, -0.14285714285714285, 0.1111111111111111, -0.09090909090909091, 0.07692307692307693]


def fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (finite arguments)"""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:                                    # (an exact zero: the product is then a double, and a * b + c has the zero's sign)
        return a * b + c
    return float(r)


evpk_exp = dev_exp                                # the header's evpk_exp is dev_exp, operation for operation


def evpk_log_hl(x: float):
    ix = struct.unpack("<q", struct.pack("<d", x))[0]
    hx = ix >> 32
    k = (hx >> 20) - 1023
    hx &= 0x000fffff
    i = (hx + 0x95f64) & 0x100000
    ix = ((hx | (i ^ 0x3ff00000)) << 32) | (ix & 0xffffffff)
    k += i >> 20
    m = struct.unpack("<d", struct.pack("<q", ix))[0]
    f = m - 1.0
    dh = 2.0 + f
    dl = f - (dh - 2.0)
    sh = f / dh
    r = fma(-sh, dh, f)
    sl = (r - sh * dl) / dh
    z = sh * sh
    P = LG[0] + z * (LG[1] + z * (LG[2] + z * (LG[3] + z * (LG[4] + z * (LG[5] + z * (LG[6] + z * (LG[7] + z * (LG[8] + z * LG[9]))))))))
    fk = float(k)
    a, b = fk * LN2_HI, 2.0 * sh
    h0 = a + b
    bb = h0 - a
    e = (a - (h0 - bb)) + (b - bb)
    l = e + (fk * LN2_LO + (2.0 * sl + (sh * z) * P))
    H = h0 + l
    return H, l - (H - h0)


def evpk_log(x: float) -> float:
    return evpk_log_hl(x)[0]


def evpk_atan2(y: float, x: float) -> float:
    ax, ay = abs(x), abs(y)
    if ay == 0.0:                                 # (the header drops what its main path computes here)
        a = 0.0
    else:
        swap = ay > ax
        t = (ax if swap else ay) / (ay if swap else ax)
        fk0 = float(math.floor(t * 16.0))
        fk = fk0 if (fk0 >= 0.0 and fk0 <= 16.0) else 0.0
        k = int(fk)
        cpt = fk * 0.0625
        u = (t - cpt) / fma(t, cpt, 1.0)
        z = u * u
        p = fma(z, fma(z, fma(z, fma(z, fma(z, A_SER[5], A_SER[4]), A_SER[3]), A_SER[2]), A_SER[1]), A_SER[0])
        a = ATAN_TAB[2 * k] + (fma(u * z, p, u) + ATAN_TAB[2 * k + 1])
        if swap:
            a = PIO2_HI - (a - PIO2_LO)
    ar = PI_HI - (a - PI_LO)
    xneg = (math.copysign(1.0, x) < 0.0) and (ay == 0.0 or x < 0.0)
    if xneg:
        a = ar
    return math.copysign(a, y)


def evpk_atan(x: float) -> float:
    return evpk_atan2(x, 1.0)


def evpk_pow_pos(x: float, y: float) -> float:
    if x == 0.0:
        return 0.0
    hi, lo = evpk_log_hl(x)
    p = y * hi
    e = fma(y, hi, -p)
    t = e + y * lo
    E = evpk_exp(p)
    return E + E * t
