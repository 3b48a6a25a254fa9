"""Search for a (D, c, max_skew) with c < 2^24 where the fused and the unfused evaluation of spec S14's
x = c * LOGTAB[D] + (max_skew - 1) round to different integers (floor(x + 0.5)).  CPU only.

Unfused: RN(RN(c w) + t).  Fused: RN(c w + t).  The two can differ in the last place only, so the
integers differ only where c w + t lies within a few ulps of k + 1/2.  Per D the candidates are the c
whose RN(c w) has a fraction within 2^-20 of 1/2 (numpy, all 2^24 values at once); each candidate is
then evaluated exactly with fractions for every t.  Prints every hit and the number of candidates.
"""
import json
import math
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LOGTAB = [float.fromhex(v) for v in json.load(open(os.path.join(HERE, "..", "tests", "golden", "soft_spread_logtab.json")))["logtab"]]


def rn(fr):
    """The double nearest to a non-negative Fraction (ties to even)."""
    if fr == 0:
        return 0.0
    e = fr.numerator.bit_length() - fr.denominator.bit_length() - 53
    while True:
        q = fr / Fraction(2) ** e
        if q >= 2 ** 53:
            e += 1
        elif q < 2 ** 52:
            e -= 1
        else:
            break
    fl = q.numerator // q.denominator
    rem = q - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    return math.ldexp(float(fl), e)


def main():
    c = np.arange(1 << 24, dtype=np.float64)
    hits, cands = [], 0
    for D in range(1, 65):
        w = LOGTAB[D - 1]
        p = c * w
        near = np.flatnonzero(np.abs((p - np.floor(p)) - 0.5) < 2.0 ** -20)
        cands += len(near)
        for ci in near:
            exact = Fraction(int(ci)) * Fraction(w)
            for t in range(31):
                unf = float(p[ci]) + float(t)
                fus = rn(exact + t)
                if math.floor(unf + 0.5) != math.floor(fus + 0.5):
                    hits.append((D, int(ci), t + 1, unf.hex(), fus.hex()))
    print(f"candidates {cands}, hits {len(hits)}")
    for h in hits:
        print("D=%d c=%d max_skew=%d unfused=%s fused=%s" % h)
    return 0


if __name__ == "__main__":
    sys.exit(main())
