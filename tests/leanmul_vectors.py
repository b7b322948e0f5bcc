"""Vectors of tests/test_leanmul.py (host build) and tests/test_gpu_leanmul.py (device build, one vector per lane): the LEAN products
with an addend of vgen_amd/csrc/core/fe.h at the limits the header documents.
256 vectors per operation - four waves - made once."""
import random

from test_core_field import M29, P, W0, W1, limbs_of, rand_limbs, val

N_VEC = 256
ADD_MAX3 = [3 * W0, 3 * W1] + [3 * M29] * 6 + [3 << 24]       # an addend of magnitude 3, every limb at its maximum
WEAK_MAX = [W0, W1] + [M29] * 6 + [1 << 24]                    # a multiplicand at the weak-normalisation limits
# residues a product with its addend is steered to: 0, the ends of [0, 2^256 - p) - whose representatives below 2^256 are t and t + p, the
# second one in [p, 2^256) -, and the values around p and 2^256 themselves
TARGETS = [0, 1, 2**32 + 976, 2**32 + 977, P - 1, P - 2, 2**256 - 1 - P, 977, 2**32]


def product_vectors(square):
    """-> [(a, b, c)] limb lists: r = a * b + c (square: a * a + c, b = a), a of magnitude 1, a * b within m_a * m_b <= 6, c of magnitude <= 3."""
    rng = random.Random(1291 + square)
    zero, pm1 = limbs_of(0), limbs_of(P - 1)
    out = []
    for a in (WEAK_MAX, zero, pm1, limbs_of(1)):
        for b in (WEAK_MAX, zero, pm1):
            for c in (ADD_MAX3, zero, pm1):
                out.append((a, a if square else b, c))
    out.append((WEAK_MAX, WEAK_MAX if square else rand_limbs(rng, 6, "max"), ADD_MAX3))      # the largest column sums there are
    for t in TARGETS * 4:
        # a * b + c == t (mod p) with c at or near its limits; the square takes a root where (t - c) has one (p == 3 mod 4)
        c = rng.choice([ADD_MAX3, rand_limbs(rng, 3, "mixed"), zero])
        d = (t - val(c)) % P
        if square:
            s = pow(d, (P + 1) // 4, P)
            if s * s % P != d:
                c = limbs_of((t - 4) % P)       # then a = 2 does: 4 + c == t
                s = 2
            out.append((limbs_of(s), limbs_of(s), c))
        else:
            u = rng.randrange(1, P)
            out.append((limbs_of(u), limbs_of(d * pow(u, -1, P) % P), c))
    while len(out) < N_VEC:
        style = rng.choice(["max", "mixed", "rand"])
        a = rand_limbs(rng, 1, style)
        b = a if square else rand_limbs(rng, rng.choice([1, 3, 6]), rng.choice(["max", "mixed", "rand"]))
        out.append((a, b, rand_limbs(rng, 3, rng.choice(["max", "mixed", "rand"]))))
    return out[:N_VEC]
