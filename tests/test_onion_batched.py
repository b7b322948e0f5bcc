"""The batched onion reference (tests/onion_batch_vectors.py: every key as U_j +- R_u, one pow per dispatch) against the plain one
(tests/onion_vectors.py: the affine law with an inversion per point, the walk with an inversion per key) and the golden digests of
tests/golden/onion.json.  The GPU tests of the walk's kernels at many lane counts compare with the batched one; this is what lets them."""
import json
import os
import random

from tests import onion_batch_vectors as obv
from tests import onion_vectors as ov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "onion.json")))


def test_batched_pairs_equal_the_plain_law_on_edge_and_random_pairs():
    """obv.pairs shares one pow among all denominators; ov.pair (sv.add) inverts each on its own.  Every edge pair in both roles, the edge
    points among themselves, each also in ONE call (a zero numerator or a denominator of 2 must not disturb its neighbours' inverses),
    and 200 random pairs."""
    rng = random.Random(31)
    for _ in range(3):
        p = ov.point_of(rng.getrandbits(253) * 8)
        for q in ov.edge_points(p):
            assert obv.pairs([p], [q]) == [[ov.pair(p, q)]], q
            assert obv.pairs([q], [p]) == [[ov.pair(q, p)]], q
        qs = ov.edge_points(p)
        assert obv.pairs([p] + qs, qs + [p]) == [[ov.pair(a, b) for a in [p] + qs] for b in qs + [p]]
    es = ov.edge_points((0, 1))
    assert obv.pairs(es, es) == [[ov.pair(a, b) for a in es] for b in es]
    U = [ov.point_of(rng.getrandbits(255)) for _ in range(10)]
    R = [ov.point_of(rng.getrandbits(255)) for _ in range(20)]
    got = obv.pairs(U, R)
    assert len(got) == 20 and all(len(row) == 10 for row in got)
    assert got == [[ov.pair(p, q) for p in U] for q in R]


def test_batched_walk_equals_the_plain_walk_and_the_golden_digests():
    n = FIXTURE["batch"]
    assert n == 8192
    for d in FIXTURE["dumps"]:
        assert ov.digest(obv.walk_payloads_batched(int(d["base"], 16), d["first"], n)) == d["sha256"]
    assert len(FIXTURE["dumps"]) == 3
    d = FIXTURE["dumps"][1]
    assert obv.walk_payloads_batched(int(d["base"], 16), d["first"], n) == ov.walk_payloads(int(d["base"], 16), d["first"], n)
    # base 0: slot 0 has no key; and a lane count that is no multiple of anything
    assert obv.walk_payloads_batched(0, 0, 64 * 3) == ov.walk_payloads(0, 0, 64 * 3)
    assert obv.walk_payloads_batched(8 * 999, 5, 64) == ov.walk_payloads(8 * 999, 5, 64)
