"""The onion walk staged the way the kernels stage it, in Python integers: every key of a dispatch is U_j + R_u or U_j - R_u
(device_types.h: OnionArgs), and all denominators of a dispatch share ONE pow - a few microseconds a key where
tests/onion_vectors.py walk_payloads, which inverts per key, takes 150.  Built on tests/onion_vectors.py and nothing else: nothing on the
expected side of the tests comes from the code under test.  (tests/test_onion_batched.py holds it against the plain law and walk.)"""
from tests import onion_vectors as ov

P, D = ov.P, ov.D

S = 32                      # shared points per dispatch, keys per lane and sign
NO_SLOT = 0xFFFFFFFF


def batch_inverse(vals):
    """1 / v for every v (none 0) with one pow: Montgomery's trick."""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % P
    inv = pow(acc, P - 2, P)
    assert acc and inv * acc % P == 1
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % P
        inv = inv * vals[i] % P
    return out


def pairs(U, R):
    """out[u][j] = (x(U_j + R_u), y(U_j + R_u), x(U_j - R_u), y(U_j - R_u)) for every lane point R_u and shared point U_j."""
    dens = []
    for x2, y2 in R:
        t2 = D * x2 * y2 % P
        for x1, y1 in U:
            k = t2 * x1 * y1 % P
            dens.append((1 - k) % P)
            dens.append(1 + k)
    inv = batch_inverse(dens)
    out, i = [], 0
    for x2, y2 in R:
        row = []
        for x1, y1 in U:
            im, ip = inv[i], inv[i + 1]
            i += 2
            a, b, c, d = x1 * x2, y1 * y2, x1 * y2, y1 * x2
            row.append(((c + d) * ip % P, (b + a) * im % P, (c - d) * im % P, (b - a) * ip % P))
        out.append(row)
    return out


def place(rows, L, zero_slot=NO_SLOT):
    """The 64 L payloads from pairs' rows: U_j + R_u at slot (L + u) S + j, U_j - R_u at slot (L - 1 - u) S + j, 32 zero bytes at zero_slot."""
    assert len(rows) == L and all(len(row) == S for row in rows)
    out = [None] * (2 * S * L)
    for u, row in enumerate(rows):
        for j, (xs, ys, xd, yd) in enumerate(row):
            out[(L + u) * S + j] = (ys | (xs & 1) << 255).to_bytes(32, "little")
            out[(L - 1 - u) * S + j] = (yd | (xd & 1) << 255).to_bytes(32, "little")
    if zero_slot != NO_SLOT:
        out[zero_slot] = bytes(32)
    return out


def batch_payloads(U, R, L, zero_slot=NO_SLOT):
    """The 64 L payloads of a dispatch over the S shared points U and the L lane points R."""
    assert len(U) == S and len(R) == L
    return place(pairs(U, R), L, zero_slot)


_LANE_POINTS = []


def lane_points(L):
    """R_u = (u S + S/2) (8B), u < L (each from the fixed-base table on its own; kept, a longer table extends a shorter one)."""
    while len(_LANE_POINTS) < L:
        _LANE_POINTS.append(ov.point_of(8 * (S * len(_LANE_POINTS) + S // 2)))
    return _LANE_POINTS[:L]


def shared_points(start, L):
    """U_j = (start + 8 (L S - S/2 + j)) B, j < S."""
    return [ov.point_of(start + 8 * (L * S - S // 2 + j)) for j in range(S)]


def walk_payloads_batched(base, first, n):
    """walk_payloads for n a multiple of 2 S, staged as a dispatch of n / (2 S) lanes: a few microseconds a key."""
    assert n % (2 * S) == 0
    L, start = n // (2 * S), base + 8 * first
    assert start + 8 * (n - 1) < 2**255
    return batch_payloads(shared_points(start, L), lane_points(L), L, 0 if start == 0 else NO_SLOT)
