"""seq_bwd_kernel's product-tree down-sweep (vgen_amd/csrc/device/kernels.hip: tree_down_sweep, one child per lane) at the smallest
shapes at which a wrong sibling or level bound shows: ONE workgroup - every one of its 255 nodes feeds some lane of the dispatch -
and two, at 2 and 8 points per lane, for P2PKH (a compressed key: the LEAN products of core/fe.h) and for the uncompressed format (the canonical y as well; the plain products).

vgen_create takes no batch below 8 192 keys, so the dispatches go through the test-only driver of the launchers
(tests/native/seq_dev.hip, over the product's own kernels.o) with the real tables: R_u = (u S + S / 2) G, Q_j = (k0 + n / 2 + j - S / 2) G,
which is what runtime.cpp hands the kernels.  Every payload of every dump is compared with the oracle's for the keys k0 .. k0 + n - 1."""
import numpy as np
import pytest

from test_gpu_seq_kernels import dev, launch  # noqa: F401  (the fixture and the driver's call)

pytestmark = pytest.mark.gpu

K0 = 0x5EC0DE5EC0DE5EC0DE5EC0DE5EC0DE5EC0DE5EC0DE5EC0DE5EC0DE5EC0DE0001
M29 = (1 << 29) - 1


def limbs(v):
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def point(vo, k):
    pub = vo.pubkey(k)
    return int.from_bytes(pub[1:33], "big"), int.from_bytes(pub[33:65], "big")


_tables = {}


def tables(vo, S, lanes):
    """-> (rtab [18][lanes], q [S][18]) of a dispatch of n = 2 S lanes keys from K0; the 512-lane table's first half is the 256-lane one."""
    if (S, 512) not in _tables:
        pts = [point(vo, u * S + S // 2) for u in range(512)]
        _tables[S, 512] = np.array([limbs(x) + limbs(y) for x, y in pts], dtype=np.uint32)
    rtab = np.ascontiguousarray(_tables[S, 512][:lanes].T)
    half = S * lanes
    q = np.array([limbs(x) + limbs(y) for x, y in (point(vo, K0 + half + j - S // 2) for j in range(S))], dtype=np.uint32)
    return rtab, q


@pytest.mark.parametrize("fmt", [0, 4], ids=["p2pkh", "uncompressed"])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("S", [2, 8])
def test_every_payload_of_one_and_two_workgroups(dev, S, groups, fmt):  # noqa: F811
    from oracle import pyoracle as vo
    lanes = 256 * groups
    n = 2 * S * lanes
    rtab, q = tables(vo, S, lanes)
    o = launch(dev, fmt=fmt, lanes=lanes, S=S, rtab=rtab, q=q)
    assert o.err == 0, (o.err, o.stage)
    got = o.dump.view(np.uint8).reshape(-1, 20)
    want = np.frombuffer(bytes(vo.payload_seq(fmt, K0, n)), dtype=np.uint8).reshape(-1, 20)
    assert got.shape == want.shape == (n, 20)
    bad = np.flatnonzero((got != want).any(axis=1))
    # key index i = n/2 + u S + j (+R_u) or n/2 - (u + 1) S + j (-R_u): the lane u of a wrong payload names the tree node that fed it
    assert bad.size == 0, (S, groups, fmt, bad.size, "first at index", int(bad[0]), "lane",
                           int(bad[0] - n // 2) // S if bad[0] >= n // 2 else int(n // 2 - 1 - bad[0]) // S)
    assert o.guards_intact, "guard words written"
