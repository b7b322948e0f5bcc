"""The onion format (VGEN_FMT_ONION, format 13) on the MI355X at more than one workgroup.  tests/test_gpu_onion.py runs batch 8192: 128
lanes, one workgroup of onion_fwd_kernel / onion_bwd_kernel with two live waves.  Here batch 32768 is 512 lanes - one workgroup with all
eight waves live - and batch 40960 is 640 lanes: a second workgroup (blockIdx.x = 1) with two live waves, whose scratch, inverses and
hit-mask words lie at g >= 512.  Two frames each.  Expected values: the batched reference walk (tests/onion_batch_vectors.py: one pow per
dispatch), computed once per batch and shared.  (Lane counts below 128 and crafted points: tests/test_gpu_onion_kernels.py.)"""
import functools

import pytest

from tests import onion_batch_vectors as obv
from tests import onion_vectors as ov
import vgen_amd as vg
from vgen_amd import api

pytestmark = pytest.mark.gpu

FMT = ov.FMT_ONION
E_INVALID = -1

WIDE_BATCHES = (32768, 40960)
WIDE_SEED, WIDE_FIRST = 2025, 3


@pytest.fixture(scope="module", params=WIDE_BATCHES, ids=["L512", "L640"])
def wide(request):
    r = vg.GpuRunner(batch_size=request.param, fmt=FMT, device=0, frames=2)
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def wide_expected(batch):
    return obv.walk_payloads_batched(ov.base_scalar(WIDE_SEED, 0), WIDE_FIRST, batch)


def test_wide_dump_equals_the_batched_reference(wide):
    batch = wide.batch_size
    want = wide_expected(batch)
    base = ov.base_scalar(WIDE_SEED, 0)
    assert want[0] == ov.point_bytes(base + 8 * WIDE_FIRST) and want[-1] == ov.point_bytes(base + 8 * (WIDE_FIRST + batch - 1))
    for frame in (0, 1):
        wide.set_filter(None)
        wide.dispatch_onion(base, WIDE_FIRST, frame)
        blob, _, tested = wide.await_result(frame)
        assert tested == batch and len(blob) == 32 * batch
        bad = [i for i in range(batch) if blob[32 * i:32 * i + 32] != want[i]]
        assert not bad, (frame, len(bad), bad[:8])


def test_wide_prefix_filter_returns_the_references_hits_in_order(wide):
    batch = wide.batch_size
    L = batch // 64
    want = wide_expected(batch)
    prefix = ov.address(want[batch - 5])[:1]                            # a key of the last lane
    mask, value = ov.prefix_mask(prefix)
    hits = [i for i, p in enumerate(want) if int.from_bytes(p, "big") & mask == value]
    assert batch - 5 in hits and 512 <= len(hits) <= 2048                # about batch / 32, below the ring's 4096
    if L == 640:
        # the reference alone: hits among the slots of both workgroups on either side (lanes 512 .. 639 own the first and last 128 * 32)
        sides = {"wg1 -": (0, (L - 512) * 32), "wg0 -": ((L - 512) * 32, L * 32), "wg0 +": (L * 32, (L + 512) * 32), "wg1 +": ((L + 512) * 32, batch)}
        for name, (lo, hi) in sides.items():
            assert sum(1 for i in hits if lo <= i < hi) >= 16, name
    p = vg.Pattern("^" + prefix, False, FMT)
    assert p.device_kind == 2
    wide.set_filter(p)
    wide.dispatch_onion(ov.base_scalar(WIDE_SEED, 0), WIDE_FIRST, 1)
    recs, n, tested = wide.await_result(1)
    assert tested == batch and n == len(recs) == len(hits)
    assert [i for i, _ in recs] == hits
    assert all(pl == want[i] for i, pl in recs)


def test_wide_match_all_reports_every_key_and_the_first_records(wide):
    batch = wide.batch_size
    want = wide_expected(batch)
    api._check(api._L.vgen_set_match_cap(wide._h, 256), wide._h)
    wide.match_cap = 256
    try:
        wide.set_filter(vg.Pattern(".", False, FMT))
        wide.dispatch_onion(ov.base_scalar(WIDE_SEED, 0), WIDE_FIRST, 0)
        recs, n, tested = wide.await_result(0)
        assert n == batch and tested == batch and len(recs) == 256
        assert recs == [(i, want[i]) for i in range(256)]
    finally:
        api._check(api._L.vgen_set_match_cap(wide._h, 4096), wide._h)
        wide.match_cap = 4096


@pytest.mark.parametrize("batch", [64, 8256])
def test_a_batch_that_is_no_multiple_of_8192_is_refused(batch):
    """include/vgen_hip.h: batch_size is a multiple of 8192, for every format - 64 and 8192 + 64 would suit the walk (a multiple of 64)
    and are refused all the same."""
    with pytest.raises(vg.VgenError) as e:
        vg.GpuRunner(batch_size=batch, fmt=FMT, device=0, frames=2)
    assert e.value.status == E_INVALID
