"""The resources of the onion walk's kernels, read from the code-object metadata in the assembly hipcc emits for gfx950 (no GPU
needed): no scratch (private segment size 0) and no MFMA in onion_points_kernel, onion_fwd_kernel and both forms of onion_bwd_kernel,
and no LDS beyond the 576 B of the inversion tree.  A resource check only."""
import os
import re

import pytest

from conftest import locked_make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISA = os.path.join(ROOT, "build", "lib", "device", "kernels.s")


@pytest.fixture(scope="module")
def kernels():
    # (a no-op when __graft_entry__.build() has just run; ~1 min of hipcc otherwise)
    locked_make("-s", "-C", os.path.join(ROOT, "vgen_amd", "csrc"), "../../build/lib/device/kernels.s")
    txt = open(ISA).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.M | re.S):
        sym, meta = m.group(1), m.group(2)
        if "onion" not in sym:
            continue
        field = lambda name: int(re.search(r"\." + name + r"\s+(\d+)", meta).group(1))
        body = txt.split("\n" + sym + ":", 1)[1].split(".Lfunc_end", 1)[0]
        out[sym] = {"scratch": field("amdhsa_private_segment_fixed_size"), "lds": field("amdhsa_group_segment_fixed_size"),
                    "vgpr": field("amdhsa_next_free_vgpr"), "body": body}
    return out


def test_the_four_kernels_are_there(kernels):
    names = sorted(kernels)
    assert len(names) == 4, names
    assert sum("onion_points_kernel" in n for n in names) == 1 and sum("onion_fwd_kernel" in n for n in names) == 1
    assert sum("onion_bwd_kernelILb0" in n for n in names) == 1 and sum("onion_bwd_kernelILb1" in n for n in names) == 1


def test_no_scratch_no_mfma_and_the_trees_lds_only(kernels):
    for sym, k in kernels.items():
        assert k["scratch"] == 0, (sym, k["scratch"])
        assert not re.search(r"^\s+v_(s?mfma|mfma)", k["body"], re.M), sym
        assert "scratch_" not in k["body"], sym
        assert k["lds"] == (576 if "onion_fwd_kernel" in sym else 0), (sym, k["lds"])
        assert k["vgpr"] <= 256, (sym, k["vgpr"])
