"""CPU tests of the forms of vgen_amd/csrc/core/fe.h that the sequential scan kernels' key loop takes, through the host build of the header
(tests/native/leanmul_shim.cpp): fe_mul_add<LEAN> / fe_sqr_add<LEAN>, whose addend is the starting value of the column accumulators, against
Python integers and - bit for bit - against the plain forms.  The same vectors run one per
lane on the device in tests/test_gpu_leanmul.py (there the squaring's doubled limbs are the device-only v_add_u32)."""
import ctypes
import os

import pytest

import leanmul_vectors as lv
from conftest import locked_make
from test_core_field import P, check_weak, val

HERE = os.path.dirname(os.path.abspath(__file__))
A9 = ctypes.c_uint32 * 9


@pytest.fixture(scope="module")
def lean():
    locked_make("-s", "-C", os.path.join(HERE, "native"), "-f", "leanmul.mk", "libleantest.so")
    return ctypes.CDLL(os.path.join(HERE, "native", "libleantest.so"))


@pytest.mark.parametrize("square", [0, 1], ids=["mul_add", "sqr_add"])
def test_seeded_products_against_python_integers_and_the_plain_form(lean, square):
    at_or_above_p = 0
    for a, b, c in lv.product_vectors(square):
        r, plain = A9(), A9()
        lean.leanmul_mul_add(A9(*a), A9(*b), A9(*c), r, square, 1)
        lean.leanmul_mul_add(A9(*a), A9(*b), A9(*c), plain, square, 0)
        check_weak(list(r))
        assert val(r) % P == (val(a) * val(b) + val(c)) % P, (a, b, c)
        assert list(r) == list(plain), (a, b, c)
        at_or_above_p += P <= val(r) < 2**256
    assert at_or_above_p >= 1     # (the vectors steered to the residues below 2^256 - p: some come out as t + p)


def test_the_vectors_hold_the_limits():
    for square in (0, 1):
        vs = lv.product_vectors(square)
        assert len(vs) == lv.N_VEC
        assert any(a == lv.WEAK_MAX and b == lv.WEAK_MAX and c == lv.ADD_MAX3 for a, b, c in vs)
        assert any(val(a) == 0 for a, _, _ in vs) and any(val(a) == P - 1 and val(b) == P - 1 for a, b, _ in vs)
        for t in lv.TARGETS:
            assert any((val(a) * val(b) + val(c)) % P == t % P for a, b, c in vs), t
