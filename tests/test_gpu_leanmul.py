"""The key loop's forms of vgen_amd/csrc/core/fe.h AS HIPCC COMPILES THEM (tests/native/leanmul_dev.hip, one vector per lane, 256 lanes):
fe_mul_add<LEAN> / fe_sqr_add<LEAN> - the squaring's doubled limbs are a v_add_u32 written in asm on the device, which no host build
contains - against Python integers and bit for bit against the plain forms compiled beside them.  The vectors are those of tests/test_leanmul.py (tests/leanmul_vectors.py)."""
import ctypes
import os

import pytest

import leanmul_vectors as lv
from conftest import locked_make
from test_core_field import P, check_weak, val

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OP_MUL_ADD, OP_SQR_ADD, OP_MUL_ADD_PLAIN, OP_SQR_ADD_PLAIN = range(4)


@pytest.fixture(scope="module")
def dev():
    locked_make("-s", "-C", os.path.join(HERE, "native"), "-f", "leanmul.mk", "libleandev.so")
    lib = ctypes.CDLL(os.path.join(HERE, "native", "libleandev.so"))
    assert lib.leandev_device_count() >= 1, "no HIP device: the gpu-marked tests need an MI355X"
    return lib


def run(dev, op, a, b, c):
    n = len(a)
    flat = lambda rows: (ctypes.c_uint32 * (9 * n))(*[x for r in rows for x in r])
    out = (ctypes.c_uint32 * (9 * n))()
    rc = dev.leandev_run(op, n, flat(a), flat(b), flat(c), out)
    assert rc == 0, f"leandev_run failed: {rc}"
    return [list(out[9 * i:9 * i + 9]) for i in range(n)]


@pytest.mark.parametrize("square", [0, 1], ids=["mul_add", "sqr_add"])
def test_device_seeded_products(dev, square):
    vs = lv.product_vectors(square)
    assert len(vs) == 256
    a, b, c = [v[0] for v in vs], [v[1] for v in vs], [v[2] for v in vs]
    lean = run(dev, OP_SQR_ADD if square else OP_MUL_ADD, a, b, c)
    plain = run(dev, OP_SQR_ADD_PLAIN if square else OP_MUL_ADD_PLAIN, a, b, c)
    for x, y, z, r, q in zip(a, b, c, lean, plain):
        check_weak(r)
        assert val(r) % P == (val(x) * val(y) + val(z)) % P, (x, y, z)
        assert r == q, (x, y, z)
