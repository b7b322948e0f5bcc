"""core/filter_eval.h and core/dfa_eval.h AS HIPCC COMPILES THEM, on crafted payloads, every address format.

The two headers decide on the device whether a key is reported; a wrong "no" is the one failure nothing downstream can see.
The product's kernels reach them only with payloads that hashes produce: no payload at a range bound, none that shares its
leading word with one, hardly a zero run of three bytes.  Here a test-only driver (tests/native/match_dev.hip ->
libmatchdev.so: one payload per thread, the instantiations of the product's MatchFmt, the product's flags and generated hash
blocks) runs the cases of tests/match_vectors.py, and every verdict is compared, exactly, with references that share no code
with the headers (match_vectors: Python integers over the exported ranges and masks, the oracle's regex on the oracle's
address, Python `re` for Ethereum's case-folded automaton).  tests/test_match_edges.py runs the same cases on the host build.

For every case and every instantiation that serves its format: ranges and masks equal the model on every payload and accept
every payload the oracle's regex accepts; the full matcher equals the oracle's regex (Ethereum: `re` with re.I, a superset
of the exact verdict); all instantiations agree payload by payload; and for formats 0, 1, 2 and 4 the shipped
payload_filter_kernel (liblistdev.so, the product's own kernels.o) gives the hit mask of the <5, -1> instantiation, except
that an all-zero payload never hits there."""
import ctypes
import os

import numpy as np
import pytest

from conftest import locked_make
from test_gpu_list_kernels import Job, launch as list_launch

import match_vectors as mv

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_N = 8192
# instantiations of match_dev.hip, and those that serve a format (device/kernels.hip: MatchFmt)
INST_NAMES = ["<5, P2PKH>", "<5, P2SH_P2WPKH>", "<5, P2PKH_UNCOMPRESSED>", "<5, -1>", "<8, -1>"]
ANY5 = 3
INSTS = {0: (0, ANY5), 1: (0, ANY5), 2: (1, ANY5), 3: (4,), 4: (2, ANY5), 5: (ANY5,)}


@pytest.fixture(scope="module")
def dev():
    locked_make("-s", "-C", os.path.join(HERE, "native"), "libmatchdev.so")
    lib = ctypes.CDLL(os.path.join(HERE, "native", "libmatchdev.so"))
    lib.matchdev_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p]
    lib.matchdev_filter_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.matchdev_divmod.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.matchdev_device_count() >= 1, "no HIP device: the gpu-marked tests need an MI355X"
    return lib


@pytest.fixture(scope="module")
def listdev():
    locked_make("-s", "-C", os.path.join(HERE, "native"), "liblistdev.so")
    lib = ctypes.CDLL(os.path.join(HERE, "native", "liblistdev.so"))
    assert lib.listdev_job_size() == ctypes.sizeof(Job)
    return lib


@pytest.fixture(scope="module")
def vg():
    import vgen_amd
    assert vgen_amd.device_count() >= 1
    return vgen_amd


def words_of(case):
    nw = mv.payload_len(case.fmt) // 4
    return np.frombuffer(b"".join(case.payloads), dtype="<u4").reshape(-1, nw).astype(np.uint32)


def device_run(dev, pat, pay, inst):
    """Every payload through one instantiation, at most MAX_N per launch (a multiple of 64: the waves of a layout stay whole)."""
    got = np.empty(pay.shape[0], dtype=np.uint32)
    for at in range(0, pay.shape[0], MAX_N):
        part = np.ascontiguousarray(pay[at:at + MAX_N])
        out = np.zeros(part.shape[0], dtype=np.uint32)
        rc = dev.matchdev_run(pat._h, part.ctypes.data, inst, part.shape[0], out.ctypes.data)
        assert rc == 0, f"matchdev_run failed: {rc}"
        got[at:at + MAX_N] = out
    assert set(got.tolist()) <= {0, 1}, "a payload without a verdict"
    return got.tolist()


def shipped_run(listdev, pat, pay):
    """The same filter and payloads through payload_filter_kernel, the way test_gpu_list_kernels.test_payload_filter runs it:
    one image, the slots behind the payloads zero and not counted, no ring."""
    n = pay.shape[0]
    stride = -(-n // 256) * 256
    slots = np.zeros((stride, 5), dtype=np.uint32)
    slots[:n] = pay
    o = list_launch(listdev, slots, stride=stride, count=n, images=1, filt=pat._h, cap=0)
    assert o.err == 0, o.err
    bits = np.unpackbits(o.hits[:o.words].view(np.uint8), bitorder="little")
    assert not bits[n:].any()
    assert o.header[0] == int(bits.sum())
    return bits[:n].tolist()


def run(dev, listdev, vg, cases):
    zero_hits = 0
    for case in cases:
        ref = mv.reference(case)
        pat = vg.Pattern(case.pattern, case.ci, vg.AddressFormat(case.fmt))
        info = (ctypes.c_uint32 * 6)()
        assert dev.matchdev_filter_info(pat._h, info) == 0
        assert list(info) == mv.compiled(case.pattern, case.ci, case.fmt).header, case.tag     # the library compiled what the host build exports
        assert pat.device_kind == ref.kind
        pay = words_of(case)
        got = {}
        for inst in INSTS[case.fmt]:
            got[inst] = device_run(dev, pat, pay, inst)
            mv.check(case, got[inst], INST_NAMES[inst])
        first = got[INSTS[case.fmt][0]]
        assert all(g == first for g in got.values()), (case.tag, "the instantiations disagree")
        if case.fmt in (0, 1, 2, 4):
            nonzero = pay.any(axis=1)
            shipped = shipped_run(listdev, pat, pay)
            want = [int(g and nz) for g, nz in zip(got[ANY5], nonzero)]
            bad = [i for i, (s, w) in enumerate(zip(shipped, want)) if s != w]
            assert not bad, (case.tag, "payload_filter_kernel", len(bad), [(case.payloads[i].hex(), shipped[i], want[i]) for i in bad[:4]])
            zero_hits += sum(1 for g, nz in zip(got[ANY5], nonzero) if g and not nz)
        print(mv.line(case, ref) + f"; {len(got)} instantiation(s)")
    return zero_hits


def test_ranges_at_their_bounds(dev, listdev, vg):
    cases = mv.range_cases()
    assert len(cases) == 15
    # '^11' and its like accept the all-zero hash160 (their first range starts at 0): the shipped kernel's "no key" mark was met
    assert run(dev, listdev, vg, cases) >= 3


def test_ranges_in_wave_layouts(dev, listdev, vg):
    """As test_device_canonicalize_product_slow_path_fires_per_wave: the wave-uniform branch behind VG_ANY_LANE(near) not
    taken, taken for one lane's sake at lane 0, 31, 32 and 63, taken by all, and in a ragged last wave."""
    cases = mv.wave_cases()
    assert len(cases) == 15 and all(len(c.payloads) % 64 == 10 for c in cases)
    run(dev, listdev, vg, cases)


@pytest.mark.parametrize("fmt", [1, 3, 5])
def test_masks_on_single_bit_neighbours(dev, listdev, vg, fmt):
    run(dev, listdev, vg, mv.mask_cases(fmt))


@pytest.mark.parametrize("fmt,idx", [(fmt, idx) for fmt in (0, 2, 4) for idx in range(mv.BASE58_CASES[fmt])])
def test_full_matcher_base58(dev, listdev, vg, fmt, idx):
    cases = mv.full_base58_cases(fmt)
    run(dev, listdev, vg, cases[idx:idx + 1])


@pytest.mark.parametrize("fmt", [1, 3, 5])
def test_full_matcher_symbols(dev, listdev, vg, fmt):
    run(dev, listdev, vg, mv.full_symbol_cases(fmt))


def test_divmod_d5(dev):
    vals = mv.divmod_inputs()
    hi = np.array([v >> 32 for v in vals], dtype=np.uint32)
    lo = np.array([v & mv.M32 for v in vals], dtype=np.uint32)
    q, r = np.zeros_like(hi), np.zeros_like(hi)
    assert dev.matchdev_divmod(hi.ctypes.data, lo.ctypes.data, hi.size, q.ctypes.data, r.ctypes.data) == 0
    for v, qq, rr in zip(vals, q.tolist(), r.tolist()):
        assert (qq, rr) == divmod(v, mv.D5), hex(v)


def test_arguments_that_are_not_run(dev, vg):
    """The driver starts nothing for a count of 0 or above 8192, an instantiation that does not serve the filter's format, a
    filter without a device test, or a divmod input outside the function's domain."""
    pat = vg.Pattern("^1Cat", False, vg.AddressFormat(0))
    pay = np.zeros((MAX_N + 1, 5), dtype=np.uint32)
    out = np.full(MAX_N + 1, 7, dtype=np.uint32)
    run_ = lambda p, inst, n: dev.matchdev_run(p._h, pay.ctypes.data, inst, n, out.ctypes.data)
    assert run_(pat, 0, 0) == -1 and run_(pat, 0, MAX_N + 1) == -1
    assert [run_(pat, inst, 64) for inst in (1, 2, 4, 5, -1)] == [-1] * 5
    assert run_(vg.Pattern("^1", False, vg.AddressFormat(0)), 0, 64) == -1          # DEVF_ALL: no device test to run
    assert (out == 7).all()
    assert run_(pat, 0, 64) == 0 and (out[:64] == 0).all() and (out[64:] == 7).all()
    hi = np.array([mv.D5], dtype=np.uint32)
    assert dev.matchdev_divmod(hi.ctypes.data, hi.ctypes.data, 1, out.ctypes.data, out.ctypes.data) == -1
