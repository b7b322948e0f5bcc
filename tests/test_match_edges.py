"""The crafted payloads of tests/match_vectors.py through core/filter_eval.h and core/dfa_eval.h as g++ compiles them
(tests/native/core_shim.cpp): range bounds, masks on single-bit neighbours, zero runs, chunk edges.  The same cases and
the same assertions run on the device in tests/test_gpu_match_device.py; here they also prove, without a GPU, that every
reference meets the conditions that keep a case from passing vacuously (match_vectors.reference)."""
import ctypes

import pytest

import match_vectors as mv


def run(cases):
    for case in cases:
        dev, host_exact = mv.host_run(case)
        r = mv.check(case, dev, "host build")
        assert host_exact == r.exact, case.tag        # the product's automaton on the product's encoding == the oracle's on its own
        print(mv.line(case, r))


def test_ranges_at_their_bounds():
    cases = mv.range_cases()
    assert len(cases) == 15
    run(cases)


def test_ranges_in_wave_layouts():
    # (the host build has no waves: what is checked here is that the layouts hold what they claim and the model accepts them)
    run(mv.wave_cases())


@pytest.mark.parametrize("fmt", [1, 3, 5])
def test_masks_on_single_bit_neighbours(fmt):
    run(mv.mask_cases(fmt))


@pytest.mark.parametrize("fmt,idx", [(fmt, idx) for fmt in (0, 2, 4) for idx in range(mv.BASE58_CASES[fmt])])
def test_full_matcher_base58(fmt, idx):
    cases = mv.full_base58_cases(fmt)
    run(cases[idx:idx + 1])


@pytest.mark.parametrize("fmt", [1, 3, 5])
def test_full_matcher_symbols(fmt):
    run(mv.full_symbol_cases(fmt))


def test_divmod_d5():
    lib = mv.core()
    vals = mv.divmod_inputs()
    for v in vals:
        q, r = ctypes.c_uint32(), ctypes.c_uint32()
        lib.core_divmod_d5(ctypes.c_uint32(v >> 32), ctypes.c_uint32(v & mv.M32), ctypes.byref(q), ctypes.byref(r))
        assert (q.value, r.value) == divmod(v, mv.D5), hex(v)
