"""Shared by the score tests: a plain Python model of the four metrics, one hex digit at a time, and the crafted payloads the
tests aim at the word-wise evaluation of core/score_eval.h."""
import random

ZERO_BYTES, LEADING_ZERO_BYTES, LEADING_DIGIT, COUNT_DIGIT = 0, 1, 2, 3
METRIC_MAX = {ZERO_BYTES: 20, LEADING_ZERO_BYTES: 20, LEADING_DIGIT: 40, COUNT_DIGIT: 40}


def metric(m, digit, payload: bytes) -> int:
    assert len(payload) == 20
    if m == ZERO_BYTES:
        return sum(1 for b in payload if b == 0)
    if m == LEADING_ZERO_BYTES:
        n = 0
        for b in payload:
            if b != 0:
                break
            n += 1
        return n
    digits = payload.hex()
    want = "0123456789abcdef"[digit]
    if m == COUNT_DIGIT:
        return sum(1 for d in digits if d == want)
    n = 0
    for d in digits:
        if d != want:
            break
        n += 1
    return n


def parse(spec: str):
    """[(metric, digit, min)] of a well-formed specification."""
    assert spec.startswith("score:")
    out = []
    for term in spec[6:].split("&"):
        name, n = term.split(">=")
        if name == "zero-bytes":
            out.append((ZERO_BYTES, 0, int(n)))
        elif name == "leading-zero-bytes":
            out.append((LEADING_ZERO_BYTES, 0, int(n)))
        elif name.startswith("leading:"):
            out.append((LEADING_DIGIT, int(name[8:], 16), int(n)))
        else:
            assert name.startswith("count:")
            out.append((COUNT_DIGIT, int(name[6:], 16), int(n)))
    return out


def accepts(spec: str, payload: bytes) -> bool:
    return all(metric(m, d, payload) >= n for m, d, n in parse(spec))


def score(spec: str, payload: bytes) -> int:
    m, d, _ = parse(spec)[0]
    return metric(m, d, payload)


def crafted_payloads():
    """Every digit value in every one of the 40 positions; a zero byte at each of the 20 positions; runs of 0 .. 40 leading digits
    (they end on and across word boundaries); the near misses of a borrowing zero-byte test (0x01 0x00, 0x00 0x01, 0x10, 0x0f,
    0x80 0x00) within a word and across a word boundary; the all-zero and the all-f payload.  Deterministic."""
    out = []
    fill = [0x5a, 0xa5]                      # no zero byte, no digit 0 / f
    for pos in range(40):
        for v in range(16):
            for base in fill:
                p = bytearray([base] * 20)
                b = p[pos // 2]
                p[pos // 2] = (v << 4 | (b & 15)) if pos % 2 == 0 else ((b & 0xf0) | v)
                out.append(bytes(p))
    for pos in range(20):
        p = bytearray([0x11] * 20)
        p[pos] = 0
        out.append(bytes(p))
        p = bytearray([0xff] * 20)
        p[pos] = 0
        out.append(bytes(p))
    for v in (0, 1, 7, 8, 0xa, 0xf):
        for run in range(41):
            digits = [v] * run + [(v + 1) & 15] * (40 - run)
            out.append(bytes(digits[2 * i] << 4 | digits[2 * i + 1] for i in range(20)))
            digits = [v] * run + [(v ^ 8)] + [v] * (39 - run) if run < 40 else [v] * 40   # the run resumes behind one foreign digit
            out.append(bytes(digits[2 * i] << 4 | digits[2 * i + 1] for i in range(20)))
    near = [(0x01, 0x00), (0x00, 0x01), (0x10, 0x00), (0x00, 0x10), (0x0f, 0x00), (0x00, 0x0f), (0x80, 0x00), (0x00, 0x80), (0x10, 0x33), (0x0f, 0x33)]
    for a, b in near:
        for at in (0, 1, 2, 3, 7, 11, 15, 18):   # 3, 7, 11, 15: the pair straddles a word boundary
            for base in (0x33, 0x00):
                p = bytearray([base] * 20)
                p[at], p[at + 1] = a, b
                out.append(bytes(p))
    out.append(bytes(20))
    out.append(b"\xff" * 20)
    return out


def random_payloads(n, seed=0x5c0e):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        p = bytearray(rng.getrandbits(8) for _ in range(20))
        if i % 3 == 0:                        # thin out: plenty of zero bytes, zero digits and f digits
            for k in range(20):
                r = rng.random()
                if r < 0.3:
                    p[k] = 0
                elif r < 0.4:
                    p[k] &= 0x0f
                elif r < 0.5:
                    p[k] |= 0xf0
        out.append(bytes(p))
    return out
