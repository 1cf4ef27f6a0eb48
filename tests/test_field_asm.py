"""GPU: the device Field128 primitives (compiler-built and hand-scheduled asm) against Python
integers, on random and edge-case canonical operands.  The hand-written blocks keep their
VCC carry chains back to back and keep scratch in fixed VGPRs, so they get their own test
next to the end-to-end parity suite (tests/test_gpu_parity.py)."""
import random

import numpy as np
import pytest

from janus_amd import prio3 as J

pytestmark = pytest.mark.gpu

P = 2**128 - 28 * 2**64 + 1
EDGE = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, 2**127, 2**64 - 1, 2**64, 28 * 2**64,
        2**96 - 1, 2**128 - 28 * 2**64 - 2**32, P - 2**64]


def enc(xs):
    return np.frombuffer(b"".join(x.to_bytes(16, "little") for x in xs), np.uint8).reshape(-1, 16)


def dec(arr):
    return [int.from_bytes(r.tobytes(), "little") for r in arr]


def operands(n, seed):
    rnd = random.Random(seed)
    a = [rnd.choice(EDGE) if rnd.random() < 0.15 else rnd.randrange(P) for _ in range(n)]
    b = [rnd.choice(EDGE) if rnd.random() < 0.15 else rnd.randrange(P) for _ in range(n)]
    a[:len(EDGE)] = EDGE
    b[:len(EDGE)] = EDGE[::-1]
    return a, b


@pytest.mark.parametrize("op,fn", [(0, lambda x, y: x * y % P), (1, lambda x, y: x * y % P),
                                   (2, lambda x, y: (x + y) % P), (3, lambda x, y: (x - y) % P)])
def test_binary_ops(op, fn):
    a, b = operands(1 << 16, op)
    got = dec(J.selftest_field(op, enc(a), enc(b)))
    want = [fn(x, y) for x, y in zip(a, b)]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"op {op}: {len(bad)} mismatches, first at {bad[0]}"


@pytest.mark.parametrize("op", [4, 5])
def test_mac_reduce(op):
    n = 1 << 13
    a, b = operands(16 * n, 10 + op)
    # all-(p-1) rows maximise every column and overflow word
    a[16:32] = [P - 1] * 16
    b[16:32] = [P - 1] * 16
    got = dec(J.selftest_field(op, enc(a), enc(b)))
    want = [sum(a[16 * i + k] * b[16 * i + k] for k in range(16)) % P for i in range(n)]
    assert got == want


# ---- Field64 and the limit-operand pieces of Field128 (prio3_selftest_field64) -----------------
P64 = 2**64 - 2**32 + 1
M32 = 0xFFFFFFFF
EDGE64 = [0, 1, 2, P64 - 1, P64 - 2, (P64 - 1) // 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63,
          2**64 - 2**33, M32 << 32, 0x12345678 << 32, 0x12345678, (0x12345678 << 32) | M32,
          0xFFFFFFFEFFFFFFFF]


def enc64(xs):
    return np.array(xs, dtype=np.uint64).view(np.uint8).reshape(-1, 8)


def dec64(arr):
    return [int(x) for x in np.ascontiguousarray(arr).view(np.uint64).reshape(-1)]


def operands64(n, seed):
    rnd = random.Random(seed)
    pick = lambda: rnd.choice(EDGE64) if rnd.random() < 0.15 else rnd.randrange(P64)  # noqa: E731
    a, b = [pick() for _ in range(n)], [pick() for _ in range(n)]
    k = len(EDGE64)
    # every edge against every edge
    a[:k * k] = [x for x in EDGE64 for _ in EDGE64]
    b[:k * k] = [y for _ in EDGE64 for y in EDGE64]
    return a, b


def test_edge64_is_canonical():
    assert all(0 <= x < P64 for x in EDGE64)


@pytest.mark.parametrize("op,fn", [(0, lambda x, y: x * y % P64), (1, lambda x, y: (x + y) % P64),
                                   (2, lambda x, y: (x - y) % P64)], ids=["mul", "add", "sub"])
def test_field64_binary_ops(op, fn):
    n = 1 << 16
    a, b = operands64(n, 20 + op)
    got = dec64(J.selftest_field64(op, n, 0, enc64(a), enc64(b)))
    bad = [i for i in range(n) if got[i] != fn(a[i], b[i])]
    assert not bad, f"op {op}: {len(bad)} mismatches, first at {bad[0]}: {a[bad[0]]:#x} {b[bad[0]]:#x}"


def test_red128_64_raw_inputs_take_every_branch():
    """red128_64 on raw (lo, hi): the cross product of edge words, plus random; the reference
    also counts the inputs that take the borrow branch, the carry branch, both, and the final
    subtraction."""
    words = [0, 1, 2, 0x7FFFFFFF, 0x80000000, M32 - 1, M32]
    w64 = [(h << 32) | l for h in words for l in words]
    rnd = random.Random(7)
    lo = [x for x in w64 for _ in w64] + [rnd.getrandbits(64) for _ in range(1 << 14)]
    hi = [y for _ in w64 for y in w64] + [rnd.getrandbits(64) for _ in range(1 << 14)]
    n = len(lo)
    cnt = dict(borrow=0, carry=0, both=0, final=0)
    for l, h in zip(lo, hi):
        x2, x3 = h & M32, h >> 32
        t0 = (l - x3) % 2**64
        borrow = l < x3
        if borrow:
            t0 = (t0 - M32) % 2**64
        t1 = (x2 << 32) - x2
        r = (t0 + t1) % 2**64
        carry = r < t1
        if carry:
            r = (r + M32) % 2**64
        cnt["borrow"] += borrow
        cnt["carry"] += carry
        cnt["both"] += borrow and carry
        cnt["final"] += r >= P64
    assert all(v > 0 for v in cnt.values()), cnt
    got = dec64(J.selftest_field64(3, n, 0, enc64(lo), enc64(hi)))
    bad = [i for i in range(n) if got[i] != (lo[i] + (hi[i] << 64)) % P64]
    assert not bad, f"{len(bad)} mismatches, first (lo, hi) = {lo[bad[0]]:#x}, {hi[bad[0]]:#x}"


@pytest.mark.parametrize("k", [1, 16, 4096])
def test_mac64_sums_of_products(k):
    n = max(8, (1 << 16) // k)
    a, b = operands64(n * k, 30 + k)
    a[:k] = [P64 - 1] * k  # rows of all (p - 1) (p - 1): every column and overflow word at its top
    b[:k] = [P64 - 1] * k
    a[k:2 * k] = [2**64 - 2**33] * k
    b[k:2 * k] = [P64 - 1] * k
    got = dec64(J.selftest_field64(4, n, k, enc64(a), enc64(b)))
    want = [sum(x * y for x, y in zip(a[i * k:(i + 1) * k], b[i * k:(i + 1) * k])) % P64
            for i in range(n)]
    assert got == want


def _lt_p_inputs(p, bits):
    words = bits // 32
    xs = [p - 1, p, p + 1, 0, 2**bits - 1] + [2**k - 1 for k in range(1, bits + 1)]
    for w in range(words):  # values that differ from p in exactly one 32-bit word
        pw = (p >> (32 * w)) & M32
        for v in {0, 1, pw - 1, pw + 1, M32 - 1, M32, 0x80000000}:
            if 0 <= v <= M32 and v != pw:
                xs.append(p - (pw << (32 * w)) + (v << (32 * w)))
    return xs


def test_lt_p_on_raw_input():
    xs = _lt_p_inputs(P64, 64)
    got = dec64(J.selftest_field64(5, len(xs), 0, enc64(xs)))
    assert got == [int(x < P64) for x in xs]
    xs = _lt_p_inputs(P, 128)
    got = dec64(J.selftest_field64(6, len(xs), 0, enc(xs)))
    assert got == [int(x < P) for x in xs]
    assert 0 in got and 1 in got


@pytest.mark.parametrize("k", [1, 1 << 16])
def test_lazy_sum_of_limit_operands(k):
    xs = [P - 1, P - 2, 0, 1, 2**127, 2**64 - 1, (P - 1) // 2] + \
        [random.Random(k).randrange(P) for _ in range(57)]
    got = dec(J.selftest_field64(7, len(xs), k, enc(xs)))
    assert got == [x * k % P for x in xs]


@pytest.mark.parametrize("nb", [1, 8, 31, 32])
def test_truncation_accumulator(nb):
    """TruncSink over two entries per lane: all elements p - 1 (at nb = 32 the 160-bit
    accumulator is filled to its last bit), edges, and random ones."""
    n = 96
    rnd = random.Random(nb)
    rows = [[P - 1] * (2 * nb), [0] * (2 * nb), [P - 1] * nb + [1] * nb]
    rows += [[rnd.choice(EDGE) if rnd.random() < 0.2 else rnd.randrange(P) for _ in range(2 * nb)]
             for _ in range(n - len(rows))]
    out = J.selftest_field64(8, n, nb, enc([x for r in rows for x in r]))
    for e in range(2):
        want = [sum(r[e * nb + b] << b for b in range(nb)) % P for r in rows]
        assert dec(out[e]) == want, e
