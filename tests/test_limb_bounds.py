"""The unsaturated X448 (28-bit limbs) and P-521 (29-bit limbs) field code restated on Python
integer limbs -- carry / add / sub / mul_small and the product's column scan and fold, as in
x448_device.h and p521_device.h -- to check what the two headers only state in comments: the
limbs that enter a product stay below 2^29 (X448) and 2^29 + 2^6 (P-521), its 64-bit column
accumulator and the 32-bit fold sums do not wrap, on the chained operations the device test runs
(janus_hpke_selftest_field ops 6..9), where products take the outputs of add / sub / mul_small
as they do in the ladder and in the Jacobian formulas.  No GPU needed."""
import random

import pytest

P448 = 2**448 - 2**224 - 1
P521 = 2**521 - 1
CHAINED_OPS = (6, 7, 8, 9)


class Limbs:
    """One field's limb arithmetic; `seen` records the largest limb entering any product."""

    def __init__(self, field):
        self.field = field
        if field == 1:
            self.p, self.bits, self.nl, self.w, self.k = P448, 448, 16, 28, 39081
            self.top_w = 28
            self.bound = [2**29] * 16                       # "< 2^29 in every use here"
            self.nominal = [2**28] * 16
        else:
            self.p, self.bits, self.nl, self.w, self.k = P521, 521, 18, 29, 8
            self.top_w = 28
            self.bound = [2**29 + 2**6] + [2**29] * 16 + [2**28]   # "limbs < 2^29 + 2^6"
            self.nominal = [2**29] * 17 + [2**28]
        self.m = 2**self.w - 1
        self.seen = [0] * self.nl

    def value(self, v):
        return sum(x << self.w * i for i, x in enumerate(v))

    def from_int(self, x):
        assert 0 <= x < 2**self.bits
        return [x >> self.w * i & self.m for i in range(self.nl)]

    def _u32(self, x):
        assert 0 <= x < 2**32, "a 32-bit limb expression wraps"
        return x

    def _u64(self, x):
        assert 0 <= x < 2**64, "a 64-bit accumulator wraps"
        return x

    def carry(self, v):
        v = list(v)
        for i in range(self.nl - 1):
            v[i + 1] = self._u32(v[i + 1] + (v[i] >> self.w))
            v[i] &= self.m
        t = v[-1] >> self.top_w
        v[-1] &= 2**self.top_w - 1
        v[0] = self._u32(v[0] + t)
        if self.field == 1:
            v[8] = self._u32(v[8] + t)
        return v

    def add(self, a, b):
        return self.carry([self._u32(x + y) for x, y in zip(a, b)])

    def sub(self, a, b):
        if self.field == 1:
            two_p = [0x1ffffffc if i == 8 else 0x1ffffffe for i in range(16)]
        else:
            two_p = [0x3ffffffe] * 17 + [0x1ffffffe]
        return self.carry([self._u32(x + t - y) for x, t, y in zip(a, two_p, b)])

    def mul_small(self, a, k):
        r = [self._u64(x * k) for x in a]
        for i in range(self.nl - 1):
            r[i + 1] = self._u64(r[i + 1] + (r[i] >> self.w))
            r[i] &= self.m
        t = r[-1] >> self.top_w
        r[-1] &= 2**self.top_w - 1
        r[0] += t
        if self.field == 1:
            r[8] += t
        return self.carry([self._u32(x) for x in r])

    def _enter(self, a):
        for i, x in enumerate(a):
            assert x < self.bound[i], (f"field {self.field}: limb {i} = {x:#x} enters a product, "
                                       f"bound {self.bound[i]:#x}")
            self.seen[i] = max(self.seen[i], x)

    def mul(self, a, b):
        self._enter(a)
        self._enter(b)
        nl, w, m = self.nl, self.w, self.m
        digits, acc = [], 0
        for k in range(2 * nl - 1):
            for i in range(max(0, k - nl + 1), min(k, nl - 1) + 1):
                acc = self._u64(acc + a[i] * b[k - i])
            digits.append(acc & m)
            acc >>= w
        digits.append(acc & m)
        top = self._u32(acc >> w)
        lo, hi = digits[:nl], digits[nl:]
        if self.field == 1:   # fold_ps: 2^448 = 2^224 + 1, top 2^896 = 3 2^224 + 2
            r = [self._u32(lo[k] + hi[k] + hi[k + 8] + (2 * top if k == 0 else 0))
                 for k in range(8)]
            r += [self._u32(lo[k] + 2 * hi[k] + hi[k - 8] + (3 * top if k == 8 else 0))
                  for k in range(8, 16)]
            o = [0] * 16
            for k in range(15):
                r[k + 1] = self._u32(r[k + 1] + (r[k] >> 28))
                o[k] = r[k] & m
            t = r[15] >> 28
            o[15] = r[15] & m
            o[0] += t
            o[8] += t
            return o
        o, c = [0] * nl, 0     # fold: 2^522 = 2, 2^521 = 1
        for k in range(nl):
            x = self._u32(lo[k] + 2 * hi[k] + (4 * top if k == 0 else 0) + c)
            assert x < 2**31
            sh = 28 if k == nl - 1 else 29
            c = x >> sh
            o[k] = x & (2**sh - 1)
        o[0] += c
        return o

    def sqr(self, a):
        # sqr_ps / sqr_i sum the same products with the off-diagonal ones doubled first: the same
        # column sums as mul(a, a), and d[i] = 2 a[i] must fit 32 bits
        for x in a:
            self._u32(2 * x)
        return self.mul(a, a)

    def chained(self, op, a, b):
        """The limbs of janus_hpke_selftest_field's chained op for fields 1 / 2."""
        k = self.k
        if op == 6:
            return self.mul(self.add(a, b), self.sub(a, b))
        if op == 7:
            return self.sqr(self.sub(self.mul_small(a, k), b))
        if op == 8:
            AA, BB = self.sqr(self.add(a, b)), self.sqr(self.sub(a, b))
            E = self.sub(AA, BB)
            return self.mul(E, self.add(AA, self.mul_small(E, k)))
        x = self.add(self.add(a, a), self.add(b, b))
        return self.mul(x, x)


def chained_int(field, op, a, b):
    """The same operation on plain integers."""
    p, k = (P448, 39081) if field == 1 else (P521, 8)
    if op == 6:
        return (a + b) * (a - b) % p
    if op == 7:
        return (k * a - b) ** 2 % p
    if op == 8:
        AA, BB = (a + b) ** 2, (a - b) ** 2
        E = AA - BB
        return E * (AA + k * E) % p
    return (2 * a + 2 * b) ** 2 % p


def edge_values(field):
    """The edge operands of test_gpu_x448_p521_field_ops_match_python for fields 1 / 2; the
    all-ones values 2^448 - 1 and 2^521 - 1 (every limb maximal) are among them."""
    P, bits = (P448, 448) if field == 1 else (P521, 521)
    e = [0, 1, 2, P - 1, P - 2, P, 2**bits - 1, 2**bits - 2, (P - 1) // 2, 2**(bits - 1),
         {1: 2**224, 2: 2**260}[field], {1: 2**224 - 1, 2: 2**29 - 1}[field]]
    if field == 1:
        e.append(P + 1)
    return e


def chained_operands(field, n_random=512):
    """(a, b): the full edge x edge cross product, then random pairs below 2^bits."""
    e = edge_values(field)
    bits = 448 if field == 1 else 521
    rnd = random.Random(1000 + field)
    a = [x for x in e for _ in e] + [rnd.randrange(2**bits) for _ in range(n_random)]
    b = [y for _ in e for y in e] + [rnd.randrange(2**bits) for _ in range(n_random)]
    return a, b


@pytest.mark.parametrize("op", CHAINED_OPS)
@pytest.mark.parametrize("field", [1, 2])
def test_limbs_entering_products_stay_within_the_stated_bounds(field, op):
    L = Limbs(field)
    a, b = chained_operands(field)
    assert 2**L.bits - 1 in a and 2**L.bits - 1 in b
    for x, y in zip(a, b):
        r = L.chained(op, L.from_int(x), L.from_int(y))   # asserts every bound on the way
        assert L.value(r) % L.p == chained_int(field, op, x, y), (field, op, hex(x), hex(y))
    # the chained ops do feed the products limbs above their nominal width
    over = [i for i in range(L.nl) if L.seen[i] >= L.nominal[i]]
    assert over and set(over) <= ({0, 8} if field == 1 else {0}), \
        (over, [hex(s) for s in L.seen])
    print(f"field {field} op {op}: largest limbs entering a product:",
          {i: hex(L.seen[i]) for i in over})


def test_a_limb_past_the_bound_is_caught():
    L = Limbs(1)
    with pytest.raises(AssertionError, match="enters a product"):
        L.mul([2**29] + [0] * 15, L.from_int(1))
    L = Limbs(2)
    with pytest.raises(AssertionError, match="enters a product"):
        L.mul(L.from_int(1), [2**29 + 2**6] + [0] * 17)
