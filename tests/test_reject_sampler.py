"""The test-rejection predicate of the two CPU restatements (test infrastructure, default off):
with it on, the C restatement and prio3_py -- independent implementations -- agree on shard and
on the helper's prepare_init, on reports that hold real rejections."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import prio3_py as P

VK = bytes(range(0x40, 0x50))
BITS = 6


@pytest.fixture
def reject_bits():
    O.set_test_reject(BITS)
    P.reject_bits = BITS
    yield BITS
    O.set_test_reject(0)
    P.reject_bits = 0


def test_predicate_is_off_by_default_and_a_superset():
    assert O.get_test_reject() == 0 and P.reject_bits == 0
    for F in (P.Field64, P.Field128):
        top = (1 << (8 * F.es)) - (1 << (8 * F.es - 10))  # smallest value with 10 top ones
        for v in (0, 1, top - 1, F.p - 1):
            assert P.accept(F, v, 0) == (v < F.p)
        assert P.accept(F, top - 1, 10) and not P.accept(F, top, 10)
        assert not P.accept(F, F.p - 1, 24) and not P.accept(F, F.p, 0)


@pytest.mark.parametrize("cfg", [dict(kind="count"),
                                 dict(kind="histogram", length=10, chunk_length=3)],
                         ids=["count", "hist_10_c3"])
def test_c_and_python_restatements_agree(cfg, reject_bits):
    o = O.Oracle(**cfg)
    py = P.Prio3(P.Prio3Type(**cfg))
    rng = np.random.default_rng(5)
    rejected, plain = 0, []
    for i in range(12):
        m = int(rng.integers(0, 2 if cfg["kind"] == "count" else cfg["length"]))
        nonce, rand = rng.bytes(16), rng.bytes(o.rand_size)
        with O.RejectRecord() as rec:
            pub, leader, helper = o.shard(m, nonce, rand)
            rc, state, ps = o.prepare_init(VK, 1, nonce, pub, helper)
        assert rc == 0
        rejected += any(c for c, _ in rec.streams().values())
        assert py.shard(m, nonce, rand) == (pub, leader, helper), i
        (meas, corrected), pps, _ = py.prepare_init(VK, 1, nonce, pub, helper)
        assert pps == ps, i
        assert b"".join(py.F.enc(x) for x in meas) + corrected == state[:len(state) - (
            0 if o.jr_len else 16)], i
        # the report still verifies: both prep shares combine and the output share comes out
        rc0, st0, lps = o.prepare_init(VK, 0, nonce, pub, leader)
        rc1, msg = o.prep_shares_to_prep_msg(lps, ps)
        assert rc0 == 0 and rc1 == 0 and o.prepare_next(state, msg)[0] == 0, i
        plain.append((m, nonce, rand, pub, leader, helper))
    assert rejected >= 2, rejected
    # with the predicate off again the same inputs give other shares wherever it had rejected
    O.set_test_reject(0)
    assert sum(o.shard(m, n, r) != (a, b, c) for m, n, r, a, b, c in plain) >= 1
