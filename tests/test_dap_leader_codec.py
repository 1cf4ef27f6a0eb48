"""The leader's half of the DAP-09 marshaling (include/janus_dap.h "Leader side"): the host
request encoder against the reference fixtures and the oracle's encoder, the host response
decoder against a pure-Python restatement of what the leader reads
(aggregation_job_driver.rs:657-752) that is first pinned by the reference fixtures, and the
Python wrappers' argument checks.  No GPU: the host forms make no HIP call.

The fixture requests hold two PrepareInits of different public share / enc lengths, the second
with a Finish message.  The encoder's contract is one length per field and Initialize messages
(what a leader's init step sends), so the fixtures are rebuilt one PrepareInit per call and the
lists stitched; the second record's message type byte (2 in the fixture, 0 by the encoder's
contract) is the single byte that is asserted to differ and then compared as such."""
import json
import os
import struct

import numpy as np
import pytest

from oracle import dap_codec as D

FX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "dap_fixtures.json")))
NONE = 0xFFFFFFFF
E_LISTLEN, E_TRAILING, E_MALFORMED, E_REJECT_CODE, E_COUNT, E_ID = -3, -4, -5, -6, -7, -8


# ---- the expected leader decode (pure Python) ------------------------------------------------
def parse_resp(body: bytes):
    """AggregationJobResp -> [(report_id, result)] in oracle.dap_codec's result form, or a
    negative JANUS_DAP_RESP_E* code when the message does not decode."""
    if len(body) < 4:
        return E_LISTLEN
    ln = struct.unpack(">I", body[:4])[0]
    if 4 + ln > len(body):
        return E_LISTLEN
    if 4 + ln < len(body):
        return E_TRAILING
    r = D._R(body)
    r.o = 4
    recs = []
    while r.o < len(body):
        try:
            rid = r.take(16)
            ty = r.u8()
            if ty == 0:
                recs.append((rid, ("continue", D.decode_ping_pong(r.take(r.u32())))))
            elif ty == 1:
                recs.append((rid, ("finished",)))
            elif ty == 2:
                code = r.u8()
                if code > 9:  # PrepareError::decode, messages/src/lib.rs:2185-2196
                    return E_REJECT_CODE
                recs.append((rid, ("reject", code)))
            else:
                return E_MALFORMED
        except D.DecodeError:
            return E_MALFORMED
    return recs


def leader_decode(body: bytes, expected_ids, pml: int):
    """What the leader makes of a response to a request of the reports expected_ids (in request
    order): [(prepare_error, prep_msg bytes)] per position, or the negative error code."""
    recs = parse_resp(body)
    if isinstance(recs, int):
        return recs
    if len(recs) != len(expected_ids):
        return E_COUNT
    out = []
    for (rid, res), want in zip(recs, expected_ids):
        if rid != bytes(want):
            return E_ID
        if res[0] == "reject":
            out.append((res[1], bytes(pml)))
        elif res[0] == "continue" and res[1]["type"] == "finish" and len(res[1]["prep_msg"]) == pml:
            out.append((0xFF, res[1]["prep_msg"]))
        else:  # Finished, or a message leader_continued fails on: VdafPrepError
            out.append((5, bytes(pml)))
    return out


def expected_rows(body, index, ids, pml):
    """leader_decode scattered into the engine's row order through index: (msgs, perr) or code."""
    index = np.asarray(index).astype(np.int64) & 0xFFFFFFFF
    order = sorted((int(j), r) for r, j in enumerate(index) if j != NONE)
    dec = leader_decode(body, [ids[r].tobytes() for _, r in order], pml)
    if isinstance(dec, int):
        return dec
    msgs = np.zeros((len(ids), pml), np.uint8)
    pe = np.full(len(ids), 0xFF, np.uint8)
    for (j, r), (e, m) in zip(order, dec):
        pe[r] = e
        msgs[r] = np.frombuffer(m, np.uint8)
    return msgs, pe


def test_expected_decode_is_pinned_by_the_reference_fixtures():
    rid1, rid2 = bytes(range(1, 17)), bytes(range(16, 0, -1))
    body = bytes.fromhex(FX["agg_job_resp"])
    recs = parse_resp(body)
    assert recs == [(rid1, ("continue", dict(type="continue", prep_msg=b"01234",
                                             prep_share=b"56789"))), (rid2, ("finished",))]
    assert D.encode_agg_job_resp(recs) == body
    three = bytes.fromhex(FX["prepare_resps"])
    recs3 = parse_resp(struct.pack(">I", len(three)) + three)
    assert [r[1][0] for r in recs3] == ["continue", "finished", "reject"]
    assert recs3[2] == (bytes([255] * 16), ("reject", 5))
    assert b"".join(D.encode_prepare_resp(*r) for r in recs3) == three
    assert leader_decode(body, [rid1, rid2], 5) == [(5, bytes(5)), (5, bytes(5))]
    assert leader_decode(body, [rid1, rid1], 5) == E_ID
    assert leader_decode(body, [rid1], 5) == E_COUNT


# ---- request encode ---------------------------------------------------------------------------
def make_job(n, psl, enc_len, stride, ps_len, seed, mixed_ct=True, excluded=()):
    rng = np.random.default_rng(seed)
    u8 = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)  # noqa: E731
    j = dict(report_ids=u8(n, 16), times=(1_700_000_000 + rng.integers(0, 1 << 33, n)).astype(np.uint64),
             public_shares=u8(n, psl), config_ids=u8(n), enc=u8(n, enc_len), ct=u8(n, stride),
             prep_shares=u8(n, ps_len), leader_status=np.zeros(n, np.uint8))
    j["ct_len"] = (rng.integers(0, stride + 1, n) if mixed_ct else np.full(n, stride - 3)).astype(np.uint32)
    for r in excluded:
        j["leader_status"][r] = 1 + r % 7
    return j


def oracle_body(j, agg_param, qt, bid):
    inits = [dict(report_id=j["report_ids"][r].tobytes(), time=int(j["times"][r]),
                  public_share=j["public_shares"][r].tobytes(), config_id=int(j["config_ids"][r]),
                  enc=j["enc"][r].tobytes(), payload=j["ct"][r, :j["ct_len"][r]].tobytes(),
                  message=dict(type="initialize", prep_share=j["prep_shares"][r].tobytes()))
             for r in range(len(j["times"])) if j["leader_status"][r] == 0]
    return D.encode_agg_init_req(agg_param, qt, bid, inits)


def expected_index(status):
    inc = status == 0
    return np.where(inc, np.cumsum(inc) - 1, NONE).astype(np.uint32)


def job_args(j):
    return (j["report_ids"], j["times"], j["public_shares"], j["config_ids"], j["enc"], j["ct"],
            j["ct_len"], j["prep_shares"], j["leader_status"])


@pytest.mark.parametrize("key,qt", [("agg_init_req_time_interval", 1), ("agg_init_req_fixed_size", 2)])
def test_host_req_encoder_reproduces_the_reference_fixtures(key, qt):
    from janus_amd import dap as J
    fx = bytes.fromhex(FX[key])
    d = D.decode_agg_init_req(fx)
    lists = []
    for i, p in enumerate(d["prepare_inits"]):
        share = p["message"].get("prep_share", p["message"].get("prep_msg"))
        a = lambda b: np.frombuffer(b, np.uint8).reshape(1, -1)  # noqa: E731
        body, index, ninc = J.encode_req_host(
            d["aggregation_parameter"], qt, d["batch_id"], a(p["report_id"]),
            np.array([p["time"]], np.uint64), a(p["public_share"]),
            np.array([p["config_id"]], np.uint8), a(p["enc"]), a(p["payload"]),
            np.array([len(p["payload"])], np.uint32), a(share), np.zeros(1, np.uint8))
        assert index.tolist() == [0] and ninc == 1
        as_init = dict(p, message=dict(type="initialize", prep_share=share))
        assert body == D.encode_agg_init_req(d["aggregation_parameter"], qt, d["batch_id"], [as_init])
        lists.append(body)
    hdr_len = 4 + 6 + 1 + (32 if qt == 2 else 0) + 4
    assert lists[0][:hdr_len - 4] == lists[1][:hdr_len - 4] == fx[:hdr_len - 4]
    rec0, rec1 = lists[0][hdr_len:], lists[1][hdr_len:]
    got = fx[:hdr_len - 4] + struct.pack(">I", len(rec0) + len(rec1)) + rec0 + rec1
    # record 0 (an Initialize message) and everything around it byte for byte; record 1 differs
    # in its message type byte alone: the fixture's Finish, where a leader's init sends Initialize
    assert got[:hdr_len + len(rec0)] == fx[:hdr_len + len(rec0)]
    diff = [i for i in range(len(fx)) if got[i] != fx[i]]
    assert len(got) == len(fx) and diff == [len(fx) - 5] and (fx[-5], got[-5]) == (2, 0)


@pytest.mark.parametrize("qt", [1, 2])
@pytest.mark.parametrize("case", ["mixed", "uniform", "edges", "all_excluded", "empty", "no_pub"])
def test_host_req_encoder_matches_oracle(case, qt):
    from janus_amd import dap as J
    n, psl = (0 if case == "empty" else 37), (0 if case == "no_pub" else 32)
    excluded = {"edges": (0, 1, 17, 18, 19, 36), "all_excluded": range(n), "mixed": (5,)}.get(case, ())
    j = make_job(n, psl, 32, 80, 48, seed=len(case) + qt, mixed_ct=case != "uniform",
                 excluded=excluded)
    bid = bytes(range(32)) if qt == 2 else None
    body, index, ninc = J.encode_req_host(b"param"[:qt * 2], qt, bid, *job_args(j))
    assert body == oracle_body(j, b"param"[:qt * 2], qt, bid)
    np.testing.assert_array_equal(index, expected_index(j["leader_status"]))
    assert ninc == int((j["leader_status"] == 0).sum())
    # an excluded report's ct_len is not looked at
    if excluded:
        j["ct_len"][list(excluded)[0]] = 10_000
        assert J.encode_req_host(b"param"[:qt * 2], qt, bid, *job_args(j))[0] == body


# ---- response decode --------------------------------------------------------------------------
def make_resp(ids, kinds, pml, seed):
    """kinds[j]: 'c' Continue-Finish(pml), 'f' Finished, 0..9 Reject, or a ping-pong message dict
    (Continue with that message)."""
    rng = np.random.default_rng(seed)
    resps = []
    for rid, k in zip(ids, kinds):
        if isinstance(k, dict):
            res = ("continue", k)
        elif k == "c":
            res = ("continue", dict(type="finish", prep_msg=bytes(rng.integers(0, 256, pml, dtype=np.uint8))))
        elif k == "f":
            res = ("finished",)
        else:
            res = ("reject", int(k))
        resps.append((bytes(rid), res))
    return D.encode_agg_job_resp(resps)


def index_with_holes(n, holes):
    st = np.zeros(n, np.uint8)
    st[list(holes)] = 1
    return expected_index(st)


def host_decode(body, index, ids, pml):
    """J.unpack_resp_host -> (msgs, perr) or the error code."""
    from janus_amd import dap as J
    try:
        return J.unpack_resp_host(body, index, ids, int((np.asarray(index) != NONE).sum()), pml)
    except J.RespError as e:
        return e.code


def assert_same_decode(got, want):
    if isinstance(want, int):
        assert got == want
    else:
        assert not isinstance(got, int), got
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[0], want[0])


def test_host_resp_decoder_on_the_fixture():
    ids = np.array([list(range(1, 17)), list(range(16, 0, -1))], np.uint8)
    body = bytes.fromhex(FX["agg_job_resp"])
    msgs, pe = host_decode(body, np.array([0, 1], np.uint32), ids, 5)
    assert pe.tolist() == [5, 5] and not msgs.any()  # Continue{Continue}, Finished
    assert host_decode(body, np.array([1, 0], np.uint32), ids, 5) == E_ID
    # a third engine row that was left out of the request
    ids3 = np.vstack([ids[:1], np.zeros((1, 16), np.uint8), ids[1:]])
    msgs, pe = host_decode(body, np.array([0, NONE, 1], np.uint32), ids3, 5)
    assert pe.tolist() == [5, 0xFF, 5]


@pytest.mark.parametrize("pml", [16, 0, 5])
def test_host_resp_decoder_random_mixes(pml):
    rng = np.random.default_rng(pml)
    for trial in range(6):
        n = int(rng.integers(1, 90))
        ids = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        index = index_with_holes(n, rng.choice(n, n // 5, replace=False))
        inc = [r for r in range(n) if index[r] != NONE]
        kinds = [("c" if x < 0.6 else "f" if x < 0.7 else int(rng.integers(0, 10)))
                 for x in rng.random(len(inc))]
        body = make_resp(ids[inc], kinds, pml, seed=trial)
        got = host_decode(body, index, ids, pml)
        assert_same_decode(got, expected_rows(body, index, ids, pml))
        assert (got[1][inc] == 0xFF).tolist() == [k == "c" for k in kinds]
    # a permuted index (rows in another order than the request)
    ids = rng.integers(0, 256, (4, 16), dtype=np.uint8)
    index = np.array([2, NONE, 0, 1], np.uint32)
    body = make_resp(ids[[2, 3, 0]], ["c", 3, "f"], pml, seed=9)
    got = host_decode(body, index, ids, pml)
    assert_same_decode(got, expected_rows(body, index, ids, pml))
    assert got[1].tolist() == [5, 0xFF, 0xFF, 3]


def test_host_resp_decoder_other_wellformed_messages_fail_the_report():
    pml = 16
    ids = np.arange(5 * 16, dtype=np.uint8).reshape(5, 16)
    kinds = ["c", dict(type="initialize", prep_share=b"s" * 16),
             dict(type="continue", prep_msg=b"m" * 16, prep_share=b"s" * 7),
             dict(type="finish", prep_msg=b"m" * 15), dict(type="finish", prep_msg=b"m" * 17)]
    body = make_resp(ids, kinds, pml, seed=1)
    msgs, pe = host_decode(body, np.arange(5, dtype=np.uint32), ids, pml)
    assert pe.tolist() == [0xFF, 5, 5, 5, 5]
    assert msgs[0].any() and not msgs[1:].any()
    assert_same_decode((msgs, pe), expected_rows(body, np.arange(5), ids, pml))


def test_host_resp_decoder_whole_response_errors():
    pml = 16
    ids = np.arange(3 * 16, dtype=np.uint8).reshape(3, 16)
    index = np.arange(3, dtype=np.uint32)
    good = make_resp(ids, ["c", 4, "f"], pml, seed=2)
    assert not isinstance(host_decode(good, index, ids, pml), int)
    codes = {}
    bad = bytearray(good)
    bad[4 + 42 + 17] = 10  # the Reject's code
    codes["reject_code"] = host_decode(bytes(bad), index, ids, pml)
    bad = bytearray(good)
    bad[4 + 42 + 3] ^= 1  # the second record's report ID
    codes["id"] = host_decode(bytes(bad), index, ids, pml)
    codes["too_few"] = host_decode(make_resp(ids[:2], ["c", 4], pml, 2), index, ids, pml)
    more = np.vstack([ids, ids[:1]])
    codes["too_many"] = host_decode(make_resp(more, ["c", 4, "f", "f"], pml, 2), index, ids, pml)
    codes["trailing"] = host_decode(good + b"\0", index, ids, pml)
    codes["truncated"] = host_decode(good[:-1], index, ids, pml)
    assert codes == dict(reject_code=E_REJECT_CODE, id=E_ID, too_few=E_COUNT, too_many=E_COUNT,
                         trailing=E_TRAILING, truncated=E_LISTLEN)
    for k, code in codes.items():
        assert code < 0, k
    assert len({codes[k] for k in ("reject_code", "id", "too_few", "trailing", "truncated")}) == 5
    # every truncation of the body: as sent (the list length runs past the body), and with the
    # list length patched to the cut (a cut record does not decode; a cut at a record boundary
    # is a count mismatch)
    bounds = {4, 4 + 42, 4 + 42 + 18}
    for cut in range(len(good)):
        assert host_decode(good[:cut], index, ids, pml) == E_LISTLEN, cut
        if cut >= 4:
            patched = struct.pack(">I", cut - 4) + good[4:cut]
            want = E_COUNT if cut in bounds else E_MALFORMED
            assert host_decode(patched, index, ids, pml) == want, cut
            assert leader_decode(patched, [i.tobytes() for i in ids], pml) == want, cut
    # malformed ping-pong messages: an unknown type, an inner length that disagrees, and an
    # unknown PrepareStepResult type
    for pos, val in ((4 + 21, 3), (4 + 25, 15), (4 + 16, 3)):
        bad = bytearray(good)
        bad[pos] = val
        assert host_decode(bytes(bad), index, ids, pml) == E_MALFORMED, pos
        assert leader_decode(bytes(bad), [i.tobytes() for i in ids], pml) == E_MALFORMED, pos


# ---- wrappers ---------------------------------------------------------------------------------
def test_wrapper_argument_checks():
    import torch
    from janus_amd import dap as J
    j = make_job(5, 32, 32, 64, 48, seed=1)
    args = list(job_args(j))
    with pytest.raises(ValueError):
        J.encode_req_host(b"", 3, None, *args)            # no such query type
    with pytest.raises(ValueError):
        J.encode_req_host(b"", 2, None, *args)            # FixedSize without a batch ID
    with pytest.raises(ValueError):
        J.encode_req_host(b"", 1, bytes(32), *args)       # TimeInterval with one
    with pytest.raises(ValueError):
        J.encode_req_host(b"", 2, bytes(31), *args)
    for pos, bad in ((0, j["report_ids"][:, :15]), (1, j["times"][:4]), (4, j["enc"][:4]),
                     (6, j["ct_len"][:4]), (8, j["leader_status"][:3])):
        a = list(args)
        a[pos] = bad
        with pytest.raises(ValueError):
            J.encode_req_host(b"", 1, None, *a)
    a = list(args)
    a[6] = j["ct_len"].copy()
    a[6][2] = 65                                          # above the row length
    with pytest.raises(ValueError, match="ct_len"):
        J.encode_req_host(b"", 1, None, *a)
    ids = j["report_ids"]
    with pytest.raises(ValueError):
        J.unpack_resp_host(b"\0\0\0\0", np.array([0, 0, 1, 2, 3]), ids, 4, 16)   # not a numbering
    with pytest.raises(ValueError):
        J.unpack_resp_host(b"\0\0\0\0", np.arange(5), ids, 4, 16)                # n_included off
    with pytest.raises(ValueError):
        J.unpack_resp_host(b"\0\0\0\0", np.arange(4), ids, 4, 16)                # index length
    # the device forms refuse host tensors before any call into the library
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                          np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else
                          np.ascontiguousarray(x)) for x in args]
    with pytest.raises(ValueError):
        J.encode_req_device(b"", 1, None, *t)
    with pytest.raises(ValueError):
        J.unpack_resp_device(torch.zeros(8, dtype=torch.uint8), 4, t[6], t[0], 0, 16)
    # the merged outcome
    out = J.leader_outcome(np.array([0, 3, 0, 0, 0], np.uint8),
                           np.array([0xFF, 0xFF, 4, 0xFF, 9], np.uint8),
                           np.array([0, 0, 0, 4, 4], np.uint8))
    assert out.tolist() == [0xFF, 5, 4, 5, 9]
    tt = lambda x: torch.tensor(x, dtype=torch.uint8)  # noqa: E731
    assert J.leader_outcome(tt([0, 3, 0, 0, 0]), tt([0xFF, 0xFF, 4, 0xFF, 9]),
                            tt([0, 0, 0, 4, 4])).tolist() == [0xFF, 5, 4, 5, 9]
