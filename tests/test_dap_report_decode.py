"""Host form of the DAP `Report` decoder (janus_dap_report_decode_host), the leader's
`Report::get_decoded`: the reference codec's fixture bytes field by field, decode(encode(x)) == x on
random rows, every way a Report fails to decode (each truncation point, a trailing byte,
report_len above the row) and the argument rules.  No GPU."""
import json
import os

import numpy as np
import pytest

from tests.conftest import ROOT

FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "dap_report_fixtures.json")))["reports"]
OUTPUTS = ("report_ids", "times", "fields", "leader_config_ids", "helper_config_ids", "helper_enc",
           "helper_ct", "helper_ct_len")


def _parse_report(b: bytes) -> dict:
    """Plain-Python Report parser; raises ValueError where the reference's decode fails."""
    def take(o, k):
        if o + k > len(b):
            raise ValueError("a field runs past the Report")
        return b[o:o + k], o + k
    out = {}
    out["report_id"], o = take(0, 16)
    t, o = take(o, 8)
    out["time"] = int.from_bytes(t, "big")
    ln, o = take(o, 4)
    out["public_share_off"] = o
    out["public_share"], o = take(o, int.from_bytes(ln, "big"))
    for who in ("leader", "helper"):
        cfg, o = take(o, 1)
        el, o = take(o, 2)
        enc_off = o
        enc, o = take(o, int.from_bytes(el, "big"))
        pl, o = take(o, 4)
        pay_off = o
        pay, o = take(o, int.from_bytes(pl, "big"))
        out[who] = dict(config_id=cfg[0], enc=enc, payload=pay, enc_off=enc_off, payload_off=pay_off)
    if o != len(b):
        raise ValueError("trailing bytes after the Report")
    return out


def _rows(bodies, stride=None, poison=0xEE):
    """Report rows from byte strings; the bytes of a row past its report are poison."""
    stride = max(map(len, bodies)) if stride is None else stride
    rows = np.full((len(bodies), stride), poison, np.uint8)
    for i, b in enumerate(bodies):
        rows[i, :min(len(b), stride)] = np.frombuffer(b[:stride], np.uint8)
    return rows, np.array([len(b) for b in bodies], np.uint32)


def _check(d, i, body, enc_len, ct_stride):
    """Outputs of row i against the plain-Python parse of `body`."""
    from janus_amd import dap
    try:
        p = _parse_report(body)
    except ValueError:
        assert d["malformed"][i] == 1
        for k in OUTPUTS:
            assert not np.any(d[k][i]), k
        return False
    assert d["malformed"][i] == 0
    assert d["report_ids"][i].tobytes() == p["report_id"] and int(d["times"][i]) == p["time"]
    f = d["fields"][i].tolist()
    assert f[dap.F_PUBLIC_SHARE_OFF] == p["public_share_off"] == 28
    assert f[dap.F_PUBLIC_SHARE_LEN] == len(p["public_share"])
    for who, base in (("leader", dap.F_LEADER_ENC_OFF), ("helper", dap.F_HELPER_ENC_OFF)):
        c = p[who]
        assert f[base:base + 4] == [c["enc_off"], len(c["enc"]), c["payload_off"],
                                    len(c["payload"])], who
        assert int(d[who + "_config_ids"][i]) == c["config_id"]
        # the offsets address the row itself
        assert body[f[base]:f[base] + f[base + 1]] == c["enc"]
        assert body[f[base + 2]:f[base + 2] + f[base + 3]] == c["payload"]
    h = p["helper"]
    if len(h["enc"]) == enc_len and len(h["payload"]) <= ct_stride:
        assert int(d["helper_ct_len"][i]) == len(h["payload"])
        assert d["helper_enc"][i].tobytes() == h["enc"]
        assert d["helper_ct"][i].tobytes() == h["payload"] + bytes(ct_stride - len(h["payload"]))
    else:
        assert d["helper_ct_len"][i] == 0
        assert not d["helper_enc"][i].any() and not d["helper_ct"][i].any()
    return True


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("pad", [0, 9])
def test_host_decode_of_the_reference_fixture(i, pad):
    from janus_amd import dap
    r = FIX[i]
    body = bytes.fromhex(r["hex"])
    rows, ln = _rows([body], len(body) + pad)
    d = dap.report_decode_host(rows, ln, 4, 4 + pad)
    assert d["malformed"].tolist() == [0]
    assert d["report_ids"][0].tobytes() == bytes.fromhex(r["report_id"])
    assert int(d["times"][0]) == r["time"]
    f = d["fields"][0].tolist()
    cut = lambda off, n: body[f[off]:f[off] + f[n]].hex()  # noqa: E731
    assert cut(dap.F_PUBLIC_SHARE_OFF, dap.F_PUBLIC_SHARE_LEN) == r["public_share"]
    assert cut(dap.F_LEADER_ENC_OFF, dap.F_LEADER_ENC_LEN) == r["leader"]["enc"]
    assert cut(dap.F_LEADER_PAYLOAD_OFF, dap.F_LEADER_PAYLOAD_LEN) == r["leader"]["payload"]
    assert cut(dap.F_HELPER_ENC_OFF, dap.F_HELPER_ENC_LEN) == r["helper"]["enc"]
    assert cut(dap.F_HELPER_PAYLOAD_OFF, dap.F_HELPER_PAYLOAD_LEN) == r["helper"]["payload"]
    assert int(d["leader_config_ids"][0]) == r["leader"]["config_id"] == 42
    assert int(d["helper_config_ids"][0]) == r["helper"]["config_id"] == 13
    assert d["helper_enc"][0].tobytes().hex() == r["helper"]["enc"]
    assert d["helper_ct"][0].tobytes() == bytes.fromhex(r["helper"]["payload"]) + bytes(pad)
    assert d["helper_ct_len"].tolist() == [4]
    assert _check(d, 0, body, 4, 4 + pad)


def _random_soa(n, psl, seed):
    rng = np.random.default_rng([seed, n, psl])
    r = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)  # noqa: E731
    lstride, hstride = 208, 64
    return dict(report_ids=r(n, 16), times=rng.integers(0, 1 << 64, n, dtype=np.uint64),
                public_shares=r(n, psl), leader_config_id=42, leader_enc=r(n, 65),
                leader_ct=r(n, lstride),
                leader_ct_len=rng.integers(1, lstride + 1, n).astype(np.uint32),
                helper_config_id=13, helper_enc=r(n, 32), helper_ct=r(n, hstride),
                helper_ct_len=rng.integers(1, hstride + 1, n).astype(np.uint32))


@pytest.mark.parametrize("psl", [0, 32, 5])
def test_decode_of_encode_is_the_identity(psl):
    from janus_amd import dap
    n = 37
    x = _random_soa(n, psl, 11)
    skip = (np.arange(n) % 9 == 4).astype(np.uint8)
    rows, ln = dap.report_encode_host(**x, skip=skip, out_stride=dap.report_max_len(
        psl, 65, 208, 32, 64) + 3)
    d = dap.report_decode_host(rows, ln, 32, 64)
    # a report the encoder left out is an empty body: it does not decode
    assert np.array_equal(d["malformed"], skip)
    ok = skip == 0
    assert np.array_equal(d["report_ids"][ok], x["report_ids"][ok])
    assert np.array_equal(d["times"][ok], x["times"][ok])
    assert (d["leader_config_ids"][ok] == 42).all() and (d["helper_config_ids"][ok] == 13).all()
    assert np.array_equal(d["helper_enc"][ok], x["helper_enc"][ok])
    assert np.array_equal(d["helper_ct_len"][ok], x["helper_ct_len"][ok])
    for i in np.flatnonzero(ok):
        f = d["fields"][i].tolist()
        cut = lambda o, k: rows[i, f[o]:f[o] + f[k]]  # noqa: E731
        assert np.array_equal(cut(dap.F_PUBLIC_SHARE_OFF, dap.F_PUBLIC_SHARE_LEN),
                              x["public_shares"][i])
        assert np.array_equal(cut(dap.F_LEADER_ENC_OFF, dap.F_LEADER_ENC_LEN), x["leader_enc"][i])
        assert np.array_equal(cut(dap.F_LEADER_PAYLOAD_OFF, dap.F_LEADER_PAYLOAD_LEN),
                              x["leader_ct"][i, :x["leader_ct_len"][i]])
        hl = int(x["helper_ct_len"][i])
        assert np.array_equal(d["helper_ct"][i, :hl], x["helper_ct"][i, :hl])
        assert not d["helper_ct"][i, hl:].any()
        assert _check(d, i, rows[i, :ln[i]].tobytes(), 32, 64)
    for i in np.flatnonzero(skip):
        for k in OUTPUTS:
            assert not np.any(d[k][i]), k


def test_every_truncation_a_trailing_byte_and_a_short_row_are_malformed():
    from janus_amd import dap
    body = bytes.fromhex(FIX[1]["hex"])
    cuts = [body[:k] for k in range(len(body))]
    bodies = cuts + [body, body + b"\x00", body]
    rows, ln = _rows(bodies, len(body) + 1)
    ln[-1] = len(body) + 2  # report_len above report_stride: the row itself is whole
    d = dap.report_decode_host(rows, ln, 4, 8)
    want = np.ones(len(bodies), np.uint8)
    want[len(cuts)] = 0
    assert np.array_equal(d["malformed"], want)
    for i, b in enumerate(bodies[:-1]):
        assert _check(d, i, b, 4, 8) == (i == len(cuts))
    for k in OUTPUTS:
        assert not np.any(d[k][-1]), k
    # a cut can leave a shorter Report that decodes only if a length prefix says so: rewrite the
    # helper payload's prefix to the bytes that are left and it decodes again
    short = bytearray(body[:-1])
    short[-4] = 3
    d2 = dap.report_decode_host(*_rows([bytes(short)]), 4, 8)
    assert d2["malformed"].tolist() == [0] and d2["helper_ct_len"].tolist() == [3]
    assert _check(d2, 0, bytes(short), 4, 8)


def test_length_prefix_extremes_do_not_wrap():
    """A prefix of 0xFFFFFFFF (or one that lands exactly on 2^32 with its offset) is malformed."""
    from janus_amd import dap
    body = bytearray.fromhex(FIX[1]["hex"])
    p = _parse_report(bytes(body))
    bodies = []
    for off in (24, p["leader"]["payload_off"] - 4, p["helper"]["payload_off"] - 4):
        for v in (0xFFFFFFFF, (1 << 32) - off - 4, len(body) - off - 4 + 1):
            b = bytearray(body)
            b[off:off + 4] = v.to_bytes(4, "big")
            bodies.append(bytes(b))
    for off in (p["leader"]["enc_off"] - 2, p["helper"]["enc_off"] - 2):
        b = bytearray(body)
        b[off:off + 2] = b"\xff\xff"
        bodies.append(bytes(b))
    rows, ln = _rows(bodies)
    d = dap.report_decode_host(rows, ln, 4, 8)
    assert d["malformed"].all()
    for i, b in enumerate(bodies):
        assert not _check(d, i, b, 4, 8)


def test_unexpected_lengths_are_not_malformed():
    """A public share or enc of another length decodes; a helper enc of another length, or a
    helper payload above the row, only empties the helper rows."""
    from janus_amd import dap
    body = bytes.fromhex(FIX[1]["hex"])
    rows, ln = _rows([body, body, body])
    for enc_len, stride, want_len in ((4, 4, 4), (5, 4, 0), (4, 3, 0), (0, 0, 0)):
        d = dap.report_decode_host(rows, ln, enc_len, stride)
        assert not d["malformed"].any()
        assert d["helper_ct_len"].tolist() == [want_len] * 3
        assert d["fields"][0].tolist() == [28, 4, 35, 6, 45, 6, 54, 4, 62, 4]
        for i in range(3):
            assert _check(d, i, body, enc_len, stride)


def test_argument_rules():
    from janus_amd import dap
    body = bytes.fromhex(FIX[0]["hex"])
    rows, ln = _rows([body])
    with pytest.raises(ValueError):
        dap.report_decode_host(rows, ln, 0x10000, 8)
    with pytest.raises(ValueError):
        dap.report_decode_host(rows, np.zeros(2, np.uint32), 4, 8)
    with pytest.raises(ValueError):
        dap.report_decode_host(rows[0], ln, 4, 8)
    empty = dap.report_decode_host(np.zeros((0, 64), np.uint8), np.zeros(0, np.uint32), 4, 8)
    assert empty["malformed"].shape == (0,) and empty["helper_ct"].shape == (0, 8)
    # the C entry point itself: JANUS_DAP_EARG and nothing written
    L = dap._lib()
    p = lambda a: a.ctypes.data  # noqa: E731
    ids, times = np.full(16, 0x55, np.uint8), np.full(1, 77, np.uint64)
    fields, cfg = np.full(10, 77, np.uint32), np.full(2, 0x55, np.uint8)
    enc, ct, cl = np.full(4, 0x55, np.uint8), np.full(8, 0x55, np.uint8), np.full(1, 77, np.uint32)
    bad = np.full(1, 0x55, np.uint8)

    def call(enc_len=4, stride=rows.shape[1], **null):
        a = dict(rows=p(rows), ln=p(ln), ids=p(ids), times=p(times), fields=p(fields), lcfg=p(cfg),
                 hcfg=p(cfg[1:]), enc=p(enc), ct=p(ct), cl=p(cl), bad=p(bad))
        a.update(null)
        return L.janus_dap_report_decode_host(1, a["rows"], stride, a["ln"], a["ids"], a["times"],
                                              a["fields"], a["lcfg"], a["hcfg"], a["enc"], enc_len,
                                              a["ct"], a["cl"], 8, a["bad"])
    assert call(enc_len=0x10000) == -1
    assert call(stride=1 << 31) == -1
    for k in ("rows", "ln", "ids", "times", "fields", "lcfg", "hcfg", "enc", "ct", "cl", "bad"):
        assert call(**{k: None}) == -1, k
    assert (ids == 0x55).all() and times[0] == 77 and (fields == 77).all() and bad[0] == 0x55
    assert (enc == 0x55).all() and (ct == 0x55).all() and cl[0] == 77
    assert call() == 1
    assert bad[0] == 0 and ids.tobytes() == body[:16] and cl[0] == 4
    assert ct.tobytes() == bytes.fromhex(FIX[0]["helper"]["payload"]) + bytes(4)
