"""Both roles of an aggregation job's init step over the bytes that cross the wire, all on the
device: the synthetic client shards and seals (generate_sealed_reports_device), the leader runs
prepare_init and encodes the AggregationJobInitializeReq (encode_req_device), the helper runs its
pipeline of tests/test_gpu_pipeline.py on those bytes (scan, unpack_device, HPKE open,
prepare_aggregate_device, encode_resp_device), the leader decodes the AggregationJobResp
(unpack_resp_device), runs prepare_next and accumulates.  Tampered leader input shares are left
out of the request; tampered ciphertexts and prepare shares come back as Reject(4) / Reject(5).
Request and response bytes, every report's outcome and both aggregates are checked against the
CPU oracles, and leader + helper aggregate unshards to the plaintext sum of the accepted
measurements (integration_tests/.../common.rs:332-554 over real message bodies)."""
import numpy as np
import pytest

from oracle import dap_codec as D
from oracle import hpke as H
from tests.conftest import CONFIGS
from tests.test_dap_leader_codec import expected_index, expected_rows
from tests.test_gpu_sealed_client import _client_inputs, _instance

pytestmark = pytest.mark.gpu


def _expected_helper(o, vk, skR, pkR, task, body, share_len):
    """The helper's response and aggregate for a request body, from the CPU oracles."""
    P = D.decode_agg_init_req(body)["prepare_inits"]
    n = len(P)
    arr = lambda k: np.frombuffer(b"".join(p[k] for p in P), np.uint8).reshape(  # noqa: E731
        n, len(P[0][k])).copy()
    ids, pubs, enc = arr("report_id"), arr("public_share"), arr("enc")
    times = np.array([p["time"] for p in P], np.uint64)
    stride = -(-max(len(p["payload"]) for p in P) // 16) * 16
    ct = np.zeros((n, stride), np.uint8)
    cl = np.array([len(p["payload"]) for p in P], np.uint32)
    for r, p in enumerate(P):
        ct[r, :cl[r]] = np.frombuffer(p["payload"], np.uint8)
    shares, hs = H.open_input_shares(skR, pkR, task, enc, ct, cl, ids, times,
                                     pubs if pubs.shape[1] else None, share_len)
    assert all(p["message"]["type"] == "initialize" for p in P)
    lps = np.frombuffer(b"".join(p["message"]["prep_share"] for p in P), np.uint8).reshape(n, -1)
    msgs, st, agg, cnt = o.helper_batch(vk, ids, pubs, shares, lps,
                                        accept_mask=(hs == 0).astype(np.uint8), n_threads=8)
    pe = np.where(hs == 0, 0xFF, hs).astype(np.uint8)
    return D.helper_init_resp(ids, pe, st, msgs), agg, cnt


@pytest.mark.parametrize("n", [64, 700])
@pytest.mark.parametrize("name", ["hist_256_c16", "count"])
def test_two_roles_over_wire_bytes(name, n):
    import torch
    from janus_amd import dap as DJ
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    from oracle.oracle import field_modulus
    vdaf, o, vk = _instance(name)
    cfg = CONFIGS[name]
    leader, helper = J.HelperEngine(vdaf, vk, device=0), J.HelperEngine(vdaf, vk, device=0)
    sz = leader.sz
    pml = sz.prep_msg_len
    rng = np.random.default_rng(n + len(name))
    skR = H.kem_private(rng)
    pkR = H.kem_public(skR)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    sealer, opener = G.HpkeSealer(pkR, device=0), G.HpkeOpener(skR, pkR, device=0)
    dev = torch.device("cuda", 0)
    u8 = dict(dtype=torch.uint8, device=dev)

    # 1. the client
    times, sk_e = _client_inputs(n, H.KEM_X25519, 9, dev)
    d = leader.generate_sealed_reports_device(sealer, task, n, times, sk_e, seed=5,
                                              with_checks=True, with_leader_inputs=True)
    pick = rng.permutation(n)
    bad_leader, bad_ct, bad_ps = pick[:3], pick[3:6], pick[6:9]
    d["leader_input_shares"][torch.from_numpy(bad_leader).to(dev), :o.es] = 0xFF  # non-canonical
    d["ct"][torch.from_numpy(bad_ct).to(dev), 5] ^= 1

    # 2. the leader's init
    lps = torch.zeros((n, sz.prep_share_len), **u8)
    lst = torch.zeros(n, **u8)
    leader.leader_prepare_init_device(d["nonces"], d["public_shares"] if sz.public_share_len
                                      else None, d["leader_input_shares"], lps, lst)
    lps[torch.from_numpy(bad_ps).to(dev), 20] ^= 1  # the helper's decide fails on these

    # 3. the request bytes
    cfg_ids = torch.full((n,), 1, **u8)
    req = DJ.encode_req_device(b"", 1, None, d["nonces"], times, d["public_shares"], cfg_ids,
                               d["enc"], d["ct"], d["ct_len"], lps, lst)
    torch.cuda.synchronize()
    assert not d["seal_status"].any() and not req["err"].any()
    h = {k: d[k].cpu().numpy() for k in ("nonces", "public_shares", "enc", "ct", "ct_len",
                                         "leader_input_shares", "measurements")}
    h_lps, h_times = lps.cpu().numpy(), times.cpu().numpy().view(np.uint64)
    exp_lst, states = np.zeros(n, np.uint8), []
    for r in range(n):
        rc, state, ps = o.prepare_init(vk, 0, h["nonces"][r].tobytes(),
                                       h["public_shares"][r].tobytes(),
                                       h["leader_input_shares"][r].tobytes())
        exp_lst[r] = rc != 0
        states.append(state)
        if rc == 0 and r not in bad_ps:
            assert ps == h_lps[r].tobytes(), r
    assert sorted(np.nonzero(exp_lst)[0]) == sorted(bad_leader)
    np.testing.assert_array_equal(lst.cpu().numpy() != 0, exp_lst != 0)
    index = expected_index(exp_lst)
    inc = np.nonzero(exp_lst == 0)[0]
    body = req["out"][:int(req["out_len"][0])].cpu().numpy().tobytes()
    assert body == D.encode_agg_init_req(b"", 1, None, [
        dict(report_id=h["nonces"][r].tobytes(), time=int(h_times[r]),
             public_share=h["public_shares"][r].tobytes(), config_id=1, enc=h["enc"][r].tobytes(),
             payload=h["ct"][r, :h["ct_len"][r]].tobytes(),
             message=dict(type="initialize", prep_share=h_lps[r].tobytes())) for r in inc])
    np.testing.assert_array_equal(req["index"].cpu().numpy().view(np.uint32), index)
    assert int(req["n_included"][0]) == len(inc) == n - 3

    # 4. the helper, on the request as it lies in device memory
    lay = DJ.scan(body, public_share_len=sz.public_share_len, enc_len=32,
                  prep_share_len=sz.prep_share_len)
    m = len(inc)
    assert lay.uniform and lay.n == m
    u, mism = DJ.unpack_device(lay, req["out"], DJ.ct_stride_for(lay))
    shares = torch.empty((m, sz.helper_share_len), **u8)
    hs = torch.empty(m, **u8)
    opener.open_input_shares_device(task, u["enc"], u["ct"], u["ct_len"], u["report_ids"],
                                    u["times"], u["public_shares"] if sz.public_share_len else None,
                                    shares, hs)
    msgs = torch.empty((m, max(pml, 1)), **u8)
    st = torch.empty(m, **u8)
    seg = torch.zeros(m, dtype=torch.int32, device=dev)  # read again by the finish call
    helper.prepare_aggregate_device(u["report_ids"], u["public_shares"] if sz.public_share_len
                                    else None, shares, u["prep_shares"], seg, 1, msgs, st)
    accept = ((hs == 0) & (u["msg_status"] == 0)).to(torch.uint8)
    hagg = torch.zeros((1, sz.agg_share_len), **u8)
    hcnt = torch.zeros(1, dtype=torch.int64, device=dev)
    helper.aggregate_finish_device(st, accept, hagg, hcnt)
    resp, resp_len = DJ.encode_resp_device(u["report_ids"], DJ.prepare_error(hs, u["msg_status"]),
                                           st | u["msg_status"], msgs, pml)
    torch.cuda.synchronize()
    assert int(mism[0]) == 0
    rlen = int(resp_len[0])
    exp_resp, exp_hagg, exp_hcnt = _expected_helper(o, vk, skR, pkR, task, body,
                                                    sz.helper_share_len)
    assert resp[:rlen].cpu().numpy().tobytes() == exp_resp
    np.testing.assert_array_equal(hagg.cpu().numpy(), exp_hagg)

    # 5. the leader reads the response where the helper wrote it
    pmsgs, perr, flags = DJ.unpack_resp_device(resp, rlen, req["index"], d["nonces"], m, pml)
    st2 = torch.where(perr != DJ.NO_ERROR, torch.full_like(lst, DJ.VDAF_PREP_ERROR), lst)
    leader.leader_prepare_next_device(n, pmsgs, st2)
    lagg = torch.zeros((1, sz.agg_share_len), **u8)
    lcnt = torch.zeros(1, dtype=torch.int64, device=dev)
    leader.accumulate_device(n, st2, None, None, 1, lagg, lcnt)
    outcome = DJ.leader_outcome(lst, perr, st2)
    torch.cuda.synchronize()
    assert int(flags[0]) == 0

    # 6. outcomes, counts and the unsharded aggregate
    exp_msgs, exp_perr = expected_rows(exp_resp, index, h["nonces"], pml)
    np.testing.assert_array_equal(perr.cpu().numpy(), exp_perr)
    np.testing.assert_array_equal(pmsgs.cpu().numpy()[:, :pml], exp_msgs)
    assert sorted(np.nonzero(exp_perr == 4)[0]) == sorted(bad_ct)
    assert sorted(np.nonzero(exp_perr == 5)[0]) == sorted(bad_ps)
    exp_next = np.zeros(n, np.uint8)
    for r in range(n):
        if exp_lst[r] == 0 and exp_perr[r] == 0xFF:
            exp_next[r] = o.prepare_next(states[r], exp_msgs[r].tobytes())[0] != 0
    exp_outcome = DJ.leader_outcome(exp_lst, exp_perr, exp_next)
    np.testing.assert_array_equal(outcome.cpu().numpy(), exp_outcome)
    ok = exp_outcome == 0xFF
    assert int(ok.sum()) == n - 9
    assert int(lcnt[0]) == int(hcnt[0]) == int(exp_hcnt[0]) == n - 9
    p, es = field_modulus(cfg["kind"]), o.es
    dec = lambda t: [int.from_bytes(b[i:i + es], "little")  # noqa: E731
                     for b in [t.cpu().numpy().tobytes()] for i in range(0, len(b), es)]
    total = [(a + b) % p for a, b in zip(dec(lagg[0]), dec(hagg[0]))]
    meas = h["measurements"][ok, 0]
    want = np.bincount(meas, minlength=cfg["length"]).tolist() if cfg["kind"] == "histogram" \
        else [int(meas.sum())]
    assert total == want
