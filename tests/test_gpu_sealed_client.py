"""The sealed synthetic client: HelperEngine.generate_sealed_reports_device produces on the GPU what
a helper actually receives (HPKE-sealed helper input shares), and the helper's one-call init
(prio3_helper_aggregate_init_batch[_ex]) opens, prepares and aggregates them to the same bytes as
the prepare path on the plaintext shares of the same reports -- at test size against the oracle,
and at a size the host sealer could not afford against the two-call device path."""
import numpy as np
import pytest

from oracle import hpke as H
from tests.conftest import CONFIGS
from tests.test_gpu_init_contract import MP_CASES, NO_DEADLINE, VK32

pytestmark = pytest.mark.gpu

VK = bytes(range(0x40, 0x50))
T0 = 1_700_000_000


def _instance(name):
    """(engine VDAF, oracle, verify key) of a CONFIGS name or of the first multiproof case."""
    from janus_amd import prio3 as J
    from oracle.oracle import Oracle
    if name == "multiproof":
        proofs, bits, length, chunk, _ = MP_CASES[0]
        return (J.Prio3SumVecField64MultiproofHmacSha256Aes128(proofs, bits, length, chunk),
                Oracle("sumvec_f64_mp", bits=bits, length=length, chunk_length=chunk,
                       num_proofs=proofs), VK32)
    cfg = CONFIGS[name]
    v = J.Prio3Count() if cfg["kind"] == "count" else J.Prio3Histogram(cfg["length"],
                                                                      cfg["chunk_length"])
    return v, Oracle(**cfg), VK


def _client_inputs(n, kem, seed, dev):
    """times [n] and one ephemeral private key per report (P-256: below 2^255, hence below n)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    times = T0 + torch.randint(0, 3600, (n,), generator=g, device=dev, dtype=torch.int64)
    sk_e = torch.randint(0, 256, (n, 32), generator=g, device=dev, dtype=torch.uint8)
    if kem == H.KEM_P256:
        sk_e[:, 0] &= 0x7F
    return times, sk_e


@pytest.mark.parametrize("name,kem", [("hist_256_c16", H.KEM_X25519), ("count", H.KEM_X25519),
                                      ("multiproof", H.KEM_X25519), ("hist_256_c16", H.KEM_P256)])
def test_sealed_reports_through_the_one_call_init(name, kem):
    import torch
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    n = 437
    vdaf, o, vk = _instance(name)
    eng = J.HelperEngine(vdaf, vk, device=0)
    rng = np.random.default_rng(n)
    skR = H.kem_private(rng, kem)
    pkR = H.kem_public(skR, kem)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    sealer = G.HpkeSealer(pkR, device=0, kem_id=kem)
    opener = G.HpkeOpener(skR, pkR, device=0, kem_id=kem)
    dev = torch.device("cuda", 0)
    times, sk_e = _client_inputs(n, kem, 3, dev)
    d = eng.generate_sealed_reports_device(sealer, task, n, times, sk_e, seed=21)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    assert not h["seal_status"].any()
    assert h["enc"].shape == (n, H.nenc(kem)) and h["ct"].shape[1] % 16 == 0
    pub = h["public_shares"] if eng.sz.public_share_len else None
    kw = dict(report_deadline=NO_DEADLINE) if name == "multiproof" else {}
    msgs, st, agg, cnt = eng.aggregate_init_batch(
        opener, task, h["nonces"], times.cpu().numpy().view(np.uint64), pub, h["enc"], h["ct"],
        h["ct_len"].view(np.uint32), h["leader_prep_shares"], **kw)
    assert not st.any() and int(cnt[0]) == n
    # the prepare path on the plaintext helper shares of the same reports
    pm, ps, pa, pc = eng.prepare_aggregate_batch(h["nonces"], pub, h["helper_shares"],
                                                 h["leader_prep_shares"])
    np.testing.assert_array_equal(st, ps)
    np.testing.assert_array_equal(msgs, pm)
    np.testing.assert_array_equal(agg, pa)
    np.testing.assert_array_equal(cnt, pc)
    # and the oracle
    rm, rs, ra, rc = o.helper_batch(vk, h["nonces"], h["public_shares"], h["helper_shares"],
                                    h["leader_prep_shares"], n_threads=4)
    np.testing.assert_array_equal(st, rs)
    np.testing.assert_array_equal(msgs, rm)
    np.testing.assert_array_equal(agg, ra)
    np.testing.assert_array_equal(cnt, rc)


def test_one_call_init_at_64ki_device_sealed_reports():
    """Histogram(256,16), 65,536 reports sealed on the device (X25519 / AES-128-GCM), three
    segments: the one-call init accepts every report and its aggregate shares and counts equal
    those of prio3_device_prepare_aggregate + finish on the plaintext shares.  No oracle run."""
    import torch
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    n, S = 65536, 3
    eng = J.HelperEngine(J.Prio3Histogram(256, 16), VK, device=0)
    sz = eng.sz
    rng = np.random.default_rng(64)
    skR = H.kem_private(rng)
    pkR = H.kem_public(skR)
    task = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    sealer = G.HpkeSealer(pkR, device=0)
    opener = G.HpkeOpener(skR, pkR, device=0)
    dev = torch.device("cuda", 0)
    times, sk_e = _client_inputs(n, H.KEM_X25519, 5, dev)
    d = eng.generate_sealed_reports_device(sealer, task, n, times, sk_e, seed=77)
    seg_np = np.sort(rng.integers(0, S, n)).astype(np.uint32)
    # the two-call device path on the plaintext shares
    seg = torch.from_numpy(seg_np.astype(np.int32)).to(dev)
    pmsgs = torch.empty((n, max(sz.prep_msg_len, 1)), dtype=torch.uint8, device=dev)
    pst = torch.empty(n, dtype=torch.uint8, device=dev)
    pagg = torch.zeros((S, sz.agg_share_len), dtype=torch.uint8, device=dev)
    pcnt = torch.zeros(S, dtype=torch.int64, device=dev)
    eng.prepare_aggregate_device(d["nonces"], d["public_shares"], d["helper_shares"],
                                 d["leader_prep_shares"], seg, S, pmsgs, pst)
    eng.aggregate_finish_device(pst, None, pagg, pcnt)
    torch.cuda.synchronize()
    assert not d["seal_status"].any() and not pst.any()
    h = {k: d[k].cpu().numpy() for k in ("nonces", "public_shares", "enc", "ct", "ct_len",
                                         "leader_prep_shares")}
    msgs, st, agg, cnt = eng.aggregate_init_batch(
        opener, task, h["nonces"], times.cpu().numpy().view(np.uint64), h["public_shares"],
        h["enc"], h["ct"], h["ct_len"].view(np.uint32), h["leader_prep_shares"],
        segment_ids=seg_np, n_segments=S)
    assert not st.any()
    np.testing.assert_array_equal(cnt, pcnt.cpu().numpy().astype(np.uint64))
    np.testing.assert_array_equal(cnt, np.bincount(seg_np, minlength=S).astype(np.uint64))
    np.testing.assert_array_equal(agg, pagg.cpu().numpy())
    np.testing.assert_array_equal(msgs, pmsgs[:, :sz.prep_msg_len].cpu().numpy())
