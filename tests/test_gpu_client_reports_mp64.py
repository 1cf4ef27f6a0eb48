"""Client::prepare_report in one device call for Prio3SumVecField64MultiproofHmacSha256Aes128
(prio3_client_prepare_reports_device with the 64-byte public share and 160 bytes of randomness):
every field of every emitted DAP `Report` against the Python restatement's shard and OpenSSL's
HPKE (oracle.hpke), the per-report statuses, and the whole chain on the device -- client, leader
upload, leader init, the helper's sealed one-call init, the leader's next and both aggregates."""
import functools

import numpy as np
import pytest

from oracle import hpke as H
from tests.test_gpu_client_reports import (CFG_HELPER, CFG_LEADER, INFO_HELPER, INFO_LEADER,
                                           PRECISION, T0, _parse_report)
from tests.test_gpu_client_shard_mp64 import P64, SHAPES, _engine, _inputs, _ref_row

pytestmark = pytest.mark.gpu

N = 67
X, P = H.KEM_X25519, H.KEM_P256
TASKPROV_EXT = ((0xFF00, b""),)


@functools.lru_cache(maxsize=None)
def _case(shape, n, lkem, hkem):
    """Keys, times and ephemeral keys of one batch over the first n reports of the shape's inputs
    (numpy, read-only), shared by the tests of a (shape, KEM pair)."""
    rng = np.random.default_rng([n, lkem, hkem, *shape])
    m, ids, rand = _inputs(shape, n)
    keys = {}
    for who, kem in (("leader", lkem), ("helper", hkem)):
        skR = H.kem_private(rng, kem)
        keys[who] = (skR, H.kem_public(skR, kem), kem)
    sk = lambda kem: np.stack([np.frombuffer(H.kem_private(rng, kem), np.uint8)  # noqa: E731
                               for _ in range(n)])
    c = dict(m=m, ids=ids, rand=rand, times=(T0 + rng.integers(0, 7200, n)).astype(np.uint64),
             sk_l=sk(lkem), sk_h=sk(hkem), keys=keys,
             task=bytes(rng.integers(0, 256, 32, dtype=np.uint8)))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def _run(eng, c, **kw):
    import torch
    from janus_amd import hpke as G
    t = lambda a: torch.from_numpy(  # noqa: E731 (a copy: the inputs are read-only)
        np.array(a).view(np.int64) if a.dtype == np.uint64 else np.array(a)).cuda()
    lk, hk = c["keys"]["leader"], c["keys"]["helper"]
    ls = G.HpkeSealer(lk[1], INFO_LEADER, device=0, kem_id=lk[2])
    hs = G.HpkeSealer(hk[1], INFO_HELPER, device=0, kem_id=hk[2])
    args = dict(leader_sealer=ls, helper_sealer=hs, task_id=c["task"], time_precision=PRECISION,
                measurements=t(c["m"]), report_ids=t(c["ids"]), times=t(c["times"]),
                rand=t(c["rand"]), sk_e_leader=t(c["sk_l"]), sk_e_helper=t(c["sk_h"]),
                leader_config_id=CFG_LEADER, helper_config_id=CFG_HELPER)
    args.update(kw)
    out = eng.prepare_reports_device(**args)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _good_run(shape, n, lkem, hkem):
    return _run(_engine(shape), _case(shape, n, lkem, hkem))


def _check_report(c, shape, i, raw, ext=()):
    """Every field of report i against the restatements."""
    r = _parse_report(raw)
    pub, lshare, hshare = _ref_row(shape, i)
    t = int(c["times"][i])
    assert r["report_id"] == c["ids"][i].tobytes()
    assert r["time"] == t - t % PRECISION and r["time"] % PRECISION == 0
    assert r["public_share"] == pub and len(pub) == 64
    aad = H.input_share_aad(c["task"], r["report_id"], r["time"], pub)
    for who, cfgid, info, share, sk in (("leader", CFG_LEADER, INFO_LEADER, lshare, c["sk_l"]),
                                        ("helper", CFG_HELPER, INFO_HELPER, hshare, c["sk_h"])):
        skR, pkR, kem = c["keys"][who]
        pt = H.plaintext_input_share(share, ext)
        enc, ct = H.seal(pkR, sk[i].tobytes(), info, aad, pt, kem=kem)
        assert r[who]["config_id"] == cfgid
        assert r[who]["enc"] == H.kem_public(sk[i].tobytes(), kem) == enc, who
        assert r[who]["payload"] == ct, who
        assert H.open_(skR, pkR, r[who]["enc"], info, aad, r[who]["payload"], kem=kem) == pt, who


@pytest.mark.parametrize("lkem,hkem,taskprov", [(X, P, False), (P, X, False), (X, P, True)])
def test_every_field_of_every_report(lkem, hkem, taskprov):
    shape = SHAPES[1]
    c = _case(shape, N, lkem, hkem)
    out = _run(_engine(shape), c, with_taskprov_extension=True) if taskprov \
        else _good_run(shape, N, lkem, hkem)
    assert not out["status"].any()
    assert (c["times"] % PRECISION != 0).any()  # the rounding is exercised
    for i in range(N):
        ln = out["report_len"][i]
        _check_report(c, shape, i, out["reports"][i, :ln].tobytes(),
                      TASKPROV_EXT if taskprov else ())
        assert not out["reports"][i, ln:].any()


def test_statuses():
    """An invalid measurement gives 1 and a zero P-256 ephemeral key the sealer's 0x40: no report
    (length 0, a zero row); the neighbouring reports are those of the clean run."""
    shape = SHAPES[1]
    c = dict(_case(shape, N, X, P))
    good = _good_run(shape, N, X, P)
    m, sk_h = c["m"].copy(), c["sk_h"].copy()
    m[3, 2] = 1 << shape[1]
    m[64, 9] = (1 << 64) - 1
    sk_h[5] = 0
    sk_h[65] = 0
    c["m"], c["sk_h"] = m, sk_h
    out = _run(_engine(shape), c)
    want = np.zeros(N, np.uint8)
    want[[3, 64]] = 1
    want[[5, 65]] = 0x40
    assert np.array_equal(out["status"], want)
    for i in range(N):
        if want[i]:
            assert out["report_len"][i] == 0 and not out["reports"][i].any()
        else:
            assert out["report_len"][i] == good["report_len"][i] > 0
            assert np.array_equal(out["reports"][i], good["reports"][i])


def test_whole_chain_on_the_device():
    """prepare_reports_device -> leader_upload_batch -> leader_prepare_init_batch; the helper's
    ciphertext rows and the leader's prep shares into prio3_helper_aggregate_init_batch_ex; the
    leader's prepare_next + aggregate.  Everything is accepted and the aggregates unshard to the
    plaintext column sums."""
    from janus_amd import hpke as G
    shape = SHAPES[3]
    n, length = 130, shape[2]
    eng = _engine(shape)
    c = _case(shape, n, X, P)
    out = _run(eng, c)
    assert not out["status"].any()
    lk, hk = c["keys"]["leader"], c["keys"]["helper"]
    now = T0 + 10_000
    deadline = now + 60
    ct_stride = -(-(6 + eng.sz.helper_share_len + 16) // 16) * 16
    rows = np.pad(out["reports"], ((0, 0), (0, -out["reports"].shape[1] % 16)))  # stride % 4 == 0
    up = eng.leader_upload_batch(
        rows, out["report_len"].view(np.uint32), c["task"], now, deadline,
        task_opener=G.HpkeOpener(lk[0], lk[1], INFO_LEADER, device=0, kem_id=lk[2]),
        task_config_id=CFG_LEADER, helper_enc_len=H.nenc(hk[2]), helper_ct_stride=ct_stride)
    assert not up["status"].any()
    assert np.array_equal(up["report_ids"], c["ids"])
    assert np.array_equal(up["times"], c["times"] - c["times"] % PRECISION)
    assert (up["helper_config_ids"] == CFG_HELPER).all()
    lps, lst, lbatch = eng.leader_prepare_init_batch(up["report_ids"], up["public_shares"],
                                                     up["leader_input_shares"])
    assert not lst.any()
    opener = G.HpkeOpener(hk[0], hk[1], INFO_HELPER, device=0, kem_id=hk[2])
    msgs, hst, hagg, hcnt = eng.aggregate_init_batch(
        opener, c["task"], up["report_ids"], up["times"], up["public_shares"], up["helper_enc"],
        up["helper_ct"], up["helper_ct_len"], lps, report_deadline=deadline)
    assert not hst.any() and int(hcnt[0]) == n
    lst2, lagg, lcnt = lbatch.leader_prepare_next_aggregate(msgs, lst)
    lbatch.free()
    assert not lst2.any() and int(lcnt[0]) == n
    dec = lambda a: [int.from_bytes(a[0, 8 * e:8 * e + 8].tobytes(), "little")  # noqa: E731
                     for e in range(length)]
    got = [(a + b) % P64 for a, b in zip(dec(lagg), dec(hagg))]
    assert got == [int(x) for x in c["m"].astype(object).sum(axis=0)]
