"""The launch table of the prepare chains: which kernels one call launches, per instance, role,
entry point and option set (tests/golden/launch_table.json, recorded by
tests/golden/gen_launch_table.py with engine option timing = 2, which counts launches by name).

Every row is replayed on generated reports: the ordered launch list must equal the recorded one,
and the call's statuses, prepare messages (helper) and prepare shares (leader) must equal the CPU
restatement's bit for bit.  The launch plan (plan_prepare / plan_leader, prio3_prepare.hip) may
be rewritten under this table; a row changes only when a launch is meant to change.

Rows: {config, role, entry, options, n, launches}.  config is a name of tests/conftest.py CONFIGS,
"fpvec_<length>x<bits>" or "mp64_<proofs>x<bits>x<length>_c<chunk>"; entry is one of ENTRIES.
"""
import json
import os

import numpy as np
import pytest

from tests.conftest import CONFIGS
from tests.test_gpu_parity import VK, _engine, _oracle, _tamper

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_table.json")
ENTRIES = {"helper": ("prepare", "prepare_aggregate", "prepare_aggregate_batch"),
           "leader": ("leader_prepare_init", "leader_prepare_init_batch")}
# every kernel name launch_prepare, launch_slow_redo and leader_init_run pass to TIMED
KERNEL_NAMES = ["k_mp64_prepare", "k_xof_pair", "k_xofd", "k_xof", "k_xof_a", "k_jrpart",
                "k_xof_slow", "k_query_fpw", "k_query_fp", "k_prep_sum", "k_prep_h", "k_prep_hp",
                "k_query_w", "k_query_h", "k_query_ps", "k_query_sum", "k_query", "k_prep_gen",
                "k_slow_redo", "k_leader_unpack", "k_leader_prep", "k_leader_slowfix",
                "k_leader_init"]
# k_xof is launched by the FPVec chain for a share of fewer than two joint-rand blocks
# (meas_len <= 18); the shortest FPVec share (length 1, 16 bits) has 47 elements, so no valid
# instance reaches it.
UNREACHABLE = {"k_xof"}


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def row_id(row):
    opts = ",".join(f"{k}={v}" for k, v in sorted(row["options"].items()))
    return f"{row['config']}-{row['entry']}-n{row['n']}" + (f"-{opts}" if opts else "")


def _special(config):
    """(family, shape) of the two instances outside CONFIGS, else None."""
    if config.startswith("fpvec_"):
        return "fpvec", tuple(int(x) for x in config[6:].split("x"))
    if config.startswith("mp64_"):
        shape, chunk = config[5:].split("_c")
        return "mp64", tuple(int(x) for x in shape.split("x")) + (int(chunk),)
    return None


def _make_engine(config):
    from janus_amd import prio3 as J
    sp = _special(config)
    if not sp:
        return _engine(CONFIGS[config])
    if sp[0] == "fpvec":
        from tests.test_fpvec import VK as FVK
        return J.HelperEngine(J.Prio3FixedPointBoundedL2VecSum(*sp[1]), FVK, allow_unpinned=True)
    from tests.test_mp64 import VK as MVK
    return J.HelperEngine(J.Prio3SumVecField64MultiproofHmacSha256Aes128(*sp[1]), MVK)


_CASES = {}


def _special_case(config, n):
    """FPVec / multiproof reports from the Python restatement (16 distinct, tiled), with the
    leader input shares kept; the helper's expectation from the compiled restatement."""
    from oracle.oracle import Oracle
    fam, shape = _special(config)
    rng = np.random.default_rng(1000 + n)
    if fam == "fpvec":
        from tests import test_fpvec as T
        v = T._vdaf(*shape)
        o = Oracle("fpvec", bits=shape[1], length=shape[0])
        meas = lambda: T._vector(rng, *shape)
        rand_len = 80
    else:
        from tests import test_mp64 as T
        v = T._vdaf(*shape)
        o = Oracle("sumvec_f64_mp", bits=shape[1], length=shape[2], chunk_length=shape[3],
                   num_proofs=shape[0])
        meas = lambda: [int(x) for x in rng.integers(0, 2 ** shape[1], shape[2])]
        rand_len = 160
    rows = []
    for _ in range(min(n, 16)):
        m = meas()
        nonce = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
        pub, leader, helper = v.shard(m, nonce, bytes(rng.integers(0, 256, rand_len,
                                                                  dtype=np.uint8)))
        _, lps, _ = v.prepare_init(T.VK, 0, nonce, pub, leader)
        rows.append((nonce, pub, leader, helper, bytes(lps)))
    A = lambda k: np.array([list(rows[i % len(rows)][k]) for i in range(n)], np.uint8)
    d = dict(nonces=A(0), public_shares=A(1), leader_shares=A(2), helper_shares=A(3),
             leader_prep_shares=A(4))
    lref = d["leader_prep_shares"].copy()
    # helper: a tampered verifier element and a tampered joint-rand part
    d["leader_prep_shares"][1::17, o.es] ^= 1
    d["leader_prep_shares"][5::23, -1] ^= 0x80
    return o, T.VK, d, lref


def _case(config, role, n):
    """Reports and the restatement's outputs for them, made once per (config, role, n)."""
    key = (config, role, n)
    if key in _CASES:
        return _CASES[key]
    if _special(config):
        o, vk, d, lref = _special_case(config, n)
    else:
        from tests.test_gpu_leader import _reports
        cfg = CONFIGS[config]
        o, vk, lref = _oracle(cfg), VK, None
        if role == "helper":
            d = o.gen_reports(VK, n, seed=7, n_threads=8)
            d = _tamper(o, d, np.random.default_rng(7))
        else:
            d = _reports(o, cfg, n, seed=7)
    if role == "helper":
        ref = o.helper_batch(vk, d["nonces"], d["public_shares"], d["helper_shares"],
                             d["leader_prep_shares"], n_threads=8)
    else:
        # one non-canonical leader measurement-share element: status 6 (InputShareDecode)
        d["leader_shares"][9, :o.es] = 0xFF
        status = np.zeros(n, np.uint8)
        status[9] = 6
        if lref is None:
            lref = np.zeros((n, o.prep_share_len), np.uint8)
            for i in range(n):
                rc, _, lps = o.prepare_init(vk, 0, d["nonces"][i].tobytes(),
                                            d["public_shares"][i].tobytes(),
                                            d["leader_shares"][i].tobytes())
                assert (rc == 0) == (i != 9)
                if rc == 0:
                    lref[i] = np.frombuffer(lps, np.uint8)
        ref = (lref, status)
    _CASES[key] = (d, ref)
    return _CASES[key]


def _call(eng, row, d):
    """The row's call as a closure returning its outputs as numpy arrays."""
    import torch
    entry, n, sz = row["entry"], row["n"], eng.sz
    pub = d["public_shares"] if sz.public_share_len else None
    if entry == "prepare_aggregate_batch":
        return lambda: eng.prepare_aggregate_batch(d["nonces"], pub, d["helper_shares"],
                                                   d["leader_prep_shares"])
    if entry == "leader_prepare_init_batch":
        return lambda: eng.leader_prepare_init_batch(d["nonces"], pub, d["leader_shares"])[:2]
    dev = torch.device("cuda", 0)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nonces, pub = t(d["nonces"]), t(pub)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    if entry == "leader_prepare_init":
        ls = t(d["leader_shares"])
        ps = torch.zeros((n, sz.prep_share_len), dtype=torch.uint8, device=dev)
        run = lambda: eng.leader_prepare_init_device(nonces, pub, ls, ps, status)
        out = ps
    else:
        hs, lps = t(d["helper_shares"]), t(d["leader_prep_shares"])
        out = torch.zeros((n, max(sz.prep_msg_len, 1)), dtype=torch.uint8, device=dev)
        if entry == "prepare":
            run = lambda: eng.prepare_device(nonces, pub, hs, lps, out, status)
        else:
            assert entry == "prepare_aggregate"
            seg = torch.zeros(n, dtype=torch.int32, device=dev)
            run = lambda: eng.prepare_aggregate_device(nonces, pub, hs, lps, seg, 1, out, status)

    def call():
        run()
        torch.cuda.synchronize()
        return out.cpu().numpy(), status.cpu().numpy()
    return call


def run_row(row):
    """Makes the row's call once on a warmed engine with launch counting on; checks its outputs
    against the restatement and returns the ordered launch list [[name, count], ...]."""
    assert row["entry"] in ENTRIES[row["role"]]
    d, ref = _case(row["config"], row["role"], row["n"])
    eng = _make_engine(row["config"])
    for k, v in row["options"].items():
        eng.set_option(k, v)
    call = _call(eng, row, d)
    call()  # once-per-stream and once-per-engine set-up is not part of the table
    eng.set_option("timing", 2)
    got = call()
    launches = [[k, v[1]] for k, v in eng.timing().items()]
    eng.close()
    if row["role"] == "helper":
        np.testing.assert_array_equal(got[1], ref[1])
        np.testing.assert_array_equal(got[0][:, :ref[0].shape[1]], ref[0])
        if row["entry"] == "prepare_aggregate_batch":
            np.testing.assert_array_equal(got[3], ref[3])
            np.testing.assert_array_equal(got[2], ref[2])
    else:
        ok = ref[1] == 0
        np.testing.assert_array_equal(got[1], ref[1])
        np.testing.assert_array_equal(got[0][ok], ref[0][ok])
    return launches


_ROWS = load_table() if os.path.exists(TABLE) else []


def test_table_names_every_prepare_kernel():
    seen = {name for row in _ROWS for name, count in row["launches"] if count}
    assert set(KERNEL_NAMES) - seen == UNREACHABLE


@pytest.mark.parametrize("row", _ROWS, ids=row_id)
def test_launch_table_row(row):
    assert run_row(row) == row["launches"]
