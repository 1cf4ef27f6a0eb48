"""CPU checks of the sealer's boundary: the generated Rust declarations carry the six new entry
points and the new status constant, INTEGRATION.md is in sync with the headers, and the Python
wrappers refuse mismatched shapes before any library call."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests.conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import ffi_rs as F  # noqa: E402

SEAL_FUNCS = ("janus_hpke_sealer_create", "janus_hpke_sealer_destroy", "janus_hpke_seal_device",
              "janus_hpke_seal", "janus_hpke_seal_input_shares_device",
              "janus_hpke_seal_input_shares")


def test_ffi_check_passes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ffi_rs.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_generated_declarations_have_the_sealer():
    r = F.parse_rust(F.gen_rust())
    for f in SEAL_FUNCS:
        assert f in r["funcs"], f
    assert r["consts"]["JANUS_HPKE_SEAL_KEY_ERROR"] == 0x40
    # no DAP PrepareError code (messages/src/lib.rs: 0..=9) and not the engine's merged form of one
    assert r["consts"]["JANUS_HPKE_SEAL_KEY_ERROR"] not in set(range(10)) | {0x80 | c
                                                                            for c in range(10)}
    p = dict(r["funcs"]["janus_hpke_seal_input_shares_device"]["params"])
    assert p["sealer"] == "*mut janus_hpke_sealer" and p["d_sk_e"] == "*const u8"
    assert p["d_times"] == "*const u64" and p["d_ct_len"] == "*mut u32" and p["d_ct"] == "*mut u8"
    assert dict(r["funcs"]["janus_hpke_sealer_create"]["params"])["out"] == \
        "*mut *mut janus_hpke_sealer"
    assert "pub struct janus_hpke_sealer { _p: [u8; 0] }" in F.gen_rust()
    # and the block a maintainer copies from INTEGRATION.md
    block = F.parse_rust(F.integration_block())
    for f in SEAL_FUNCS:
        assert block["funcs"][f] == r["funcs"][f], f
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    assert set(SEAL_FUNCS) <= set(J.HPKE_EXPORTED_SYMBOLS)
    assert G.SEAL_KEY_ERROR == r["consts"]["JANUS_HPKE_SEAL_KEY_ERROR"]
    assert G.SEAL_LENGTH_ERROR == r["consts"]["JANUS_HPKE_SEAL_LENGTH_ERROR"]


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library fails the test."""
    from janus_amd import hpke as G
    from janus_amd import prio3 as J

    def boom(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(J, "load_library", boom)
    monkeypatch.setattr(G, "load_library", boom)
    monkeypatch.setattr(G, "_lib", boom)


def test_sealer_refuses_mismatched_shapes_before_any_library_call(no_library):
    from janus_amd import hpke as G
    s = G.HpkeSealer(bytes(32))
    n = 4
    task = bytes(32)
    sk = np.zeros((n, 32), np.uint8)
    ids = np.zeros((n, 16), np.uint8)
    t = np.zeros(n, np.uint64)
    pub = np.zeros((n, 32), np.uint8)
    hs = np.zeros((n, 48), np.uint8)
    bad = [
        (task[:31], sk, ids, t, pub, hs),             # task ID
        (task, sk[:, :31], ids, t, pub, hs),          # key length
        (task, sk[:3], ids, t, pub, hs),              # one key short
        (task, sk, ids[:, :15], t, pub, hs),          # report IDs
        (task, sk, ids, t[:3], pub, hs),              # times
        (task, sk, ids, t, pub[:3], hs),              # public shares: rows
        (task, sk, ids, t, np.zeros((n, 16), np.uint8), hs),  # public shares: 16 bytes
        (task, sk, ids, t, pub, hs[:3]),              # helper shares
        (task, sk, ids, t, pub, np.zeros(n, np.uint8)),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            s.seal_input_shares(*args)
    with pytest.raises(ValueError):
        s.seal_input_shares(task, sk, ids, t, pub, hs, ct_stride=64)   # < 6 + 48 + 16
    with pytest.raises(ValueError):
        s.seal_input_shares(task, sk, ids, t, pub, hs, ct_stride=88)   # not a multiple of 16
    with pytest.raises(ValueError):
        s.seal([bytes(32)] * 2, [b"a"] * 3, [b""] * 3)
    with pytest.raises(ValueError):
        s.seal([bytes(31)], [b"a"], [b""])
    with pytest.raises(ValueError):
        s.seal([bytes(32)], [b"a"], [b"", b""])
    with pytest.raises(ValueError):
        s.seal(np.zeros((2, 31), np.uint8), [b"a"] * 2, [b""] * 2)


def test_sealer_device_form_refuses_mismatched_shapes(no_library):
    import torch
    from janus_amd import hpke as G
    s = G.HpkeSealer(bytes(32))
    n = 4
    Z = lambda *shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype)  # noqa: E731
    good = dict(task_id=bytes(32), sk_e=Z(n, 32), report_ids=Z(n, 16),
                times=Z(n, dtype=torch.int64), public_shares=Z(n, 32), helper_shares=Z(n, 48),
                enc=Z(n, 32), ct=Z(n, 80), ct_len=Z(n, dtype=torch.int32), status=Z(n))
    for key, val in [("sk_e", Z(n, 31)), ("report_ids", Z(n + 1, 16)), ("times", Z(n - 1)),
                     ("public_shares", Z(n, 48)), ("helper_shares", Z(n - 1, 48)),
                     ("enc", Z(n, 65)), ("ct", Z(n, 64)), ("ct", Z(n, 72)), ("ct", Z(n - 1, 80)),
                     ("ct_len", Z(n - 1, dtype=torch.int32)), ("status", Z(n + 1)),
                     ("times", Z(n, dtype=torch.int32)), ("ct_len", Z(n, dtype=torch.int64)),
                     ("task_id", bytes(16))]:
        with pytest.raises(ValueError) as e:
            s.seal_input_shares_device(**{**good, key: val})
        assert "GPU" not in str(e.value), key
    with pytest.raises(ValueError, match="on the sealer's GPU"):  # every shape right, host tensors
        s.seal_input_shares_device(**good)


def test_generate_sealed_reports_refuses_mismatched_shapes(no_library):
    import torch
    from janus_amd import hpke as G
    from janus_amd import prio3 as J
    eng = types.SimpleNamespace(device=0, sz=types.SimpleNamespace(public_share_len=32,
                                                                   helper_share_len=48))
    gen = J.HelperEngine.generate_sealed_reports_device
    s = G.HpkeSealer(bytes(32))
    n = 8
    times = torch.zeros(n, dtype=torch.int64)
    sk = torch.zeros((n, 32), dtype=torch.uint8)
    with pytest.raises(ValueError):
        gen(eng, s, bytes(31), n, times, sk)
    with pytest.raises(ValueError):
        gen(eng, s, bytes(32), n, times[:7], sk)
    with pytest.raises(ValueError):
        gen(eng, s, bytes(32), n, times, sk[:, :16])
    with pytest.raises(ValueError):
        gen(eng, s, bytes(32), n + 1, times, sk)
    with pytest.raises(ValueError):
        gen(eng, G.HpkeSealer(bytes(32), device=1), bytes(32), n, times, sk)
