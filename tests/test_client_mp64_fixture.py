"""CPU checks for the device client of Prio3SumVecField64MultiproofHmacSha256Aes128: the
rejection fixture tests/golden/client_reject_mp64.json (found by tools/find_reject_mp64.py)
against the Python restatement's XOF, and the instance's shard randomness length."""
import ctypes as C
import json
import os

from tests.conftest import ROOT

P64 = 2**64 - 2**32 + 1


def test_fixture_rejects_at_the_recorded_index():
    from oracle.prio3_py import Field64, Prio3, Prio3Type, XofHmacSha256Aes128
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "client_reject_mp64.json")))
    v = Prio3(Prio3Type("sumvec_f64_mp", bits=fx["bits"], length=fx["length"],
                        chunk_length=fx["chunk_length"], num_proofs=fx["num_proofs"]))
    M, idx = v.t.meas_len, fx["element_index"]
    assert M == fx["bits"] * fx["length"] and idx < M
    rand = bytes.fromhex(fx["rand"])
    seed = bytes.fromhex(fx["seed"])
    assert len(rand) == 160 and rand[:32] == seed and len(bytes.fromhex(fx["nonce"])) == 16
    assert len(fx["measurement"]) == fx["length"]
    assert all(0 <= x < 1 << fx["bits"] for x in fx["measurement"])
    raw = XofHmacSha256Aes128(seed, v.dst("meas"), b"\x01").next(8 * (M + 8))
    cand = [int.from_bytes(raw[8 * k:8 * k + 8], "little") for k in range(M + 8)]
    assert cand[idx] >= P64 and all(x < P64 for x in cand[:idx])
    # the expansion skips it: elements before it are their candidates, those after it the next ones
    share = v.helper_meas(1, seed)
    assert len(share) == M and share == [x for x in cand if x < Field64.p][:M]
    assert share[:idx] == cand[:idx] and share[idx] == cand[idx + 1]
    # the tool's own check agrees
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "find_reject_mp64", os.path.join(ROOT, "tools", "find_reject_mp64.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.first_reject(seed, M) == (idx, cand[idx])


def test_rand_len_is_five_32_byte_seeds():
    from janus_amd import prio3 as J
    for shape in ((2, 16, 15, 16), (3, 4, 9, 4)):
        vdaf = J.Prio3SumVecField64MultiproofHmacSha256Aes128(*shape)
        assert J.load_library().prio3_client_rand_len(C.byref(vdaf.params())) == 160
