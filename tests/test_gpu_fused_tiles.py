"""The fused accumulate's tile reduction through LDS (tile_stage / tile_halfsum, xofd_body).

Two layers: the self-test op feeds chosen Field128 values to the reduction of one wave (real
shares are XOF output and never present all-ones limbs), and the engine runs Histogram instances
whose measurement lengths leave every tile residue, with ragged last waves, segment runs that
split waves, out-of-range lanes, the accept mask and the slow path, against the CPU restatement.
"""
import numpy as np
import pytest

from tests.conftest import CONFIGS
from tests.test_gpu_parity import VK, _engine, _oracle

pytestmark = pytest.mark.gpu

P128 = 2**128 - 28 * 2**64 + 1
T = 8  # elements per tile


def _enc(vals):
    """[8][64] Python ints -> uint8 [8, 64, 16] little-endian."""
    return np.frombuffer(b"".join(int(v).to_bytes(16, "little") for row in vals for v in row),
                         np.uint8).reshape(T, 64, 16)


def _check_tile(vals, n_elems=T):
    from janus_amd import prio3 as J
    out = J.selftest_tile(_enc(vals), n_elems)
    assert out.shape == (n_elems, 8)
    for s in range(n_elems):
        slots = [int(x) for x in out[s]]
        assert all(x < 2**22 for x in slots), (s, slots)
        assert sum(x << (16 * h) for h, x in enumerate(slots)) == sum(vals[s]), s


def _rand128(rng):
    return int.from_bytes(rng.bytes(16), "little")


@pytest.mark.parametrize("value", [2**128 - 1, P128 - 1, 0], ids=["all_ones", "p_minus_1", "zero"])
def test_tile_constant_values(value):
    _check_tile([[value] * 64 for _ in range(T)])


@pytest.mark.parametrize("lane", [0, 7, 8, 31, 32, 63])
def test_tile_one_nonzero_lane(lane):
    rng = np.random.default_rng(100 + lane)
    vals = [[0] * 64 for _ in range(T)]
    for s in range(T):
        vals[s][lane] = _rand128(rng) | 1
    vals[T - 1][lane] = 2**128 - 1
    _check_tile(vals)


def test_tile_alternating_half_limbs():
    a = int.from_bytes(np.array([0xFFFF0000, 0x0000FFFF] * 2, "<u4").tobytes(), "little")
    b = int.from_bytes(np.array([0x0000FFFF, 0xFFFF0000] * 2, "<u4").tobytes(), "little")
    _check_tile([[a if (s + l) & 1 else b for l in range(64)] for s in range(T)])
    _check_tile([[a if s & 1 else b] * 64 for s in range(T)])


def test_tile_random_values():
    rng = np.random.default_rng(7)
    _check_tile([[_rand128(rng) for _ in range(64)] for _ in range(T)])


@pytest.mark.parametrize("n_elems", [1, 5, 7])
def test_tile_partial_with_garbage_in_unused_slots(n_elems):
    rng = np.random.default_rng(n_elems)
    vals = [[_rand128(rng) for _ in range(64)] for _ in range(T)]
    for s in range(n_elems, T):  # staged, but not part of the tile
        vals[s] = [2**128 - 1] * 64
    _check_tile(vals, n_elems)


# Instances and the kernel that carries xofd_body for each.  The tiles follow the pairs of share
# blocks (21 elements: 8 + 8 + 5), so M mod 21 selects the end-of-share path: 4 and 16 end inside
# a tile flushed in place, 9 and 10 leave one or two elements for the tail flush after an even
# block, 17 .. 20 a partial last tile after an odd block.  The timing names do not tell the fused
# instantiation from the unfused one; that the tiles ran shows in the aggregate of the waves that
# fuse (one segment, n a multiple of 64), which only they produce.
INSTANCES = {
    "hist_256_c16": (CONFIGS["hist_256_c16"], "k_prep_h"),  # M mod 21 = 4, M mod 8 = 0
    "hist_100_c10": (CONFIGS["hist_100_c10"], "k_xofd"),    # 16, M mod 8 = 4
    "hist_241_c16": (dict(kind="histogram", length=241, chunk_length=16), "k_prep_h"),  # 10
    "hist_240_c16": (dict(kind="histogram", length=240, chunk_length=16), "k_xofd"),  # 9, P = 16
    "hist_250_c16": (dict(kind="histogram", length=250, chunk_length=16), "k_prep_h"),  # 19
    "hist_500_c8": (CONFIGS["hist_500_c8"], "k_xofd"),      # 17
    # One share block: never enters xofd_body and tests nothing of the tiles.  Kept as the
    # project's M = 2 (mod 8) instance, a non-regression case of the fused aggregate.
    "hist_10_c3": (CONFIGS["hist_10_c3"], "k_jrpart"),
}


def _run(name, n, n_segments, seed, force_slow=False):
    import torch
    cfg, kernel = INSTANCES[name]
    o = _oracle(cfg)
    eng = _engine(cfg)
    eng.set_option("fuse_acc", 1)
    eng.set_option("pair_max", 0)  # the one-lane kernel also below the lane-pair threshold
    eng.set_option("timing", 1)
    if force_slow:
        eng.set_option("force_slow_path", 1)
    d = o.gen_reports(VK, n, seed=seed, n_threads=8)
    rng = np.random.default_rng(seed)
    seg = np.zeros(n, np.uint32)
    if n_segments > 1:  # contiguous runs whose boundaries fall inside waves
        for c in np.sort(rng.choice(np.arange(1, n), n_segments - 1, replace=False)):
            seg[c:] += 1
    accept = (rng.random(n) < 0.9).astype(np.uint8)
    oob = np.zeros(n, bool)
    for w in range((n + 63) // 64):  # a few lanes of every wave carry an out-of-range segment id
        lanes = 64 * w + rng.choice(64, 3, replace=False)
        oob[lanes[lanes < n]] = True
    dev_seg = np.where(oob, n_segments + 5 + (np.arange(n) % 3), seg).astype(np.uint32)
    ref_msgs, ref_status, ref_agg, ref_cnt = o.helper_batch(
        VK, d["nonces"], d["public_shares"], d["helper_shares"], d["leader_prep_shares"],
        segment_ids=np.where(oob, 0, seg).astype(np.uint32),
        accept_mask=np.where(oob, 0, accept).astype(np.uint8), n_segments=n_segments, n_threads=8)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sz = eng.sz
    msgs = torch.zeros((n, max(sz.prep_msg_len, 1)), dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    agg = torch.zeros((n_segments, sz.agg_share_len), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(n_segments, dtype=torch.int64, device=dev)
    pub = t(d["public_shares"]) if sz.public_share_len else None
    eng.prepare_aggregate_device(t(d["nonces"]), pub, t(d["helper_shares"]),
                                 t(d["leader_prep_shares"]), t(dev_seg), n_segments, msgs, status)
    eng.aggregate_finish_device(status, t(accept), agg, cnt)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(status.cpu().numpy(), ref_status)
    np.testing.assert_array_equal(msgs.cpu().numpy()[:, :sz.prep_msg_len], ref_msgs)
    np.testing.assert_array_equal(cnt.cpu().numpy().astype(np.uint64), ref_cnt)
    np.testing.assert_array_equal(agg.cpu().numpy(), ref_agg)
    timing = eng.timing()
    assert timing.get(kernel, (0.0, 0))[1] > 0, timing


@pytest.mark.parametrize("n_segments", [1, 3])
@pytest.mark.parametrize("n", [64, 192, 200])
@pytest.mark.parametrize("name", ["hist_256_c16", "hist_100_c10", "hist_10_c3"])
def test_engine_tile_residues(name, n, n_segments):
    _run(name, n, n_segments, seed=1000 + n + n_segments)


@pytest.mark.parametrize("n,n_segments", [(128, 1), (200, 3)])
@pytest.mark.parametrize("name", ["hist_241_c16", "hist_240_c16", "hist_250_c16", "hist_500_c8"])
def test_engine_end_of_share_tiles(name, n, n_segments):
    """The tail flush after an even block (M mod 21 = 9, 10) and the partial last tile after an
    odd block (17, 19); with one segment and whole waves every wave fuses."""
    _run(name, n, n_segments, seed=2000 + n)


def test_engine_tiles_slow_path():
    """Every report flagged: each wave stages and flushes its tiles, then is un-fused."""
    _run("hist_256_c16", 200, 3, seed=77, force_slow=True)
