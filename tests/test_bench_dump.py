"""bench.py --dump-outputs on host tensors: a batch above DUMP_SAMPLE keeps a fixed seeded sample
of the per-report outputs (the same reports every time) and the per-batch outputs whole."""
import os

import numpy as np


def test_dump_outputs_samples_large_batches(tmp_path):
    import torch
    import bench
    n = bench.DUMP_SAMPLE + 4099
    g = torch.Generator().manual_seed(7)
    msgs = torch.randint(0, 256, (n, 16), generator=g, dtype=torch.uint8)
    status = torch.randint(0, 4, (n,), generator=g, dtype=torch.uint8)
    agg = torch.randint(0, 256, (1, 4096), generator=g, dtype=torch.uint8)
    cnt = torch.tensor([n - 5], dtype=torch.int64)
    cks = torch.randint(0, 256, (1, 32), generator=g, dtype=torch.uint8)
    ivs = torch.tensor([[1_700_000_000, 3600]], dtype=torch.int64)
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        bench.dump_outputs(d, n, msgs, status, agg, cnt, cks, ivs)
    a, b = ({f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))} for d in dirs)
    assert sorted(a) == ["aggregate_share", "checksum", "count", "interval", "prep_msgs",
                         "sample_index", "status"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a[k], b[k])
    idx = a["sample_index"].astype(np.int64)
    assert idx.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(idx) > 0) and idx[-1] < n
    np.testing.assert_array_equal(a["prep_msgs"], msgs.numpy()[idx])
    np.testing.assert_array_equal(a["status"], status.numpy()[idx])
    np.testing.assert_array_equal(a["aggregate_share"], agg.numpy())
    np.testing.assert_array_equal(a["count"], cnt.numpy())
    np.testing.assert_array_equal(a["checksum"], cks.numpy())
    np.testing.assert_array_equal(a["interval"], ivs.numpy())
    # the headline's 1 Mi reports: 65,536 sampled rows of 16 + 1 + 1 values, far below 64 MB
    assert sum(v.nbytes for v in a.values()) < 8 << 20
