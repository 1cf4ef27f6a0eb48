"""Generates tests/golden/launch_table.json: the kernels one prepare call launches, for every
instance of tests/conftest.py CONFIGS (plus one FPVec and one multiproof instance) crossed with
the entry points and the options that change the chain.  Needs a GPU; every call is also checked
against the CPU restatement (tests/test_gpu_launch_table.py run_row), so a table is only ever
recorded from a build that computes the right bytes.

The table records what the build does, not what it should do: regenerate it only with a change
that means to alter a launch, and review the diff.

    python tests/golden/gen_launch_table.py [output path]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.conftest import CONFIGS  # noqa: E402
from tests import test_gpu_launch_table as T  # noqa: E402

N = 65         # one 64-report wave plus one report; three 32-report waves of the pair kernel
N_CHUNKS = 600  # with chunks = 2: two 512-column chunks on the side streams
N_JOB = 64     # host-buffer jobs: whole waves, so that the XOF can pull the leader prep shares
FPVEC, MP64 = "fpvec_5x16", "mp64_2x8x20_c7"


def specs():
    rows = []
    add = lambda config, role, entry, n, **options: rows.append(
        dict(config=config, role=role, entry=entry, options=options, n=n))
    for name, cfg in CONFIGS.items():
        hist = cfg["kind"] == "histogram"
        for entry in ("prepare", "prepare_aggregate"):  # fuse_acc applies to the second only
            add(name, "helper", entry, N)
            add(name, "helper", entry, N, force_generic_query=1)
            add(name, "helper", entry, N, force_slow_path=1)
            add(name, "helper", entry, N_CHUNKS, chunks=2)
            if hist:
                add(name, "helper", entry, N, pair_max=0)
                add(name, "helper", entry, N_CHUNKS, chunks=2, pair_max=0)
        if hist:
            add(name, "helper", "prepare_aggregate", N, fuse_acc=0)
            add(name, "helper", "prepare_aggregate", N, fuse_acc=0, pair_max=0)
        add(name, "leader", "leader_prepare_init", N)
        add(name, "leader", "leader_prepare_init", N, leader_fast=0)
        add(name, "leader", "leader_prepare_init", N, force_slow_path=1)
        if hist:
            add(name, "leader", "leader_prepare_init", N, leader_fuse_acc=0)
    for name in (FPVEC, MP64):
        add(name, "helper", "prepare", N)
        add(name, "helper", "prepare", N, force_generic_query=1)
        add(name, "helper", "prepare", N, force_slow_path=1)
        add(name, "helper", "prepare_aggregate", N)
        add(name, "leader", "leader_prepare_init", N)
    add(FPVEC, "helper", "prepare", N_CHUNKS, fp_sub_bytes=1)  # 256-column sub-batches
    add(FPVEC, "leader", "leader_prepare_init", N_CHUNKS, fp_sub_bytes=1)
    # the executor's groups: an instance whose XOF pulls the leader prep shares, one whose chain
    # takes them from the copy launch, and the leader's staging on both kinds of chain
    add("hist_256_c16", "helper", "prepare_aggregate_batch", N_JOB)
    add("hist_256_c16", "helper", "prepare_aggregate_batch", N_JOB, pair_max=0)
    add("sumvec_8x10_c9", "helper", "prepare_aggregate_batch", N_JOB)
    add("hist_256_c16", "leader", "leader_prepare_init_batch", N)
    add("sum32", "leader", "leader_prepare_init_batch", N)
    return rows


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.TABLE
    rows = specs()
    for i, row in enumerate(rows):
        row["launches"] = T.run_row(row)
        print(f"{i + 1}/{len(rows)} {T.row_id(row)}: {row['launches']}", flush=True)
    seen = {name for row in rows for name, count in row["launches"] if count}
    missing = set(T.KERNEL_NAMES) - seen
    assert missing == T.UNREACHABLE, f"no row launches {sorted(missing - T.UNREACHABLE)}"
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows -> {out}")


if __name__ == "__main__":
    main()
