"""The generated GF(2^255 - 19) and GF(p256) asm, executed by the CPU model of
tests/asm_model.py on loosely reduced operands in [0, 2^256): the full edge x edge cross product
plus random pairs, against Python integers, with every conditional second fold shown to be
taken by some edge operand (and by no random one).  No GPU needed; the device test
(tests/test_gpu_hpke_edges.py) holds model and hardware bit-equal on the same operands."""
import os
import random
import re

import pytest

from tests import asm_model as M
from tests.test_hpke import P256, P256_EDGE

P = M.P25519
# The cross product of P256_EDGE reaches the final fold of every P-256 routine (mul 34, add 6,
# sub 11, sqr 2, mul_small 2 for each k), so the list needed no addition.
P256_SMALL_K = (3, 4, 8)  # the small multiples p256_device.h takes


def _check(routine, name, a, b, k, fn, p):
    bad, folds = [], 0
    for x, y in zip(a, b):
        got, fold = routine.call(x, y, k)
        folds += fold
        if got >= 2**256 or (got - fn(x, y)) % p:
            bad.append((x, y, got))
    assert not bad, (f"{name}: {len(bad)} wrong, first a={bad[0][0]:#x} b={bad[0][1]:#x} "
                     f"got {bad[0][2]:#x}")
    return folds


def test_headers_parse_and_hold_the_expected_routines():
    fe = M.load("fe25519_asm.h")
    assert sorted(fe) == sorted(M.FE_OPS)
    p = M.load("p256_asm.h")
    assert sorted(p) == ["p256_add", "p256_mul", "p256_mul_small", "p256_sqr", "p256_sub"]
    used = {mn for rs in (fe, p) for r in rs.values() for mn, _ in r.insns}
    assert used <= set(M._ISA)
    assert len(M.edge_25519()) == 88


def test_fe25519_asm_matches_python_and_every_second_fold_is_taken():
    a, b, ne = M.operands_25519()
    assert ne == 88 * 88 and len(a) - ne == 4096
    edge = M.edge_25519()
    counts, random_counts = {}, {}
    for op, name in enumerate(M.FE_OPS):
        res = M.model_25519(op)
        fn = M.FE_PY[op]
        bad = [i for i, (got, _) in enumerate(res)
               if got >= 2**256 or (got - fn(a[i], b[i])) % P]
        assert not bad, (f"{name}: {len(bad)} wrong, first a={a[bad[0]]:#x} b={b[bad[0]]:#x} "
                         f"got {res[bad[0]][0]:#x}")
        if name in ("fe_sqr", "fe_mul121665"):  # unary: counted over the edge set itself
            counts[name] = sum(res[i * len(edge)][1] for i in range(len(edge)))
        else:
            counts[name] = sum(f for _, f in res[:ne])
        random_counts[name] = sum(f for _, f in res[ne:])
    print("second folds taken, edge operands:", counts, "random operands:", random_counts)
    assert all(c > 0 for c in counts.values()), f"a second fold is never taken: {counts}"
    assert not any(random_counts.values()), f"random operands take a second fold: {random_counts}"
    # the examples of the fold conditions
    fe = M.load("fe25519_asm.h")
    assert fe["fe_sqr"].call(2**256 - 31)[1] == 1
    assert fe["fe_add"].call(2**256 - 1, 2**256 - 1)[1] == 1
    assert fe["fe_sub"].call(0, 2**256 - 1)[1] == 1
    assert fe["fe_add"].call(2**256 - 1, 2**256 - 38)[1] == 0
    assert fe["fe_sub"].call(0, 1)[1] == 0


def test_p256_asm_matches_python_and_every_second_fold_is_taken():
    p = M.load("p256_asm.h")
    e = P256_EDGE
    rnd = random.Random(256)
    ea, eb = [x for x in e for _ in e], [y for _ in e for y in e]
    ra = [rnd.randrange(2**256) for _ in range(4096)]
    rb = [rnd.randrange(2**256) for _ in range(4096)]
    binary = [("p256_mul", lambda x, y: x * y), ("p256_add", lambda x, y: x + y),
              ("p256_sub", lambda x, y: x - y)]
    counts, random_counts = {}, {}
    for name, fn in binary:
        counts[name] = _check(p[name], name, ea, eb, 0, fn, P256)
        random_counts[name] = _check(p[name], name, ra, rb, 0, fn, P256)
    counts["p256_sqr"] = _check(p["p256_sqr"], "p256_sqr", e, e, 0, lambda x, y: x * x, P256)
    random_counts["p256_sqr"] = _check(p["p256_sqr"], "p256_sqr", ra, ra, 0,
                                       lambda x, y: x * x, P256)
    for k in P256_SMALL_K:
        name = f"p256_mul_small k={k}"
        counts[name] = _check(p["p256_mul_small"], name, e, e, k, lambda x, y: k * x, P256)
        random_counts[name] = _check(p["p256_mul_small"], name, ra, ra, k,
                                     lambda x, y: k * x, P256)
    print("P-256 final folds taken, edge operands:", counts, "random operands:", random_counts)
    assert all(c > 0 for c in counts.values()), f"a final fold is never taken: {counts}"


# ---- the model notices a broken header ---------------------------------------------------------
def _mutated(tmp_path, edit):
    src = open(os.path.join(M.CSRC, "fe25519_asm.h")).read()
    out = edit(src)
    assert out != src
    path = tmp_path / "fe25519_asm.h"
    path.write_text(out)
    return str(path)


def _fails(path):
    """Why the model test's checks reject the header at `path`, or None if they pass."""
    try:
        fe = M.parse_header(path)
        e = M.edge_25519()
        for op, name in enumerate(M.FE_OPS):
            for x in e:
                for y in (e if name in ("fe_mul", "fe_add", "fe_sub") else [0]):
                    got, _ = fe[name].call(x, y)
                    if got >= 2**256 or (got - M.FE_PY[op](x, y)) % P:
                        return f"{name} a={x:#x} b={y:#x}"
    except M.AsmModelError as ex:
        return str(ex)
    return None


def _body(src, name):
    m = re.search(r"DEV fe " + name + r"\(.*?\n\}", src, re.S)
    return m.start(), m.end()


def test_model_rejects_fe_add_without_its_second_fold(tmp_path):
    def edit(src):
        s, e = _body(src, "fe_add")
        body = src[s:e]
        tail = ('      "v_cndmask_b32_e64 %8, 0, 38, vcc\\n\\t"\n'
                '      "v_add_u32 %0, %0, %8\\n\\t"\n')
        assert body.count(tail) == 1
        return src[:s] + body.replace(tail, "") + src[e:]
    why = _fails(_mutated(tmp_path, edit))
    assert why and why.startswith("fe_add"), why


def test_model_rejects_swapped_subbrev_operands(tmp_path):
    def edit(src):
        return src.replace('"v_subbrev_co_u32 %3, vcc, 0, %3, vcc',
                           '"v_subbrev_co_u32 %3, vcc, %3, 0, vcc', 1)
    why = _fails(_mutated(tmp_path, edit))
    assert why and why.startswith("fe_sub"), why


@pytest.mark.parametrize("reg", ["v56", "vcc"])
def test_model_rejects_a_register_missing_from_the_clobbers(tmp_path, reg):
    def edit(src):
        s, e = _body(src, "fe_mul")
        body = src[s:e]
        drop = f'"{reg}", '
        assert body.count(drop) == 1
        return src[:s] + body.replace(drop, "") + src[e:]
    why = _fails(_mutated(tmp_path, edit))
    assert why and "clobber" in why, why


def test_model_rejects_unknown_mnemonic_and_late_clobber_output(tmp_path):
    why = _fails(_mutated(tmp_path, lambda s: s.replace('"v_add_u32 %0', '"v_add_nc_u32 %0', 1)))
    assert why and "unknown mnemonic" in why, why
    why = _fails(_mutated(tmp_path, lambda s: s.replace('"=&v"(r.v[3])', '"=v"(r.v[3])', 1)))
    assert why and "early-clobber" in why, why


def test_model_rejects_a_scratch_register_read_before_it_is_written(tmp_path):
    # fe_sqr clears v[40:41] first; without that, v41 is read as it came in
    line = '      "v_mov_b64 v[40:41], 0\\n\\t"\n'
    why = _fails(_mutated(tmp_path, lambda s: s.replace(line, "", 1)))
    assert why and "initial register contents" in why, why
