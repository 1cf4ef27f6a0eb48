#!/usr/bin/env python3
"""Find a helper measurement-share seed of Prio3SumVecField64MultiproofHmacSha256Aes128 whose
expansion meets a rejection: one of the 8-byte candidates of

    XofHmacSha256Aes128(seed, dst(algorithm 0xFFFF1003, usage 1), [1])

that expand_into_vec reads for the meas_len = bits * length elements is >= the Field64 modulus
(probability ~2^-32 per candidate), so the sampler discards it and every later element moves up
one candidate.  tests/golden/client_reject_mp64.json records one such seed; CPU only (hashlib's
HMAC and the restatement's AES-CTR keystream, oracle.hpke.aes128_ctr64_keystream).

    python tools/find_reject_mp64.py --bits 32 --length 64            # search from counter 0
    python tools/find_reject_mp64.py --bits 32 --length 64 --seed HEX # check one seed

Search seeds are SHA-256("janus-amd find_reject_mp64" || counter as 8 bytes LE).  Prints the
seed, the index of its first candidate >= p and the candidate, or exits 1 if there is none."""
import argparse
import hashlib
import hmac
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

P64 = 2**64 - 2**32 + 1
ALGO = 0xFFFF1003
USAGE_MEAS = 1


def dst(usage: int) -> bytes:
    return bytes([8, 0]) + ALGO.to_bytes(4, "big") + usage.to_bytes(2, "big")


def first_reject(seed: bytes, meas_len: int):
    """(index, candidate) of the first candidate >= p among those the expansion of meas_len
    elements reads, or None."""
    from oracle.hpke import aes128_ctr64_keystream
    d = dst(USAGE_MEAS)
    tag = hmac.new(seed, bytes([len(d)]) + d + b"\x01", hashlib.sha256).digest()
    # without a rejection the expansion reads exactly meas_len candidates; the first rejection,
    # if any, is therefore among them
    ks = aes128_ctr64_keystream(tag[:16], tag[16:], 8 * meas_len + (-8 * meas_len) % 16)
    c = np.frombuffer(ks, "<u8")[:meas_len]
    hit = np.nonzero(c >= np.uint64(P64))[0]
    return (int(hit[0]), int(c[hit[0]])) if len(hit) else None


def search_seed(counter: int) -> bytes:
    return hashlib.sha256(b"janus-amd find_reject_mp64" + counter.to_bytes(8, "little")).digest()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--bits", type=int, default=32)
    ap.add_argument("--length", type=int, default=64)
    ap.add_argument("--seed", help="check this 32-byte seed (hex) instead of searching")
    ap.add_argument("--start", type=int, default=0, help="first search counter")
    ap.add_argument("--max-seeds", type=int, default=1 << 26)
    a = ap.parse_args()
    meas_len = a.bits * a.length
    if a.seed:
        seed = bytes.fromhex(a.seed)
        if len(seed) != 32:
            ap.error("the seed is 32 bytes")
        hit = first_reject(seed, meas_len)
        if hit is None:
            print(f"{seed.hex()} no candidate >= p in {meas_len}")
            return 1
        print(f"{seed.hex()} index={hit[0]} candidate={hit[1]:016x}")
        return 0
    for k in range(a.start, a.start + a.max_seeds):
        seed = search_seed(k)
        hit = first_reject(seed, meas_len)
        if hit is not None:
            print(f"{seed.hex()} index={hit[0]} candidate={hit[1]:016x} counter={k}")
            return 0
    print(f"none in {a.max_seeds} seeds from counter {a.start}")
    return 1


if __name__ == "__main__":
    sys.exit(main())
