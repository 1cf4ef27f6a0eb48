"""Rates of the leader's DAP marshaling on the device against the helper's, in one run.

  python tools/leader_codec_rate.py [--out profiles/leader_codec_rate.json] [--n 500 262144]

Histogram(256,16)-shaped records (32-byte public share, 32-byte enc, 70-byte HPKE payload in an
80-byte row, 560-byte prepare share, 16-byte prepare message).  Each line is the median of 15
launches after 3 warm-ups, timed with HIP events on the stream the calls run on, buffers
allocated beforehand:

  req_encode      janus_dap_agg_init_req_encode_device          (leader; this direction is new)
  req_unpack      janus_dap_agg_init_unpack_device, same body   (helper; the comparison target)
  req_copy        device-to-device copy of the request body's bytes
  resp_encode     janus_dap_agg_job_resp_encode_device          (helper)
  resp_unpack     janus_dap_agg_job_resp_unpack_device          (leader), on a body without
                  rejects and on one with about 5 % Reject records
  resp_copy       device-to-device copy of the response body's bytes

bytes/s is the body's length over the median time.  The encode's target is half the bytes/s of
req_unpack at n = 262,144 (both move the same fields; the encode looks its offsets up)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PSL, ENC, CT_LEN, STRIDE, PS, PML = 32, 32, 70, 80, 560, 16
WARMUP, REPS = 3, 15


def timed(fn, stream):
    import torch
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def run(n, dev):
    import torch
    from janus_amd import dap as J
    from janus_amd.prio3 import _tptr
    L = J._lib()
    g = torch.Generator(device=dev).manual_seed(n)
    rnd = lambda *s: torch.randint(0, 256, s, generator=g, device=dev, dtype=torch.uint8)  # noqa: E731
    ids, pub, enc, ct, ps = rnd(n, 16), rnd(n, PSL), rnd(n, ENC), rnd(n, STRIDE), rnd(n, PS)
    times = torch.full((n,), 1_700_000_000, dtype=torch.int64, device=dev)
    cfg = torch.ones(n, dtype=torch.uint8, device=dev)
    cl = torch.full((n,), CT_LEN, dtype=torch.int32, device=dev)
    lst = torch.zeros(n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream or None)
    u8 = dict(dtype=torch.uint8, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    rows = {}

    def line(name, fn, nbytes):
        med, best = timed(fn, stream)
        rows[name] = dict(median_us=round(med * 1e3, 2), min_us=round(best * 1e3, 2), bytes=nbytes,
                          GB_per_s=round(nbytes / (med * 1e-3) / 1e9, 2))

    # ---- request ----
    cap = L.janus_dap_agg_init_req_max_len(n, 0, 1, PSL, ENC, STRIDE, PS)
    out = torch.zeros(cap, **u8)
    out_len = torch.zeros(1, dtype=torch.int64, device=dev)
    index, ninc, err = torch.zeros(n, **i32), torch.zeros(1, **i32), torch.zeros(2, **i32)
    scratch = torch.zeros((n + 1) // 2 + 2 * (n // 256 + 2), dtype=torch.int64, device=dev)

    def req_encode():
        rc = L.janus_dap_agg_init_req_encode_device(
            n, None, 0, 1, None, _tptr(ids), _tptr(times), _tptr(pub), PSL, _tptr(cfg), _tptr(enc),
            ENC, _tptr(ct), _tptr(cl), STRIDE, _tptr(ps), PS, _tptr(lst), _tptr(out),
            _tptr(out_len), _tptr(index), _tptr(ninc), _tptr(err), _tptr(scratch), sp)
        assert rc == 0

    req_encode()
    torch.cuda.synchronize(dev)
    blen = int(out_len[0])
    assert int(ninc[0]) == n and not err.any()
    body = out[:blen].cpu().numpy().tobytes()
    lay = J.scan(body, PSL, ENC, PS)
    assert lay.uniform and lay.n == n
    line("req_encode", req_encode, blen)
    o = dict(ids=torch.empty((n, 16), **u8), times=torch.empty(n, dtype=torch.int64, device=dev),
             pub=torch.empty((n, PSL), **u8), cfg=torch.empty(n, **u8),
             enc=torch.empty((n, ENC), **u8), ct=torch.zeros((n, STRIDE), **u8),
             cl=torch.empty(n, **i32), ps=torch.empty((n, PS), **u8), ms=torch.empty(n, **u8),
             mism=torch.zeros(1, **i32))

    def req_unpack():
        rc = L.janus_dap_agg_init_unpack_device(
            C.byref(lay), _tptr(out), _tptr(o["ids"]), _tptr(o["times"]), _tptr(o["pub"]),
            _tptr(o["cfg"]), _tptr(o["enc"]), _tptr(o["ct"]), _tptr(o["cl"]), STRIDE,
            _tptr(o["ps"]), _tptr(o["ms"]), _tptr(o["mism"]), sp)
        assert rc == 0

    line("req_unpack", req_unpack, blen)
    torch.cuda.synchronize(dev)
    assert int(o["mism"][0]) == 0 and torch.equal(o["ps"], ps) and torch.equal(o["ids"], ids)
    assert torch.equal(o["ct"][:, :CT_LEN], ct[:, :CT_LEN]) and torch.equal(o["pub"], pub)
    dst = torch.empty(blen, **u8)
    line("req_copy", lambda: dst.copy_(out[:blen]), blen)

    # ---- response ----
    msgs = rnd(n, PML)
    st = torch.zeros(n, **u8)
    rcap = L.janus_dap_agg_job_resp_max_len(n, PML)
    pm, perr, flags = torch.empty((n, PML), **u8), torch.empty(n, **u8), torch.zeros(1, **i32)
    rscratch = torch.zeros(2 * (n + 2), **i32)
    escratch = torch.zeros(n // 256 + 2, **i32)
    for tag, frac in (("", 0.0), ("_5pct_rejects", 0.05)):
        pe = torch.where(torch.rand(n, generator=g, device=dev) < frac,
                         torch.full((n,), 4, **u8), torch.full((n,), 0xFF, **u8))
        resp = torch.zeros(rcap, **u8)
        rlen_t = torch.zeros(1, dtype=torch.int64, device=dev)

        def resp_encode():
            rc = L.janus_dap_agg_job_resp_encode_device(n, _tptr(ids), _tptr(pe), _tptr(st),
                                                        _tptr(msgs), PML, _tptr(resp),
                                                        _tptr(rlen_t), _tptr(escratch), sp)
            assert rc == 0

        resp_encode()
        torch.cuda.synchronize(dev)
        rlen = int(rlen_t[0])
        line("resp_encode" + tag, resp_encode, rlen)

        def resp_unpack():
            rc = L.janus_dap_agg_job_resp_unpack_device(
                n, _tptr(index), _tptr(ids), n, _tptr(resp), rlen, PML, _tptr(pm), _tptr(perr),
                _tptr(flags), _tptr(rscratch), sp)
            assert rc == 0

        line("resp_unpack" + tag, resp_unpack, rlen)
        torch.cuda.synchronize(dev)
        assert int(flags[0]) == 0 and torch.equal(perr, pe)
        assert torch.equal(pm[pe == 0xFF], msgs[pe == 0xFF]) and not pm[pe != 0xFF].any()
        rows["resp_unpack" + tag]["reject_records"] = int((pe != 0xFF).sum())
        rdst = torch.empty(rlen, **u8)
        line("resp_copy" + tag, lambda: rdst.copy_(resp[:rlen]), rlen)
    rows["req_encode_over_req_unpack"] = round(rows["req_encode"]["GB_per_s"] /
                                               rows["req_unpack"]["GB_per_s"], 3)
    return rows


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leader_codec_rate.json"))
    ap.add_argument("--n", type=int, nargs="+", default=[500, 262144])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = dict(what="median of %d launches after %d warm-ups, HIP events; bytes/s = body bytes / "
                    "median time; Histogram(256,16)-shaped records" % (REPS, WARMUP),
               device=torch.cuda.get_device_name(0),
               record=dict(public_share=PSL, enc=ENC, ct_len=CT_LEN, ct_stride=STRIDE,
                           prep_share=PS, prep_msg=PML),
               target="req_encode bytes/s >= 0.5 x req_unpack bytes/s at n = 262144 (same run)",
               sizes={str(n): run(n, dev) for n in a.n})
    big = res["sizes"].get("262144")
    if big:
        res["target_met"] = big["req_encode_over_req_unpack"] >= 0.5
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
