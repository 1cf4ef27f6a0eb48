"""Extracts the two DAP-09 `Report` fixtures of the reference's own codec test
(/root/reference/messages/src/tests/upload.rs, roundtrip_report) -- data only: each Report's field
values (report ID, time, public share, the two HpkeCiphertexts) and the concatenated hex literals
of its encoding.  Run in the build container; writes tests/golden/dap_report_fixtures.json."""
import json
import os
import re

SRC = "/root/reference/messages/src/tests/upload.rs"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dap_report_fixtures.json")


def main():
    src = open(SRC).read()
    start = src.index("fn roundtrip_report()")
    end = src.find("#[test]", start)
    body = src[start:end if end > 0 else len(src)]
    reports = []
    for part in body.split("Report::new(")[1:]:
        rid = [int(x) for x in re.search(r"ReportId::from\(\[([^\]]*)\]\)", part).group(1).split(",")]
        time = int(re.search(r"from_seconds_since_epoch\((\d+)\)", part).group(1))
        meta_end = part.index("from_seconds_since_epoch")
        ct_at = part.index("HpkeCiphertext::new(")
        pub = re.search(r'Vec::from\("([^"]*)"\)', part[meta_end:ct_at])
        cts = []
        for c in part.split("HpkeCiphertext::new(")[1:3]:
            cfg = int(re.search(r"HpkeConfigId::from\((\d+)\)", c).group(1))
            enc, payload = re.findall(r'Vec::from\("([^"]*)"\)', c)[:2]
            cts.append(dict(config_id=cfg, enc=enc.encode().hex(), payload=payload.encode().hex()))
        enc_src = re.sub(r'Vec::from\("[^"]*"\)', "", part)  # field values, not encodings
        hexstr = "".join(re.findall(r'"([0-9A-Fa-f]*)"', enc_src)).lower()
        reports.append(dict(report_id=bytes(rid).hex(), time=time,
                            public_share=pub.group(1).encode().hex() if pub else "",
                            leader=cts[0], helper=cts[1], hex=hexstr))
    fx = dict(reports=reports,
              source="messages/src/tests/upload.rs roundtrip_report (reference codec fixtures)")
    json.dump(fx, open(OUT, "w"), indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
