#!/usr/bin/env python3
"""Query latency of binder_lite, direct against cached (docs/perf_resolver.md).

One in-process ensemble, one domain of N host records, one direct and one
cached binder over it. For each binder: Q UDP A queries (answer truncated to
512 bytes) and Q TCP A queries (all N records), one at a time; prints one JSON
line with the medians and the ZooKeeper reads each series cost.

    python tools/binder_latency.py [--records 1000] [--queries 200]
"""
import argparse
import json
import os
import socket
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import registrar_amd as ra  # noqa: E402
from registrar_amd.binder_lite import BinderLite, _encode_name  # noqa: E402


def query(name, txid):
    return struct.pack(">HHHHHH", txid, 0x0100, 1, 0, 0, 0) + _encode_name(name) + struct.pack(">HH", 1, 1)


def udp_once(addr, name):
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    s.settimeout(30)
    t0 = time.perf_counter()
    s.sendto(query(name, 0x1234), addr)
    buf = s.recvfrom(4096)[0]
    dt = time.perf_counter() - t0
    s.close()
    return dt, struct.unpack(">H", buf[6:8])[0]


def tcp_once(addr, name):
    q = query(name, 0x4321)
    t0 = time.perf_counter()
    s = socket.create_connection(addr, timeout=30)
    s.sendall(struct.pack(">H", len(q)) + q)
    need, buf = 2, b""
    while len(buf) < need:
        chunk = s.recv(65536)
        if not chunk:
            break
        buf += chunk
        if len(buf) >= 2:
            need = 2 + struct.unpack(">H", buf[:2])[0]
    dt = time.perf_counter() - t0
    s.close()
    return dt, struct.unpack(">H", buf[8:10])[0]


def reads(ens):
    c = ens.counters()
    return sum(c.get(k, 0) for k in ("getData", "getChildren", "exists"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=200)
    args = ap.parse_args()

    ens = ra.Ensemble(servers=1, tick_ms=100)
    ens.start()
    servers = [(hp.rsplit(":", 1)[0], int(hp.rsplit(":", 1)[1])) for hp in ens.connect_string().split(",")]
    client = ra.ZkClient(servers=servers, session_timeout_ms=30000)
    client.start()
    assert client.wait_connected(10000)
    domain = "big.latency.test"
    path = ra.domain_to_path(domain)
    assert client.mkdirp(path) == ra.ZOK
    for i in range(args.records):
        rec = {"type": "host", "address": "10.1.%d.%d" % (i // 250, i % 250)}
        assert client.create("%s/h%05d" % (path, i), json.dumps(rec).encode(), True)[0] == ra.ZOK

    out = {"records": args.records, "queries": args.queries}
    for mode, cache in (("direct", False), ("cached", True)):
        b = BinderLite(servers, cache=cache)
        b.start()
        try:
            for label, once in (("udp", udp_once), ("tcp", tcp_once)):
                _, an = once(b.address, domain)  # the first query (builds the cached view)
                before = reads(ens)
                times = []
                for _ in range(args.queries):
                    dt, got = once(b.address, domain)
                    assert got == an
                    times.append(dt * 1000.0)
                times.sort()
                out["%s_%s" % (mode, label)] = {
                    "answers": an,
                    "median_ms": round(statistics.median(times), 3),
                    "p10_ms": round(times[len(times) // 10], 3),
                    "p90_ms": round(times[len(times) * 9 // 10], 3),
                    "zk_reads_per_query": (reads(ens) - before) / float(args.queries),
                }
        finally:
            b.stop()
    client.close()
    ens.stop()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
