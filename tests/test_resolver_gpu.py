"""The consumer side on an MI355X host: the `gpu` block a Resolver hands out
comes from real KFD topology, through a registrar gated on the real liveness
check, and the host leaves the view (and DNS) when that registrar stops."""
import json
import socket
import struct

import pytest

import registrar_amd as ra
from registrar_amd.binder_lite import BinderLite, _encode_name
from conftest import orch_config, wait_for


def a_records(addr, name):
    q = struct.pack(">HHHHHH", 0x1234, 0x0100, 1, 0, 0, 0) + _encode_name(name) + struct.pack(">HH", 1, 1)
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        s.settimeout(5)
        s.sendto(q, addr)
        buf = s.recvfrom(4096)[0]
    finally:
        s.close()
    an = struct.unpack(">H", buf[6:8])[0]
    off = 12 + len(_encode_name(name)) + 4
    out = []
    for _ in range(an):
        rdlen = struct.unpack(">H", buf[off + 10:off + 12])[0]
        out.append(socket.inet_ntoa(buf[off + 12:off + 12 + rdlen]))
        off += 12 + rdlen
    return sorted(out)


@pytest.mark.gpu
def test_resolver_sees_the_gpu_gated_host_and_prefers_the_local_one(ensemble, client):
    domain = "gpu0.resolver.test"
    registration = {
        "domain": domain,
        "type": "host",
        "adminIp": "127.0.0.1",
        "hostname": "g0",
        "settleMs": 0,
        "service": {"type": "service", "service": {"srvce": "_infer", "proto": "_tcp", "port": 8000}},
    }
    cfg = orch_config(
        ensemble,
        registration,
        gpuIndex=0,
        heartbeatInterval=200,
        healthCheck={"command": "gpu-liveness", "interval": 1000, "timeout": 30000, "threshold": 3},
    )
    servers = [(s["host"], s["port"]) for s in cfg["zookeeper"]["servers"]]
    o = ra.Orchestrator(json.dumps(cfg))
    r = ra.Resolver(servers=servers, session_timeout_ms=5000, local_address="127.0.0.1")
    binder = BinderLite(servers, cache=True)
    r.start()
    binder.start()
    stopped = False
    try:
        o.start()
        assert o.wait_registered(30000)
        # a second host on another node, sorting before g0 by name
        other = {"type": "host", "address": "10.77.0.2",
                 "host": {"address": "10.77.0.2", "gpu": {"index": 3, "xgmiRank": 3, "uuid": "GPU-elsewhere"}}}
        path = ra.domain_to_path(domain)
        assert client.create(path + "/a-remote", json.dumps(other).encode(), True)[0] == ra.ZOK

        snap = r.lookup(domain, 10000, local_first=True)
        assert snap["status"] == "ok"
        assert [(h["name"], h["local"]) for h in snap["hosts"]] == [("g0", True), ("a-remote", False)]
        g0 = snap["hosts"][0]
        assert g0["gpu"]["index"] == 0
        assert g0["gpu"]["xgmiRank"] == ra.xgmi_local_rank(0)
        assert g0["address"] == "127.0.0.1" and g0["ports"] == [8000]
        assert g0["payload"] == ensemble.get(path + "/g0")["data"]
        assert snap["hosts"][1]["gpu"]["xgmiRank"] == 3
        # by name without local_first
        assert [h["name"] for h in r.snapshot(domain)["hosts"]] == ["a-remote", "g0"]
        assert a_records(binder.address, domain) == ["10.77.0.2", "127.0.0.1"]

        o.stop()
        stopped = True
        assert wait_for(lambda: [h["name"] for h in r.snapshot(domain)["hosts"]] == ["a-remote"], timeout=10)
        assert wait_for(lambda: a_records(binder.address, domain) == ["10.77.0.2"], timeout=10)
        assert ("removed", "g0") in [(e["type"], e["name"]) for e in r.poll_events()]
    finally:
        if not stopped:
            o.stop()
        binder.stop()
        r.stop()
