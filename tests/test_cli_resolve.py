"""`python -m registrar_amd resolve` and `binder --cache`: the command line over
the Resolver. These tests are about the commands, so each starts one."""
import json
import signal
import socket
import struct
import subprocess
import sys

import registrar_amd as ra
from conftest import REPO_ROOT

GPU = {"index": 3, "xgmiRank": 5, "uuid": "GPU-test"}


def register(client, domain, hostname, address, **extra):
    reg = {"domain": domain, "type": "host", "adminIp": address, "hostname": hostname, "settleMs": 0}
    reg.update(extra)
    rc, err, _ = ra.register_node(client, json.dumps(reg))
    assert rc == ra.ZOK, err


def cli(*args):
    return [sys.executable, "-m", "registrar_amd"] + list(args)


def test_resolve_prints_one_json_line(ensemble, client):
    register(client, "cli.resolve.test", "r0", "10.7.0.1", gpu=GPU)
    register(client, "cli.resolve.test", "r1", "10.7.0.2")
    r = subprocess.run(cli("resolve", "--servers", ensemble.connect_string(), "cli.resolve.test",
                           "--local-address", "10.7.0.2"),
                       capture_output=True, text=True, timeout=60, cwd=REPO_ROOT)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["domain"] == "cli.resolve.test" and out["status"] == "ok" and out["stale"] is False
    assert [(h["name"], h["address"], h["local"]) for h in out["hosts"]] == [
        ("r1", "10.7.0.2", True), ("r0", "10.7.0.1", False)]
    assert out["hosts"][1]["gpu"] == GPU


def test_resolve_absent_domain_exits_one(ensemble):
    r = subprocess.run(cli("resolve", "--servers", ensemble.connect_string(), "nosuch.resolve.test"),
                       capture_output=True, text=True, timeout=60, cwd=REPO_ROOT)
    assert r.returncode == 1
    assert json.loads(r.stdout)["status"] == "absent"


def test_resolve_follow_prints_events(ensemble, client):
    register(client, "follow.resolve.test", "f0", "10.7.1.1")
    proc = subprocess.Popen(cli("resolve", "--servers", ensemble.connect_string(), "follow.resolve.test",
                                "--follow"),
                            stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, cwd=REPO_ROOT)
    try:
        first = json.loads(proc.stdout.readline())
        assert [h["name"] for h in first["hosts"]] == ["f0"]
        rec = {"type": "host", "address": "10.7.1.2"}
        assert client.create("/test/resolve/follow/f1", json.dumps(rec).encode(), True)[0] == ra.ZOK
        event = json.loads(proc.stdout.readline())
        assert (event["event"], event["name"]) == ("added", "f1")
        snap = json.loads(proc.stdout.readline())
        assert [h["name"] for h in snap["hosts"]] == ["f0", "f1"]
        assert snap["generation"] == first["generation"] + 1
    finally:
        proc.send_signal(signal.SIGTERM)
        assert proc.wait(timeout=10) == 0


def test_binder_cache_subcommand(ensemble, client):
    register(client, "cli.cached.test", "cb0", "10.7.2.9")
    proc = subprocess.Popen(cli("binder", "--servers", ensemble.connect_string(), "--port", "0", "--cache"),
                            stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, cwd=REPO_ROOT)
    try:
        hello = json.loads(proc.stdout.readline())
        assert hello["cache"] is True
        host, port = hello["dns"].rsplit(":", 1)
        q = struct.pack(">HHHHHH", 0x31ca, 0x0100, 1, 0, 0, 0)
        for label in "cli.cached.test".split("."):
            q += bytes([len(label)]) + label.encode()
        q += b"\x00" + struct.pack(">HH", 1, 1)
        s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        s.settimeout(5)
        s.sendto(q, (host, int(port)))
        buf, _ = s.recvfrom(512)
        s.close()
        assert struct.unpack(">H", buf[6:8])[0] == 1
        assert socket.inet_ntoa(buf[-4:]) == "10.7.2.9"
    finally:
        proc.send_signal(signal.SIGTERM)
        assert proc.wait(timeout=10) == 0
