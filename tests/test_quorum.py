"""Quorum mode of the synthetic ensemble: below a majority of servers it
serves nobody and expires nobody; when a majority returns, a leader is chosen
and every session gets a fresh timeout.

Every test but the mode-off control builds its ensemble with quorum=True. Raw
sockets use hand-packed jute frames, as tests/test_wire_golden.py does."""
import json
import os
import signal
import socket
import struct
import subprocess
import sys
import time

import pytest

import registrar_amd as ra
from conftest import REPO_ROOT, make_client, orch_config, wait_for


def quorum_ensemble(**kw):
    ens = ra.Ensemble(servers=3, tick_ms=50, min_session_timeout_ms=200, quorum=True, **kw)
    ens.start()
    return ens


@pytest.fixture
def qens():
    ens = quorum_ensemble()
    yield ens
    ens.stop()


def server_addr(ens, idx):
    host, port = ens.connect_string().split(",")[idx].rsplit(":", 1)
    return host, int(port)


def client_to(ens, idx, **kw):
    """A connected ZkClient that knows server idx only."""
    kw.setdefault("session_timeout_ms", 5000)
    c = ra.ZkClient(servers=[server_addr(ens, idx)], **kw)
    c.start()
    assert c.wait_connected(10000)
    return c


def lose_quorum(ens):
    ens.kill_server(1)
    ens.kill_server(2)


def reads_eof(sock, timeout=5.0):
    sock.settimeout(timeout)
    try:
        return sock.recv(1) == b""
    except ConnectionResetError:
        return True


# ---- raw jute frames ----

def send_frame(s, body):
    s.sendall(struct.pack(">i", len(body)) + body)


def recv_frame(s):
    def exactly(n):
        buf = b""
        while len(buf) < n:
            part = s.recv(n - len(buf))
            assert part, "connection closed mid-frame"
            buf += part
        return buf

    return exactly(struct.unpack(">i", exactly(4))[0])


def zk_string(b):
    return struct.pack(">i", len(b)) + b


def raw_session(ens, idx, timeout_ms):
    """Handshake a new session on server idx; returns (socket, session id)."""
    s = socket.create_connection(server_addr(ens, idx), timeout=5)
    # ConnectRequest: protoVersion lastZxid timeout sessionId passwd
    send_frame(s, struct.pack(">iqiq", 0, 0, timeout_ms, 0) + zk_string(b"\x00" * 16))
    resp = recv_frame(s)
    negotiated = struct.unpack(">i", resp[4:8])[0]
    assert negotiated == timeout_ms
    return s, struct.unpack(">q", resp[8:16])[0]


def raw_create_ephemeral(s, path, xid=1):
    req = struct.pack(">ii", xid, 1) + zk_string(path) + zk_string(b"")
    req += struct.pack(">i", 1) + struct.pack(">i", 31) + zk_string(b"world") + zk_string(b"anyone")
    req += struct.pack(">i", 1)  # EPHEMERAL
    send_frame(s, req)
    assert struct.unpack(">iqi", recv_frame(s)[:16])[2] == 0


def registration(domain, hostname, aliases=0):
    return {
        "domain": domain,
        "type": "host",
        "adminIp": "127.0.0.1",
        "hostname": hostname,
        "settleMs": 0,
        "aliases": ["a%03d.%s" % (i, domain) for i in range(aliases)],
    }


# the orchestrator settings of the storm test: a short session, quick
# heartbeats that give up at once when the ensemble is away
STORM = dict(
    heartbeatInterval=100,
    heartbeatFailureFloor=200,
    heartbeat={"retry": {"maxAttempts": 1, "initialDelay": 50, "maxDelay": 50}},
)


def storm_config(ens, reg, **extra):
    cfg = orch_config(ens, reg, **STORM, **extra)
    cfg["zookeeper"]["timeout"] = 1000
    return cfg


# ---- 1. control: mode off ----

def test_mode_off_survivor_keeps_serving(ensemble3):
    ensemble3.kill_server(1)
    ensemble3.kill_server(2)
    assert ensemble3.server_up(0)
    c = client_to(ensemble3, 0)
    rc, _ = c.create("/q1-still-served", b"x", True)
    assert rc == ra.ZOK
    assert ensemble3.get("/q1-still-served")["exists"]
    c.close()


# ---- 2. loss drops everyone and freezes the tree ----

def test_loss_drops_everyone_and_freezes_tree(qens):
    clients = [client_to(qens, i) for i in range(3)]
    for i, c in enumerate(clients):
        rc, _ = c.create("/q2-eph%d" % i, b"", True)
        assert rc == ra.ZOK
    raw = socket.create_connection(server_addr(qens, 0), timeout=5)
    assert qens.has_quorum()
    refused0 = qens.quorum_state()["refused_connects"]

    qens.kill_server(1)
    assert qens.has_quorum() and qens.quorum_state()["losses"] == 0
    qens.kill_server(2)
    z0 = qens.zxid()

    assert reads_eof(raw)
    raw.close()
    assert not qens.has_quorum()
    st = qens.quorum_state()
    assert st["losses"] == 1
    assert st["enabled"] and not st["serving"] and st["leader"] == -1
    assert (st["servers"], st["servers_up"], st["needed"]) == (3, 1, 2)
    # the three clients' connections; the raw one too, unless it was still in
    # the listen queue and got refused at accept instead
    assert st["dropped_connections"] >= 3
    assert qens.server_up(0)  # its listener stays open; it just serves nobody

    rc, _ = clients[0].create("/q2-during-outage", b"", False)
    assert rc != ra.ZOK
    assert not qens.get("/q2-during-outage")["exists"]

    fresh = ra.ZkClient(servers=[server_addr(qens, 0)], session_timeout_ms=5000)
    fresh.start()
    assert not fresh.wait_connected(1000)
    fresh.close()

    time.sleep(0.5)
    assert qens.zxid() == z0
    assert qens.quorum_state()["refused_connects"] > refused0
    for i in range(3):
        assert qens.get("/q2-eph%d" % i)["exists"]
    for c in clients:
        c.close()


# ---- 3. sessions outlive the outage and get a fresh timer ----

def test_session_outlives_outage_and_gets_fresh_timer(qens):
    s, sid = raw_session(qens, 0, 1000)
    raw_create_ephemeral(s, b"/q3-eph")
    s.close()  # no closeSession: the session lives on server-side
    lose_quorum(qens)
    time.sleep(3.0)  # three session timeouts
    assert sid in qens.session_ids()
    assert qens.get("/q3-eph")["exists"]

    t0 = time.monotonic()
    qens.restart_server(1)
    assert wait_for(lambda: not qens.get("/q3-eph")["exists"], timeout=11.0, interval=0.01)
    t1 = time.monotonic()
    print("expired %.3f s after quorum returned" % (t1 - t0))
    assert t1 - t0 >= 1.0
    assert t1 - t0 < 1.0 + 10.0
    assert sid not in qens.session_ids()


# ---- 4. same session across the outage ----

def test_same_session_across_outage(qens):
    c = make_client(qens, session_timeout_ms=1000)
    other = make_client(qens)
    events = []
    watches = []
    sid = c.session_id()
    rc, _ = c.create("/q4-eph", b"mine", True)
    assert rc == ra.ZOK
    rc, _ = other.create("/q4-watched", b"v0", False)
    assert rc == ra.ZOK
    rc, _, _ = c.get("/q4-watched", watch=True)
    assert rc == ra.ZOK
    before = qens.get("/q4-eph")["stat"]

    lose_quorum(qens)
    time.sleep(2.5)
    qens.restart_server(1)

    def back():
        events.extend(c.poll_events())
        return c.state() == "connected"

    assert wait_for(back, timeout=15)
    assert c.session_id() == sid
    after = qens.get("/q4-eph")["stat"]
    assert after["ephemeralOwner"] == sid == before["ephemeralOwner"]
    assert after["czxid"] == before["czxid"]
    # the client answers requests again on the old session
    assert wait_for(lambda: c.exists("/q4-eph")[0] == ra.ZOK, timeout=10)

    assert wait_for(lambda: other.state() == "connected", timeout=15)
    assert wait_for(lambda: other.set("/q4-watched", b"v1") == ra.ZOK, timeout=10)

    def fired():
        watches.extend(c.poll_watches())
        return [w for w in watches if w["path"] == "/q4-watched"]

    assert wait_for(lambda: len(fired()) >= 1, timeout=5)
    time.sleep(0.3)
    assert [w["type"] for w in fired()] == ["changed"]
    events.extend(c.poll_events())
    assert [e for e in events if e["type"] == "session_expired"] == []
    c.close()
    other.close()


# ---- 5. leader loss disconnects the followers' clients ----

def test_leader_loss_disconnects_followers_clients():
    ens = quorum_ensemble(election_ms=300)
    try:
        c = make_client(ens)
        sid = c.session_id()
        assert ens.leader() == 0
        raw = socket.create_connection(server_addr(ens, 1), timeout=5)
        time.sleep(0.05)
        assert ens.kill_leader() == 0
        st = ens.quorum_state()
        assert not st["serving"] and st["leader"] == -1
        assert st["has_quorum"] and ens.has_quorum()
        assert reads_eof(raw)
        raw.close()
        assert wait_for(lambda: ens.quorum_state()["serving"], timeout=0.3 + 5.0)
        assert ens.leader() == 1 and ens.quorum_state()["leader"] == 1
        assert ens.quorum_state()["losses"] == 0
        assert wait_for(lambda: c.state() == "connected", timeout=15)
        assert c.session_id() == sid
        c.close()
    finally:
        ens.stop()


def test_kill_server_of_leader_pauses_like_kill_leader():
    ens = quorum_ensemble(election_ms=300)
    try:
        raw = socket.create_connection(server_addr(ens, 2), timeout=5)
        time.sleep(0.05)
        ens.kill_server(ens.leader())
        assert not ens.quorum_state()["serving"]
        assert reads_eof(raw)
        raw.close()
        assert wait_for(lambda: ens.quorum_state()["serving"], timeout=0.3 + 5.0)
        assert ens.leader() == 1
    finally:
        ens.stop()


def test_non_leader_kill_drops_only_its_own_clients(qens):
    c0 = client_to(qens, 0)
    c2 = client_to(qens, 2)
    dropped0 = qens.quorum_state()["dropped_connections"]
    qens.kill_server(2)
    st = qens.quorum_state()
    assert st["serving"] and st["leader"] == 0 and st["losses"] == 0
    assert st["dropped_connections"] == dropped0 + 1
    assert c0.state() == "connected"
    assert c0.exists("/")[0] == ra.ZOK
    c0.close()
    c2.close()


# ---- 6. rolling restart ----

def test_rolling_restart_never_loses_quorum(qens):
    c = make_client(qens)
    sid = c.session_id()
    paths = ["/q6-eph%d" % i for i in range(5)]
    for p in paths:
        assert c.create(p, b"", True)[0] == ra.ZOK
    for i in range(3):
        qens.kill_server(i)
        assert wait_for(lambda: c.state() == "connected" and c.exists("/")[0] == ra.ZOK, timeout=15)
        qens.restart_server(i)
    st = qens.quorum_state()
    assert st["losses"] == 0 and st["serving"] and st["servers_up"] == 3
    assert c.session_id() == sid
    for p in paths:
        assert qens.get(p)["stat"]["ephemeralOwner"] == sid
    assert qens.audit() == []
    c.close()


# ---- 7. orchestrator storm ----

N = 100


def test_orchestrator_rides_out_quorum_loss(qens):
    cfg = storm_config(qens, registration("p0.quorum.test", "h0", aliases=N - 1))
    o = ra.Orchestrator(json.dumps(cfg))
    o.start()
    try:
        assert o.wait_registered(30000)
        assert qens.ephemeral_count() == N
        sid = o.session_id()
        t_loss = time.monotonic()
        lose_quorum(qens)
        assert wait_for(lambda: o.metrics()["heartbeat_failures"] >= 2, timeout=15)
        assert qens.ephemeral_count() == N
        assert sid in qens.session_ids()
        assert o.metrics()["registers"] == 1
        time.sleep(max(0.0, 2.5 - (time.monotonic() - t_loss)))
        assert qens.ephemeral_count() == N  # 2.5 timeouts in, nothing expired
        hb0 = o.metrics()["heartbeats"]
        qens.restart_server(1)
        assert wait_for(lambda: o.metrics()["heartbeats"] >= hb0 + 3, timeout=30)
        m = o.metrics()
        assert o.session_id() == sid
        assert (m["registers"], m["session_expiries"], m["unregisters"]) == (1, 0, 0)
        assert qens.ephemeral_count() == N
        assert qens.audit() == []
    finally:
        o.stop()


# ---- 8. an expiry that is due still happens after quorum returns ----

def test_due_expiry_happens_after_quorum_returns(qens):
    reg = registration("p8.quorum.test", "h8")
    helper = make_client(qens)
    assert helper.mkdirp("/test/quorum/p8") == ra.ZOK
    helper.close()
    # a registrar whose process died: its session holds the host record
    s, sid = raw_session(qens, 0, 1000)
    raw_create_ephemeral(s, b"/test/quorum/p8/h8")
    s.close()
    lose_quorum(qens)
    time.sleep(1.5)
    assert qens.get("/test/quorum/p8/h8")["stat"]["ephemeralOwner"] == sid
    qens.restart_server(2)
    assert wait_for(lambda: not qens.get("/test/quorum/p8/h8")["exists"], timeout=1.0 + 10.0)
    assert sid not in qens.session_ids()

    o = ra.Orchestrator(json.dumps(storm_config(qens, reg)))
    o.start()
    try:
        assert o.wait_registered(30000)
        assert "/test/quorum/p8/h8" in o.znodes()
        assert qens.get("/test/quorum/p8/h8")["stat"]["ephemeralOwner"] == o.session_id()
    finally:
        o.stop()


# ---- 9. CLI ----

def test_cli_quorum_flag():
    bin_path = os.path.join(REPO_ROOT, "bin", "zkensembled")
    assert os.path.exists(bin_path), "run `make daemon` first"
    usage = subprocess.run([bin_path, "--no-such-flag"], capture_output=True, text=True, timeout=5)
    assert usage.returncode == 1 and "--quorum" in usage.stderr
    proc = subprocess.Popen([bin_path, "-n", "3", "--quorum", "--tick-ms", "100"],
                            stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    try:
        info = json.loads(proc.stdout.readline())
        assert len(info["ports"]) == 3
        c = ra.ZkClient(servers=[("127.0.0.1", p) for p in info["ports"]], session_timeout_ms=10000)
        c.start()
        assert c.wait_connected(15000)
        assert c.create("/q9-cli", b"x", True)[0] == ra.ZOK
        c.close()
    finally:
        proc.send_signal(signal.SIGTERM)
        assert proc.wait(timeout=10) == 0
    helptext = subprocess.run([sys.executable, "-m", "registrar_amd", "ensemble", "--help"],
                              cwd=REPO_ROOT, capture_output=True, text=True, timeout=30)
    assert helptext.returncode == 0 and "--quorum" in helptext.stdout


# ---- bindings ----

def test_quorum_state_with_mode_off(ensemble3):
    st = ensemble3.quorum_state()
    assert sorted(st) == ["dropped_connections", "enabled", "has_quorum", "leader", "losses", "needed",
                          "refused_connects", "servers", "servers_up", "serving"]
    assert not st["enabled"] and st["has_quorum"] and st["serving"]
    assert (st["servers"], st["servers_up"], st["needed"], st["losses"]) == (3, 3, 2, 0)
    ensemble3.kill_server(1)
    ensemble3.kill_server(2)
    assert ensemble3.has_quorum()  # any server up will do
    assert ensemble3.quorum_state()["losses"] == 0
    ensemble3.kill_server(0)
    assert not ensemble3.has_quorum()


def test_single_server_quorum_ensemble_serves():
    ens = ra.Ensemble(servers=1, tick_ms=50, min_session_timeout_ms=200, quorum=True)
    ens.start()
    try:
        assert ens.has_quorum() and ens.quorum_state()["needed"] == 1
        c = make_client(ens)
        assert c.create("/q-single", b"", True)[0] == ra.ZOK
        c.close()
    finally:
        ens.stop()


# ---- 10. the per-GPU registrar on a real GPU host ----

@pytest.mark.gpu
def test_gpu_gated_registration_rides_out_quorum_loss(qens):
    reg = {
        "domain": "gpu0.quorum.mi355x.test",
        "type": "host",
        "adminIp": "127.0.0.1",
        "hostname": "g0",
        "settleMs": 0,
        "service": {"type": "service", "service": {"srvce": "_infer", "proto": "_tcp", "port": 8000}},
    }
    cfg = storm_config(
        qens, reg, gpuIndex=0,
        healthCheck={"command": "gpu-liveness", "interval": 1000, "timeout": 30000, "threshold": 3})
    o = ra.Orchestrator(json.dumps(cfg))
    o.start()
    try:
        assert o.wait_registered(30000)
        sid = o.session_id()
        host_node = [n for n in o.znodes() if n.endswith("/g0")][0]
        lose_quorum(qens)
        time.sleep(2.5)
        assert not qens.has_quorum()
        hb0 = o.metrics()["heartbeats"]
        qens.restart_server(1)
        assert wait_for(lambda: o.metrics()["heartbeats"] >= hb0 + 3, timeout=30)
        assert o.session_id() == sid
        gpu = json.loads(qens.get(host_node)["data"])["host"]["gpu"]
        assert gpu["index"] == 0
        assert gpu["xgmiRank"] == ra.xgmi_local_rank(0)
        m = o.metrics()
        assert (m["registers"], m["session_expiries"], m["unregisters"]) == (1, 0, 0)
    finally:
        o.stop()
