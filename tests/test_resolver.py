"""Resolver: a watch-maintained view of a domain, against the synthetic
ensemble (and, for one reply order no real tree gives on demand, the scripted
server)."""
import json
import random
import struct
import threading
import time

import pytest

import registrar_amd as ra
from conftest import make_client, wait_for
from scripted_server import (
    OP_CHILDREN, OP_EXISTS, OP_GET, Responder, ScriptedServer, reply, stat, zk_string, zk_vector)

CHANGE_KINDS = ("added", "removed", "changed")


def servers_of(ens):
    out = []
    for hp in ens.connect_string().split(","):
        host, port = hp.rsplit(":", 1)
        out.append((host, int(port)))
    return out


class Harness:
    """A started Resolver plus every event it has emitted so far."""

    def __init__(self, servers, **kw):
        kw.setdefault("session_timeout_ms", 5000)
        self.r = ra.Resolver(servers=servers, **kw)
        self.r.start()
        self.events = []

    def drain(self):
        self.events.extend(self.r.poll_events())
        return self.events

    def kinds(self, *types):
        return [(e["type"], e["name"]) for e in self.drain() if not types or e["type"] in types]

    def names(self, domain):
        return [h["name"] for h in self.r.snapshot(domain)["hosts"]]


@pytest.fixture
def resolvers():
    made = []

    def make(ens_or_servers, **kw):
        servers = ens_or_servers if isinstance(ens_or_servers, list) else servers_of(ens_or_servers)
        h = Harness(servers, **kw)
        made.append(h)
        return h

    yield make
    for h in made:
        h.r.stop()


SERVICE = {"type": "service", "service": {"srvce": "_http", "proto": "_tcp", "port": 8080, "ttl": 45}}


def register(client, domain, hostname, address, ttl=None, service=None):
    reg = {"domain": domain, "type": "host", "adminIp": address, "hostname": hostname, "settleMs": 0}
    if ttl is not None:
        reg["ttl"] = ttl
    if service is not None:
        reg["service"] = service
    rc, err, znodes = ra.register_node(client, json.dumps(reg))
    assert rc == ra.ZOK, err
    return znodes


def host_record(address, ports=None, **extra):
    rec = {"type": "host", "address": address, "host": {"address": address}}
    if ports:
        rec["host"]["ports"] = ports
    rec.update(extra)
    return json.dumps(rec).encode()


def tree_of(ens, path):
    """{name: payload} of the children of `path`, from the ensemble itself."""
    return {ch: ens.get("%s/%s" % (path, ch))["data"] for ch in ens.children(path)}


def view_of(r, domain):
    return {h["name"]: h["payload"] for h in r.snapshot(domain)["hosts"]}


# ------------------------------------------------------ empty and small domains

def test_empty_domain_exists_with_no_hosts(ensemble, client, resolvers):
    assert client.mkdirp("/test/empty") == ra.ZOK
    h = resolvers(ensemble)
    snap = h.r.lookup("empty.test", 5000)
    assert snap["status"] == "ok"
    assert snap["exists"] and snap["synced"] and not snap["stale"]
    assert snap["hosts"] == [] and snap["service"] is None
    assert snap["generation"] == 1
    assert h.r.domains() == ["empty.test"]


def test_one_child_fields_equal_what_register_node_wrote(ensemble, client, resolvers):
    znodes = register(client, "one.test", "n0", "10.0.0.1", ttl=120)
    node = [z for z in znodes if z.endswith("/n0")][0]
    stored = ensemble.get(node)
    h = resolvers(ensemble)
    snap = h.r.lookup("one.test", 5000)
    assert snap["status"] == "ok" and len(snap["hosts"]) == 1
    host = snap["hosts"][0]
    assert host["name"] == "n0"
    assert host["address"] == "10.0.0.1"
    assert host["ttl"] == 120  # as stored
    assert host["type"] == "host"
    assert host["gpu"] is None
    assert host["ports"] == []  # no ports of its own and no service record
    assert host["payload"] == stored["data"]
    assert host["ephemeral_owner"] == client.session_id() == stored["stat"]["ephemeralOwner"]
    assert host["mzxid"] == stored["stat"]["mzxid"]
    assert host["local"] is False
    assert snap["service"] is None


def test_three_children_with_a_service_record_and_the_ports_fallback(ensemble, client, resolvers):
    for i in range(3):
        register(client, "web.test", "n%d" % i, "10.0.1.%d" % i, service=SERVICE)
    # hosts with other ports of their own, with none (a gpu block instead), with a ttl
    own = host_record("10.0.1.9", ports=[9001, 9002])
    gpu = {"type": "host", "address": "10.0.1.8",
           "host": {"address": "10.0.1.8", "gpu": {"index": 2, "xgmiRank": 2, "uuid": "GPU-x"}}}
    assert client.create("/test/web/own", own, True)[0] == ra.ZOK
    assert client.create("/test/web/gpu", json.dumps(gpu).encode(), True)[0] == ra.ZOK
    h = resolvers(ensemble)
    snap = h.r.lookup("web.test", 5000)
    assert snap["status"] == "ok"
    assert snap["service"] == SERVICE["service"]
    assert [x["name"] for x in snap["hosts"]] == ["gpu", "n0", "n1", "n2", "own"]  # by name
    by = {x["name"]: x for x in snap["hosts"]}
    for i in range(3):
        assert by["n%d" % i]["address"] == "10.0.1.%d" % i
        assert by["n%d" % i]["ports"] == [8080]  # register_node wrote the service's port into the record
        assert by["n%d" % i]["ttl"] is None      # none stored: the consumer falls back to the service's
    assert by["own"]["ports"] == [9001, 9002]
    assert "ports" not in json.loads(by["gpu"]["payload"])["host"]
    assert by["gpu"]["ports"] == [8080]  # the fallback: the service record's port
    assert by["gpu"]["gpu"] == {"index": 2, "xgmiRank": 2, "uuid": "GPU-x"}
    assert view_of(h.r, "web.test") == tree_of(ensemble, "/test/web")


# ------------------------------------------------------------------ large domain

def test_large_domain_is_built_with_one_batched_read(ensemble, client, resolvers):
    n = 600
    assert client.mkdirp("/test/big") == ra.ZOK
    assert client.set("/test/big", json.dumps({"type": "service", "service": SERVICE}).encode()) == ra.ZOK
    for i in range(n):
        rec = host_record("10.%d.%d.%d" % (i // 65536 + 1, i // 256, i % 256), pad="x" * 120, seq=i)
        assert 180 <= len(rec) <= 260
        assert client.create("/test/big/h%04d" % i, rec, True)[0] == ra.ZOK
    h = resolvers(ensemble)
    assert wait_for(h.r.connected, timeout=10)
    before = ensemble.counters()
    snap = h.r.lookup("big.test", 20000)
    after = ensemble.counters()
    assert snap["status"] == "ok" and len(snap["hosts"]) == n
    assert sorted(ensemble.children("/test/big")) == [x["name"] for x in snap["hosts"]]
    assert view_of(h.r, "big.test") == tree_of(ensemble, "/test/big")
    cost = {k: after.get(k, 0) - before.get(k, 0) for k in ("getData", "getChildren", "exists")}
    assert cost == {"getData": n + 1, "getChildren": 1, "exists": 1}


# ---------------------------------------------------------- add, remove, change

def test_add_remove_change_give_one_event_each(ensemble, client, resolvers):
    # n0 has no ports of its own (register_node would copy the service's into the record)
    assert client.mkdirp("/test/ev") == ra.ZOK
    assert client.set("/test/ev", json.dumps({"type": "service", "service": SERVICE}).encode()) == ra.ZOK
    assert client.create("/test/ev/n0", host_record("10.0.2.1"), True)[0] == ra.ZOK
    h = resolvers(ensemble)
    snap = h.r.lookup("ev.test", 5000)
    gen = snap["generation"]
    assert h.kinds() == [("synced", "")]

    def one_more(kind, name):
        nonlocal gen
        assert wait_for(lambda: h.r.snapshot("ev.test")["generation"] > gen, timeout=10)
        time.sleep(0.1)  # anything spurious would follow at once
        new = [e for e in h.drain() if e["generation"] > gen]
        assert [(e["type"], e["name"], e["generation"]) for e in new] == [(kind, name, gen + 1)]
        assert h.r.snapshot("ev.test")["generation"] == gen + 1
        gen += 1

    assert client.create("/test/ev/n1", host_record("10.0.2.2"), True)[0] == ra.ZOK
    one_more("added", "n1")
    assert h.names("ev.test") == ["n0", "n1"]
    assert client.set("/test/ev/n1", host_record("10.0.2.3")) == ra.ZOK
    one_more("changed", "n1")
    assert {x["name"]: x["address"] for x in h.r.snapshot("ev.test")["hosts"]}["n1"] == "10.0.2.3"
    # and a second change of the same node: its watch was armed again
    assert client.set("/test/ev/n1", host_record("10.0.2.4")) == ra.ZOK
    one_more("changed", "n1")
    assert client.delete_("/test/ev/n1") == ra.ZOK
    one_more("removed", "n1")
    assert h.names("ev.test") == ["n0"]
    # the service record: every host without ports of its own follows it
    assert [x["ports"] for x in h.r.snapshot("ev.test")["hosts"]] == [[8080]]
    svc = {"type": "service", "service": {"type": "service", "service": dict(SERVICE["service"], port=9090)}}
    assert client.set("/test/ev", json.dumps(svc).encode()) == ra.ZOK
    one_more("service", "")
    snap = h.r.snapshot("ev.test")
    assert snap["service"]["port"] == 9090
    assert [x["ports"] for x in snap["hosts"]] == [[9090]]
    assert h.r.stats()["events_applied"] == 5


def test_a_registrars_session_expiring_removes_its_hosts_only(ensemble, resolvers):
    c1 = make_client(ensemble)
    c2 = make_client(ensemble)
    try:
        register(c1, "exp.test", "a0", "10.0.3.1")
        register(c1, "exp.test", "a1", "10.0.3.2")
        register(c2, "exp.test", "b0", "10.0.3.3")
        h = resolvers(ensemble)
        assert [x["name"] for x in h.r.lookup("exp.test", 5000)["hosts"]] == ["a0", "a1", "b0"]
        ensemble.expire_session(c1.session_id())
        assert wait_for(lambda: h.names("exp.test") == ["b0"], timeout=10)
        assert sorted(h.kinds("removed")) == [("removed", "a0"), ("removed", "a1")]
        assert h.kinds("added", "changed") == []
    finally:
        c1.close()
        c2.close()


# -------------------------------------------------------- listed child vanishes

def test_listed_child_that_answers_no_node_is_skipped_silently():
    payload = host_record("10.0.4.1")
    resp = Responder()

    def on_request(conn, xid, op, body):
        n = struct.unpack(">i", body[:4])[0]
        path = body[4:4 + n].decode()
        z = resp.zxid()
        if op == OP_EXISTS:
            return reply(xid, z, 0, stat())
        if op == OP_CHILDREN:
            assert path == "/test/vanish"
            return reply(xid, z, 0, zk_vector(["a", "b"]))
        if op == OP_GET:
            if path == "/test/vanish":
                return reply(xid, z, 0, zk_string(b"") + stat())
            if path == "/test/vanish/a":
                return reply(xid, z, 0, zk_string(payload) + stat(mzxid=7, ephemeralOwner=9))
            return reply(xid, z, -101)
        return reply(xid, z, 0)

    resp.on_request = on_request
    srv = ScriptedServer(resp)
    r = ra.Resolver(servers=[srv.addr], session_timeout_ms=30000)
    try:
        r.start()
        snap = r.lookup("vanish.test", 5000)
        assert snap["status"] == "ok" and snap["synced"]
        assert [(x["name"], x["payload"], x["mzxid"], x["ephemeral_owner"]) for x in snap["hosts"]] == [
            ("a", payload, 7, 9)]
        assert [e["type"] for e in r.poll_events()] == ["synced"]
    finally:
        r.stop()
        srv.stop()


# ------------------------------------------------------------------------ churn

def test_churn_converges_and_snapshots_stay_consistent(ensemble, client, resolvers):
    assert client.mkdirp("/test/churn") == ra.ZOK
    h = resolvers(ensemble)
    assert h.r.lookup("churn.test", 5000)["status"] == "ok"
    stop = threading.Event()
    names = ["c%02d" % i for i in range(20)]
    problems = []

    def mutate(seed):
        rng = random.Random(seed)
        c = make_client(ensemble)
        try:
            while not stop.is_set():
                name = rng.choice(names)
                path = "/test/churn/" + name
                if rng.random() < 0.5:
                    c.create(path, host_record("10.0.5.%d" % rng.randrange(250), seq=rng.randrange(1 << 30)))
                else:
                    c.delete_(path)
        finally:
            c.close()

    def read():
        last = 0
        while not stop.is_set():
            snap = h.r.snapshot("churn.test")
            if snap["generation"] < last:
                problems.append("generation fell from %d to %d" % (last, snap["generation"]))
            last = snap["generation"]
            for x in snap["hosts"]:
                if not x["payload"] or x["address"] is None:
                    problems.append("host %s with an empty payload" % x["name"])
            got = [x["name"] for x in snap["hosts"]]
            if got != sorted(set(got)):
                problems.append("hosts not sorted or not unique: %r" % got)

    threads = [threading.Thread(target=mutate, args=(s,)) for s in (1, 2)] + [threading.Thread(target=read)]
    for t in threads:
        t.start()
    time.sleep(1.0)
    stop.set()
    for t in threads:
        t.join(20)
        assert not t.is_alive()
    assert wait_for(lambda: view_of(h.r, "churn.test") == tree_of(ensemble, "/test/churn"), timeout=15)
    assert problems == []
    assert h.r.snapshot("churn.test")["generation"] > 1  # something did happen
    gens = [e["generation"] for e in h.drain()]
    assert gens == sorted(gens)


# ------------------------------------------------------- same-session reconnect

def test_same_session_reconnect_catches_up_through_set_watches(ensemble3, resolvers):
    servers = servers_of(ensemble3)
    writer = ra.ZkClient(servers=[servers[1]], session_timeout_ms=5000)
    writer.start()
    assert writer.wait_connected(10000)
    try:
        assert writer.mkdirp("/test/rc") == ra.ZOK
        for name in ("keep", "drop", "edit"):
            assert writer.create("/test/rc/" + name, host_record("10.0.6.1", tag=name), True)[0] == ra.ZOK
        # the resolver knows server 0 only, so it stays away for as long as that server does
        h = resolvers([servers[0]])
        assert h.names("rc.test") == [] and h.r.lookup("rc.test", 5000)["status"] == "ok"
        sid = h.r.session_id()
        gets_before = ensemble3.counters()["getData"]
        ensemble3.kill_server(0)
        assert wait_for(lambda: not h.r.connected(), timeout=10)
        # while it is away
        assert writer.create("/test/rc/new", host_record("10.0.6.2"), True)[0] == ra.ZOK
        assert writer.delete_("/test/rc/drop") == ra.ZOK
        assert writer.set("/test/rc/edit", host_record("10.0.6.3", tag="edited")) == ra.ZOK
        stale = h.r.snapshot("rc.test")
        assert stale["stale"] and [x["name"] for x in stale["hosts"]] == ["drop", "edit", "keep"]
        ensemble3.restart_server(0)
        assert wait_for(lambda: view_of(h.r, "rc.test") == tree_of(ensemble3, "/test/rc")
                        and not h.r.snapshot("rc.test")["stale"], timeout=15)
        assert h.names("rc.test") == ["edit", "keep", "new"]
        assert h.r.session_id() == sid
        assert h.r.stats()["resyncs_after_expiry"] == 0
        kinds = h.kinds()
        assert kinds.index(("stale", "")) < kinds.index(("fresh", ""))
        assert sorted(h.kinds(*CHANGE_KINDS)) == [("added", "new"), ("changed", "edit"), ("removed", "drop")]
        # no full re-read: "keep" was not read again (service record, new, drop, edit at the most)
        assert ensemble3.counters()["getData"] - gets_before <= 4
    finally:
        writer.close()


# ------------------------------------------------------------------ quorum mode

def test_below_quorum_the_last_view_is_served_stale(resolvers):
    ens = ra.Ensemble(servers=3, tick_ms=50, min_session_timeout_ms=200, quorum=True)
    ens.start()
    writer = None
    try:
        writer = make_client(ens)
        register(writer, "q.test", "n0", "10.0.7.1")
        register(writer, "q.test", "n1", "10.0.7.2")
        register(writer, "later.test", "m0", "10.0.7.9")
        h = resolvers(ens)
        assert [x["name"] for x in h.r.lookup("q.test", 5000)["hosts"]] == ["n0", "n1"]
        ens.kill_server(1)
        ens.kill_server(2)
        assert wait_for(lambda: h.r.snapshot("q.test")["stale"], timeout=10)
        snap = h.r.snapshot("q.test")
        assert snap["exists"] and snap["synced"] and snap["stale"]
        assert [x["name"] for x in snap["hosts"]] == ["n0", "n1"]
        # lookup of a viewed domain is served too; one of a new domain cannot be
        assert [x["name"] for x in h.r.lookup("q.test", 300)["hosts"]] == ["n0", "n1"]
        assert h.r.lookup("later.test", 300)["status"] == "unavailable"
        assert h.r.domains() == ["q.test"]
        ens.restart_server(1)
        ens.restart_server(2)
        assert wait_for(lambda: writer.state() == "connected" and writer.exists("/test/q")[0] == ra.ZOK, timeout=15)
        assert writer.create("/test/q/n2", host_record("10.0.7.3"), True)[0] == ra.ZOK
        assert wait_for(lambda: h.names("q.test") == ["n0", "n1", "n2"]
                        and not h.r.snapshot("q.test")["stale"], timeout=15)
        assert h.r.lookup("later.test", 5000)["status"] == "ok"
        kinds = h.kinds("stale", "fresh")
        assert kinds[0] == ("stale", "") and kinds[-1] == ("fresh", "")
    finally:
        if writer:
            writer.close()
        ens.stop()


# ------------------------------------------------ the resolver's session expired

@pytest.mark.parametrize("remove_one", [False, True])
def test_own_session_expiry_resyncs_and_reports_real_differences_only(ensemble, client, resolvers, remove_one):
    for i in range(3):
        register(client, "own.test", "n%d" % i, "10.0.8.%d" % i, service=SERVICE)
    h = resolvers(ensemble)
    assert len(h.r.lookup("own.test", 5000)["hosts"]) == 3
    sid = h.r.session_id()
    ensemble.expire_session(sid)
    if remove_one:
        assert client.delete_("/test/own/n1") == ra.ZOK
    want = ["n0", "n2"] if remove_one else ["n0", "n1", "n2"]
    assert wait_for(lambda: h.r.stats()["resyncs_after_expiry"] == 1 and h.names("own.test") == want
                    and not h.r.snapshot("own.test")["stale"], timeout=15)
    assert h.r.session_id() not in (0, sid)
    assert h.kinds(*CHANGE_KINDS) == ([("removed", "n1")] if remove_one else [])
    # the new session's watches work
    assert client.create("/test/own/n9", host_record("10.0.8.9"), True)[0] == ra.ZOK
    assert wait_for(lambda: h.names("own.test") == want + ["n9"], timeout=10)
    assert h.r.stats()["resyncs_after_expiry"] == 1


# ------------------------------------------------------- absent, dropped, capped

def test_absent_domain_is_not_cached(ensemble, client, resolvers):
    h = resolvers(ensemble)
    snap = h.r.lookup("nosuch.test", 5000)
    assert snap["status"] == "absent" and not snap["exists"] and snap["hosts"] == []
    assert h.r.domains() == []
    before = ensemble.counters()
    assert h.r.lookup("nosuch.test", 5000)["status"] == "absent"
    after = ensemble.counters()
    assert after["exists"] - before["exists"] == 1
    for op in ("getData", "getChildren"):
        assert after.get(op, 0) == before.get(op, 0)
    register(client, "nosuch.test", "n0", "10.0.9.1")
    assert h.drain() == []  # no watch was left behind to fire
    snap = h.r.lookup("nosuch.test", 5000)
    assert snap["status"] == "ok" and [x["name"] for x in snap["hosts"]] == ["n0"]
    assert h.r.domains() == ["nosuch.test"]


def test_view_is_dropped_with_its_domain_node(ensemble, client, resolvers):
    assert client.mkdirp("/test/drop") == ra.ZOK
    assert client.create("/test/drop/n0", host_record("10.0.10.1"))[0] == ra.ZOK
    h = resolvers(ensemble)
    assert h.r.lookup("drop.test", 5000)["status"] == "ok"
    assert client.delete_("/test/drop/n0") == ra.ZOK
    assert client.delete_("/test/drop") == ra.ZOK
    assert wait_for(lambda: ("dropped", "") in h.kinds(), timeout=10)
    assert h.r.domains() == []
    assert h.r.snapshot("drop.test")["exists"] is False
    assert h.r.lookup("drop.test", 5000)["status"] == "absent"
    # n0's own "removed" comes first if its deletion was read before the domain
    # node's; a pass that finds the domain node gone drops the view as a whole
    assert h.kinds("removed") in ([("removed", "n0")], [])


def test_domain_cap_falls_back_to_direct_reads(ensemble, client, resolvers):
    for d in ("d1", "d2", "d3"):
        register(client, d + ".test", "h-" + d, "10.0.11.1", service=SERVICE)
    h = resolvers(ensemble, max_domains=2)
    assert h.r.lookup("d1.test", 5000)["status"] == "ok"
    assert h.r.lookup("d2.test", 5000)["status"] == "ok"
    assert h.r.stats()["direct_reads"] == 0
    for n in (1, 2):
        snap = h.r.lookup("d3.test", 5000)
        assert snap["status"] == "ok" and snap["synced"]
        assert [(x["name"], x["ports"]) for x in snap["hosts"]] == [("h-d3", [8080])]
        assert snap["service"] == SERVICE["service"]
        assert h.r.stats()["direct_reads"] == n
        assert sorted(h.r.domains()) == ["d1.test", "d2.test"]
    # a direct read leaves no watch: a change under d3 reaches nobody
    assert client.create("/test/d3/extra", host_record("10.0.11.2"), True)[0] == ra.ZOK
    assert client.create("/test/d1/extra", host_record("10.0.11.3"), True)[0] == ra.ZOK
    assert wait_for(lambda: ("added", "extra") in h.kinds(), timeout=10)
    assert [e["domain"] for e in h.drain() if e["type"] == "added"] == ["d1.test"]


# --------------------------------------------------------------------- locality

def test_local_first_orders_matching_addresses_first(ensemble, client, resolvers):
    assert client.mkdirp("/test/loc") == ra.ZOK
    for name, addr in (("a", "10.0.12.9"), ("b", "10.0.12.5"), ("c", "10.0.12.5"), ("d", "10.0.12.7")):
        assert client.create("/test/loc/" + name, host_record(addr), True)[0] == ra.ZOK
    h = resolvers(ensemble, local_address="10.0.12.5")
    snap = h.r.lookup("loc.test", 5000, local_first=True)
    assert [(x["name"], x["local"]) for x in snap["hosts"]] == [("b", True), ("c", True), ("a", False), ("d", False)]
    assert [x["name"] for x in h.r.snapshot("loc.test", local_first=True)["hosts"]] == ["b", "c", "a", "d"]
    # the default order is by name, the flag is there all the same
    assert [(x["name"], x["local"]) for x in h.r.snapshot("loc.test")["hosts"]] == [
        ("a", False), ("b", True), ("c", True), ("d", False)]


# --------------------------------------------------- malformed and nested records

def test_malformed_and_nested_records_are_skipped_like_the_direct_path(ensemble, client, resolvers):
    from registrar_amd.binder_lite import BinderLite

    assert client.mkdirp("/test/mixed") == ra.ZOK
    assert client.create("/test/mixed/good", host_record("10.0.13.1"), True)[0] == ra.ZOK
    assert client.create("/test/mixed/bad", b"{not json")[0] == ra.ZOK
    assert client.create("/test/mixed/empty", b"")[0] == ra.ZOK
    # a nested domain: sub.mixed.test has a service record of its own
    register(client, "sub.mixed.test", "s0", "10.0.13.2", service=SERVICE)
    assert json.loads(ensemble.get("/test/mixed/sub")["data"])["type"] == "service"
    h = resolvers(ensemble)
    snap = h.r.lookup("mixed.test", 5000)
    assert [x["name"] for x in snap["hosts"]] == ["good"]
    binder = BinderLite(servers_of(ensemble))
    binder.start()
    try:
        hosts, service, _ = binder._lookup("mixed.test")
    finally:
        binder.stop()
    assert [x["name"] for x in hosts] == ["good"]
    # a skipped record that becomes a host record joins the view
    assert client.set("/test/mixed/bad", host_record("10.0.13.3")) == ra.ZOK
    assert wait_for(lambda: h.names("mixed.test") == ["bad", "good"], timeout=10)
    # the nested domain is a domain of its own
    assert [x["name"] for x in h.r.lookup("sub.mixed.test", 5000)["hosts"]] == ["s0"]
