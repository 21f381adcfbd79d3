"""binder_lite with cache=True: DNS answers served from a Resolver view. The
claim is a count (no ZooKeeper read per query once a domain is viewed) and an
equality (the same bytes as the direct binder), not a time."""
import json
import socket
import struct

import pytest

import registrar_amd as ra
from registrar_amd.binder_lite import BinderLite, _encode_name
from conftest import make_client, orch_config, wait_for

READS = ("getData", "getChildren", "exists")


def servers_of(ens):
    out = []
    for hp in ens.connect_string().split(","):
        host, port = hp.rsplit(":", 1)
        out.append((host, int(port)))
    return out


def query_bytes(name, qtype, txid=0x1234):
    return struct.pack(">HHHHHH", txid, 0x0100, 1, 0, 0, 0) + _encode_name(name) + struct.pack(">HH", qtype, 1)


def udp(addr, name, qtype, timeout=5):
    """The whole reply datagram, or None when none came."""
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        s.settimeout(timeout)
        s.sendto(query_bytes(name, qtype), addr)
        return s.recvfrom(4096)[0]
    except socket.timeout:
        return None
    finally:
        s.close()


def tcp(addr, name, qtype):
    q = query_bytes(name, qtype, txid=0x4321)
    s = socket.create_connection(addr, timeout=10)
    try:
        s.sendall(struct.pack(">H", len(q)) + q)

        def exactly(n):
            out = b""
            while len(out) < n:
                chunk = s.recv(n - len(out))
                assert chunk, "server closed the TCP connection mid-response"
                out += chunk
            return out

        return exactly(struct.unpack(">H", exactly(2))[0])
    finally:
        s.close()


def header(buf):
    txid, flags, qd, an, ns, ar = struct.unpack(">HHHHHH", buf[:12])
    return flags, an


def parse_answers(buf, an=None):
    """[(type, ttl, rdata)]; asserts that the message is whole RRs and nothing else."""
    assert an is None or an == header(buf)[1]
    _, an = header(buf)
    off = 12
    while buf[off] != 0:
        off += 1 + buf[off]
    off += 1 + 4
    answers = []
    for _ in range(an):
        off += 2
        rtype, rclass, ttl, rdlen = struct.unpack(">HHIH", buf[off:off + 10])
        off += 10
        answers.append((rtype, ttl, buf[off:off + rdlen]))
        off += rdlen
    assert off == len(buf)
    return answers


def addresses(buf):
    return sorted(socket.inet_ntoa(rd) for _, _, rd in parse_answers(buf))


def read_count(ens):
    c = ens.counters()
    return sum(c.get(k, 0) for k in READS)


@pytest.fixture
def binders(ensemble):
    made = {}
    for cache in (False, True):
        b = BinderLite(servers_of(ensemble), cache=cache)
        b.start()
        made[cache] = b
    yield made
    for b in made.values():
        b.stop()


SERVICE = {"type": "service", "service": {"srvce": "_http", "proto": "_tcp", "port": 8080, "ttl": 45}}


def register(client, domain, hostname, address, **extra):
    reg = {"domain": domain, "type": "host", "adminIp": address, "hostname": hostname, "settleMs": 0}
    reg.update(extra)
    rc, err, znodes = ra.register_node(client, json.dumps(reg))
    assert rc == ra.ZOK, err
    return znodes


def test_cached_binder_reads_nothing_per_query(ensemble, client, binders):
    for i in range(3):
        register(client, "zero.dns.test", "n%d" % i, "10.0.0.%d" % (i + 1), service=SERVICE)
    want = ["10.0.0.1", "10.0.0.2", "10.0.0.3"]
    for cache in (True, False):
        addr = binders[cache].address
        assert addresses(udp(addr, "zero.dns.test", 1)) == want  # the first query builds the view
        before = read_count(ensemble)
        for _ in range(100):
            assert addresses(udp(addr, "zero.dns.test", 1)) == want
        spent = read_count(ensemble) - before
        print("cache=%s: %d reads for 100 queries" % (cache, spent))
        if cache:
            assert spent == 0
        else:
            assert spent >= 100  # the control: the direct binder reads per query


def test_answers_are_byte_identical_between_the_modes(ensemble, client, binders):
    # hosts with a ttl of their own and with none, ports of their own and none
    register(client, "same.dns.test", "n0", "10.1.0.1", ttl=120, service=SERVICE)
    register(client, "same.dns.test", "n1", "10.1.0.2", service=SERVICE)
    bare = {"type": "host", "address": "10.1.0.3", "host": {"address": "10.1.0.3"}}
    assert client.create("/test/dns/same/bare", json.dumps(bare).encode(), True)[0] == ra.ZOK
    ported = {"type": "host", "address": "10.1.0.4", "ttl": 9, "host": {"address": "10.1.0.4", "ports": [9000]}}
    assert client.create("/test/dns/same/ported", json.dumps(ported).encode(), True)[0] == ra.ZOK
    assert client.mkdirp("/test/dns/hollow") == ra.ZOK
    big = "/test/dns/big"
    assert client.mkdirp(big) == ra.ZOK
    nrec = 1000
    for i in range(nrec):
        rec = {"type": "host", "address": "10.2.%d.%d" % (i // 250, i % 250)}
        assert client.create("%s/h%04d" % (big, i), json.dumps(rec).encode(), True)[0] == ra.ZOK

    direct, cached = binders[False].address, binders[True].address
    cases = [("A", "same.dns.test", 1), ("SRV", "same.dns.test", 33), ("NXDOMAIN", "nosuch.dns.test", 1),
             ("empty domain", "hollow.dns.test", 1), ("empty domain SRV", "hollow.dns.test", 33),
             ("unsupported type", "same.dns.test", 16), ("1000 records", "big.dns.test", 1)]
    for label, name, qtype in cases:
        for ask in (udp, tcp):
            for _ in range(2):  # the cached binder's first answer and its later ones
                a, b = ask(direct, name, qtype), ask(cached, name, qtype)
                assert a is not None and a == b, "%s over %s differs" % (label, ask.__name__)

    # and the answers are what they should be, so that "identical" is not "identically wrong"
    buf = udp(cached, "same.dns.test", 1)
    assert sorted((socket.inet_ntoa(rd), ttl) for _, ttl, rd in parse_answers(buf)) == [
        ("10.1.0.1", 120), ("10.1.0.2", 45), ("10.1.0.3", 45), ("10.1.0.4", 9)]
    buf = udp(cached, "same.dns.test", 33)
    assert sorted(struct.unpack(">HHH", rd[:6])[2] for _, _, rd in parse_answers(buf)) == [8080, 8080, 8080, 9000]
    assert header(udp(cached, "nosuch.dns.test", 1)) == (0x8183, 0)
    assert header(udp(cached, "hollow.dns.test", 1)) == (0x8180, 0)
    buf = udp(cached, "big.dns.test", 1)
    flags, an = header(buf)
    assert flags & 0x0200 and len(buf) <= 512
    assert 0 < len(parse_answers(buf)) < nrec  # whole RRs only
    buf = tcp(cached, "big.dns.test", 1)
    flags, an = header(buf)
    assert not flags & 0x0200 and an == nrec
    assert len(set(addresses(buf))) == nrec


@pytest.fixture
def binder(ensemble):
    b = BinderLite(servers_of(ensemble), cache=True)
    b.start()
    yield b
    b.stop()


def dns_query(addr, name, qtype):
    buf = udp(addr, name, qtype)
    flags, an = header(buf)
    return buf, flags & 0xF, an


def test_full_triangle_health_drives_dns(ensemble, binder, tmp_path):
    """tests/test_binder_lite.py's scenario of the same name, with the cached
    binder: in DNS, out on a health failure, back on recovery."""
    import registrar_amd as ra
    from conftest import orch_config, wait_for

    gate = tmp_path / "gate"
    gate.write_text("")
    cfg = orch_config(
        ensemble,
        {"domain": "tri.dns.test", "type": "host", "adminIp": "10.9.0.1", "hostname": "t0",
         "settleMs": 0,
         "service": {"type": "service", "service": {"srvce": "_svc", "proto": "_tcp", "port": 9000}}},
        heartbeatInterval=100,
        healthCheck={"command": "test -e %s" % gate, "interval": 40, "timeout": 500,
                     "threshold": 2, "period": 60000},
    )
    o = ra.Orchestrator(json.dumps(cfg))
    o.start()
    assert o.wait_registered(15000)

    def answers(qtype=1):
        buf, rcode, an = dns_query(binder.address, "tri.dns.test", qtype)
        return an

    assert wait_for(lambda: answers() == 1, timeout=5)
    # SRV answer carries the service port
    buf, rcode, an = dns_query(binder.address, "tri.dns.test", 33)
    assert an == 1
    assert struct.unpack(">HHH", parse_answers(buf, an)[0][2][:6])[2] == 9000

    gate.unlink()  # GPU/instance goes sick → flap damping → unregister
    assert wait_for(lambda: answers() == 0, timeout=10)

    gate.write_text("")  # recovery → re-register → back in DNS
    assert wait_for(lambda: answers() == 1, timeout=10)
    o.stop()


def test_cached_binder_serves_through_an_outage():
    ens = ra.Ensemble(servers=3, tick_ms=50, min_session_timeout_ms=200, quorum=True)
    ens.start()
    made = []
    clients = []
    try:
        for i in range(2):
            c = make_client(ens)
            clients.append(c)
            register(c, "out.dns.test", "n%d" % i, "10.3.0.%d" % (i + 1))
        for cache in (False, True):
            b = BinderLite(servers_of(ens), cache=cache, lookup_timeout_ms=1000)
            b.start()
            made.append(b)
        direct, cached = made
        full = ["10.3.0.1", "10.3.0.2"]
        assert addresses(udp(direct.address, "out.dns.test", 1)) == full
        assert addresses(udp(cached.address, "out.dns.test", 1)) == full
        ens.kill_server(1)
        ens.kill_server(2)
        assert wait_for(lambda: cached.resolver.snapshot("out.dns.test")["stale"], timeout=10)
        assert addresses(udp(cached.address, "out.dns.test", 1)) == full  # the last set
        buf = udp(direct.address, "out.dns.test", 1, timeout=2)
        assert buf is None or parse_answers(buf) == []  # the direct binder has nothing to say
        ens.restart_server(1)
        ens.restart_server(2)
        assert wait_for(lambda: not cached.resolver.snapshot("out.dns.test")["stale"], timeout=15)
        clients.pop().close()  # a registrar leaves
        assert wait_for(lambda: addresses(udp(cached.address, "out.dns.test", 1)) == ["10.3.0.1"], timeout=15)
        assert wait_for(lambda: (udp(direct.address, "out.dns.test", 1, timeout=2) or b"") ==
                        udp(cached.address, "out.dns.test", 1), timeout=15)
    finally:
        for b in made:
            b.stop()
        for c in clients:
            c.close()
        ens.stop()
