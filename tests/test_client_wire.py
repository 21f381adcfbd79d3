"""What the native ZooKeeper client puts on the wire, and how it decodes.

The peer is tests/scripted_server.py, which shares no code with the client.
Expected bytes are packed here with struct from the ZooKeeper wire layout and
compared with whole recorded frames; replies are packed the same way and
checked through the Python bindings."""
import contextlib
import struct
import threading

import pytest

import registrar_amd as ra
from conftest import wait_for
from scripted_server import (
    DEFAULT_PASSWD, DEFAULT_SESSION, EV_CHANGED, EV_CHILD, EV_DELETED, OP_CHILDREN, OP_CLOSE, OP_CREATE,
    OP_DELETE, OP_EXISTS, OP_GET, OP_MULTI, OP_PING, OP_SET, OP_SETWATCHES, XID_PING, XID_SETWATCHES,
    Responder, ScriptedServer, connect_request, create_body, parse_header, reply, request, stat, watch_event,
    zk_string, zk_vector)

SESSION_TIMEOUT = 30000  # long: no ping lands between the frames under test


def start_client(srv, **kw):
    kw.setdefault("session_timeout_ms", SESSION_TIMEOUT)
    c = ra.ZkClient(servers=[srv.addr], randomize_start=False, **kw)
    c.start()
    return c


@contextlib.contextmanager
def session(script, **kw):
    """A scripted server and a connected client; the client is closed from
    the calling (main) thread on the way out, then the server is stopped."""
    srv = ScriptedServer(script)
    c = None
    try:
        c = start_client(srv, **kw)
        assert c.wait_connected(5000), "client did not connect to the scripted server"
        yield srv, c
    finally:
        if c is not None:
            c.close()
        srv.stop()


def first_string(payload):
    n = struct.unpack(">i", payload[:4])[0]
    return payload[4:4 + n]


def canned(resp):
    """Well-formed OK replies for every single-op verb."""
    def on_request(conn, xid, op, payload):
        z = resp.zxid()
        if op == OP_CREATE:
            return reply(xid, z, 0, zk_string(first_string(payload)))
        if op in (OP_EXISTS, OP_SET):
            return reply(xid, z, 0, stat(version=1))
        if op == OP_GET:
            return reply(xid, z, 0, zk_string(b"d") + stat(dataLength=1))
        if op == OP_CHILDREN:
            return reply(xid, z, 0, zk_vector([]))
        return reply(xid, z, 0)
    return on_request


def canned_responder(**handshake):
    resp = Responder(**handshake)
    resp.on_request = canned(resp)
    return resp


def reconnect(srv, c, index):
    """Drop connection `index` from the server side; wait for the client to
    come back on connection index+1."""
    srv.accepted()[index].close()
    assert wait_for(lambda: len(srv.frames(index + 1)) >= 1 and c.state() == "connected", timeout=5)


# ---------------------------------------------------------------- requests

def test_first_connect_request_is_44_zero_bytes_but_the_timeout():
    with session(canned_responder(), session_timeout_ms=12345) as (srv, c):
        raw = srv.frames(0)[0]
        # protocolVersion(i) lastZxidSeen(q) timeOut(i) sessionId(q) passwd(len 16 + 16 bytes)
        expected = struct.pack(">i", 44) + struct.pack(">iqiq", 0, 0, 12345, 0) + struct.pack(">i", 16) + bytes(16)
        assert len(expected) == 48
        assert raw == expected


def test_reconnect_request_carries_session_and_highest_zxid():
    """The reconnect's lastZxidSeen is the HIGHEST zxid of any reply header so
    far: with reply zxids 5, 9, 7 the client must report 9, not the latest. A
    watch event's zxid of -1 must not lower it either."""
    zxids = iter([5, 9, 7])
    resp = Responder(lambda conn, xid, op, payload: reply(xid, next(zxids), 0))
    with session(resp) as (srv, c):
        for p in ("/a", "/b", "/c"):
            assert c.delete_(p) == ra.ZOK
        srv.accepted()[0].send_raw(watch_event(EV_CHANGED, "/a", zxid=-1))
        assert wait_for(lambda: c.poll_watches() != [], timeout=5)
        reconnect(srv, c, 0)
        assert srv.frames(1)[0] == connect_request(SESSION_TIMEOUT, last_zxid=9, session_id=DEFAULT_SESSION,
                                                   passwd=DEFAULT_PASSWD)
        assert c.session_id() == DEFAULT_SESSION


def test_one_golden_frame_per_verb_and_rising_xids():
    def on_multi(conn, xid, op, payload):
        if op != OP_MULTI:
            return inner(conn, xid, op, payload)
        body = struct.pack(">ibi", OP_CREATE, 0, 0) + zk_string("/m/c") + struct.pack(">ibi", OP_DELETE, 0, 0)
        return reply(xid, resp.zxid(), 0, body + struct.pack(">ibi", -1, 1, -1))

    resp = Responder()
    inner = canned(resp)
    resp.on_request = on_multi
    with session(resp) as (srv, c):
        expected = []
        xid = 0

        def expect(op, body):
            nonlocal xid
            xid += 1  # xids start at 1 and rise by one per request
            expected.append(request(xid, op, body))

        # create: path, data, ACL vector [perms 31, "world", "anyone"], flags
        assert c.create("/p", b"data") == (ra.ZOK, "/p")
        expect(OP_CREATE, zk_string("/p") + zk_string(b"data") + struct.pack(">i", 1) + struct.pack(">i", 31) +
               zk_string("world") + zk_string("anyone") + struct.pack(">i", 0))
        assert c.create("/e", b"", True) == (ra.ZOK, "/e")
        expect(OP_CREATE, create_body("/e", b"", 1))  # EPHEMERAL
        # delete: path, version
        assert c.delete_("/p", 7) == ra.ZOK
        expect(OP_DELETE, zk_string("/p") + struct.pack(">i", 7))
        assert c.delete_("/p") == ra.ZOK
        expect(OP_DELETE, zk_string("/p") + struct.pack(">i", -1))
        # exists / getData / getChildren: path, watch
        for watch in (False, True):
            assert c.exists("/x", watch)[0] == ra.ZOK
            expect(OP_EXISTS, zk_string("/x") + (b"\x01" if watch else b"\x00"))
            assert c.get("/x", watch)[0] == ra.ZOK
            expect(OP_GET, zk_string("/x") + (b"\x01" if watch else b"\x00"))
            assert c.get_children("/x", watch)[0] == ra.ZOK
            expect(OP_CHILDREN, zk_string("/x") + (b"\x01" if watch else b"\x00"))
        # setData: path, data, version
        assert c.set("/x", b"new", 3) == ra.ZOK
        expect(OP_SET, zk_string("/x") + zk_string(b"new") + struct.pack(">i", 3))
        # the pipelined batches: one plain request per element
        assert c.create_many(["/b/1", "/b/2"], b"v", True) == [ra.ZOK, ra.ZOK]
        expect(OP_CREATE, create_body("/b/1", b"v", 1))
        expect(OP_CREATE, create_body("/b/2", b"v", 1))
        assert c.exists_many(["/b/1", "/b/2"]) == [ra.ZOK, ra.ZOK]
        expect(OP_EXISTS, zk_string("/b/1") + b"\x00")
        expect(OP_EXISTS, zk_string("/b/2") + b"\x00")
        assert c.delete_many(["/b/1", "/b/2"]) == [ra.ZOK, ra.ZOK]
        expect(OP_DELETE, zk_string("/b/1") + struct.pack(">i", -1))
        expect(OP_DELETE, zk_string("/b/2") + struct.pack(">i", -1))
        # multi: op 14; MultiHeader{type, done=false, err=-1} before each op,
        # then the terminator {-1, true, -1}
        assert c.multi([("create", "/m/c", b"x", True), ("delete", "/m/d")]) == (ra.ZOK, [ra.ZOK, ra.ZOK])
        expect(OP_MULTI,
               struct.pack(">ibi", OP_CREATE, 0, -1) + create_body("/m/c", b"x", 1) +
               struct.pack(">ibi", OP_DELETE, 0, -1) + zk_string("/m/d") + struct.pack(">i", -1) +
               struct.pack(">ibi", -1, 1, -1))
        # heartbeat: one exists without a watch per node
        assert c.heartbeat(["/hb/a", "/hb/b"])[0] == ra.ZOK
        expect(OP_EXISTS, zk_string("/hb/a") + b"\x00")
        expect(OP_EXISTS, zk_string("/hb/b") + b"\x00")

        got = srv.frames(0)[1:]
        assert len(got) == len(expected)
        for i, (g, e) in enumerate(zip(got, expected)):
            assert g == e, "request %d (xid %d)" % (i, i + 1)


def test_mkdirp_is_three_creates_in_one_burst():
    """The server answers nothing until it has all three creates: a client
    that waited for each reply before the next request would stall here."""
    def script(conn):
        conn.handshake()
        reqs = [conn.read_request(timeout=3.0) for _ in range(3)]
        conn.send_raw(b"".join(reply(xid, 10 + i, 0, zk_string(first_string(payload)))
                               for i, (xid, op, payload) in enumerate(reqs)))
        Responder().serve(conn)

    with session(script) as (srv, c):
        assert c.mkdirp("/a/b/c") == ra.ZOK
        assert srv.frames(0)[1:] == [request(1, OP_CREATE, create_body("/a", b"", 0)),
                                     request(2, OP_CREATE, create_body("/a/b", b"", 0)),
                                     request(3, OP_CREATE, create_body("/a/b/c", b"", 0))]


def test_ping_frame():
    # negotiated timeout 300 ms: the client pings every 100 ms
    with session(canned_responder(timeout_ms=300)) as (srv, c):
        ping = request(XID_PING, OP_PING)
        assert ping == struct.pack(">iii", 8, -2, 11)
        assert wait_for(lambda: ping in srv.frames(0), timeout=5, interval=0.01)
        assert c.session_timeout_ms() == 300
        # nothing but pings follows the handshake on an idle session
        assert set(srv.frames(0)[1:]) == {ping}


def test_close_sends_close_session_before_the_fin():
    seen = {}
    done = threading.Event()

    def script(conn):
        conn.handshake()
        xid, op, payload = conn.read_request()
        conn.send_raw(reply(xid, 1, 0))
        seen["close"] = conn.read_frame()
        seen["eof"] = conn.wait_eof()  # nothing after it but the FIN
        done.set()

    srv = ScriptedServer(script)
    try:
        c = start_client(srv)
        try:
            assert c.wait_connected(5000)
            assert c.delete_("/x") == ra.ZOK
        finally:
            c.close()
        assert done.wait(5)
        # closeSession takes the next xid; op -11, no body
        assert seen["close"] == request(2, OP_CLOSE) == struct.pack(">iii", 8, 2, -11)
        assert seen["eof"]
    finally:
        srv.stop()


# ------------------------------------------------------- re-arming watches

def parse_set_watches(raw):
    xid, op, p = parse_header(raw)
    rel = struct.unpack(">q", p[:8])[0]
    pos = 8
    vecs = []
    for _ in range(3):
        n = struct.unpack(">i", p[pos:pos + 4])[0]
        pos += 4
        items = []
        for _ in range(n):
            ln = struct.unpack(">i", p[pos:pos + 4])[0]
            items.append(p[pos + 4:pos + 4 + ln].decode())
            pos += 4 + ln
        vecs.append(items)
    assert pos == len(p), "bytes after the three path vectors"
    return xid, op, rel, vecs


def watch_responder():
    """exists on a path under /absent answers NO_NODE, everything else OK."""
    resp = Responder()
    ok = canned(resp)

    def on_request(conn, xid, op, payload):
        if op == OP_EXISTS and first_string(payload).startswith(b"/absent"):
            return reply(xid, resp.zxid(), -101)
        return ok(conn, xid, op, payload)

    resp.on_request = on_request
    return resp


def test_set_watches_follows_a_same_session_reconnect():
    resp = watch_responder()
    with session(resp) as (srv, c):
        assert c.exists("/w1", True)[0] == ra.ZOK          # data watch
        assert c.exists("/absent/w2", True)[0] == ra.ZNONODE  # exist watch
        assert c.get("/w3", True)[0] == ra.ZOK             # data watch
        assert c.get_children("/w4", True)[0] == ra.ZOK    # child watch
        assert c.exists("/w5", False)[0] == ra.ZOK         # no watch asked for
        highest = resp.zxid() - 1  # the zxid of the last reply sent
        reconnect(srv, c, 0)
        assert wait_for(lambda: len(srv.frames(1)) >= 2, timeout=5)
        xid, op, rel, (data, exist, child) = parse_set_watches(srv.frames(1)[1])
        assert (xid, op) == (XID_SETWATCHES, OP_SETWATCHES) == (-8, 101)
        assert rel == highest == 5
        for v in (data, exist, child):
            assert len(v) == len(set(v))
        assert set(data) == {"/w1", "/w3"}
        assert set(exist) == {"/absent/w2"}
        assert set(child) == {"/w4"}
        # the session goes on: the next request takes the next xid
        assert c.delete_("/z") == ra.ZOK
        assert srv.frames(1)[2] == request(6, OP_DELETE, zk_string("/z") + struct.pack(">i", -1))


def test_fired_watches_are_not_sent_again():
    """One-shot semantics by event type: NodeDataChanged consumes the data
    watch, NodeChildrenChanged only the child watch, NodeDeleted all three."""
    with session(watch_responder()) as (srv, c):
        assert c.get("/fired", True)[0] == ra.ZOK
        assert c.get("/kept", True)[0] == ra.ZOK
        # /p: data and child watch; /absent/q: exist, data and child watch
        assert c.get("/p", True)[0] == ra.ZOK
        assert c.get_children("/p", True)[0] == ra.ZOK
        assert c.exists("/absent/q", True)[0] == ra.ZNONODE
        assert c.get("/absent/q", True)[0] == ra.ZOK
        assert c.get_children("/absent/q", True)[0] == ra.ZOK
        conn = srv.accepted()[0]
        conn.send_raw(watch_event(EV_CHANGED, "/fired") + watch_event(EV_CHILD, "/p") +
                      watch_event(EV_DELETED, "/absent/q"))
        seen = []
        assert wait_for(lambda: seen.extend(c.poll_watches()) or len(seen) == 3, timeout=5)
        assert seen == [{"type": "changed", "path": "/fired"}, {"type": "child", "path": "/p"},
                        {"type": "deleted", "path": "/absent/q"}]
        reconnect(srv, c, 0)
        assert wait_for(lambda: len(srv.frames(1)) >= 2, timeout=5)
        xid, op, rel, (data, exist, child) = parse_set_watches(srv.frames(1)[1])
        assert (xid, op) == (XID_SETWATCHES, OP_SETWATCHES)
        assert set(data) == {"/kept", "/p"}
        assert exist == []
        assert child == []


# ----------------------------------------------------------- decoding replies

# eleven distinct values; the 64-bit fields above 2^31 (and one above 2^62)
STAT = dict(czxid=(1 << 33) + 1, mzxid=(1 << 34) + 2, ctime=(1 << 40) + 3, mtime=(1 << 41) + 4, version=5,
            cversion=6, aversion=7, ephemeralOwner=(1 << 62) + 8, dataLength=9, numChildren=10,
            pzxid=(1 << 35) + 11)
# the bindings' Stat dict has every field but aversion
STAT_DICT = {k: v for k, v in STAT.items() if k != "aversion"}


def test_stat_fields_through_exists_get_and_set():
    def on_request(conn, xid, op, payload):
        if op == OP_GET:
            return reply(xid, 1, 0, zk_string(b"payload") + stat(**STAT))
        return reply(xid, 1, 0, stat(**STAT))

    assert len(set(STAT.values())) == 11
    with session(Responder(on_request)) as (srv, c):
        rc, st = c.exists("/s")
        assert rc == ra.ZOK and st == STAT_DICT
        rc, data, st = c.get("/s")
        assert rc == ra.ZOK and data == b"payload" and st == STAT_DICT
        # set() hands back the rc alone; the 68-byte body must still be taken
        # whole, or the next reply would not parse
        assert c.set("/s", b"v") == ra.ZOK
        rc, st = c.exists("/s")
        assert rc == ra.ZOK and st == STAT_DICT


@pytest.mark.parametrize("length", [0, -1])
def test_get_empty_and_null_buffer(length):
    def on_request(conn, xid, op, payload):
        return reply(xid, 1, 0, struct.pack(">i", length) + stat(**STAT))

    with session(Responder(on_request)) as (srv, c):
        assert c.get("/n") == (ra.ZOK, b"", STAT_DICT)


@pytest.mark.parametrize("names", [[], ["a", "bb", "c-0000000003"]])
def test_get_children_names(names):
    with session(Responder(lambda conn, xid, op, payload: reply(xid, 1, 0, zk_vector(names)))) as (srv, c):
        assert c.get_children("/d") == (ra.ZOK, names)


def test_create_returns_the_servers_path():
    # a SEQUENCE create answers with a path that differs from the request
    with session(Responder(lambda conn, xid, op, payload: reply(xid, 1, 0, zk_string("/q/n-0000000007")))) \
            as (srv, c):
        assert c.create("/q/n-", b"") == (ra.ZOK, "/q/n-0000000007")


# every error code the bindings name, with ZooKeeper's number for it
ERROR_CODES = {"ZNONODE": -101, "ZNODEEXISTS": -110, "ZNOTEMPTY": -111, "ZBADVERSION": -103,
               "ZSESSIONEXPIRED": -112, "ZCONNECTIONLOSS": -4, "ZNOCHILDRENFOREPHEMERALS": -108}


def test_the_bindings_name_these_error_codes():
    named = {n for n in dir(ra._core) if n.startswith("Z") and n.isupper() and isinstance(getattr(ra, n, None), int)}
    assert named == set(ERROR_CODES) | {"ZOK"}
    assert ra.ZOK == 0


@pytest.mark.parametrize("name", sorted(ERROR_CODES))
def test_error_code_in_a_header_only_reply(name):
    code = ERROR_CODES[name]
    assert getattr(ra, name) == code
    zero = {k: 0 for k in STAT_DICT}
    with session(Responder(lambda conn, xid, op, payload: reply(xid, 1, code))) as (srv, c):
        assert c.create("/e", b"") == (code, "")
        assert c.delete_("/e") == code
        assert c.exists("/e") == (code, zero)
        assert c.get("/e") == (code, b"", zero)
        assert c.set("/e", b"") == code
        assert c.get_children("/e") == (code, [])
        assert c.exists_many(["/e", "/f"]) == [code, code]
        assert c.state() == "connected"
        assert len(srv.accepted()) == 1


def test_multi_reply_success_and_abort():
    """MultiResponse as ZooKeeper shapes it. Success: MultiHeader{type, false,
    0} and the op's result (create: the path; delete: nothing). Abort: every
    op is an ErrorResult, MultiHeader{-1, false, err} and an int body: 0 before
    the failing op, its code at it, RUNTIMEINCONSISTENCY (-2) after it; the
    reply header carries the first non-zero code. Both end {-1, true, -1}."""
    end = struct.pack(">ibi", -1, 1, -1)
    bodies = iter([
        (0, struct.pack(">ibi", OP_CREATE, 0, 0) + zk_string("/m/a") + struct.pack(">ibi", OP_DELETE, 0, 0) +
         struct.pack(">ibi", OP_CREATE, 0, 0) + zk_string("/m/c") + end),
        (-110, b"".join(struct.pack(">ibi", -1, 0, e) + struct.pack(">i", e) for e in (0, -110, -2)) + end),
    ])

    def on_request(conn, xid, op, payload):
        err, body = next(bodies)
        return reply(xid, 1, err, body)

    ops = [("create", "/m/a", b"1"), ("delete", "/m/b"), ("create", "/m/c", b"3")]
    with session(Responder(on_request)) as (srv, c):
        assert c.multi(ops) == (ra.ZOK, [0, 0, 0])
        ops[1] = ("create", "/m/a", b"dup")
        assert c.multi(ops) == (ra.ZNODEEXISTS, [0, ra.ZNODEEXISTS, -2])


@pytest.mark.parametrize("read_only", [None, False, True])
def test_connect_response_with_and_without_read_only_byte(read_only):
    resp = canned_responder(timeout_ms=20000, session_id=0x7766554433221100, read_only=read_only)
    with session(resp) as (srv, c):
        assert c.session_id() == 0x7766554433221100
        assert c.session_timeout_ms() == 20000
        assert [e["type"] for e in c.poll_events()] == ["connect"]
        # the reply stream is in step after either form
        assert c.create("/ro", b"") == (ra.ZOK, "/ro")


def test_reply_delivered_one_byte_at_a_time():
    def on_request(conn, xid, op, payload):
        conn.send_bytewise(reply(xid, 1, 0, zk_string(b"slow") + stat(**STAT)))

    with session(Responder(on_request)) as (srv, c):
        assert c.get("/slow") == (ra.ZOK, b"slow", STAT_DICT)
        assert c.get("/slow") == (ra.ZOK, b"slow", STAT_DICT)


def test_three_replies_and_a_watch_event_in_one_send():
    def script(conn):
        conn.handshake()
        xids = [conn.read_request(timeout=3.0)[0] for _ in range(3)]
        conn.send_raw(reply(xids[0], 1, 0, stat(**STAT)) + reply(xids[1], 2, -101) +
                      watch_event(EV_CHILD, "/burst") + reply(xids[2], 3, 0, stat(**STAT)))
        Responder().serve(conn)

    with session(script) as (srv, c):
        assert c.exists_many(["/1", "/2", "/3"]) == [ra.ZOK, ra.ZNONODE, ra.ZOK]
        assert c.poll_watches() == [{"type": "child", "path": "/burst"}]
