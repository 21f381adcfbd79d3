"""ZkClient.get_many against the scripted server: N getData requests in one
submission, completed as a unit."""
import contextlib
import struct
import threading

import pytest

import registrar_amd as ra
from conftest import make_client, wait_for
from scripted_server import (
    OP_GET, OP_SETWATCHES, XID_SETWATCHES, Responder, ScriptedServer, parse_header, reply, request,
    stat, zk_string)

SESSION_TIMEOUT = 30000  # long: no ping lands between the frames under test

# eleven distinct values, the 64-bit ones above 2^31
STAT = dict(czxid=(1 << 33) + 1, mzxid=(1 << 34) + 2, ctime=(1 << 40) + 3, mtime=(1 << 41) + 4, version=5,
            cversion=6, aversion=7, ephemeralOwner=(1 << 62) + 8, dataLength=9, numChildren=10,
            pzxid=(1 << 35) + 11)
STAT_DICT = {k: v for k, v in STAT.items() if k != "aversion"}  # the bindings leave aversion out
ZERO_STAT = {k: 0 for k in STAT_DICT}
NULL_BUFFER = struct.pack(">i", -1)


@contextlib.contextmanager
def session(script):
    srv = ScriptedServer(script)
    c = None
    try:
        c = ra.ZkClient(servers=[srv.addr], randomize_start=False, session_timeout_ms=SESSION_TIMEOUT)
        c.start()
        assert c.wait_connected(5000), "client did not connect to the scripted server"
        yield srv, c
    finally:
        if c is not None:
            c.close()
        srv.stop()


def first_string(payload):
    n = struct.unpack(">i", payload[:4])[0]
    return payload[4:4 + n].decode()


def get_responder(answers):
    """getData answered from `answers`: path -> (err, body)."""
    resp = Responder()

    def on_request(conn, xid, op, payload):
        if op == OP_GET:
            err, body = answers[first_string(payload)]
            return reply(xid, resp.zxid(), err, body)
        return reply(xid, resp.zxid(), 0)

    resp.on_request = on_request
    return resp


def get_body(path, watch):
    return zk_string(path) + (b"\x01" if watch else b"\x00")


def requests_of(srv, index):
    """Raw frames of connection `index` after the ConnectRequest."""
    return srv.frames(index)[1:]


@pytest.mark.parametrize("watch", [False, True])
@pytest.mark.parametrize("n", [0, 1, 3])
def test_request_bytes(n, watch):
    paths = ["/d/p%d" % i for i in range(n)]
    answers = {p: (0, zk_string(b"x") + stat()) for p in paths}
    with session(get_responder(answers)) as (srv, c):
        rcs, datas, stats = c.get_many(paths, watch)
        assert rcs == [0] * n and len(datas) == n and len(stats) == n
        # a verb after it: everything get_many sent is in front of this frame,
        # and it takes the xid after the batch's last
        assert c.delete_("/z") == ra.ZOK
        assert wait_for(lambda: len(requests_of(srv, 0)) == n + 1, timeout=5)
        sent = requests_of(srv, 0)
        assert sent[:n] == [request(1 + i, OP_GET, get_body(paths[i], watch)) for i in range(n)]
        assert parse_header(sent[n])[0] == n + 1


def test_replies_data_empty_null_and_no_node_in_the_middle():
    answers = {
        "/r/data": (0, zk_string(b"payload \x00\xff bytes") + stat(**STAT)),
        "/r/empty": (0, zk_string(b"") + stat(version=3)),
        "/r/gone": (-101, b""),
        "/r/null": (0, NULL_BUFFER + stat(version=4)),
    }
    paths = ["/r/data", "/r/empty", "/r/gone", "/r/null"]
    with session(get_responder(answers)) as (srv, c):
        rcs, datas, stats = c.get_many(paths)
        assert rcs == [ra.ZOK, ra.ZOK, ra.ZNONODE, ra.ZOK]
        assert datas == [b"payload \x00\xff bytes", b"", b"", b""]
        assert stats[0] == STAT_DICT
        assert stats[1]["version"] == 3 and stats[3]["version"] == 4
        assert stats[2] == ZERO_STAT


def parse_set_watches(raw):
    xid, op, p = parse_header(raw)
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
    assert pos == len(p)
    return xid, op, vecs


def test_watch_is_armed_for_the_ok_paths_only():
    answers = {
        "/w/a": (0, zk_string(b"a") + stat()),
        "/w/gone": (-101, b""),
        "/w/c": (0, zk_string(b"c") + stat()),
        "/w/unwatched": (0, zk_string(b"u") + stat()),
    }
    with session(get_responder(answers)) as (srv, c):
        assert c.get_many(["/w/unwatched"], False)[0] == [ra.ZOK]
        assert c.get_many(["/w/a", "/w/gone", "/w/c"], True)[0] == [ra.ZOK, ra.ZNONODE, ra.ZOK]
        srv.accepted()[0].close()  # forced same-session reconnect
        assert wait_for(lambda: len(srv.frames(1)) >= 2 and c.state() == "connected", timeout=5)
        xid, op, (data, exist, child) = parse_set_watches(srv.frames(1)[1])
        assert (xid, op) == (XID_SETWATCHES, OP_SETWATCHES)
        assert sorted(data) == ["/w/a", "/w/c"]
        assert exist == [] and child == []


def test_truncated_body_in_reply_two_of_three_fails_the_batch_once():
    """Reply 2 carries a buffer length that runs past the end of its frame:
    the connection is dropped, every rc of the batch is CONNECTION_LOSS (the
    first reply's good answer included), the call returns exactly once, and
    the client reconnects with its session."""
    good = zk_string(b"fine") + stat(version=1)
    resp = Responder()

    def on_request(conn, xid, op, payload):
        if op != OP_GET:
            return reply(xid, resp.zxid(), 0)
        path = first_string(payload)
        if conn.index == 0 and path == "/t/2":
            return reply(xid, resp.zxid(), 0, struct.pack(">i", 100) + b"short")
        return reply(xid, resp.zxid(), 0, good)

    resp.on_request = on_request
    with session(resp) as (srv, c):
        results = []
        t = threading.Thread(target=lambda: results.append(c.get_many(["/t/1", "/t/2", "/t/3"], True)), daemon=True)
        t.start()
        t.join(10)
        assert not t.is_alive(), "get_many did not return after a malformed reply body"
        assert len(results) == 1
        rcs, datas, stats = results[0]
        assert rcs == [ra.ZCONNECTIONLOSS] * 3
        assert datas == [b"", b"", b""]
        assert stats == [ZERO_STAT] * 3
        assert wait_for(lambda: len(srv.accepted()) >= 2 and c.state() == "connected", timeout=5)
        # the session goes on, and the same paths read fine on the new connection
        rcs, datas, _ = c.get_many(["/t/1", "/t/2", "/t/3"])
        assert rcs == [ra.ZOK] * 3 and datas == [b"fine"] * 3


def test_get_many_on_the_ensemble_matches_get(ensemble, client):
    paths = []
    for i in range(5):
        p = "/gm%d" % i
        assert client.create(p, b"v%d" % i)[0] == ra.ZOK
        paths.append(p)
    paths.insert(2, "/gm-missing")
    rcs, datas, stats = client.get_many(paths, True)
    for p, rc, d, st in zip(paths, rcs, datas, stats):
        erc, ed, est = client.get(p)
        assert (rc, d) == (erc, ed)
        if rc == ra.ZOK:
            assert st == est
    # the watches are live: a change shows up as an event, the missing path armed nothing
    assert client.set("/gm0", b"changed") == ra.ZOK
    assert client.create("/gm-missing", b"")[0] == ra.ZOK
    seen = []
    assert wait_for(lambda: seen.extend(client.poll_watches()) or len(seen) >= 1, timeout=5)
    assert seen == [{"type": "changed", "path": "/gm0"}]


@pytest.mark.parametrize("queue", [True, False])
def test_queue_watches_off_keeps_nothing_for_poll_watches(ensemble, client, queue):
    """With queue_watches=False (what a Resolver sets on its own client) an
    event is delivered and its watch consumed, but no entry stays behind for a
    poll_watches() nobody calls. The event travels ahead of the next reply on
    the same connection, so once that reply is in, the event has been handled."""
    c = make_client(ensemble, queue_watches=queue)
    try:
        for i in range(3):
            path = "/qw%d" % i
            assert client.create(path, b"0")[0] == ra.ZOK
            assert c.get_many([path], True)[0] == [ra.ZOK]
            assert client.set(path, b"1") == ra.ZOK
        assert wait_for(lambda: c.get("/qw2")[1] == b"1", timeout=5)
        assert c.get("/qw0")[0] == ra.ZOK  # a reply behind every event
        got = c.poll_watches()
        if queue:
            assert wait_for(lambda: got.extend(c.poll_watches()) or len(got) >= 3, timeout=5)
            assert sorted(e["path"] for e in got) == ["/qw0", "/qw1", "/qw2"]
        else:
            assert got == []
    finally:
        c.close()
