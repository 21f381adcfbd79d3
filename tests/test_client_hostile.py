"""The native ZooKeeper client against a server that misbehaves.

The peer is tests/scripted_server.py. Every blocking client call runs in a
daemon thread that is joined with a timeout, so a call that never returns
fails its test instead of hanging the suite; every client is closed from the
main thread.

A malformed reply costs the connection, not the caller: the call returns
ZCONNECTIONLOSS (the code the caller already handles for a dropped
connection, and the one the bindings export), and the client reconnects on
the same session."""
import json
import struct
import threading
import time

import pytest

import registrar_amd as ra
from conftest import free_port, wait_for
from scripted_server import (
    DEFAULT_PASSWD, DEFAULT_SESSION, OP_EXISTS, Responder, ScriptedServer, accept_and_close, connect_request,
    connect_response, frame, read_and_close, reply, reply_two_byte_frame, request, stat, zk_string, zk_vector)
from test_client_wire import SESSION_TIMEOUT, canned, canned_responder, session, start_client

JOIN_TIMEOUT = 5.0


def blocking(fn, *args):
    """fn(*args) in a daemon thread; fails if it has not returned in time.
    Returns (value, monotonic time of the return)."""
    box = {}

    def run():
        box["value"] = fn(*args)
        box["at"] = time.monotonic()

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(JOIN_TIMEOUT)
    assert not t.is_alive(), "the call did not return within %.0f s" % JOIN_TIMEOUT
    return box["value"], box["at"]


def event_types(c):
    return [e["type"] for e in c.poll_events()]


class BadFirstReply(Responder):
    """Connection 0: the handshake, then `bad(xid)` in answer to the first
    request and nothing more. Later connections: a well-behaved server."""

    def __init__(self, bad, **handshake):
        super().__init__(**handshake)
        self.on_request = canned(self)
        self.bad = bad

    def __call__(self, conn):
        conn.handshake(**self.handshake_args)
        if conn.index == 0:
            xid, op, payload = conn.read_request()
            conn.send_raw(self.bad(xid))
            conn.wait_eof()
        else:
            self.serve(conn)


def check_dropped_and_resumed(srv, c, last_zxid):
    """After a reply that cost the connection: one `close`, a reconnect that
    carries the same session, and a client that serves the next call."""
    assert wait_for(lambda: len(srv.accepted()) == 2 and c.state() == "connected", timeout=5)
    assert event_types(c) == ["close", "connect"]
    assert srv.frames(1)[0] == connect_request(SESSION_TIMEOUT, last_zxid=last_zxid, session_id=DEFAULT_SESSION,
                                               passwd=DEFAULT_PASSWD)
    (rc, st), _ = blocking(c.exists, "/next")
    assert rc == ra.ZOK and st["version"] == 1
    assert len(srv.accepted()) == 2


# ------------------------------------------- 1. malformed bodies of OK replies

GOOD_BODY = {
    "create": zk_string("/x"),
    "exists": stat(version=1),
    "get": zk_string(b"abc") + stat(version=1),
    "set": stat(version=1),
    "get_children": zk_vector(["a", "b"]),
    "exists_many": stat(version=1),
}
CALL = {
    "create": lambda c: c.create("/x", b"")[0],
    "exists": lambda c: c.exists("/x")[0],
    "get": lambda c: c.get("/x")[0],
    "set": lambda c: c.set("/x", b"v"),
    "get_children": lambda c: c.get_children("/x")[0],
    "exists_many": lambda c: c.exists_many(["/x"], stats=True)[0][0],
}
HUGE_STRING = struct.pack(">i", 1 << 30) + b"abc"
MALFORMED = [(verb, "empty", b"") for verb in sorted(GOOD_BODY)]
MALFORMED += [(verb, "one_byte_short", GOOD_BODY[verb][:-1]) for verb in sorted(GOOD_BODY)]
MALFORMED += [
    ("create", "string_len_1<<30", HUGE_STRING),
    ("get", "string_len_1<<30", HUGE_STRING),
    ("get_children", "string_len_1<<30", struct.pack(">i", 1) + HUGE_STRING),
    ("get_children", "count_1<<28", struct.pack(">i", 1 << 28) + zk_string("a")),
]


@pytest.mark.parametrize("verb,kind,body", MALFORMED, ids=["%s-%s" % (v, k) for v, k, _ in MALFORMED])
def test_ok_reply_with_malformed_body_returns_connection_loss(verb, kind, body):
    with session(BadFirstReply(lambda xid: reply(xid, 1, 0, body))) as (srv, c):
        assert event_types(c) == ["connect"]
        rc, _ = blocking(CALL[verb], c)
        assert rc == ra.ZCONNECTIONLOSS
        check_dropped_and_resumed(srv, c, last_zxid=1)


def test_well_formed_bodies_of_the_same_calls():
    # the control for the table above: the same calls, the uncut bodies
    def on_request(conn, xid, op, payload):
        return reply(xid, 1, 0, bodies.pop(0))

    verbs = sorted(GOOD_BODY)
    bodies = [GOOD_BODY[v] for v in verbs]
    with session(Responder(on_request)) as (srv, c):
        for v in verbs:
            assert blocking(CALL[v], c)[0] == ra.ZOK
        rcs, stats = c.exists_many([], stats=True)
        assert (rcs, stats) == ([], [])
        assert len(srv.accepted()) == 1


# ------------------- 2. the connection dies before the handshake, no session

PRE_HANDSHAKE = {
    "accept_and_close": accept_and_close,
    "read_request_and_close": read_and_close,
    "two_byte_frame": reply_two_byte_frame,
}
INITIAL_MS, MAX_MS = 200, 400


def pre_handshake_client(srv, **kw):
    c = ra.ZkClient(servers=[srv.addr], connect_initial_delay_ms=INITIAL_MS, connect_max_delay_ms=MAX_MS,
                    connect_timeout_ms=2000, randomize_start=False, **kw)
    c.start()
    return c


@pytest.mark.parametrize("variant", sorted(PRE_HANDSHAKE))
def test_no_session_death_before_handshake_backs_off(variant):
    """Backoff has no jitter: with delays 200, 400, 400, ... a window of W ms
    that opens at the first accept holds at most 1 + W/200 connections, plus
    one for the window's edge."""
    window = 1.0
    srv = ScriptedServer(PRE_HANDSHAKE[variant], inline=True)
    c = None
    try:
        c = pre_handshake_client(srv)
        assert wait_for(lambda: len(srv.accepted()) >= 1, timeout=5, interval=0.002)
        t0 = srv.accepted()[0].accepted_at
        time.sleep(max(0.0, t0 + window - time.monotonic()) + 0.02)
        conns = srv.accepted()
        events = c.poll_events()
        in_window = sum(1 for k in conns if k.accepted_at - t0 <= window)
        print("connections in %.1f s: %d" % (window, in_window))
        assert in_window <= 1 + window * 1000 / INITIAL_MS + 1
        assert in_window >= 2, "the client stopped retrying"
        attempts = [e for e in events if e["type"] == "attempt"]
        assert len(attempts) >= 2
        assert [e["attempt"] for e in attempts] == list(range(1, len(attempts) + 1))
        assert [e["delay_ms"] for e in attempts] == ([INITIAL_MS] + [MAX_MS] * len(attempts))[:len(attempts)]
        # nothing was ever connected, so nothing is ever closed
        assert {e["type"] for e in events} == {"attempt"}
        assert c.state() == "connecting"
    finally:
        if c is not None:
            c.close()
        srv.stop()


@pytest.mark.parametrize("variant", sorted(PRE_HANDSHAKE))
def test_no_session_death_before_handshake_exhausts_attempts(variant):
    srv = ScriptedServer(PRE_HANDSHAKE[variant], inline=True)
    c = None
    try:
        c = pre_handshake_client(srv, connect_max_attempts=3)
        # three retries, 200 + 400 + 400 ms apart, then the client gives up
        assert c.wait_connected(3000) is False
        assert c.state() == "closed"
        assert event_types(c) == ["attempt", "attempt", "attempt", "closed"]
        assert len(srv.accepted()) == 4
    finally:
        if c is not None:
            c.close()
        srv.stop()


# -------------------------------------------- 3. the same, with a session

def test_with_session_death_before_handshake_uses_reconnect_backoff():
    """An established session whose server then accepts and closes for 2 s.
    The first retry after the loss is immediate; each later one waits the
    reconnect backoff, 10 ms doubling to 1 s, which only a completed
    handshake resets. Connections in the outage: the delays whose running sum
    fits in it, plus two (the immediate retry, and the window's edge)."""
    outage = 2.0
    delays, d = [], 10
    while len(delays) < 16:
        delays.append(min(d, 1000))
        d *= 2
    fit, total = 0, 0
    for d in delays:
        total += d
        if total <= outage * 1000:
            fit += 1
    assert fit == 7  # 10+20+40+80+160+320+640 = 1270; the 1000 after it does not fit
    good = canned_responder()
    srv = ScriptedServer(good)
    c = None
    try:
        c = start_client(srv)
        assert c.wait_connected(5000)
        assert event_types(c) == ["connect"]
        srv.set_script(accept_and_close, inline=True)
        t0 = time.monotonic()
        srv.accepted()[0].close()
        time.sleep(outage)
        srv.set_script(good)
        assert wait_for(lambda: c.state() == "connected", timeout=5, interval=0.005)
        conns = srv.accepted()
        in_outage = sum(1 for k in conns[1:] if t0 <= k.accepted_at <= t0 + outage)
        print("connections in the %.0f s outage: %d" % (outage, in_outage))
        assert in_outage <= fit + 2
        events = c.poll_events()
        types = [e["type"] for e in events]
        assert types[0] == "close" and types[-1] == "connect"
        assert types.count("close") == 1 and types.count("connect") == 1
        attempts = [e for e in events if e["type"] == "attempt"]
        assert len(attempts) == len(events) - 2
        # one rising sequence for the whole outage: an accepted connection
        # that dies before the handshake does not start the backoff over
        assert 6 <= len(attempts) <= fit + 2
        assert [e["attempt"] for e in attempts] == list(range(1, len(attempts) + 1))
        assert [e["delay_ms"] for e in attempts] == delays[:len(attempts)]
        # the good handshake resumed the session it was asked for
        assert conns[-1].frames[0] == connect_request(SESSION_TIMEOUT, last_zxid=0, session_id=DEFAULT_SESSION,
                                                      passwd=DEFAULT_PASSWD)
        assert c.session_id() == DEFAULT_SESSION
        # ... and reset the backoff: the next outage starts at attempt 1 again
        n = len(conns)
        srv.set_script(accept_and_close, inline=True)
        conns[-1].close()
        assert wait_for(lambda: len(srv.accepted()) >= n + 2, timeout=5, interval=0.002)
        srv.set_script(good)
        assert wait_for(lambda: c.state() == "connected", timeout=5, interval=0.005)
        events = c.poll_events()
        assert [(e["type"], e["attempt"], e["delay_ms"]) for e in events[:2]] == [("close", 0, 0), ("attempt", 1, 10)]
        (rc, _), _ = blocking(c.exists, "/after")
        assert rc == ra.ZOK
    finally:
        if c is not None:
            c.close()
        srv.stop()


def test_reconnect_delay_leaves_room_for_a_turn_through_the_server_list():
    """With a session waiting, a retry delay is never more than a third of
    the session timeout divided by the number of addresses: whenever service
    comes back, the client has been through the whole list, dead addresses
    included, with two thirds of the timeout to spare. 600 ms and two
    addresses: 10, 20, 40, 80, then 100 and no more."""
    good = canned_responder(timeout_ms=600)
    srv = ScriptedServer(good)
    c = None
    try:
        c = ra.ZkClient(servers=[srv.addr, ("127.0.0.1", free_port())], session_timeout_ms=600,
                        randomize_start=False)
        c.start()
        assert c.wait_connected(5000)
        assert event_types(c) == ["connect"]
        srv.set_script(accept_and_close, inline=True)
        srv.accepted()[0].close()
        events = []
        assert wait_for(lambda: events.extend(c.poll_events()) or
                        sum(1 for e in events if e["type"] == "attempt") >= 7, timeout=5, interval=0.005)
        attempts = [e for e in events if e["type"] == "attempt"]
        assert [e["delay_ms"] for e in attempts][:7] == [10, 20, 40, 80, 100, 100, 100]
        assert [e["type"] for e in events].count("close") == 1
    finally:
        if c is not None:
            c.close()
        srv.stop()


# ---------------------------- 4. accepts, never answers the handshake

def test_unanswered_handshake_times_out_and_the_next_address_is_tried():
    def never_answers(conn):
        conn.read_frame()
        conn.wait_eof()

    silent = ScriptedServer(never_answers)
    good = ScriptedServer(canned_responder())
    c = None
    try:
        c = ra.ZkClient(servers=[silent.addr, good.addr], session_timeout_ms=SESSION_TIMEOUT, connect_timeout_ms=300,
                        connect_initial_delay_ms=50, connect_max_delay_ms=100, randomize_start=False)
        c.start()
        assert c.wait_connected(5000)
        assert event_types(c) == ["attempt", "connect"]
        assert len(silent.accepted()) == 1 and len(good.accepted()) == 1
        gap = good.accepted()[0].accepted_at - silent.accepted()[0].accepted_at
        print("gave up on the silent server after %.3f s" % gap)
        # connect_timeout_ms, then the first backoff delay, then the next address
        assert 0.300 <= gap < 0.350 + 0.5
        assert silent.frames(0) == [connect_request(SESSION_TIMEOUT)]
        assert wait_for(lambda: silent.accepted()[0].eof, timeout=5)
        assert good.frames(0)[0] == connect_request(SESSION_TIMEOUT)
    finally:
        if c is not None:
            c.close()
        silent.stop()
        good.stop()


# ---------------------------- 5. silent after the handshake, T = 900 ms

class SleepLateness(threading.Thread):
    """The worst lateness of a plain 20 ms time.sleep while it runs: what
    this machine's scheduler adds to any timer in the same run."""

    def __init__(self):
        super().__init__(daemon=True)
        self.worst = 0.0
        self.stopping = False

    def run(self):
        while not self.stopping:
            t = time.monotonic()
            time.sleep(0.02)
            self.worst = max(self.worst, time.monotonic() - t - 0.02)


def test_silent_server_is_given_up_between_two_thirds_and_the_whole_timeout():
    """The client presumes a server dead that has sent nothing for 2T/3, and
    notices on a ping tick (every T/3). The blocked call's ZCONNECTIONLOSS and
    the `close` event must come no earlier than 2T/3 after the last byte the
    server sent (taken just before that send) and no later than T plus a
    scheduling margin. Margin: five times the worst lateness of a plain 20 ms
    time.sleep measured alongside (the event is also found by polling every
    millisecond with time.sleep, which that lateness covers)."""
    T = 0.9

    def script(conn):
        conn.handshake(timeout_ms=900)
        while True:
            conn.read_frame(timeout=5.0)  # takes everything, answers nothing

    srv = ScriptedServer(script)
    lateness = SleepLateness()
    c = None
    try:
        lateness.start()
        c = start_client(srv, session_timeout_ms=900)
        assert c.wait_connected(5000)
        assert c.session_timeout_ms() == 900
        assert event_types(c) == ["connect"]
        t_sent = srv.accepted()[0].last_send
        box = {}

        def call():
            box["rc"] = c.exists("/blocked")[0]
            box["at"] = time.monotonic()

        t = threading.Thread(target=call, daemon=True)
        t.start()
        t_close = None
        deadline = time.monotonic() + 3.0
        while t_close is None and time.monotonic() < deadline:
            if any(e["type"] == "close" for e in c.poll_events()):
                t_close = time.monotonic()
            else:
                time.sleep(0.001)
        t.join(JOIN_TIMEOUT)
        assert not t.is_alive(), "exists did not return"
        lateness.stopping = True
        lateness.join(1)
        margin = 5 * lateness.worst
        print("exists returned %.4f s, close event seen %.4f s after the server's last byte; margin %.4f s"
              % (box["at"] - t_sent, (t_close or 0) - t_sent, margin))
        assert box["rc"] == ra.ZCONNECTIONLOSS
        assert t_close is not None, "no close event"
        for at in (box["at"], t_close):
            assert 2 * T / 3 <= at - t_sent <= T + margin
    finally:
        lateness.stopping = True
        if c is not None:
            c.close()
        srv.stop()


# ---------------------------------------- 6. frame and reply anomalies

ANOMALY = {
    "frame_length_-1": lambda xid: struct.pack(">i", -1),
    "frame_length_0x7fffffff": lambda xid: struct.pack(">i", 0x7FFFFFFF),
    "frame_length_64MiB+1": lambda xid: struct.pack(">i", 64 * 1024 * 1024 + 1),
    "wrong_xid": lambda xid: reply(xid + 5, 1, 0, stat(version=1)),
    # xid -1, then a WatcherEvent cut inside its path
    "truncated_watch_event": lambda xid: frame(struct.pack(">iqi", -1, -1, 0) + struct.pack(">ii", 3, 3) +
                                               struct.pack(">i", 10) + b"/ab"),
}
# a reply header is taken in before its xid is matched, a frame length is not
ANOMALY_ZXID = {"wrong_xid": 1}


@pytest.mark.parametrize("name", sorted(ANOMALY))
def test_anomaly_fails_the_call_in_flight_and_reconnects(name):
    with session(BadFirstReply(ANOMALY[name])) as (srv, c):
        assert event_types(c) == ["connect"]
        (rc, _), _ = blocking(c.exists, "/x")
        assert rc == ra.ZCONNECTIONLOSS
        check_dropped_and_resumed(srv, c, last_zxid=ANOMALY_ZXID.get(name, 0))


def test_reply_when_nothing_is_pending_drops_the_connection():
    def script(conn):
        conn.handshake()
        if conn.index == 0:
            assert go.wait(5)
            conn.send_raw(reply(99, 1, 0))
            conn.wait_eof()
        else:
            canned_responder().serve(conn)

    go = threading.Event()
    with session(script) as (srv, c):
        assert event_types(c) == ["connect"]
        go.set()
        check_dropped_and_resumed(srv, c, last_zxid=1)


# ------------------------------ 7. replies through the batch-record path

def test_wrong_xid_in_the_middle_of_a_batch_record_run():
    """PreparedRegistration.heartbeat sends its exists run as one pre-built
    batch answered through a single pending record. Reply 0 is good, reply 1
    carries a wrong xid: the rest of the run fails with ZCONNECTIONLOSS and
    the caller returns."""
    reg = {"domain": "a.b.c", "type": "host", "adminIp": "127.0.0.1", "hostname": "h",
           "aliases": ["x.b.c", "y.b.c", "z.b.c"]}
    prep = ra.PreparedRegistration(json.dumps(reg))
    nodes = prep.nodes
    assert nodes == ["/c/b/a/h", "/c/b/x", "/c/b/y", "/c/b/z"]

    def script(conn):
        conn.handshake()
        if conn.index == 0:
            xids = [conn.read_request(timeout=3.0)[0] for _ in nodes]
            conn.send_raw(reply(xids[0], 1, 0, stat(version=1)) + reply(xids[1] + 7, 2, 0, stat(version=1)))
            conn.wait_eof()
        else:
            canned_responder().serve(conn)

    with session(script) as (srv, c):
        assert event_types(c) == ["connect"]
        (rc, _), _ = blocking(prep.heartbeat, c, {"maxAttempts": 0})
        assert rc == ra.ZCONNECTIONLOSS
        assert srv.frames(0)[1:] == [request(1 + i, OP_EXISTS, zk_string(n) + b"\x00") for i, n in enumerate(nodes)]
        assert wait_for(lambda: len(srv.accepted()) == 2 and c.state() == "connected", timeout=5)
        assert event_types(c) == ["close", "connect"]
        # the same template again, on the new connection, with fresh xids
        (rc, _), _ = blocking(prep.heartbeat, c, {"maxAttempts": 0})
        assert rc == ra.ZOK
        assert srv.frames(1)[1:] == [request(5 + i, OP_EXISTS, zk_string(n) + b"\x00") for i, n in enumerate(nodes)]


# ---------------------------------- 8. session refused on reconnect

def test_session_refused_on_reconnect_is_expiry_and_the_end():
    def script(conn):
        if conn.index == 0:
            canned_responder()(conn)
        else:
            conn.read_frame()
            conn.send_raw(connect_response(0, 0, bytes(16)))  # sessionId 0: the session is gone
            conn.wait_eof()

    with session(script) as (srv, c):
        assert event_types(c) == ["connect"]
        srv.accepted()[0].close()
        assert wait_for(lambda: c.state() == "expired", timeout=5)
        assert srv.frames(1)[0] == connect_request(SESSION_TIMEOUT, session_id=DEFAULT_SESSION, passwd=DEFAULT_PASSWD)
        time.sleep(0.1)  # ten times the first reconnect delay
        assert event_types(c) == ["close", "session_expired"]
        assert len(srv.accepted()) == 2
        (rc, _), _ = blocking(c.exists, "/x")
        assert rc == ra.ZSESSIONEXPIRED
