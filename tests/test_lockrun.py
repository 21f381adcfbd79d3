"""Locks carried across sibling requests of one drain (docs/perf_lockrun.md).

A drain keeps its parent's shard lock and its own session's eph_mu from one
create / create2 / delete frame to the next. Nothing a client can observe may
depend on that: the same request script gives the same reply bytes whether it
arrives as one write (one drain, locks carried) or frame by frame (nothing to
carry), sessions deleting each other's ephemerals keep both indexes right, and
two IO loops working under each other's parents while a session is expired
neither deadlock nor lose a node. Every wait here has a timeout, so a deadlock
fails a test instead of hanging it. Every test ends on ens.audit() == []."""
import json
import os
import socket
import struct
import subprocess
import threading
import time

import registrar_amd as ra
from conftest import REPO_ROOT, make_client, wait_for

OP_CREATE, OP_DELETE, OP_EXISTS, OP_GETDATA, OP_SETDATA, OP_GETCHILDREN, OP_CREATE2 = 1, 2, 3, 4, 5, 8, 15
EPHEMERAL, SEQUENCE = 1, 2
STAT_LEN = 68
REPLY_HDR = 16  # xid(4) zxid(8) err(4)
ZNONODE = -101
CARRY_BOUND = 32  # Ensemble::Impl::kCarryBound


# ---------------------------------------------------------------- raw wire

def jstr(s):
    b = s if isinstance(s, bytes) else s.encode()
    return struct.pack(">i", len(b)) + b


def frame(body):
    return struct.pack(">i", len(body)) + body


ACL = struct.pack(">i", 1) + struct.pack(">i", 31) + jstr("world") + jstr("anyone")


def create_req(xid, path, data=b"", flags=0, op=OP_CREATE):
    return frame(struct.pack(">ii", xid, op) + jstr(path) + jstr(data) + ACL + struct.pack(">i", flags))


def delete_req(xid, path):
    return frame(struct.pack(">ii", xid, OP_DELETE) + jstr(path) + struct.pack(">i", -1))


def path_req(xid, op, path):
    return frame(struct.pack(">ii", xid, op) + jstr(path) + struct.pack(">?", False))


def setdata_req(xid, path, data):
    return frame(struct.pack(">ii", xid, OP_SETDATA) + jstr(path) + jstr(data) + struct.pack(">i", -1))


class Raw:
    """A session on a plain socket; every receive times out after 10 s."""

    def __init__(self, ens):
        host, port = ens.connect_string().split(",")[0].rsplit(":", 1)
        self.sock = socket.create_connection((host, int(port)), timeout=10)
        self.sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        body = struct.pack(">iqiq", 0, 0, 20000, 0) + struct.pack(">i", 16) + b"\x00" * 16
        self.sock.sendall(frame(body))
        rep = self.recv_frame()
        # ConnectResponse: protocolVersion, timeOut, sessionId, passwd
        self.sid = struct.unpack(">iiq", rep[4:20])[2]
        assert self.sid != 0

    def recv_exact(self, n):
        out = b""
        while len(out) < n:
            chunk = self.sock.recv(n - len(out))
            if not chunk:
                raise EOFError("connection closed")
            out += chunk
        return out

    def recv_frame(self):
        hdr = self.recv_exact(4)
        return hdr + self.recv_exact(struct.unpack(">i", hdr)[0])

    def replies(self, n):
        return [self.recv_frame() for _ in range(n)]

    def close(self):
        self.sock.close()


def err_of(rep):
    return struct.unpack(">iqi", rep[4:4 + REPLY_HDR])[2]


def fresh(io_threads=1):
    ens = ra.Ensemble(servers=1, tick_ms=50, min_session_timeout_ms=200, io_threads=io_threads)
    ens.start()
    return ens


# ---------------------------------------------------------------- script equality

def equality_script():
    """(frame, reply ends in a Stat) pairs. 200 children under /p, so that
    with 64 shards the children land in every shard, /p's own included. The
    first run of creates is 120 long: more than three carries of CARRY_BOUND
    plus one."""
    xid = [0]
    out = []

    def add(maker, *a, stat=False, **kw):
        xid[0] += 1
        out.append((maker(xid[0], *a, **kw), stat))

    kids = ["/p/c%03d" % i for i in range(200)]
    add(create_req, "/p", b"parent")
    add(create_req, "/q", b"other")
    assert 120 > 3 * CARRY_BOUND + 1
    for k in kids[:120]:
        add(create_req, k, b"payload", EPHEMERAL)
    # reads and a write of the carried parent itself, between creates
    add(path_req, OP_EXISTS, "/p", stat=True)
    add(create_req, kids[120], b"payload", EPHEMERAL)
    add(path_req, OP_GETDATA, "/p", stat=True)
    add(create_req, kids[121], b"payload", EPHEMERAL)
    add(setdata_req, "/p", b"parent-2", stat=True)
    for k in kids[122:150]:
        add(create_req, k, b"payload", EPHEMERAL)
    add(create_req, "/p/seq-", b"s", SEQUENCE)  # inside the run
    for k in kids[150:170]:
        add(create_req, k, b"payload", EPHEMERAL)
    for i in range(20):  # a second parent mid-run
        add(create_req, "/q/d%02d" % i, b"", EPHEMERAL)
    for k in kids[170:]:
        add(create_req, k, b"payload", EPHEMERAL)
    add(create_req, "/nope/x", b"")   # missing parent
    add(delete_req, "/p/zzz")         # missing node
    add(create_req, "/p/two", b"2", 0, op=OP_CREATE2, stat=True)
    add(create_req, kids[0], b"again", EPHEMERAL)  # NODE_EXISTS
    for i, k in enumerate(kids):
        add(delete_req, k)
        if i % 10 == 0:
            add(delete_req, "/q/d%02d" % (i // 10))
    add(path_req, OP_EXISTS, "/p", stat=True)
    add(path_req, OP_EXISTS, "/q", stat=True)
    add(path_req, OP_GETCHILDREN, "/p")
    add(path_req, OP_GETCHILDREN, "/q")
    return out


def mask(rep, has_stat):
    """ctime/mtime are wall-clock reads; everything else in a reply is a
    function of the request sequence. The Stat, where there is one, ends the
    reply."""
    if not has_stat or err_of(rep) != 0:
        return rep
    off = len(rep) - STAT_LEN + 16
    return rep[:off] + b"\x00" * 16 + rep[off + 16:]


def run_equality(script, single_write):
    ens = fresh()
    try:
        s = Raw(ens)
        if single_write:
            s.sock.sendall(b"".join(f for f, _ in script))
            reps = s.replies(len(script))
        else:
            reps = []
            for f, _ in script:
                s.sock.sendall(f)
                reps += s.replies(1)
        locks = ens.counters()["tree_locks"]
        audit = ens.audit()
        survivors = (ens.children("/p"), ens.children("/q"), ens.ephemeral_count())
        s.close()
        return [mask(r, st) for r, (_, st) in zip(reps, script)], audit, locks, survivors
    finally:
        ens.stop()


def test_script_equality():
    """One script, once as a single write (one drain carries) and once frame
    by frame (no drain carries): byte-equal replies, both trees sound."""
    script = equality_script()
    one, audit_one, locks_one, left_one = run_equality(script, True)
    each, audit_each, locks_each, left_each = run_equality(script, False)
    assert audit_one == [] and audit_each == []
    assert len(one) == len(each) == len(script)
    diff = [i for i in range(len(script)) if one[i] != each[i]]
    assert diff == [], "replies differ at frames %s" % diff[:5]
    # the reference is right, not merely equal: spot checks of its return codes
    errs = [err_of(r) for r in each]
    assert errs.count(0) == len(script) - 3
    assert sorted(e for e in errs if e != 0) == [-110, ZNONODE, ZNONODE]
    assert left_one == left_each
    assert left_each == (["seq-0000000150", "two"], [], 0)
    # and the single write did carry: far fewer lock acquisitions
    print("tree_locks: single write %d, frame by frame %d" % (locks_one, locks_each))
    assert locks_one < locks_each


# ---------------------------------------------------------------- cross-session delete

def test_cross_session_delete_in_one_batch():
    """B deletes 100 of A's ephemerals in one pipelined batch, interleaved with
    creates and deletes of its own: every delete leaves the right session's
    index, under the right eph_mu, while B's own is carried."""
    ens = fresh()
    try:
        a, b = Raw(ens), Raw(ens)
        a.sock.sendall(create_req(1, "/x"))
        assert err_of(a.recv_frame()) == 0
        a.sock.sendall(b"".join(create_req(2 + i, "/x/a%03d" % i, b"A", EPHEMERAL) for i in range(100)))
        assert [err_of(r) for r in a.replies(100)] == [0] * 100
        assert ens.ephemeral_count() == 100

        frames, kept = [], []
        for i in range(100):
            frames.append(delete_req(0, "/x/a%03d" % i))            # A's
            frames.append(create_req(0, "/x/b%03d" % i, b"B", EPHEMERAL))  # own
            if i % 3 == 0:
                frames.append(delete_req(0, "/x/b%03d" % i))        # own
            else:
                kept.append("b%03d" % i)
        b.sock.sendall(b"".join(frames))
        assert [err_of(r) for r in b.replies(len(frames))] == [0] * len(frames)

        assert ens.children("/x") == kept
        owners = [ens.get("/x/" + k)["stat"]["ephemeralOwner"] for k in kept]
        assert owners == [b.sid] * len(kept)  # B's count; A's is zero
        assert ens.ephemeral_count() == len(kept)
        assert ens.audit() == []  # each session's list length against its eph_count
        # A goes: nothing of B's may go with it
        ens.expire_session(a.sid)
        assert wait_for(lambda: a.sid not in ens.session_ids())
        assert ens.children("/x") == kept and ens.ephemeral_count() == len(kept)
        assert ens.audit() == []
        a.close()
        b.close()
    finally:
        ens.stop()


# ---------------------------------------------------------------- crossed parents

def crossed_batch(who, rnd):
    """Runs of 8 siblings under the session's own parent, then 8 under the
    other's: each drain carries one parent's shard, the other loop wants it."""
    paths = []
    for j in range(64):
        under = who if (j // 8) % 2 == 0 else 1 - who
        paths.append("/x/p%d/s%d_%d_%02d" % (under, who, rnd % 2, j))
    return paths


def test_crossed_parents_under_load():
    ens = fresh(io_threads=2)
    reader = None
    try:
        s = [Raw(ens), Raw(ens)]  # round-robin: one per IO loop
        s[0].sock.sendall(create_req(1, "/x") + create_req(2, "/x/p0") + create_req(3, "/x/p1"))
        assert [err_of(r) for r in s[0].replies(3)] == [0, 0, 0]
        reader = make_client(ens, session_timeout_ms=30000)
        stop = threading.Event()
        problems = []
        rounds = [0, 0]

        def worker(who):
            try:
                rnd = 0
                while not stop.is_set():
                    paths = crossed_batch(who, rnd)
                    blob = b"".join(create_req(0, p, b"c", EPHEMERAL) for p in paths)
                    blob += b"".join(delete_req(0, p) for p in paths)
                    s[who].sock.sendall(blob)
                    errs = [err_of(r) for r in s[who].replies(2 * len(paths))]
                    if who == 0 and errs != [0] * len(errs):
                        problems.append("session 0 got %s" % sorted(set(errs)))
                        return
                    rnd += 1
                    rounds[who] = rnd
            except (EOFError, OSError) as e:
                # the expired session's connection is closed under it
                if who == 0:
                    problems.append("session 0: %r" % (e,))

        def observer():
            try:
                while not stop.is_set():
                    for p in ("/x/p0", "/x/p1", "/x/p0/s0_0_00"):
                        rc = reader.exists(p)[0]
                        if rc not in (ra.ZOK, ra.ZNONODE):
                            problems.append("exists %s: %s" % (p, ra.error_name(rc)))
                            return
                    ens.audit()  # mid-expiry findings are expected; it must return
            except Exception as e:  # noqa: BLE001
                problems.append("observer: %r" % (e,))

        threads = [threading.Thread(target=worker, args=(0,)), threading.Thread(target=worker, args=(1,)),
                   threading.Thread(target=observer)]
        t0 = time.monotonic()
        for t in threads:
            t.start()
        assert wait_for(lambda: rounds[0] >= 100 and rounds[1] >= 100, timeout=10, interval=0.005)
        ens.expire_session(s[1].sid)  # mid-stream
        before = rounds[0]
        assert wait_for(lambda: rounds[0] >= before + 100 or problems, timeout=10, interval=0.005)
        stop.set()
        for t in threads:
            t.join(max(0.1, 20 - (time.monotonic() - t0)))
        assert not any(t.is_alive() for t in threads), "a thread did not come back within 20 s"
        assert problems == []
        assert wait_for(lambda: s[1].sid not in ens.session_ids())

        # the survivor's last batch is all that is left
        last = crossed_batch(0, 0)
        s[0].sock.sendall(b"".join(create_req(0, p, b"last", EPHEMERAL) for p in last))
        assert [err_of(r) for r in s[0].replies(len(last))] == [0] * len(last)
        have = sorted("/x/p%d/%s" % (i, c) for i in (0, 1) for c in ens.children("/x/p%d" % i))
        assert have == sorted(last)
        assert all(ens.get(p)["stat"]["ephemeralOwner"] == s[0].sid for p in last)
        assert ens.ephemeral_count() == len(last)
        assert ens.audit() == []
        print("crossed parents: %d + %d rounds in %.2f s" % (rounds[0], rounds[1], time.monotonic() - t0))
        for x in s:
            x.close()
    finally:
        if reader is not None:
            reader.close()
        ens.stop()


# ---------------------------------------------------------------- lock guard

# bin/hotpath 100 5 2, register phase: 100 deletes, 103 creates (3 directories).
# The parent commit took 3 mutexes for each, 609 per step, read off its
# handlers. This build measures 220.0 per step: one child shard per request
# where the child is not in its parent's shard, and the carried pair once per
# CARRY_BOUND requests.
LOCKS_MEASURED = 220.0
LOCKS_PARENT = 3 * (103 + 100)


def test_lock_guard():
    assert LOCKS_MEASURED < LOCKS_PARENT / 2
    subprocess.run(["make", "hotpath"], cwd=REPO_ROOT, check=True, capture_output=True)
    out = subprocess.run([os.path.join(REPO_ROOT, "bin", "hotpath"), "100", "5", "2"], check=True,
                         capture_output=True, text=True, timeout=60)
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print("hotpath N=100: tree_locks_register_per_step %.1f, caller allocs/step %.1f"
          % (res["tree_locks_register_per_step"], res["caller"]["allocs_per_step"]))
    assert res["tree_locks_register_per_step"] <= LOCKS_MEASURED * 1.10
    # the parent commit made 105 at N=100: one string per znode in the result
    assert res["caller"]["allocs_per_step"] <= 10


# ---------------------------------------------------------------- large template

def test_large_template_with_single_ops():
    """A 20 000-create template (with its 20 000 cleanup deletes: ~4 MB, more
    than a loopback send buffer takes at once, so part of it waits in the
    client's output buffer for EPOLLOUT) is submitted while another thread
    issues single ops on the same client: order between the two kinds of
    request holds, and nothing is lost."""
    n = 20000
    ens = fresh()
    c = make_client(ens, session_timeout_ms=30000)
    try:
        reg = {"domain": "big.lockrun.test", "type": "host", "adminIp": "127.0.0.1", "hostname": "h0",
               "settleMs": 0, "aliases": ["a%05d.big.lockrun.test" % i for i in range(n - 1)]}
        prep = ra.PreparedRegistration(json.dumps(reg))
        assert len(prep.nodes) == n
        assert c.mkdirp("/single") == ra.ZOK
        stop = threading.Event()
        singles = []

        def single_ops():
            i = 0
            while not stop.is_set():
                p = "/single/n%d" % i
                singles.append((c.create(p, b"s", False)[0], c.exists(p)[0], c.delete_(p)))
                i += 1

        th = threading.Thread(target=single_ops)
        th.start()
        try:
            for _ in range(2):  # the second run's deletes find the first's nodes
                rc, err, znodes = prep.register_(c)
                assert rc == ra.ZOK, err  # every one of the 40 003 return codes passed its check
                assert znodes == prep.nodes
        finally:
            stop.set()
            th.join(20)
        assert not th.is_alive()
        # a reply out of order is an xid mismatch, which drops the connection
        # and fails everything in flight: none of that happened
        assert singles and all(t == (ra.ZOK, ra.ZOK, ra.ZOK) for t in singles)
        assert c.state() == "connected"
        assert c.exists_many(prep.nodes) == [ra.ZOK] * n
        assert ens.ephemeral_count() == n
        assert ens.audit() == []
    finally:
        c.close()
        ens.stop()
