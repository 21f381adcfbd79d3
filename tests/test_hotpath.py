"""The ensemble/client hot path after the allocation-and-locking cut
(docs/perf_hotpath.md): requests are parsed in place out of the receive
buffer, paths are hashed once and looked up by view, children and ephemerals
are indexed by intrusive links, replies are staged per drain, and a template
batch completes as one pending record. These tests pin the behaviour that
rework could have broken; all are hermetic and small."""
import json
import os
import random
import socket
import struct
import subprocess
import threading
import time

import pytest

import registrar_amd as ra
from conftest import REPO_ROOT, make_client, wait_for

OP_CREATE, OP_DELETE, OP_EXISTS, OP_GETDATA, OP_GETCHILDREN = 1, 2, 3, 4, 8
EPHEMERAL, SEQUENCE = 1, 2
STAT_LEN = 68
REPLY_HDR = 16  # xid(4) zxid(8) err(4)


# ---------------------------------------------------------------- raw wire

def jstr(s):
    b = s if isinstance(s, bytes) else s.encode()
    return struct.pack(">i", len(b)) + b


def frame(body):
    return struct.pack(">i", len(body)) + body


def create_req(xid, path, data=b"", flags=0):
    acl = struct.pack(">i", 1) + struct.pack(">i", 31) + jstr("world") + jstr("anyone")
    return frame(struct.pack(">ii", xid, OP_CREATE) + jstr(path) + jstr(data) + acl + struct.pack(">i", flags))


def delete_req(xid, path, version=-1):
    return frame(struct.pack(">ii", xid, OP_DELETE) + jstr(path) + struct.pack(">i", version))


def exists_req(xid, path, watch=False):
    return frame(struct.pack(">ii", xid, OP_EXISTS) + jstr(path) + struct.pack(">?", watch))


def getdata_req(xid, path):
    return frame(struct.pack(">ii", xid, OP_GETDATA) + jstr(path) + struct.pack(">?", False))


def getchildren_req(xid, path):
    return frame(struct.pack(">ii", xid, OP_GETCHILDREN) + jstr(path) + struct.pack(">?", False))


def recv_exact(sock, n):
    out = b""
    while len(out) < n:
        chunk = sock.recv(n - len(out))
        if not chunk:
            raise EOFError("connection closed after %d of %d bytes" % (len(out), n))
        out += chunk
    return out


def recv_frame(sock):
    """One whole reply frame, length prefix included."""
    hdr = recv_exact(sock, 4)
    return hdr + recv_exact(sock, struct.unpack(">i", hdr)[0])


class RawSession:
    def __init__(self, ens):
        host, port = ens.connect_string().split(",")[0].rsplit(":", 1)
        self.sock = socket.create_connection((host, int(port)), timeout=5)
        self.sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        body = struct.pack(">iqiq", 0, 0, 5000, 0) + struct.pack(">i", 16) + b"\x00" * 16
        self.sock.sendall(frame(body))
        recv_frame(self.sock)

    def send_split(self, data, at):
        """Two writes; the pause lets the server read the first part alone, so
        the frame is completed by a second read into the same buffer."""
        self.sock.sendall(data[:at])
        time.sleep(0.001)
        self.sock.sendall(data[at:])

    def replies(self, n):
        return [recv_frame(self.sock) for _ in range(n)]

    def close(self):
        self.sock.close()


def reply_fields(rep):
    xid, zxid, err = struct.unpack(">iqi", rep[4:4 + REPLY_HDR])
    return xid, zxid, err, rep[4 + REPLY_HDR:]


def parse_stat(b):
    names = ("czxid", "mzxid", "ctime", "mtime", "version", "cversion", "aversion",
             "ephemeral_owner", "data_length", "num_children", "pzxid")
    return dict(zip(names, struct.unpack(">qqqqiiiqiiq", b[:STAT_LEN])))


def mask_times(rep):
    """ctime/mtime are wall-clock reads and differ from run to run; every
    other byte of a reply is a function of the request sequence alone."""
    if len(rep) == 4 + REPLY_HDR + STAT_LEN:
        off = 4 + REPLY_HDR + 16
        return rep[:off] + b"\x00" * 16 + rep[off + 16:]
    return rep


def fresh_ensemble():
    ens = ra.Ensemble(servers=1, tick_ms=50, min_session_timeout_ms=200, io_threads=1)
    ens.start()
    return ens


SPLIT_PATH = "/split-node"
SPLIT_DATA = b"payload-bytes"


def split_script():
    """create, exists, delete, exists(NO_NODE), exists("/") — frames 0, 1, 2 are
    the create / exists / delete whose every split point is exercised."""
    return [
        create_req(1, SPLIT_PATH, SPLIT_DATA),
        exists_req(2, SPLIT_PATH),
        delete_req(3, SPLIT_PATH),
        exists_req(4, SPLIT_PATH),
        exists_req(5, "/"),
    ]


def run_script(frames, split_frame=None, split_at=None, pipelined=False):
    """Run the script against a fresh ensemble (so zxids and session state are
    the same every time) and return the masked reply bytes."""
    ens = fresh_ensemble()
    try:
        s = RawSession(ens)
        out = []
        if pipelined:
            blob = b"".join(frames)
            cut = sum(len(f) for f in frames[:split_frame]) + split_at
            s.send_split(blob, cut)
            out = s.replies(len(frames))
        else:
            for i, f in enumerate(frames):
                if i == split_frame:
                    s.send_split(f, split_at)
                else:
                    s.sock.sendall(f)
                out += s.replies(1)
        s.close()
        return [mask_times(r) for r in out]
    finally:
        ens.stop()


@pytest.fixture(scope="module")
def unsplit_replies():
    ref = run_script(split_script())
    # sanity of the reference itself, so "identical" means "identical and right"
    assert [reply_fields(r)[2] for r in ref] == [0, 0, 0, -101, 0]
    assert reply_fields(ref[0])[3] == jstr(SPLIT_PATH)
    st = parse_stat(reply_fields(ref[1])[3])
    assert st["data_length"] == len(SPLIT_DATA) and st["czxid"] == reply_fields(ref[0])[1]
    return ref


@pytest.mark.parametrize("which", [0, 1, 2], ids=["create", "exists", "delete"])
def test_frame_split_at_every_byte(unsplit_replies, which):
    """A request split across two writes at every offset (inside the length
    prefix, the header, the path, the payload, the ACL) is answered with the
    same bytes as the unsplit request: views into the receive buffer survive
    partial frames, growth and compaction."""
    frames = split_script()
    for at in range(1, len(frames[which])):
        got = run_script(frames, split_frame=which, split_at=at)
        assert got == unsplit_replies, "split of frame %d at byte %d" % (which, at)


def test_pipelined_frames_split_inside_second(unsplit_replies):
    """All frames in one stream, cut at every offset inside the second."""
    frames = split_script()
    for at in range(1, len(frames[1])):
        got = run_script(frames, split_frame=1, split_at=at, pipelined=True)
        assert got == unsplit_replies, "pipelined split at byte %d of frame 1" % at


def test_frame_larger_than_one_read(ensemble):
    """A ~200 KB create (several reads, buffer growth) followed at once by a
    pipelined exists: both answered, payload intact."""
    payload = random.Random(7).randbytes(200 * 1024)
    s = RawSession(ensemble)
    s.sock.sendall(create_req(1, "/big", payload) + exists_req(2, "/big"))
    r_create, r_exists = s.replies(2)
    xid, zxid, err, body = reply_fields(r_create)
    assert (xid, err, body) == (1, 0, jstr("/big"))
    xid, _, err, body = reply_fields(r_exists)
    assert (xid, err) == (2, 0)
    assert parse_stat(body)["data_length"] == len(payload)
    s.sock.sendall(getdata_req(3, "/big"))
    xid, _, err, body = reply_fields(s.replies(1)[0])
    assert (xid, err) == (3, 0)
    assert body[:4] == struct.pack(">i", len(payload)) and body[4:4 + len(payload)] == payload
    assert ensemble.get("/big")["data"] == payload
    s.close()


# ------------------------------------------------------------ tree semantics

def test_depth1_and_deep_paths(ensemble, client):
    """/a (parent "/") and a five-level path: the parent's num_children,
    cversion and pzxid move exactly as one create / one delete should."""
    assert client.mkdirp("/l1/l2/l3/l4") == ra.ZOK
    for parent, path in (("/", "/a"), ("/l1/l2/l3/l4", "/l1/l2/l3/l4/l5")):
        before = ensemble.get(parent)["stat"]
        rc, created = client.create(path, b"x")
        assert (rc, created) == (ra.ZOK, path)
        rc, st = client.exists(path)
        assert rc == ra.ZOK and st["dataLength"] == 1 and st["numChildren"] == 0
        mid = ensemble.get(parent)["stat"]
        assert mid["numChildren"] == before["numChildren"] + 1
        assert mid["cversion"] == before["cversion"] + 1
        assert mid["pzxid"] == st["czxid"] == ensemble.zxid()
        assert path.rsplit("/", 1)[1] in ensemble.children(parent)
        assert client.delete_(path) == ra.ZOK
        assert client.exists(path)[0] == ra.ZNONODE
        after = ensemble.get(parent)["stat"]
        assert after["numChildren"] == before["numChildren"]
        assert after["cversion"] == before["cversion"] + 2
        assert after["pzxid"] == ensemble.zxid() == mid["pzxid"] + 1
        assert path.rsplit("/", 1)[1] not in ensemble.children(parent)
    # a parent with a child refuses deletion; the root cannot be deleted
    assert client.delete_("/l1/l2/l3") == ra.ZNOTEMPTY
    assert client.delete_("/") == ra.ZNONODE


def test_sequence_create(ensemble, client):
    """SEQUENCE appends the parent's cversion as a ten-digit suffix; the final
    path (which may hash to another shard than the request path) is what is
    returned, stored and listed."""
    assert client.create("/seq")[0] == ra.ZOK
    s = RawSession(ensemble)
    names = []
    for i in range(12):  # enough that final paths land in several shards
        s.sock.sendall(create_req(10 + i, "/seq/n-", b"d", SEQUENCE))
        xid, _, err, body = reply_fields(s.replies(1)[0])
        assert (xid, err) == (10 + i, 0)
        (n,) = struct.unpack(">i", body[:4])
        path = body[4:4 + n].decode()
        assert path == "/seq/n-%010d" % i
        assert ensemble.get(path)["exists"] and ensemble.get(path)["data"] == b"d"
        names.append(path.rsplit("/", 1)[1])
    assert not ensemble.get("/seq/n-")["exists"]
    assert ensemble.children("/seq") == sorted(names)
    assert client.get_children("/seq") == (ra.ZOK, sorted(names))
    assert ensemble.get("/seq")["stat"]["numChildren"] == 12
    s.close()


def test_children_listing_after_shuffled_creates_and_deletes(ensemble, client):
    rng = random.Random(42)
    assert client.create("/kids")[0] == ra.ZOK
    names = ["c%03d" % i for i in range(50)]
    order = names[:]
    rng.shuffle(order)
    assert client.create_many(["/kids/" + n for n in order], b"") == [ra.ZOK] * 50
    gone = order[:]
    rng.shuffle(gone)
    gone = gone[:25]
    assert client.delete_many(["/kids/" + n for n in gone]) == [ra.ZOK] * 25
    left = sorted(set(names) - set(gone))
    assert ensemble.children("/kids") == left
    assert client.get_children("/kids") == (ra.ZOK, left)
    assert ensemble.get("/kids")["stat"]["numChildren"] == 25
    assert ensemble.get("/kids")["stat"]["cversion"] == 75


def test_ephemeral_index(ensemble):
    """20 ephemerals, 5 deleted by hand, then the session expires: the other
    15 go, the index is empty, the parent's counts are right, and a second
    session's ephemerals under the same parent survive."""
    a = make_client(ensemble)
    b = make_client(ensemble)
    try:
        assert a.create("/eph")[0] == ra.ZOK
        mine = ["/eph/a%02d" % i for i in range(20)]
        theirs = ["/eph/b%02d" % i for i in range(4)]
        assert a.create_many(mine, b"", True) == [ra.ZOK] * 20
        assert b.create_many(theirs, b"", True) == [ra.ZOK] * 4
        assert ensemble.ephemeral_count() == 24
        assert a.delete_many(mine[:3]) == [ra.ZOK] * 3
        assert b.delete_many(mine[3:5]) == [ra.ZOK] * 2  # another session's hand too
        assert ensemble.ephemeral_count() == 19
        ensemble.expire_session(a.session_id())
        assert wait_for(lambda: ensemble.children("/eph") == [t.rsplit("/", 1)[1] for t in theirs])
        assert ensemble.ephemeral_count() == 4
        assert ensemble.get("/eph")["stat"]["numChildren"] == 4
        for t in theirs:
            assert ensemble.get(t)["stat"]["ephemeralOwner"] == b.session_id()
        ensemble.expire_session(b.session_id())
        assert wait_for(lambda: ensemble.children("/eph") == [])
        assert ensemble.ephemeral_count() == 0
        assert ensemble.get("/eph")["stat"]["numChildren"] == 0
        assert ensemble.node_count() == 1  # only /eph is left
    finally:
        a.close()
        b.close()


def test_two_io_threads_share_one_parent():
    """Two connections on different IO threads create 200 siblings each under
    one parent and delete half of them, concurrently: the children are exact
    and the per-loop request counters sum to the requests sent."""
    ens = ra.Ensemble(servers=1, tick_ms=50, min_session_timeout_ms=200, io_threads=2)
    ens.start()
    clients = [make_client(ens), make_client(ens)]  # round-robin: one per loop
    try:
        assert clients[0].create("/shared")[0] == ra.ZOK
        results = {}

        def work(k):
            paths = ["/shared/t%d-%03d" % (k, i) for i in range(200)]
            rc_create = clients[k].create_many(paths, b"v", True)
            rc_delete = clients[k].delete_many(paths[::2])
            results[k] = (rc_create, rc_delete)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(30)
            assert not t.is_alive()
        for k in range(2):
            assert results[k] == ([ra.ZOK] * 200, [ra.ZOK] * 100)
        expect = sorted("t%d-%03d" % (k, i) for k in range(2) for i in range(1, 200, 2))
        assert ens.children("/shared") == expect
        assert ens.get("/shared")["stat"]["numChildren"] == 200
        assert ens.get("/shared")["stat"]["cversion"] == 600
        assert ens.ephemeral_count() == 200
        counters = ens.counters()
        assert counters["connect"] == 2
        assert counters["create"] == 401
        assert counters["delete"] == 200
        assert "exists" not in counters  # zero counters are left out, as before
    finally:
        for c in clients:
            c.close()
        ens.stop()


# ------------------------------------------------------- template batches

def small_registration(tag, n_aliases=2):
    return json.dumps({
        "domain": "%s.hot.test" % tag, "type": "host", "adminIp": "127.0.0.1",
        "hostname": "h-" + tag, "settleMs": 0,
        "aliases": ["x%d.%s.hot.test" % (i, tag) for i in range(n_aliases)],
    })


def call_with_timeout(fn, timeout=20):
    box = {}
    t = threading.Thread(target=lambda: box.setdefault("v", fn()), daemon=True)
    t.start()
    t.join(timeout)
    assert not t.is_alive(), "call hung"
    return box["v"]


def test_template_batch_interleaved_with_single_ops(ensemble, client):
    """A 3-znode template batch (one pending record for the run of xids)
    against a slow server while another thread issues single exists calls on
    the same client: everything completes with rc 0, in order."""
    prep = ra.PreparedRegistration(small_registration("mix"))
    assert client.create("/probe")[0] == ra.ZOK
    ensemble.set_latency_ms(20)
    singles = []

    def probe():
        for _ in range(6):
            singles.append(client.exists("/probe")[0])

    t = threading.Thread(target=probe)
    t.start()
    for _ in range(3):
        rc, err, znodes = call_with_timeout(lambda: prep.register_(client))
        assert (rc, err) == (ra.ZOK, "")
        assert znodes == prep.nodes and len(znodes) == 3
        assert call_with_timeout(lambda: prep.heartbeat(client))[0] == ra.ZOK
    t.join(20)
    assert not t.is_alive()
    ensemble.set_latency_ms(0)
    assert singles == [ra.ZOK] * 6
    for n in prep.nodes:
        assert ensemble.get(n)["stat"]["ephemeralOwner"] == client.session_id()


def test_template_batch_fails_whole_on_connection_loss(ensemble):
    """kill_server while a batch's replies are still held back: the batch
    fails as a unit with CONNECTION_LOSS (first failing stage named, as
    before) and nothing hangs."""
    c = make_client(ensemble)
    try:
        prep = ra.PreparedRegistration(small_registration("kill"))
        assert prep.register_(c)[0] == ra.ZOK
        ensemble.set_latency_ms(300)
        before = ensemble.counters().get("create", 0)
        box = {}
        t = threading.Thread(target=lambda: box.setdefault("v", prep.register_(c)), daemon=True)
        t.start()
        # the whole batch has reached the server; its replies sit in timers
        assert wait_for(lambda: ensemble.counters().get("create", 0) >= before + 3)
        ensemble.kill_server(0)
        t.join(20)
        assert not t.is_alive(), "register_ hung after the server was killed"
        rc, err, znodes = box["v"]
        assert rc == ra.ZCONNECTIONLOSS
        assert err == "cleanupPreviousEntries: unlink %s failed: CONNECTION_LOSS" % prep.nodes[0]
        assert znodes == []
        # a heartbeat batch submitted while disconnected fails the same way
        rc, _ = call_with_timeout(lambda: prep.heartbeat(c, {"maxAttempts": 0}))
        assert rc == ra.ZCONNECTIONLOSS
    finally:
        ensemble.set_latency_ms(0)
        c.close()


def test_mixed_outcomes_in_one_batch(ensemble, client):
    """One alias already exists as another session's PERSISTENT node. Recorded
    from the parent commit: cleanupPreviousEntries unlinks it like any stale
    entry, so the register succeeds (rc 0, no error text, all three znodes)
    and the node comes back as this session's ephemeral. If that node has a
    child the unlink fails instead, and the parent commit reports rc -111
    with the text below, having still run the rest of the pipelined batch."""
    other = make_client(ensemble)
    try:
        prep = ra.PreparedRegistration(small_registration("mixed"))
        alias = prep.nodes[1]
        assert other.mkdirp(alias) == ra.ZOK
        rc, err, znodes = prep.register_(client)
        assert (rc, err, znodes) == (0, "", prep.nodes)
        st = ensemble.get(alias)["stat"]
        assert st["ephemeralOwner"] == client.session_id()

        prep2 = ra.PreparedRegistration(small_registration("mixed2"))
        alias2 = prep2.nodes[1]
        assert other.mkdirp(alias2 + "/child") == ra.ZOK
        rc, err, znodes = prep2.register_(client)
        assert rc == -111
        assert err == "cleanupPreviousEntries: unlink %s failed: NOT_EMPTY" % alias2
        assert znodes == []
        # per-op outcomes of that one batch: the other two creates went
        # through, the occupied alias stayed the other session's
        assert ensemble.get(prep2.nodes[0])["stat"]["ephemeralOwner"] == client.session_id()
        assert ensemble.get(prep2.nodes[2])["stat"]["ephemeralOwner"] == client.session_id()
        assert ensemble.get(alias2)["stat"]["ephemeralOwner"] == 0
        assert ensemble.children(alias2) == ["child"]
    finally:
        other.close()


# --------------------------------------------------------- allocation guard

# ensemble IO thread allocations per step at N=100 (bin/hotpath 100 5 2):
PARENT_ENS_ALLOCS_N100 = 1607.0  # parent commit (16 007 at N=1000)
NEW_ENS_ALLOCS_N100 = 300.0      # this tree (3 000 at N=1000): 3 per create —
                                 # map node, key string, payload string
ENS_ALLOC_CAP_N100 = NEW_ENS_ALLOCS_N100 * 1.10


@pytest.fixture(scope="module")
def hotpath_bin():
    subprocess.run(["make", "hotpath"], cwd=REPO_ROOT, check=True, capture_output=True)
    return os.path.join(REPO_ROOT, "bin", "hotpath")


def test_allocation_guard(hotpath_bin):
    """Steady-state allocations of the ensemble IO thread, counted by the
    hotpath tool's operator new at N=100: the parent commit made 1607.0 per
    step (1506 in the register phase, 101 per 100-exists heartbeat, 201 per
    100-delete batch); this tree makes 300.0 per step, all of them in the
    creates, and none for exists or delete handling. The cap is the new
    figure plus 10 %, and must itself stay at or below half the parent's."""
    assert ENS_ALLOC_CAP_N100 <= PARENT_ENS_ALLOCS_N100 / 2
    out = subprocess.run([hotpath_bin, "100", "5", "2"], check=True, capture_output=True,
                         text=True, timeout=60).stdout
    res = json.loads(out.strip().splitlines()[-1])
    print("hotpath N=100:", json.dumps(res))
    assert res["znodes"] == 100 and res["steps"] == 5
    assert res["ens_io_allocs_heartbeat_per_step"] == 0  # exists
    assert res["ens_io_allocs_delete_per_batch"] == 0    # delete
    assert res["ens_io"]["allocs_per_step"] <= ENS_ALLOC_CAP_N100
    assert res["ens_io"]["allocs_per_step"] == res["ens_io_allocs_register_per_step"]
