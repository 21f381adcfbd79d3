"""The ensemble's node store (docs/perf_nodestore.md): a znode is one block
(header, path bytes, data bytes) in a per-shard intrusive hash table, blocks
are recycled through bounded per-shard free lists, and the hot replies are
encoded in place. These tests pin what that could break: the reply bytes, the
contents of a recycled block, setData across the inline capacity, table
growth, bounded retention and recycling from two IO threads. All hermetic."""
import json
import os
import struct
import subprocess
import threading

import pytest

import registrar_amd as ra
from conftest import REPO_ROOT, make_client, wait_for
from test_hotpath import (EPHEMERAL, REPLY_HDR, SEQUENCE, STAT_LEN, RawSession, create_req,
                          delete_req, exists_req, frame, getchildren_req, getdata_req, jstr,
                          parse_stat, recv_frame, reply_fields)

OP_SETDATA, OP_PING, OP_GETCHILDREN2, OP_MULTI, OP_CREATE2, OP_CHECK = 5, 11, 12, 14, 15, 13
OP_CREATE, OP_DELETE = 1, 2

GOLDEN = os.path.join(REPO_ROOT, "tests", "golden", "nodestore_replies.json")
# The fixture was recorded from commit 2836edf ("Cut per-request allocation
# and locking in the ensemble hot path"), the parent of the node-store change,
# with NODESTORE_RECORD=2836edf python -m pytest tests/test_nodestore.py -k byte_for_byte
RECORD_ENV = "NODESTORE_RECORD"


def acl_bytes():
    return struct.pack(">i", 1) + struct.pack(">i", 31) + jstr("world") + jstr("anyone")


def create2_req(xid, path, data=b"", flags=0):
    return frame(struct.pack(">ii", xid, OP_CREATE2) + jstr(path) + jstr(data) + acl_bytes()
                 + struct.pack(">i", flags))


def setdata_req(xid, path, data, version=-1):
    return frame(struct.pack(">ii", xid, OP_SETDATA) + jstr(path) + jstr(data) + struct.pack(">i", version))


def getchildren2_req(xid, path):
    return frame(struct.pack(">ii", xid, OP_GETCHILDREN2) + jstr(path) + struct.pack(">?", False))


def multi_req(xid, ops):
    """ops: (type, body bytes) pairs; each goes out behind a MultiHeader."""
    body = struct.pack(">ii", xid, OP_MULTI)
    for typ, b in ops:
        body += struct.pack(">i?i", typ, False, -1) + b
    return frame(body + struct.pack(">i?i", -1, True, -1))


def m_create(path, data=b"", flags=0):
    return (OP_CREATE, jstr(path) + jstr(data) + acl_bytes() + struct.pack(">i", flags))


def m_delete(path, version=-1):
    return (OP_DELETE, jstr(path) + struct.pack(">i", version))


def m_setdata(path, data, version=-1):
    return (OP_SETDATA, jstr(path) + jstr(data) + struct.pack(">i", version))


def m_check(path, version):
    return (OP_CHECK, jstr(path) + struct.pack(">i", version))


MULTI_HDR = 9  # type(4) done(1) err(4)


def wire_script():
    """(request frame, bytes between the reply's Stat and the end of the reply,
    or None when an OK reply carries no Stat). Only ctime/mtime of a Stat
    depend on the clock; they are masked before comparing."""
    big = bytes(range(256)) + b"x" * 44
    return [
        (create_req(1, "/a", b"A"), None),                              # depth 1
        (create_req(2, "/a/b/c", b"orphan"), None),                     # NO_NODE parent
        (create_req(3, "/a/b", b"bb"), None),
        (create_req(4, "/a/b/c", b"c" * 40), None),                     # deeper
        (create2_req(5, "/a/d", b"dd"), 0),                             # create2: path + Stat
        (create_req(6, "/a/seq-", b"s0", SEQUENCE), None),
        (create_req(7, "/a/seq-", b"s1", SEQUENCE), None),
        (create_req(8, "/a/e", b"eph", EPHEMERAL), None),
        (create2_req(9, "/a/e2-", b"", EPHEMERAL | SEQUENCE), 0),
        (create_req(10, "/a", b"again"), None),                         # NODE_EXISTS
        (create_req(11, "/a/e/kid", b""), None),                        # child of ephemeral
        (delete_req(12, "/a/b/c", 5), None),                            # BAD_VERSION
        (delete_req(13, "/a/b"), None),                                 # NOT_EMPTY
        (delete_req(14, "/a/b/c", 0), None),                            # good version
        (delete_req(15, "/nope"), None),                                # NO_NODE
        (exists_req(16, "/a"), 0),
        (exists_req(17, "/absent"), None),
        (getdata_req(18, "/a/b"), 0),
        (setdata_req(19, "/a/b", big, 0), 0),                           # good version, grows
        (setdata_req(20, "/a/b", b"no", 7), None),                      # BAD_VERSION
        (setdata_req(21, "/a/b", b"tiny", -1), 0),                      # shrinks
        (getdata_req(22, "/a/b"), 0),
        (getchildren_req(23, "/a"), None),
        (getchildren2_req(24, "/a"), 0),
        (multi_req(25, [m_create("/a/m1", b"m"), m_setdata("/a", b"AA"), m_delete("/a/d"),
                        m_check("/a/b", 2)]), 3 * MULTI_HDR),
        (multi_req(26, [m_create("/a/m2", b""), m_delete("/absent")]), None),   # fails whole
        (exists_req(27, "/a/m1"), 0),
        (exists_req(28, "/a/d"), None),
        (exists_req(29, "/a/m2"), None),
        (getchildren2_req(30, "/"), 0),
        (getdata_req(31, "/a"), 0),
        (frame(struct.pack(">ii", -2, OP_PING)), None),
    ]


def mask_stat_times(rep, tail):
    err = reply_fields(rep)[2]
    if tail is None or err != 0:
        return rep
    off = len(rep) - tail - STAT_LEN + 16
    assert off >= 4 + REPLY_HDR + 16
    return rep[:off] + b"\x00" * 16 + rep[off + 16:]


def run_wire_script():
    ens = ra.Ensemble(servers=1, tick_ms=50, min_session_timeout_ms=200, io_threads=1)
    ens.start()
    try:
        host, port = ens.connect_string().split(",")[0].rsplit(":", 1)
        import socket
        sock = socket.create_connection((host, int(port)), timeout=5)
        sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        sock.sendall(frame(struct.pack(">iqiq", 0, 0, 5000, 0) + struct.pack(">i", 16) + b"\x00" * 16))
        out = [recv_frame(sock)]  # the ConnectResponse: session id and password included
        for req, tail in wire_script():
            sock.sendall(req)
            out.append(mask_stat_times(recv_frame(sock), tail))
        # once more, all requests in one write: the replies of one drain
        sock2 = RawSession(ens)
        script = [(delete_req(100 + i, p), None) for i, p in
                  enumerate(["/a/m1", "/a/e", "/a/b", "/a/seq-0000000003", "/a/seq-0000000004"])]
        script += [(create2_req(110, "/a/pipelined", b"p" * 10, EPHEMERAL), 0), (exists_req(111, "/a"), 0),
                   (getchildren2_req(112, "/a"), 0)]
        sock2.sock.sendall(b"".join(r for r, _ in script))
        for (_, tail), rep in zip(script, sock2.replies(len(script))):
            out.append(mask_stat_times(rep, tail))
        sock2.close()
        sock.close()
        return out
    finally:
        ens.stop()


def test_replies_byte_for_byte():
    """One fixed request script over a raw socket; every reply (ctime/mtime
    masked) equals what the parent commit's build sent."""
    got = [r.hex() for r in run_wire_script()]
    if os.environ.get(RECORD_ENV):
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as f:
            json.dump({"recorded_from": os.environ[RECORD_ENV], "replies": got}, f, indent=0)
            f.write("\n")
    with open(GOLDEN) as f:
        want = json.load(f)["replies"]
    # sanity of the fixture itself: the outcomes the script is written to hit
    errs = [reply_fields(bytes.fromhex(r))[2] for r in want[1:33]]
    assert errs == [0, -101, 0, 0, 0, 0, 0, 0, 0, -110, -108, -103, -111, 0, -101, 0, -101, 0, 0, -103,
                    0, 0, 0, 0, 0, -101, 0, -101, -101, 0, 0, 0]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "reply %d differs" % i


# ------------------------------------------------------------ recycled blocks

def layout():
    """Header size, block size classes and free-list bound of the node store."""
    return ra.Ensemble.node_store_layout()


def boundary_lengths(path_len):
    """Data lengths 0, 1, and one below / at / one above the capacity of each
    size class for a node with a path of path_len bytes, and one beyond the
    largest class."""
    out = {0, 1}
    for cls in layout()["classes"]:
        cap = cls - layout()["header_bytes"] - path_len
        for d in (cap - 1, cap, cap + 1):
            if d >= 0:
                out.add(d)
    out.add(64 * 1024)
    return sorted(out)


def test_layout_is_sane():
    assert layout()["shards"] == 64
    assert layout()["classes"] == sorted(set(layout()["classes"])) and len(layout()["classes"]) >= 2
    assert layout()["classes"][0] > layout()["header_bytes"]
    assert 125 < layout()["max_cached_per_class"] <= 1024


def pattern(n, seed):
    return bytes((seed * 31 + i * 7) & 0xFF for i in range(n))


def test_no_stale_bytes_from_recycled_block(ensemble, client):
    """Nodes of every boundary length and of path lengths 2..~1 KB are created,
    deleted and replaced by the same number of nodes with other paths and
    other lengths: reads return exactly what the last occupant wrote."""
    assert client.create("/r")[0] == ra.ZOK
    lens = boundary_lengths(len("/r/n000"))
    first = []
    # short path at depth 1 ("/x": 2 bytes), and long names up to ~1 KB
    odd_paths = ["/x", "/r/" + "p" * 100, "/r/" + "q" * 500, "/r/" + "w" * 1020]
    for i, d in enumerate(lens):
        first.append(("/r/n%03d" % i, pattern(d, i)))
    for i, p in enumerate(odd_paths):
        first.append((p, pattern(37 + i, 200 + i)))
    for p, d in first:
        assert client.create(p, d) == (ra.ZOK, p)
    for p, d in first:
        assert client.get(p)[:2] == (ra.ZOK, d)
    cached0 = ensemble.counters()["node_blocks_cached"]
    assert client.delete_many([p for p, _ in first]) == [ra.ZOK] * len(first)
    assert ensemble.counters()["node_blocks_cached"] > cached0
    assert ensemble.node_count() == 1

    # different paths (other shards, other lengths), lengths rotated so a block
    # gets an occupant of another size
    rot = lens[3:] + lens[:3]
    second = [("/r/second-%d-%s" % (i, "z" * (i % 40)), pattern(d, 77 + i)) for i, d in enumerate(rot)]
    second += [("/y" + "k" * i, pattern(11 * (i + 1), 300 + i)) for i in range(len(odd_paths))]
    assert len(second) == len(first)
    for p, d in second:
        assert client.create(p, d) == (ra.ZOK, p)
    for p, d in second:
        rc, data, st = client.get(p)
        assert (rc, data) == (ra.ZOK, d), p
        assert st["dataLength"] == len(d)
        rc, st = client.exists(p)
        assert rc == ra.ZOK and st["dataLength"] == len(d) and st["version"] == 0
        assert ensemble.get(p)["data"] == d
    for p, _ in first:
        assert client.exists(p)[0] == ra.ZNONODE
    want_r = sorted(p.rsplit("/", 1)[1] for p, _ in second if p.startswith("/r/"))
    assert client.get_children("/r") == (ra.ZOK, want_r)
    assert ensemble.children("/r") == want_r
    want_root = sorted(["r"] + [p[1:] for p, _ in second if not p.startswith("/r/")])
    assert client.get_children("/") == (ra.ZOK, want_root)


def test_set_data_across_inline_capacity(ensemble):
    """Grow past the block's capacity, shrink back, grow again: on a node with
    children and on an ephemeral. The node does not move: its children, its
    session link and its parent link all still work afterwards."""
    a = make_client(ensemble)
    b = make_client(ensemble)
    try:
        assert a.create("/s", b"seed")[0] == ra.ZOK
        kids = ["/s/k%02d" % i for i in range(10)]
        assert a.create_many(kids, b"kid") == [ra.ZOK] * 10
        assert b.create("/s/eph", b"e", True)[0] == ra.ZOK
        top = layout()["classes"][-1]
        sizes = [layout()["classes"][0], 5, top + 1000, 0, 3 * top, 17, 200, 199]
        for target in ("/s", "/s/eph"):
            for v, n in enumerate(sizes):
                d = pattern(n, v + len(target))
                assert a.set(target, d, v) == ra.ZOK
                rc, data, st = a.get(target)
                assert (rc, data) == (ra.ZOK, d)
                assert st["dataLength"] == n and st["version"] == v + 1
                assert ensemble.get(target)["data"] == d
            assert a.set(target, b"late", 0) == ra.ZBADVERSION
        names = sorted([k.rsplit("/", 1)[1] for k in kids] + ["eph"])
        assert a.get_children("/s") == (ra.ZOK, names)
        assert ensemble.get("/s")["stat"]["numChildren"] == 11
        assert ensemble.get("/s/eph")["stat"]["ephemeralOwner"] == b.session_id()
        # the ephemeral is still on its session's list: expiry removes it
        ensemble.expire_session(b.session_id())
        assert wait_for(lambda: not ensemble.get("/s/eph")["exists"])
        assert ensemble.ephemeral_count() == 0
        assert a.delete_("/s") == ra.ZNOTEMPTY
        assert a.delete_many(kids) == [ra.ZOK] * 10
        assert a.delete_("/s") == ra.ZOK
        assert ensemble.node_count() == 0
        assert ensemble.audit() == []
    finally:
        a.close()
        b.close()


def test_table_growth(ensemble, client):
    """5000 nodes under five parents (each shard's table grows several times):
    all found; every other one deleted; the rest still found."""
    parents = ["/g%d" % i for i in range(5)]
    for p in parents:
        assert client.create(p)[0] == ra.ZOK
    paths = ["%s/n%04d" % (parents[i % 5], i) for i in range(5000)]
    assert client.create_many(paths, b"v") == [ra.ZOK] * 5000
    assert ensemble.node_count() == 5005
    assert client.exists_many(paths) == [ra.ZOK] * 5000
    assert client.delete_many(paths[::2]) == [ra.ZOK] * 2500
    assert ensemble.node_count() == 2505
    got = client.exists_many(paths)
    assert got[1::2] == [ra.ZOK] * 2500
    assert got[::2] == [ra.ZNONODE] * 2500
    for p in parents:
        assert ensemble.get(p)["stat"]["numChildren"] == 500
        assert len(ensemble.children(p)) == 500
    assert client.delete_many(paths[1::2]) == [ra.ZOK] * 2500
    assert ensemble.node_count() == 5


def test_bounded_retention(ensemble, client):
    """20 000 ephemerals created and deleted in one session: the free lists
    keep at most their bound, and the store goes on working."""
    bound = layout()["shards"] * len(layout()["classes"]) * layout()["max_cached_per_class"]
    assert client.create("/b")[0] == ra.ZOK
    paths = ["/b/e%05d" % i for i in range(20000)]
    assert client.create_many(paths, b"payload", True) == [ra.ZOK] * 20000
    assert ensemble.ephemeral_count() == 20000
    assert client.delete_many(paths) == [ra.ZOK] * 20000
    cached = ensemble.counters()["node_blocks_cached"]
    print("node_blocks_cached after 20000 deletes:", cached, "bound", bound)
    assert 0 < cached <= bound
    # one class is in play here, so the tighter per-class figure holds too
    assert cached <= layout()["shards"] * layout()["max_cached_per_class"]
    assert ensemble.node_count() == 1 and ensemble.ephemeral_count() == 0
    assert client.create_many(paths[:300], b"again", True) == [ra.ZOK] * 300
    assert ensemble.counters()["node_blocks_cached"] == cached - 300
    assert client.get(paths[7])[:2] == (ra.ZOK, b"again")
    assert client.delete_many(paths[:300]) == [ra.ZOK] * 300
    assert ensemble.counters()["node_blocks_cached"] == cached


def test_two_io_threads_recycle_and_kill():
    """Four sessions on two IO threads run create / exists / delete rounds, so
    blocks released by one thread are reused by the other: one pair under
    different parents, one pair under the same parent. One session of the
    shared pair is expired mid-stream: none of its nodes survives, and the
    other sessions' final sets and the counts are exact."""
    ens = ra.Ensemble(servers=1, tick_ms=50, min_session_timeout_ms=200, io_threads=2)
    ens.start()
    clients = [make_client(ens) for _ in range(4)]  # round-robin: loops 0, 1, 0, 1
    parents = ["/p0", "/p1", "/shared", "/shared"]
    try:
        for p in sorted(set(parents)):
            assert clients[0].create(p)[0] == ra.ZOK
        victim = 3
        victim_sid = clients[victim].session_id()
        rounds = 30
        errors = []
        started = threading.Event()
        victim_rounds = []

        def work(k):
            c = clients[k]
            # the victim keeps going until its session is gone, so the kill
            # always lands mid-stream (the cap only bounds a broken run)
            for r in range(rounds if k != victim else 100000):
                # lengths differ per round, so recycled blocks change occupants
                paths = ["%s/c%d-r%02d-%03d%s" % (parents[k], k, r, i, "x" * ((r * 5 + i) % 30))
                         for i in range(100)]
                rc_c = c.create_many(paths, pattern(10 + 7 * (r % 60), k), True)
                if k == victim:
                    if r == 2:
                        started.set()
                    if rc_c != [ra.ZOK] * 100:
                        victim_rounds.append(r)
                        return  # expired: whatever it had is gone with the session
                rc_e = c.exists_many(paths)
                last = r == rounds - 1 and k != victim
                rc_d = c.delete_many(paths if not last else paths[::2])
                if k != victim:
                    want_d = [ra.ZOK] * (100 if not last else 50)
                    if (rc_c, rc_e, rc_d) != ([ra.ZOK] * 100, [ra.ZOK] * 100, want_d):
                        errors.append((k, r))

        threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        assert started.wait(20)
        ens.expire_session(victim_sid)
        for t in threads:
            t.join(60)
            assert not t.is_alive()
        assert errors == []
        assert victim_rounds and victim_rounds[0] < 100000, "the victim was never cut off"
        assert wait_for(lambda: victim_sid not in ens.session_ids())
        survivors = {}
        for k in range(3):
            survivors[k] = sorted(n for n in ens.children(parents[k]) if n.startswith("c%d-" % k))
            assert len(survivors[k]) == 50
        assert ens.children("/shared") == survivors[2]  # nothing of the victim's is left
        for k in range(3):
            for n in survivors[k]:
                st = ens.get(parents[k] + "/" + n)["stat"]
                assert st["ephemeralOwner"] == clients[k].session_id()
                assert st["dataLength"] == 10 + 7 * (rounds - 1)
        assert ens.ephemeral_count() == 150
        assert ens.node_count() == 3 + 150
        for p in ("/p0", "/p1", "/shared"):
            assert ens.get(p)["stat"]["numChildren"] == 50
        assert ens.audit() == []  # the expiry is over: the victim's id is gone and so are its nodes
    finally:
        for c in clients:
            c.close()
        ens.stop()


# ------------------------------------------------------------ allocation figure

@pytest.fixture(scope="module")
def hotpath_bin():
    subprocess.run(["make", "hotpath"], cwd=REPO_ROOT, check=True, capture_output=True)
    return os.path.join(REPO_ROOT, "bin", "hotpath")


def test_register_phase_allocations(hotpath_bin):
    """bin/hotpath 100 20 5: at most 10 ensemble IO thread allocations per step
    in the register phase (10 % of one per create; the design value is 0 once
    the free lists are warm), and still none for exists or the delete batch."""
    out = subprocess.run([hotpath_bin, "100", "20", "5"], check=True, capture_output=True,
                         text=True, timeout=60).stdout
    res = json.loads(out.strip().splitlines()[-1])
    print("hotpath N=100:", json.dumps(res))
    assert res["znodes"] == 100 and res["steps"] == 20
    assert res["ens_io_allocs_register_per_step"] <= 10
    assert res["ens_io_allocs_heartbeat_per_step"] == 0
    assert res["ens_io_allocs_delete_per_batch"] == 0
