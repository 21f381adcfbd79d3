"""The ensemble's per-request fixed cost (docs/perf_pathlock.md): the tree's
own lock type and the one-pass path check (an inline path hash and an inline
confirming compare were measured and not kept; their tests stay, since they
hold for any hash and any compare). None of it may change what a client sees:

  - which paths every op accepts, and with which return code, is recorded from
    the build BEFORE the change (tests/golden/path_validation.json),
  - a node is found at every path length and depth, and a key that differs in
    one byte anywhere is not,
  - the bench's own paths spread over the shards well enough for every
    released block to be kept,
  - the lock holds under real contention, its sleeping path included.

Host-only. Every wait has a timeout, every test ends on ens.audit() == []."""
import json
import os
import socket
import struct
import threading
import time

import registrar_amd as ra
from conftest import REPO_ROOT, make_client

OP_CREATE, OP_DELETE, OP_EXISTS, OP_GETDATA, OP_SETDATA, OP_GETCHILDREN, OP_CREATE2 = 1, 2, 3, 4, 5, 8, 15
EPHEMERAL = 1
REPLY_HDR = 16  # xid(4) zxid(8) err(4)
GOLDEN = os.path.join(REPO_ROOT, "tests", "golden", "path_validation.json")


# ---------------------------------------------------------------- raw wire
# (the helper pattern of test_lockrun.py; paths here are bytes, since the
# table holds some no str could carry)

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

    def errs(self, n):
        return [struct.unpack(">iqi", self.recv_frame()[4:4 + REPLY_HDR])[2] for _ in range(n)]

    def close(self):
        self.sock.close()


def fresh(io_threads=1):
    ens = ra.Ensemble(servers=1, tick_ms=50, min_session_timeout_ms=200, io_threads=io_threads)
    ens.start()
    return ens


# ---------------------------------------------------------------- 1. path validation

PATH_OPS = ["create", "exists", "getData", "setData", "getChildren", "create2", "delete"]


def path_table():
    """The fixed table, as bytes. Deterministic: the golden file lists the same
    paths in the same order."""
    fill = b"abcdefghijklmnopqrstuvwxyz0123456789ABCD"
    table = [b"", b"/", b"a", b"//", b"//a", b"/a/", b"/a/b/"]
    # a doubled slash at every position of paths 2..40 bytes long
    for n in range(2, 41):
        for pos in range(0, n - 1):
            p = bytearray(b"/" + fill[:n - 1])
            p[pos:pos + 2] = b"//"
            table.append(bytes(p))
    # controls the checks must let through: single slashes, every length
    for n in range(2, 41):
        p = bytearray(b"/" + fill[:n - 1])
        for pos in range(3, n - 1, 3):
            p[pos] = ord("/")
        table.append(bytes(p))
    table.append(b"/k/" + b"x" * 1021)       # 1 KB
    table.append(b"/h\xc3\xa9/\xff\x80z\xfe")  # bytes >= 0x80
    return list(dict.fromkeys(table))  # "//" and "//a" come up twice; order kept


def ancestors(p):
    """The proper prefixes of p that end before a '/', shortest first: what a
    mkdirp of p's parent would create."""
    return [p[:i] for i in range(1, len(p)) if p[i:i + 1] == b"/"]


def run_path_table(ens, parent_present):
    """Every path of the table through every op that takes a path, in
    PATH_OPS order; returns one list of return codes per path. With
    parent_present the path's ancestors are created first (where the server
    takes them; a create it refuses is part of the record too)."""
    s = Raw(ens)
    out = []
    try:
        for p in path_table():
            blob = b""
            npre = 0
            if parent_present:
                for a in ancestors(p):
                    blob += create_req(0, a)
                    npre += 1
            blob += create_req(1, p, b"v")
            blob += path_req(2, OP_EXISTS, p)
            blob += path_req(3, OP_GETDATA, p)
            blob += setdata_req(4, p, b"w")
            blob += path_req(5, OP_GETCHILDREN, p)
            blob += create_req(6, p, b"v", 0, op=OP_CREATE2)
            blob += delete_req(7, p)
            s.sock.sendall(blob)  # one write: the creates and the delete share a drain
            codes = s.errs(npre + len(PATH_OPS))
            out.append(codes[npre:])
    finally:
        s.close()
    return out


def record_path_validation():
    """What the golden file holds, from whichever build is imported. Called
    by hand with the build before the change; the test only reads the file."""
    rows = {}
    for present in (True, False):
        ens = fresh()
        try:
            rows[present] = run_path_table(ens, present)
            assert ens.audit() == []
        finally:
            ens.stop()
    return {"ops": PATH_OPS,
            "paths": [{"path_hex": p.hex(), "parent_present": rows[True][i], "parent_absent": rows[False][i]}
                      for i, p in enumerate(path_table())]}


def test_path_validation_unchanged():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["ops"] == PATH_OPS
    table = path_table()
    assert [bytes.fromhex(r["path_hex"]) for r in golden["paths"]] == table
    for present, key in ((True, "parent_present"), (False, "parent_absent")):
        ens = fresh()
        try:
            got = run_path_table(ens, present)
            assert ens.audit() == []
        finally:
            ens.stop()
        want = [r[key] for r in golden["paths"]]
        diff = [(table[i][:48], want[i], got[i]) for i in range(len(table)) if got[i] != want[i]]
        assert diff == [], "%s: %d paths differ, first %r" % (key, len(diff), diff[:3])
    # the record is not vacuous: refusals and successes are both in it
    creates = [r["parent_present"][0] for r in golden["paths"]]
    assert creates.count(0) >= 30 and creates.count(-5) >= 780  # -5: ZMARSHALLINGERROR


# ---------------------------------------------------------------- 2. lookup across lengths

def test_lookup_across_lengths():
    ens = fresh()
    c = make_client(ens, session_timeout_ms=30000)
    try:
        fill = "abcdefghijklmnopqrstuvwxyz0123456789ABCD"
        parent = ""
        for depth in range(1, 7):
            if depth > 1:
                parent += "/d%d" % depth
                assert c.mkdirp(parent) == ra.ZOK
            paths = ["%s/%s" % (parent, fill[:n]) for n in range(1, 41)]
            assert c.create_many(paths, b"x") == [ra.ZOK] * 40
            assert c.exists_many(paths) == [ra.ZOK] * 40
            assert ens.audit() == []
            assert c.delete_many(paths) == [ra.ZOK] * 40
            assert c.exists_many(paths) == [ra.ZNONODE] * 40
            assert ens.audit() == []
        # 5000 nodes under five parents: every shard's table grows more than once
        parents = ["/grow/p%d" % i for i in range(5)]
        for p in parents:
            assert c.mkdirp(p) == ra.ZOK
        nodes = ["%s/n%04d" % (parents[i % 5], i) for i in range(5000)]
        assert c.create_many(nodes, b"payload") == [ra.ZOK] * 5000
        assert ens.audit() == []
        assert c.exists_many(nodes) == [ra.ZOK] * 5000
        assert c.delete_many(nodes[::2]) == [ra.ZOK] * 2500
        rcs = c.exists_many(nodes)
        assert rcs[::2] == [ra.ZNONODE] * 2500 and rcs[1::2] == [ra.ZOK] * 2500
        assert ens.audit() == []
    finally:
        c.close()
        ens.stop()


# ---------------------------------------------------------------- 3. near-miss keys

def test_near_miss_keys():
    """One node per path length 1..24 (below 8 bytes, 8, 9..15, 16, 17 and
    more: every branch of the compare and of the hash's tail). A key of the
    same length that differs in exactly one byte, at any position, is absent."""
    ens = fresh()
    s = Raw(ens)
    try:
        fill = b"abcdefghijklmnopqrstuvwxyz"
        originals = [b"/"] + [b"/" + fill[:n - 1] for n in range(2, 25)]
        assert [len(p) for p in originals] == list(range(1, 25))
        s.sock.sendall(b"".join(create_req(0, p, b"x") for p in originals[1:]))  # "/" is there already
        assert s.errs(23) == [0] * 23
        variants = []
        for p in originals:
            for pos in range(len(p)):
                for flip in (0x01, 0x80):
                    v = bytearray(p)
                    v[pos] ^= flip  # never makes a '/' of a letter: '.' and 0xaf are the two a '/' turns into
                    assert bytes(v) != p and len(v) == len(p)
                    variants.append(bytes(v))
        assert not set(variants) & set(originals)
        s.sock.sendall(b"".join(path_req(0, OP_EXISTS, v) for v in variants))
        got = s.errs(len(variants))
        wrong = [variants[i] for i in range(len(variants)) if got[i] != ra.ZNONODE]
        assert wrong == [], "found at a key that differs in one byte: %r" % wrong[:3]
        s.sock.sendall(b"".join(path_req(0, OP_EXISTS, p) for p in originals))
        assert s.errs(len(originals)) == [0] * len(originals)
        assert ens.audit() == []
    finally:
        s.close()
        ens.stop()


# ---------------------------------------------------------------- 4. spread over shards

def test_bench_paths_spread_over_shards():
    """The 8 x 1000 paths of eight bench ranks, created and deleted: every
    released block stays cached, which with 64 shards keeping 256 blocks of a
    class each fails as soon as one shard holds more than twice the mean of
    125 nodes."""
    layout = ra.Ensemble.node_store_layout()
    assert layout["shards"] == 64 and layout["max_cached_per_class"] == 256
    ens = fresh()
    c = make_client(ens, session_timeout_ms=30000)
    try:
        payload = b"p" * 110
        ranks = []
        for r in range(8):
            base = "/mi355x/bench/rank%d" % r
            assert c.mkdirp(base) == ra.ZOK
            ranks.append(["%s/bench-r%d" % (base, r)] + ["%s/a%04d" % (base, i) for i in range(999)])
        before = ens.counters()["node_blocks_cached"]
        for paths in ranks:
            assert c.create_many(paths, payload, True) == [ra.ZOK] * 1000
        assert ens.ephemeral_count() == 8000
        assert ens.audit() == []
        for paths in ranks:
            assert c.delete_many(paths) == [ra.ZOK] * 1000
        assert ens.counters()["node_blocks_cached"] - before == 8000
        assert ens.audit() == []
    finally:
        c.close()
        ens.stop()


# ---------------------------------------------------------------- 5. the lock under contention

def test_lock_under_contention():
    """Two IO loops. Two sessions create and delete the SAME 200 siblings
    under one parent, a third reads them, and a Python thread runs audit(),
    which takes every shard with a blocking lock() while the drains hold and
    carry them: tries, spins, sleeps and wake-ups all happen. About two
    seconds."""
    ens = fresh(io_threads=2)
    clients = []
    try:
        clients = [make_client(ens, session_timeout_ms=30000) for _ in range(3)]
        assert clients[0].mkdirp("/shared/parent") == ra.ZOK
        base_nodes = ens.node_count()
        paths = ["/shared/parent/s%03d" % i for i in range(200)]
        stop = threading.Event()
        problems = []
        rounds = [0, 0]
        audits = [0]

        def worker(who):
            try:
                c = clients[who]
                while not stop.is_set():
                    bad = [rc for rc in c.create_many(paths, b"c", True) if rc not in (ra.ZOK, ra.ZNODEEXISTS)]
                    bad += [rc for rc in c.delete_many(paths) if rc not in (ra.ZOK, ra.ZNONODE)]
                    if bad:
                        problems.append("session %d got %s" % (who, sorted(set(bad))))
                        return
                    rounds[who] += 1
            except Exception as e:  # noqa: BLE001
                problems.append("worker %d: %r" % (who, e))

        def reader():
            try:
                while not stop.is_set():
                    bad = [rc for rc in clients[2].exists_many(paths) if rc not in (ra.ZOK, ra.ZNONODE)]
                    if bad:
                        problems.append("reader got %s" % sorted(set(bad)))
                        return
            except Exception as e:  # noqa: BLE001
                problems.append("reader: %r" % (e,))

        def auditor():
            try:
                while not stop.is_set():
                    ens.audit()  # no expiry runs here, but nodes come and go: it must return
                    audits[0] += 1
            except Exception as e:  # noqa: BLE001
                problems.append("auditor: %r" % (e,))

        threads = [threading.Thread(target=worker, args=(0,)), threading.Thread(target=worker, args=(1,)),
                   threading.Thread(target=reader), threading.Thread(target=auditor)]
        t0 = time.monotonic()
        for t in threads:
            t.start()
        stop.wait(2.0)
        stop.set()
        for t in threads:
            t.join(max(0.1, 20 - (time.monotonic() - t0)))
        assert not any(t.is_alive() for t in threads), "a thread did not come back within 20 s"
        assert problems == []
        assert rounds[0] > 0 and rounds[1] > 0 and audits[0] > 0
        print("contention: %d + %d rounds, %d audits in %.2f s" % (rounds[0], rounds[1], audits[0],
                                                                   time.monotonic() - t0))
        # whatever the last interleaving left goes now; then nothing but the parents is there
        for c in clients[:2]:
            assert all(rc in (ra.ZOK, ra.ZNONODE) for rc in c.delete_many(paths))
        assert ens.node_count() == base_nodes
        assert ens.ephemeral_count() == 0
        assert ens.audit() == []
    finally:
        for c in clients:
            c.close()
        ens.stop()
