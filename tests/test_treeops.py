"""The tree mutations and the reply encoder behind both the single-op
handlers and multi (docs/architecture.md, "Where a mutation is applied").
These tests pin behaviour that has to be the same whichever way a mutation
arrives: the tree a sequence of ops leaves behind, the bookkeeping of another
session's ephemeral, the order and multiplicity of the watch events one
transaction fires, the bytes several watchers of one node receive, and which
reads arm a watch on an absent path. All are hermetic and small."""
import select
import struct

import registrar_amd as ra
from conftest import make_client, wait_for
from test_hotpath import (EPHEMERAL, RawSession, create_req, delete_req, exists_req, frame,
                          fresh_ensemble, jstr, recv_frame, reply_fields)

OP_CREATE, OP_DELETE, OP_GETDATA, OP_SETDATA, OP_GETCHILDREN, OP_MULTI = 1, 2, 4, 5, 8, 14
EV_CREATED, EV_DELETED, EV_CHANGED, EV_CHILD = 1, 2, 3, 4
XID_EVENT = -1
QUIET_S = 0.2  # "nothing further arrives" window

ACL_OPEN = struct.pack(">i", 1) + struct.pack(">i", 31) + jstr("world") + jstr("anyone")


def setdata_req(xid, path, data, version=-1):
    return frame(struct.pack(">ii", xid, OP_SETDATA) + jstr(path) + jstr(data) + struct.pack(">i", version))


def watch_req(xid, op, path):
    """getData / getChildren with the watch flag set."""
    return frame(struct.pack(">ii", xid, op) + jstr(path) + struct.pack(">?", True))


def multi_req(xid, ops):
    """ops: ("create", path, data, flags) | ("delete", path) | ("set", path, data)."""
    body = struct.pack(">ii", xid, OP_MULTI)
    for op in ops:
        if op[0] == "create":
            body += struct.pack(">i?i", OP_CREATE, False, -1)
            body += jstr(op[1]) + jstr(op[2]) + ACL_OPEN + struct.pack(">i", op[3])
        elif op[0] == "delete":
            body += struct.pack(">i?i", OP_DELETE, False, -1) + jstr(op[1]) + struct.pack(">i", -1)
        else:
            body += struct.pack(">i?i", OP_SETDATA, False, -1)
            body += jstr(op[1]) + jstr(op[2]) + struct.pack(">i", -1)
    return frame(body + struct.pack(">i?i", -1, True, -1))


def ok(rep):
    assert reply_fields(rep)[2] == 0, "reply %r" % (reply_fields(rep)[:3],)
    return rep


def parse_event(rep):
    """(type, path) of a watch event frame; asserts it is one."""
    xid, zxid, err, body = reply_fields(rep)
    assert (xid, zxid, err) == (XID_EVENT, -1, 0)
    etype, state, n = struct.unpack(">iii", body[:12])
    assert state == 3  # SyncConnected
    return etype, body[12:12 + n].decode()


def assert_quiet(*raws):
    """Nothing further arrives on any of the connections within QUIET_S."""
    readable, _, _ = select.select([r.sock for r in raws], [], [], QUIET_S)
    assert not readable, "unexpected bytes %r" % ([s.recv(4096) for s in readable],)


# ------------------------------------------- 1. multi and single ops agree

SIX_OPS = [
    ("create", "/t/p", b"1", 0),
    ("create", "/t/e", b"", EPHEMERAL),
    ("set", "/t/p", b"L" * 600),  # past the inline room of the 256-byte class: out of line
    ("set", "/t/p", b"22"),       # and back inline
    ("delete", "/t/e"),
    ("create", "/t/e", b"", EPHEMERAL),
]


def single_req(xid, op):
    if op[0] == "create":
        return create_req(xid, op[1], op[2], op[3])
    if op[0] == "delete":
        return delete_req(xid, op[1])
    return setdata_req(xid, op[1], op[2])


def tree_after(as_multi):
    ens = fresh_ensemble()
    try:
        s = RawSession(ens)
        s.sock.sendall(create_req(1, "/t"))
        ok(s.replies(1)[0])
        if as_multi:
            s.sock.sendall(multi_req(2, SIX_OPS))
            ok(s.replies(1)[0])
        else:
            for i, op in enumerate(SIX_OPS):
                s.sock.sendall(single_req(2 + i, op))
                ok(s.replies(1)[0])
        stats = {}
        for path in ("/t", "/t/p", "/t/e"):
            info = ens.get(path)
            assert info["exists"], path
            st = dict(info["stat"])
            st.pop("ctime")
            st.pop("mtime")
            stats[path] = (st, info["data"])
        counters = ens.counters()
        out = {
            "stats": stats,
            "children": ens.children("/t"),
            "ephemerals": ens.ephemeral_count(),
            "counters": {k: counters.get(k, 0) for k in ("create", "delete", "setData")},
            "zxid": ens.zxid(),
            "audit": ens.audit(),
        }
        s.close()
        return out
    finally:
        ens.stop()


def test_multi_and_single_ops_build_the_same_tree():
    single = tree_after(as_multi=False)
    multi = tree_after(as_multi=True)
    assert single["audit"] == [] and multi["audit"] == []
    assert single == multi
    # and it is the tree the six ops describe, not two equal wrong ones
    st_t, _ = single["stats"]["/t"]
    st_p, data_p = single["stats"]["/t/p"]
    st_e, _ = single["stats"]["/t/e"]
    assert (st_t["czxid"], st_t["pzxid"], st_t["cversion"], st_t["numChildren"]) == (1, 7, 4, 2)
    assert (st_p["czxid"], st_p["mzxid"], st_p["version"], st_p["dataLength"], data_p) == (2, 5, 2, 2, b"22")
    assert (st_e["czxid"], st_e["mzxid"], st_e["version"]) == (7, 7, 0) and st_e["ephemeralOwner"] != 0
    assert single["children"] == ["e", "p"] and single["ephemerals"] == 1
    assert single["counters"] == {"create": 4, "delete": 1, "setData": 2} and single["zxid"] == 7


# ------------------------- 2. multi deleting another session's ephemeral

def test_multi_deletes_another_sessions_ephemeral(ensemble):
    owner = make_client(ensemble)
    actor = make_client(ensemble)
    try:
        assert owner.mkdirp("/t") == ra.ZOK
        assert owner.create("/t/theirs", b"", True)[0] == ra.ZOK
        rc, _ = actor.multi([("delete", "/t/theirs"), ("create", "/t/mine", b"", True)])
        assert rc == ra.ZOK
        assert ensemble.audit() == []
        assert ensemble.ephemeral_count() == 1
        sid = owner.session_id()
        ensemble.expire_session(sid)
        assert wait_for(lambda: sid not in ensemble.session_ids(), 5)
        assert ensemble.audit() == []
        assert ensemble.get("/t/mine")["exists"] and ensemble.children("/t") == ["mine"]
    finally:
        actor.close()
        owner.close()


# -------------------- 3. order and multiplicity of one multi's events

def test_multi_watch_event_order_and_multiplicity(ensemble):
    actor = RawSession(ensemble)
    for i, path in enumerate(("/w", "/w/a", "/w/d")):
        actor.sock.sendall(create_req(1 + i, path, b"0"))
        ok(actor.replies(1)[0])
    watcher = RawSession(ensemble)
    arm = [
        exists_req(1, "/w/new", watch=True),
        watch_req(2, OP_GETDATA, "/w/a"),
        watch_req(3, OP_GETDATA, "/w/d"),
        watch_req(4, OP_GETCHILDREN, "/w/d"),
        watch_req(5, OP_GETCHILDREN, "/w"),
    ]
    watcher.sock.sendall(b"".join(arm))
    errs = [reply_fields(r)[2] for r in watcher.replies(len(arm))]
    assert errs == [-101, 0, 0, 0, 0]
    actor.sock.sendall(multi_req(9, [("create", "/w/new", b"", 0), ("set", "/w/a", b"1"), ("delete", "/w/d")]))
    ok(actor.replies(1)[0])
    events = [parse_event(r) for r in watcher.replies(4)]
    # data events in op order, then deletions, then parents deduplicated
    assert events == [
        (EV_CREATED, "/w/new"),
        (EV_CHANGED, "/w/a"),
        (EV_DELETED, "/w/d"),  # once, although a data and a child watch were armed
        (EV_CHILD, "/w"),      # once, although two ops changed its children
    ]
    assert_quiet(watcher)
    assert ensemble.audit() == []
    watcher.close()
    actor.close()


# --------------------------------------- 4. one event, several watchers

def test_one_event_reaches_every_watcher_with_equal_bytes(ensemble):
    actor = RawSession(ensemble)
    actor.sock.sendall(create_req(1, "/shared", b"0"))
    ok(actor.replies(1)[0])
    watchers = [RawSession(ensemble) for _ in range(3)]
    for w in watchers:
        w.sock.sendall(watch_req(1, OP_GETDATA, "/shared"))
        ok(w.replies(1)[0])
    actor.sock.sendall(setdata_req(2, "/shared", b"1"))
    ok(actor.replies(1)[0])
    frames = [recv_frame(w.sock) for w in watchers]
    assert parse_event(frames[0]) == (EV_CHANGED, "/shared")
    assert frames[0] == frames[1] == frames[2]
    assert_quiet(*watchers)  # one frame each, the watch was one-shot
    for w in watchers:
        w.close()
    actor.close()


# -------- 5. exists arms a watch on an absent path, getData does not

def test_only_exists_arms_a_watch_on_an_absent_path(ensemble):
    by_exists = RawSession(ensemble)
    by_getdata = RawSession(ensemble)
    by_exists.sock.sendall(exists_req(1, "/later", watch=True))
    by_getdata.sock.sendall(watch_req(1, OP_GETDATA, "/later"))
    assert reply_fields(by_exists.replies(1)[0])[2] == -101
    assert reply_fields(by_getdata.replies(1)[0])[2] == -101
    actor = RawSession(ensemble)
    actor.sock.sendall(create_req(1, "/later", b"x"))
    ok(actor.replies(1)[0])
    assert parse_event(recv_frame(by_exists.sock)) == (EV_CREATED, "/later")
    assert_quiet(by_getdata)
    for s in (by_exists, by_getdata, actor):
        s.close()
