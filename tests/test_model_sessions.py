"""Multi-session model test: three client sessions (on both IO loops of a
two-thread ensemble) and one raw-wire session against a pure-Python model of
the tree that predicts, for every operation, the return code AND the whole
observable state: data, version, the parent's cversion, numChildren,
dataLength, ephemeralOwner, the sorted child list, the SEQUENCE name; zxids
by relation (czxid <= mzxid, a set raises mzxid, a child create/delete raises
the parent's pzxid, nothing exceeds ens.zxid(), everything untouched stays
exactly as it was). Payload lengths sit on the inline capacities of the node
store's block classes for the path at hand, and one 200-byte name puts nodes
in more than one class, so recycled blocks change occupants and data moves in
and out of line. All operations are issued from the test thread, so the model
is exact. ens.audit() == [] after every step.

tests/test_model.py (one session, watches) stays as it is; this runs beside it.
A directed table of transactions against the same model is at the end."""
import copy
import os
import struct
import time

import pytest
from hypothesis import HealthCheck, settings
from hypothesis import strategies as st
from hypothesis.stateful import RuleBasedStateMachine, initialize, invariant, rule, run_state_machine_as_test

import registrar_amd as ra
from conftest import make_client, wait_for
from test_hotpath import (EPHEMERAL, SEQUENCE, STAT_LEN, RawSession, create_req, frame, jstr, parse_stat,
                          recv_frame, reply_fields)
from test_nodestore import (MULTI_HDR, OP_CHECK, OP_CREATE, OP_DELETE, OP_SETDATA, m_check, m_create,
                            m_delete, m_setdata, multi_req, pattern)

ZMARSHALLINGERROR = -5
ZRUNTIMEINCONSISTENCY = -2

LONG = "L" * 200
NAMES = ["a", "b", "c", "d"]  # the alphabet of tests/test_model.py
ALL_NAMES = NAMES + [LONG]
VERSIONS = [-1, 0, 1, 7]
LAYOUT = ra.Ensemble.node_store_layout()


def payload_lengths(path_len):
    """0, 1, one below / at / one above the inline capacity of the first three
    block classes that can hold a path of path_len bytes, and one byte more
    than the largest class (such a node is never cached)."""
    out = {0, 1, LAYOUT["classes"][-1] + 1}
    caps = [c - LAYOUT["header_bytes"] - path_len for c in LAYOUT["classes"]]
    for cap in [c for c in caps if c >= 0][:3]:
        out.update(d for d in (cap - 1, cap, cap + 1) if d >= 0)
    return sorted(out)


def payload(path, k, seed):
    lens = payload_lengths(len(path))
    return pattern(lens[k % len(lens)], seed)


def parent_of(path):
    p = path.rsplit("/", 1)[0]
    return p if p else "/"


# ------------------------------------------------------------------- the model

class MNode:
    __slots__ = ("data", "version", "cversion", "owner")

    def __init__(self, data, owner):
        self.data, self.version, self.cversion, self.owner = data, 0, 0, owner


class Model:
    """path -> MNode, plus what the last operation must have done to zxids:
    `created` (czxid newer than anything before the operation), `m` (mzxid
    raised), `p` (pzxid raised), `deleted`. Ops are tuples:
    ("create", path, data, flags) ("delete", path, version)
    ("set", path, data, version) ("check", path, version)."""

    def __init__(self):
        self.nodes = {"/": MNode(b"", 0)}
        self.reset_effects()

    def reset_effects(self):
        self.created, self.m, self.p, self.deleted = set(), set(), set(), set()

    def children(self, path):
        return sorted(n.rsplit("/", 1)[1] for n in self.nodes if n != "/" and parent_of(n) == path)

    def ephemerals(self, sid=None):
        return [p for p, n in self.nodes.items() if n.owner and (sid is None or n.owner == sid)]

    def create(self, path, data, owner, sequence=False):
        """Returns (rc, final path)."""
        par = parent_of(path)
        if par not in self.nodes:
            return ra.ZNONODE, None
        if self.nodes[par].owner:
            return ra.ZNOCHILDRENFOREPHEMERALS, None
        if sequence:
            path = path + "%010d" % self.nodes[par].cversion
        if path in self.nodes:
            return ra.ZNODEEXISTS, None
        self.nodes[path] = MNode(data, owner)
        self.nodes[par].cversion += 1
        self.created.add(path)
        self.deleted.discard(path)
        self.p.add(par)
        return ra.ZOK, path

    def delete(self, path, version):
        if path not in self.nodes or path == "/":
            return ra.ZNONODE
        if self.children(path):
            return ra.ZNOTEMPTY
        if version != -1 and version != self.nodes[path].version:
            return ra.ZBADVERSION
        del self.nodes[path]
        self.nodes[parent_of(path)].cversion += 1
        self.p.add(parent_of(path))
        for s in (self.created, self.m, self.p):
            s.discard(path)
        self.deleted.add(path)
        return ra.ZOK

    def set(self, path, data, version):
        if path not in self.nodes:
            return ra.ZNONODE
        if version != -1 and version != self.nodes[path].version:
            return ra.ZBADVERSION
        self.nodes[path].data = data
        self.nodes[path].version += 1
        self.m.add(path)
        return ra.ZOK

    def check(self, path, version):
        if path not in self.nodes:
            return ra.ZNONODE
        if version != -1 and version != self.nodes[path].version:
            return ra.ZBADVERSION
        return ra.ZOK

    def apply(self, op, sid):
        """One op of a transaction. Returns (rc, detail): the created path or
        the version a setData reached."""
        if op[0] == "create":
            if op[3] & SEQUENCE:
                return ZMARSHALLINGERROR, None  # SEQUENCE inside a transaction is refused
            return self.create(op[1], op[2], sid if op[3] & EPHEMERAL else 0)
        if op[0] == "delete":
            return self.delete(op[1], op[2]), None
        if op[0] == "set":
            rc = self.set(op[1], op[2], op[3])
            return rc, self.nodes[op[1]].version if rc == ra.ZOK else None
        return self.check(op[1], op[2]), None

    def drop_session(self, sid):
        for p in self.ephemerals(sid):
            assert self.delete(p, -1) == ra.ZOK


def run_txn(model, ops, sid):
    """All-or-nothing on a copy. Returns (rc, index of the failing op or None,
    per-op details, the model to go on with)."""
    trial = copy.deepcopy(model)
    details = []
    for i, op in enumerate(ops):
        rc, detail = trial.apply(op, sid)
        if rc != ra.ZOK:
            return rc, i, None, model
        details.append(detail)
    return ra.ZOK, None, details, trial


# ---------------------------------------------------------------- the raw wire

class RawSeqSession(RawSession):
    """A raw session with a long timeout (it sits idle between rules) that
    remembers its session id."""

    def __init__(self, ens):
        import socket
        host, port = ens.connect_string().split(",")[0].rsplit(":", 1)
        self.sock = socket.create_connection((host, int(port)), timeout=5)
        self.sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        self.sock.sendall(frame(struct.pack(">iqiq", 0, 0, 30000, 0) + struct.pack(">i", 16) + b"\x00" * 16))
        rep = recv_frame(self.sock)
        _, _, self.sid = struct.unpack(">iiq", rep[4:20])
        assert self.sid != 0
        self.xid = 0

    def session_id(self):
        return self.sid

    def call(self, build):
        self.xid += 1
        self.sock.sendall(build(self.xid))
        xid, zxid, err, body = reply_fields(recv_frame(self.sock))
        assert xid == self.xid
        return zxid, err, body

    def create(self, path, data, flags):
        zxid, err, body = self.call(lambda xid: create_req(xid, path, data, flags))
        if err != ra.ZOK:
            return err, None
        n = struct.unpack(">i", body[:4])[0]
        assert len(body) == 4 + n
        return err, body[4:].decode()

    def multi(self, ops):
        """ops in the model's form. Returns (rc, per-op list): on success the
        created path / the setData Stat / None; on failure the per-op codes."""
        wire = []
        for op in ops:
            if op[0] == "create":
                wire.append(m_create(op[1], op[2], op[3]))
            elif op[0] == "delete":
                wire.append(m_delete(op[1], op[2]))
            elif op[0] == "set":
                wire.append(m_setdata(op[1], op[2], op[3]))
            else:
                wire.append(m_check(op[1], op[2]))
        zxid, err, body = self.call(lambda xid: multi_req(xid, wire))
        out, off = [], 0
        for typ, _ in wire:
            rtype, done, rerr = struct.unpack(">i?i", body[off:off + MULTI_HDR])
            off += MULTI_HDR
            assert not done
            if err != ra.ZOK:
                assert rtype == -1
                code = struct.unpack(">i", body[off:off + 4])[0]
                off += 4
                assert code == rerr
                out.append(code)
                continue
            assert rtype == typ and rerr == 0
            if typ == OP_CREATE:
                n = struct.unpack(">i", body[off:off + 4])[0]
                out.append(body[off + 4:off + 4 + n].decode())
                off += 4 + n
            elif typ == OP_SETDATA:
                out.append(parse_stat(body[off:off + STAT_LEN]))
                off += STAT_LEN
            else:
                out.append(None)
        assert struct.unpack(">i?i", body[off:off + MULTI_HDR]) == (-1, True, -1)
        assert off + MULTI_HDR == len(body)
        return err, out, zxid


# ------------------------------------------------------- model against ensemble

class Checker:
    """Compares the ensemble with a Model after every operation."""

    def __init__(self, ens):
        self.ens = ens
        self.model = Model()
        self.seen = {"/": ens.get("/")["stat"]}
        self.zx_before = ens.zxid()

    def begin(self):
        self.model.reset_effects()
        self.zx_before = self.ens.zxid()

    def sweep(self):
        """The whole tree, read in-process: every Stat field but the clocks."""
        ens, model = self.ens, self.model
        zx = ens.zxid()
        assert zx >= self.zx_before
        now = {}
        for path, node in model.nodes.items():
            info = ens.get(path)
            assert info["exists"], "%s is missing" % path
            s = info["stat"]
            now[path] = s
            where = "%s: %r" % (path[:40], s)
            assert info["data"] == node.data, "stale or wrong data at %s" % path[:40]
            assert s["dataLength"] == len(node.data), where
            assert s["version"] == node.version, where
            assert s["cversion"] == node.cversion, where
            assert s["ephemeralOwner"] == node.owner, where
            kids = model.children(path)
            assert s["numChildren"] == len(kids), where
            assert ens.children(path) == kids, where
            assert 0 <= s["czxid"] <= s["mzxid"] <= zx, where
            # pzxid is 0 until the first child change (Apache ZooKeeper starts it
            # at czxid; the recorded wire fixtures pin this ensemble's 0)
            assert s["pzxid"] <= zx and (s["pzxid"] == 0 or s["pzxid"] > s["czxid"]), where
            old = self.seen.get(path)
            if path in model.created or old is None:
                assert s["czxid"] > self.zx_before, where
                continue
            assert s["czxid"] == old["czxid"] and s["ctime"] == old["ctime"], where
            if path in model.m:
                assert s["mzxid"] > old["mzxid"] and s["mzxid"] > self.zx_before, where
            else:
                assert s["mzxid"] == old["mzxid"] and s["mtime"] == old["mtime"], where
            if path in model.p:
                assert s["pzxid"] > old["pzxid"] and s["pzxid"] > self.zx_before, where
            else:
                assert s["pzxid"] == old["pzxid"], where
        for path in self.seen:
            if path not in model.nodes:
                assert not ens.get(path)["exists"], "%s should be gone" % path[:40]
        assert ens.node_count() == len(model.nodes) - 1
        assert ens.ephemeral_count() == len(model.ephemerals())
        assert ens.audit() == []
        bound = LAYOUT["shards"] * len(LAYOUT["classes"]) * LAYOUT["max_cached_per_class"]
        assert ens.counters()["node_blocks_cached"] <= bound
        self.seen = now

    def read_back(self, reader):
        """What the last operation touched, over the wire through `reader`
        (another session than the writer): the reply equals the tree."""
        model = self.model
        for path in sorted(model.created | model.m | model.p):
            node = model.nodes[path]
            rc, data, s = reader.get(path)
            assert (rc, data) == (ra.ZOK, node.data), path[:40]
            assert s == self.ens.get(path)["stat"], path[:40]
            assert reader.exists(path) == (ra.ZOK, s)
            assert reader.get_children(path) == (ra.ZOK, model.children(path))
        for path in sorted(model.deleted):
            assert reader.exists(path)[0] == ra.ZNONODE
            assert reader.get(path)[0] == ra.ZNONODE
            assert reader.get_children(path)[0] == ra.ZNONODE

    def raw_multi(self, raw, ops):
        """One transaction over the raw session, verdict and reply body
        against the model. Returns (rc, failing index)."""
        self.begin()
        want, fail_at, details, after = run_txn(self.model, ops, raw.session_id())
        rc, per_op, zxid = raw.multi(ops)
        assert rc == want, "multi %r: got %s want %s" % ([o[:2] for o in ops], ra.error_name(rc),
                                                          ra.error_name(want))
        if rc != ra.ZOK:
            # the model's error at the first failing op, nothing applied
            assert per_op[fail_at] == want
            assert [c for i, c in enumerate(per_op) if i != fail_at] == [ZRUNTIMEINCONSISTENCY] * (len(ops) - 1)
            return rc, fail_at
        self.model = after
        for op, got, detail in zip(ops, per_op, details):
            if op[0] == "create":
                assert got == detail == op[1]
            elif op[0] == "set":
                assert got["version"] == detail and got["data_length"] == len(op[2])
                assert self.zx_before < got["mzxid"] <= zxid
        return rc, None


# --------------------------------------------------------------- the machine

def path_strategy():
    return st.lists(st.sampled_from(ALL_NAMES), min_size=1, max_size=3).map(lambda p: "/" + "/".join(p))


def target_strategy(existing=3, child=1, fresh=1):
    """A path from the alphabet, or an existing node by index (so SEQUENCE
    nodes and deep nodes are hit too), or a child of an existing node; the
    weights say how often each kind is drawn."""
    return st.one_of([st.integers(0, 63)] * existing
                     + [st.tuples(st.integers(0, 63), st.sampled_from(ALL_NAMES))] * child
                     + [path_strategy()] * fresh)


def create_target():
    return target_strategy(existing=1, child=3, fresh=2)


class SessionsMachine(RuleBasedStateMachine):
    @initialize()
    def setup(self):
        self.ens = ra.Ensemble(servers=1, tick_ms=50, min_session_timeout_ms=200, io_threads=2)
        self.ens.start()
        # created in order: connections go round-robin over the two IO loops
        self.clients = [make_client(self.ens, session_timeout_ms=30000) for _ in range(3)]
        self.raw = RawSeqSession(self.ens)
        self.chk = Checker(self.ens)
        self.reader = self.clients[0]
        self.seed = 0
        # a small tree to start from, made through the same checked rules:
        # every session owns something and two block classes are in use
        for k, path, size, ephemeral in [(0, "/a", 3, False), (1, "/a/b", 4, False), (2, "/a/b/c", 1, True),
                                         (1, "/b", 0, True), (0, "/" + LONG, 2, False),
                                         (2, "/" + LONG + "/d", 5, True)]:
            self.create(k, path, size, ephemeral)
            self.tree_matches_model()
        self.create_sequence("/a", 3, True, False)
        self.tree_matches_model()

    def teardown(self):
        if hasattr(self, "ens"):
            for c in getattr(self, "clients", []):
                c.close()
            if hasattr(self, "raw"):
                self.raw.close()
            self.ens.stop()

    def resolve(self, spec):
        if isinstance(spec, str):
            return spec
        existing = sorted(p for p in self.chk.model.nodes if p != "/")
        idx, name = spec if isinstance(spec, tuple) else (spec, None)
        if not existing:
            return "/" + (name or "a")
        base = existing[idx % len(existing)]
        if name is None or base.count("/") >= 3:
            return base
        return base + "/" + name

    def data_for(self, path, k):
        self.seed += 1
        return payload(path, k, self.seed)

    def wrote(self, k):
        """Session k wrote: later reads go through the next one."""
        self.reader = self.clients[(k + 1) % 3]

    # ---- single operations

    @rule(k=st.integers(0, 2), where=create_target(), size=st.integers(0, 11), ephemeral=st.booleans())
    def create(self, k, where, size, ephemeral):
        path = self.resolve(where)
        data = self.data_for(path, size)
        c = self.clients[k]
        self.chk.begin()
        want, _ = self.chk.model.create(path, data, c.session_id() if ephemeral else 0)
        rc, created = c.create(path, data, ephemeral)
        assert rc == want, "create %s: got %s want %s" % (path[:40], ra.error_name(rc), ra.error_name(want))
        if rc == ra.ZOK:
            assert created == path
        self.wrote(k)

    @rule(where=target_strategy(), size=st.integers(0, 11), ephemeral=st.booleans(),
          at_root=st.booleans())
    def create_sequence(self, where, size, ephemeral, at_root):
        prefix = "/s" if at_root else self.resolve(where) + "/s"
        data = self.data_for(prefix + "0123456789", size)
        self.chk.begin()
        want, want_path = self.chk.model.create(prefix, data, self.raw.session_id() if ephemeral else 0,
                                                sequence=True)
        rc, created = self.raw.create(prefix, data, SEQUENCE | (EPHEMERAL if ephemeral else 0))
        assert rc == want, "create SEQUENCE %s: got %s want %s" % (prefix[:40], ra.error_name(rc),
                                                                 ra.error_name(want))
        assert created == want_path
        self.reader = self.clients[0]

    @rule(k=st.integers(0, 2), where=target_strategy(), version=st.sampled_from(VERSIONS))
    def delete(self, k, where, version):
        path = self.resolve(where)
        self.chk.begin()
        want = self.chk.model.delete(path, version)
        rc = self.clients[k].delete_(path, version)
        assert rc == want, "delete %s v%d: got %s want %s" % (path[:40], version, ra.error_name(rc),
                                                              ra.error_name(want))
        self.wrote(k)

    @rule(k=st.integers(0, 2), where=target_strategy(), size=st.integers(0, 11),
          version=st.sampled_from(VERSIONS))
    def set_data(self, k, where, size, version):
        path = self.resolve(where)
        data = self.data_for(path, size)
        self.chk.begin()
        want = self.chk.model.set(path, data, version)
        rc = self.clients[k].set(path, data, version)
        assert rc == want, "set %s v%d: got %s want %s" % (path[:40], version, ra.error_name(rc),
                                                           ra.error_name(want))
        self.wrote(k)

    # create and set once more, aimed at nodes that exist: without them most
    # steps of a short run answer NO_NODE on a nearly empty tree.

    @rule(k=st.integers(0, 2), idx=st.integers(0, 63), name=st.sampled_from(ALL_NAMES),
          size=st.integers(0, 11), ephemeral=st.booleans())
    def create_child(self, k, idx, name, size, ephemeral):
        self.create(k, (idx, name), size, ephemeral)

    @rule(k=st.integers(0, 2), idx=st.integers(0, 63), size=st.integers(0, 11),
          version=st.sampled_from([-1, -1, 0, 1, 2]))
    def set_existing(self, k, idx, size, version):
        self.set_data(k, idx, size, version)

    # ---- transactions

    @rule(k=st.integers(0, 2),
          ops=st.lists(st.tuples(st.sampled_from(["create", "delete"]), target_strategy(), st.integers(0, 11),
                                 st.booleans()), min_size=1, max_size=4))
    def multi_client(self, k, ops):
        c = self.clients[k]
        mops, cops = [], []
        for kind, where, size, eph in ops:
            path = self.resolve(where)
            if kind == "create":
                data = self.data_for(path, size)
                mops.append(("create", path, data, EPHEMERAL if eph else 0))
                cops.append(("create", path, data, eph))
            else:
                mops.append(("delete", path, -1))
                cops.append(("delete", path))
        self.chk.begin()
        want, fail_at, _, after = run_txn(self.chk.model, mops, c.session_id())
        rc, per_op = c.multi(cops)
        assert rc == want, "multi %r: got %s want %s" % ([o[:2] for o in mops], ra.error_name(rc),
                                                          ra.error_name(want))
        if rc == ra.ZOK:
            self.chk.model = after
            assert per_op == [ra.ZOK] * len(mops)
        else:
            assert per_op[fail_at] == want
        self.wrote(k)

    @rule(ops=st.lists(st.tuples(st.sampled_from(["create", "delete", "set", "set", "check", "check"]),
                                 target_strategy(), st.integers(0, 11), st.booleans(),
                                 st.sampled_from(VERSIONS + [2])), min_size=1, max_size=4))
    def multi_raw(self, ops):
        mops = []
        for kind, where, size, eph, version in ops:
            path = self.resolve(where)
            if kind == "create":
                mops.append(("create", path, self.data_for(path, size), EPHEMERAL if eph else 0))
            elif kind == "delete":
                mops.append(("delete", path, version))
            elif kind == "set":
                mops.append(("set", path, self.data_for(path, size), version))
            else:
                mops.append(("check", path, version))
        self.chk.raw_multi(self.raw, mops)
        self.reader = self.clients[0]

    # ---- session death: exactly that session's ephemerals go

    def replace_client(self, k):
        self.clients[k].close()
        self.clients[k] = make_client(self.ens, session_timeout_ms=30000)
        self.reader = self.clients[(k + 1) % 3]

    @rule(k=st.integers(0, 3), expire=st.booleans())
    def end_session(self, k, expire):
        """One rule for both ways to die, so that session death stays a small
        share of the steps; the raw session can only be expired."""
        if expire or k == 3:
            self.expire_session(k)
        else:
            self.close_session(k)

    def expire_session(self, k):
        self.chk.begin()
        if k == 3:
            sid = self.raw.session_id()
            self.ens.expire_session(sid)  # returns when the drain is done
            self.raw.close()
            self.raw = RawSeqSession(self.ens)
            self.reader = self.clients[0]
        else:
            c = self.clients[k]
            sid = c.session_id()
            self.ens.expire_session(sid)
            assert wait_for(lambda: c.state() == "expired")
            self.replace_client(k)
        assert sid not in self.ens.session_ids()
        self.chk.model.drop_session(sid)

    def close_session(self, k):
        self.chk.begin()
        c = self.clients[k]
        sid = c.session_id()
        owned = self.chk.model.ephemerals(sid)
        c.close()
        # the close is acknowledged before the session's ephemerals are
        # drained: wait for the drain, so no expiry is in flight at the audit
        assert wait_for(lambda: sid not in self.ens.session_ids()
                        and not any(self.ens.get(p)["exists"] for p in owned))
        self.chk.model.drop_session(sid)
        self.replace_client(k)

    # ---- after every step

    @invariant()
    def tree_matches_model(self):
        if not hasattr(self, "chk"):
            return
        self.chk.sweep()
        self.chk.read_back(self.reader)
        self.chk.model.reset_effects()


MODEL_SETTINGS = settings(
    max_examples=int(os.environ.get("MODEL_EXAMPLES", "40")),
    stateful_step_count=40,
    deadline=None,
    derandomize=True,  # a failure on a shared machine reproduces
    suppress_health_check=[HealthCheck.too_slow],
)


def test_sessions_model():
    t0 = time.perf_counter()
    try:
        run_state_machine_as_test(SessionsMachine, settings=MODEL_SETTINGS)
    finally:
        print("sessions model: %.1f s for %d examples of up to %d steps" % (
            time.perf_counter() - t0, MODEL_SETTINGS.max_examples, MODEL_SETTINGS.stateful_step_count))


# --------------------------------------------------- directed transaction cases

def C(path, data=b"", flags=0):
    return ("create", path, data, flags)


def D(path, version=-1):
    return ("delete", path, version)


def S(path, data, version=-1):
    return ("set", path, data, version)


def K(path, version):
    return ("check", path, version)


OK, NO_NODE, NOT_EMPTY, BAD_VERSION = ra.ZOK, ra.ZNONODE, ra.ZNOTEMPTY, ra.ZBADVERSION

# (name, setup transaction, transaction, verdict, index of the failing op,
#  tree afterwards under the row's root: relative path -> (data, version,
#  cversion, ephemeral); "" is the root of the row). Paths are relative to the
# row's root. A failed transaction leaves the setup's tree.
TXN_ROWS = [
    ("delete then create the same path: version restarts, check(0) passes",
     [C("/x", b"old"), S("/x", b"old2"), S("/x", b"old3")],
     [D("/x", 2), C("/x", b"new"), K("/x", 0)], OK, None,
     {"": (b"", 0, 3, False), "/x": (b"new", 0, 0, False)}),
    ("delete then create the same path, then check the OLD version",
     [C("/x", b"old"), S("/x", b"old2")],
     [D("/x"), C("/x", b"new"), K("/x", 1)], BAD_VERSION, 2,
     {"": (b"", 0, 1, False), "/x": (b"old2", 1, 0, False)}),
    ("create then delete the same path",
     [],
     [C("/y", b"gone"), D("/y", 0)], OK, None,
     {"": (b"", 0, 2, False)}),
    ("create a parent and its child",
     [],
     [C("/p", b"P"), C("/p/c", b"C", EPHEMERAL)], OK, None,
     {"": (b"", 0, 1, False), "/p": (b"P", 0, 1, False), "/p/c": (b"C", 0, 0, True)}),
    ("create a child, then delete the parent",
     [C("/p")],
     [C("/p/c"), D("/p")], NOT_EMPTY, 1,
     {"": (b"", 0, 1, False), "/p": (b"", 0, 0, False)}),
    ("delete the children, then the parent",
     [C("/p"), C("/p/c1"), C("/p/c2", b"", EPHEMERAL)],
     [D("/p/c1"), D("/p/c2"), D("/p")], OK, None,
     {"": (b"", 0, 2, False)}),
    ("delete one child of two, then the parent",
     [C("/p"), C("/p/c1"), C("/p/c2")],
     [D("/p/c1"), D("/p")], NOT_EMPTY, 1,
     {"": (b"", 0, 1, False), "/p": (b"", 0, 2, False), "/p/c1": (b"", 0, 0, False),
      "/p/c2": (b"", 0, 0, False)}),
    ("setData twice, then check the version reached inside the transaction",
     [C("/x", b"0")],
     [S("/x", b"1", 0), S("/x", b"22", 1), K("/x", 2)], OK, None,
     {"": (b"", 0, 1, False), "/x": (b"22", 2, 0, False)}),
    ("setData twice, then check the version from before the transaction",
     [C("/x", b"0")],
     [S("/x", b"1"), S("/x", b"22"), K("/x", 0)], BAD_VERSION, 2,
     {"": (b"", 0, 1, False), "/x": (b"0", 0, 0, False)}),
    ("setData after a delete of the same path",
     [C("/x", b"0")],
     [D("/x"), S("/x", b"late")], NO_NODE, 1,
     {"": (b"", 0, 1, False), "/x": (b"0", 0, 0, False)}),
    ("create under a parent created ephemeral in the same transaction",
     [],
     [C("/e", b"", EPHEMERAL), C("/e/kid")], ra.ZNOCHILDRENFOREPHEMERALS, 1,
     {"": (b"", 0, 0, False)}),
    ("an ephemeral replaced by a persistent node in the transaction takes children",
     [C("/e", b"", EPHEMERAL)],
     [D("/e"), C("/e", b"P"), C("/e/kid", b"k")], OK, None,
     {"": (b"", 0, 3, False), "/e": (b"P", 0, 1, False), "/e/kid": (b"k", 0, 0, False)}),
    ("a create carrying SEQUENCE",
     [],
     [C("/ok"), C("/seq-", b"", SEQUENCE)], ZMARSHALLINGERROR, 1,
     {"": (b"", 0, 0, False)}),
    ("delete by a version that an earlier op of the transaction made stale",
     [C("/x", b"0")],
     [S("/x", b"1", 0), D("/x", 0)], BAD_VERSION, 1,
     {"": (b"", 0, 1, False), "/x": (b"0", 0, 0, False)}),
    ("delete by the version an earlier op of the transaction reached",
     [C("/x", b"0")],
     [S("/x", b"1", 0), D("/x", 1)], OK, None,
     {"": (b"", 0, 2, False)}),
    ("create over a node deleted and created again earlier in the transaction",
     [C("/x")],
     [D("/x"), C("/x"), C("/x")], ra.ZNODEEXISTS, 2,
     {"": (b"", 0, 1, False), "/x": (b"", 0, 0, False)}),
]


@pytest.fixture(scope="module")
def txn_bench():
    ens = ra.Ensemble(servers=1, tick_ms=50, min_session_timeout_ms=200, io_threads=2)
    ens.start()
    raw = RawSeqSession(ens)
    reader = make_client(ens, session_timeout_ms=30000)
    chk = Checker(ens)
    yield ens, raw, reader, chk
    reader.close()
    raw.close()
    ens.stop()


@pytest.mark.parametrize("row", range(len(TXN_ROWS)), ids=lambda i: TXN_ROWS[i][0][:50].replace(" ", "_"))
def test_transaction_overlay(txn_bench, row):
    """Each row: a transaction, the verdict (checked against the row AND the
    model), the index of the failing op, and the tree afterwards (checked
    against the row, the model, and over the wire)."""
    ens, raw, reader, chk = txn_bench
    name, setup, txn, verdict, fail_at, tree = TXN_ROWS[row]
    root = "/row%d" % row

    def rooted(ops):
        return [(op[0], root + op[1]) + op[2:] for op in ops]

    def step(ops):
        out = chk.raw_multi(raw, ops)
        chk.sweep()
        chk.read_back(reader)
        return out

    assert step([C(root)]) == (OK, None)
    if setup:
        assert step(rooted(setup)) == (OK, None), "setup of %r" % name
    assert step(rooted(txn)) == (verdict, fail_at), name
    got = {}
    for path, node in chk.model.nodes.items():
        if path == root or path.startswith(root + "/"):
            got[path[len(root):]] = (node.data, node.version, node.cversion, node.owner == raw.session_id())
            assert node.owner in (0, raw.session_id())
    assert got == tree, name
    # once more without the model in between: the tree itself
    for rel, (data, version, cversion, eph) in tree.items():
        info = ens.get(root + rel)
        assert info["exists"] and info["data"] == data
        s = info["stat"]
        assert (s["version"], s["cversion"], s["ephemeralOwner"]) == (version, cversion,
                                                                      raw.session_id() if eph else 0)
