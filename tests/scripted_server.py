"""A scripted ZooKeeper peer for client tests (a helper, not a test file).

A small threaded TCP server that speaks the ZooKeeper wire format with nothing
but `socket` and `struct`: it shares no code with the client under test, so a
mistake in the project's codec cannot cancel itself out. It does what a test's
script tells it, byte for byte, which is how a misbehaving server is played.

Every accepted connection becomes a `Conn`, kept in `ScriptedServer.conns`
with the monotonic time of the accept and every frame received on it as raw
bytes (length prefix included). The script is a callable over the `Conn`; it
runs in a thread of its own per connection, or, with `inline=True`, in the
accept thread, for servers that must keep up with a client reconnecting in a
busy loop. `set_script` swaps both while the server runs, for connections
accepted from then on.

Wire layout (all integers big-endian): a frame is a 4-byte length and a body.
Strings and buffers are a 4-byte length and the bytes, -1 for null; a vector is
a 4-byte count and the elements.
"""
import socket
import struct
import threading
import time

# opcodes and special xids, from the ZooKeeper protocol
OP_CREATE, OP_DELETE, OP_EXISTS, OP_GET, OP_SET, OP_CHILDREN = 1, 2, 3, 4, 5, 8
OP_PING, OP_MULTI, OP_CLOSE, OP_SETWATCHES = 11, 14, -11, 101
XID_EVENT, XID_PING, XID_SETWATCHES = -1, -2, -8

EV_CREATED, EV_DELETED, EV_CHANGED, EV_CHILD = 1, 2, 3, 4
STATE_SYNC_CONNECTED = 3

STAT_KEYS = ("czxid", "mzxid", "ctime", "mtime", "version", "cversion", "aversion",
             "ephemeralOwner", "dataLength", "numChildren", "pzxid")

DEFAULT_SESSION = 0x0123456789ABCDEF
DEFAULT_PASSWD = bytes(range(0xA0, 0xB0))


# ---- packing ----

def zk_string(b):
    if isinstance(b, str):
        b = b.encode()
    return struct.pack(">i", len(b)) + b


def zk_vector(items):
    return struct.pack(">i", len(items)) + b"".join(zk_string(i) for i in items)


def frame(body):
    return struct.pack(">i", len(body)) + body


def reply(xid, zxid, err, body=b""):
    """A framed reply: ReplyHeader{xid, zxid, err} and the body."""
    return frame(struct.pack(">iqi", xid, zxid, err) + body)


def request(xid, op, body=b""):
    """A framed request as a client must send it: RequestHeader{xid, type}."""
    return frame(struct.pack(">ii", xid, op) + body)


def stat(czxid=0, mzxid=0, ctime=0, mtime=0, version=0, cversion=0, aversion=0,
         ephemeralOwner=0, dataLength=0, numChildren=0, pzxid=0):
    return struct.pack(">qqqqiiiqiiq", czxid, mzxid, ctime, mtime, version, cversion,
                       aversion, ephemeralOwner, dataLength, numChildren, pzxid)


def watch_event(ev_type, path, zxid=-1, state=STATE_SYNC_CONNECTED):
    """A framed WatcherEvent, as ZooKeeper sends it: xid -1, zxid -1."""
    return reply(XID_EVENT, zxid, 0, struct.pack(">ii", ev_type, state) + zk_string(path))


def connect_request(timeout_ms, last_zxid=0, session_id=0, passwd=b"\x00" * 16):
    """The framed ConnectRequest a client must send (no readOnly byte)."""
    return frame(struct.pack(">iqiq", 0, last_zxid, timeout_ms, session_id) + zk_string(passwd))


def connect_response(timeout_ms, session_id, passwd, read_only=None):
    body = struct.pack(">iiq", 0, timeout_ms, session_id) + zk_string(passwd)
    if read_only is not None:
        body += b"\x01" if read_only else b"\x00"
    return frame(body)


ACL_OPEN = struct.pack(">ii", 1, 31) + zk_string("world") + zk_string("anyone")


def create_body(path, data, flags):
    return zk_string(path) + zk_string(data) + ACL_OPEN + struct.pack(">i", flags)


def parse_header(raw):
    """(xid, op, payload) of a raw request frame."""
    xid, op = struct.unpack(">ii", raw[4:12])
    return xid, op, raw[12:]


class Closed(Exception):
    """The peer closed the connection (or a read timed out)."""


class Conn:
    def __init__(self, server, sock, index, accepted_at):
        self.server = server
        self.sock = sock
        self.index = index
        self.accepted_at = accepted_at
        self.frames = []       # raw frames received, length prefix included
        self.last_send = None  # monotonic time just BEFORE the latest send
        self.eof = False       # the peer closed its side
        self.closed = False

    # -- receiving --

    def _recv_exact(self, n, timeout):
        buf = b""
        while len(buf) < n:
            try:
                self.sock.settimeout(timeout)
                chunk = self.sock.recv(n - len(buf))
            except (socket.timeout, OSError):
                raise Closed()
            if not chunk:
                self.eof = True
                raise Closed()
            buf += chunk
        return buf

    def read_frame(self, timeout=5.0):
        """One whole frame, recorded and returned raw. Raises Closed on EOF."""
        hdr = self._recv_exact(4, timeout)
        n = struct.unpack(">i", hdr)[0]
        raw = hdr + self._recv_exact(n, timeout)
        with self.server.lock:
            self.frames.append(raw)
        return raw

    def read_request(self, timeout=5.0):
        return parse_header(self.read_frame(timeout))

    def wait_eof(self, timeout=5.0):
        """True when the peer closes without sending anything more."""
        try:
            self.read_frame(timeout)
        except Closed:
            return self.eof
        return False

    # -- sending --

    def send_raw(self, data):
        self.last_send = time.monotonic()
        try:
            self.sock.sendall(data)
        except OSError:
            raise Closed()

    def send_frame(self, body):
        self.send_raw(frame(body))

    def send_bytewise(self, data):
        """One send per byte (Nagle is off, so they leave one by one)."""
        for i in range(len(data)):
            self.send_raw(data[i:i + 1])

    def handshake(self, timeout_ms=30000, session_id=DEFAULT_SESSION, passwd=DEFAULT_PASSWD,
                  read_only=None):
        """Read the ConnectRequest, answer it; returns the raw request."""
        raw = self.read_frame()
        self.send_raw(connect_response(timeout_ms, session_id, passwd, read_only))
        return raw

    def close(self):
        """End the connection; safe from any thread. Only shuts the socket
        down: that sends the FIN and wakes a script blocked in a read. The
        descriptor itself is released by the thread that runs the script, once
        the script is over, so that its number cannot pass to a newer
        connection while the script is still about to read from it."""
        self.closed = True
        try:
            self.sock.shutdown(socket.SHUT_RDWR)
        except OSError:
            pass

    def _release(self):
        self.sock.close()


class ScriptedServer:
    def __init__(self, script, inline=False):
        self._mode = (script, inline)
        self.lock = threading.Lock()
        self.conns = []
        self.errors = []  # exceptions a script raised (other than Closed)
        self._threads = []
        self._stopping = False
        self._lsock = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        self._lsock.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        self._lsock.bind(("127.0.0.1", 0))
        self._lsock.listen(128)
        self._lsock.settimeout(0.05)
        self.port = self._lsock.getsockname()[1]
        self.addr = ("127.0.0.1", self.port)
        self._accept_thread = threading.Thread(target=self._accept_loop, daemon=True)
        self._accept_thread.start()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.stop()

    def set_script(self, script, inline=False):
        """For connections accepted from now on (the pair changes as one)."""
        self._mode = (script, inline)

    def _accept_loop(self):
        while not self._stopping:
            try:
                sock, _ = self._lsock.accept()
            except socket.timeout:
                continue
            except OSError:
                return
            now = time.monotonic()
            sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            with self.lock:
                conn = Conn(self, sock, len(self.conns), now)
                self.conns.append(conn)
            script, inline = self._mode
            if inline:
                self._run(script, conn)
            else:
                t = threading.Thread(target=self._run, args=(script, conn), daemon=True)
                with self.lock:
                    self._threads.append(t)
                t.start()

    def _run(self, script, conn):
        try:
            script(conn)
        except Closed:
            pass
        except Exception as e:  # a bug in the script: surfaces in stop()
            with self.lock:
                self.errors.append(e)
        finally:
            conn.close()
            conn._release()

    # -- what the tests read --

    def accepted(self):
        with self.lock:
            return list(self.conns)

    def frames(self, index):
        with self.lock:
            return list(self.conns[index].frames) if index < len(self.conns) else []

    def stop(self):
        """Close the listener and every live socket, join every thread."""
        self._stopping = True
        for c in self.accepted():  # wakes an inline script blocked in a read
            c.close()
        self._accept_thread.join(5)
        self._lsock.close()
        with self.lock:
            conns, threads = list(self.conns), list(self._threads)
        for c in conns:
            c.close()
        for t in threads:
            t.join(5)
        for c in conns:
            c._release()
        alive = [t for t in threads if t.is_alive()] + (
            [self._accept_thread] if self._accept_thread.is_alive() else [])
        assert not alive, "scripted server: %d thread(s) did not end" % len(alive)
        assert not self.errors, "scripted server: script raised %r" % (self.errors,)


# ---- ready-made scripts ----

def accept_and_close(conn):
    pass  # _run closes the connection


def read_and_close(conn):
    conn.read_frame(timeout=2.0)


def reply_two_byte_frame(conn):
    conn.read_frame(timeout=2.0)
    conn.send_raw(frame(b"\x00\x00"))
    conn.wait_eof(timeout=2.0)


class Responder:
    """Handshake, then answer requests until the peer goes away.

    `on_request(conn, xid, op, payload)` returns the bytes to send (whole
    frames, see `reply`), or None to send nothing. Pings and closeSession are
    answered here. `zxid()` hands out rising zxids for scripts that do not care
    which. A connection whose index is in `drop` is closed right after the
    accept instead.
    """

    def __init__(self, on_request=None, **handshake):
        self.on_request = on_request or (lambda conn, xid, op, payload: reply(xid, self.zxid(), 0))
        self.handshake_args = handshake
        self._zxid = 0
        self._lock = threading.Lock()

    def zxid(self):
        with self._lock:
            self._zxid += 1
            return self._zxid

    def __call__(self, conn):
        conn.handshake(**self.handshake_args)
        self.serve(conn)

    def serve(self, conn):
        while True:
            xid, op, payload = conn.read_request(timeout=10.0)
            if op == OP_PING:
                conn.send_raw(reply(XID_PING, 0, 0))
            elif op == OP_CLOSE:
                conn.send_raw(reply(xid, self.zxid(), 0))
                conn.wait_eof()
                return
            elif op == OP_SETWATCHES:
                conn.send_raw(reply(XID_SETWATCHES, 0, 0))
            else:
                out = self.on_request(conn, xid, op, payload)
                if out:
                    conn.send_raw(out)
