#!/usr/bin/env python3
"""A Binder-style consumer: discover live instances of a service through a
Resolver, which reads the records registrar writes once and keeps its view
current with watches.

Usage:
    python examples/consumer.py --servers HOST:PORT[,HOST:PORT...] DOMAIN
        [--follow] [--local-address A]

Example (against a demo ensemble + daemon):
    ./bin/zkensembled -n 1           # note the port
    ./bin/registrard -f etc/config.example.json &
    python examples/consumer.py --servers 127.0.0.1:PORT test.coal.example.com
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import registrar_amd as ra  # noqa: E402


def show(domain, snap):
    svc = snap["service"]
    if svc:
        print("SRV %s.%s.%s port=%s ttl=%s" % (svc["srvce"], svc["proto"], domain, svc["port"], svc.get("ttl")))
    print("%d live instance(s) under %s%s:" % (len(snap["hosts"]), ra.domain_to_path(domain),
                                               " (stale)" if snap["stale"] else ""))
    for h in snap["hosts"]:  # same-node instances first
        gpu = h["gpu"]
        extra = " xgmiRank=%s gpu=%s" % (gpu["xgmiRank"], gpu["index"]) if gpu else ""
        print("  %-24s %-15s session=0x%x%s%s"
              % (h["name"], h["address"], h["ephemeral_owner"], extra, " local" if h["local"] else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--servers", required=True)
    ap.add_argument("domain")
    ap.add_argument("--follow", action="store_true", help="keep watching for changes")
    ap.add_argument("--local-address", default="", help="this node's address: its instances are listed first")
    args = ap.parse_args()

    servers = [(hp.rsplit(":", 1)[0], int(hp.rsplit(":", 1)[1])) for hp in args.servers.split(",")]
    r = ra.Resolver(servers=servers, local_address=args.local_address)
    r.start()
    try:
        snap = r.lookup(args.domain, 15000, local_first=True)
        if snap["status"] == "unavailable":
            print("could not connect", file=sys.stderr)
            return 1
        if snap["status"] == "absent":
            print("(no such domain path: %s)" % ra.domain_to_path(args.domain))
        else:
            show(args.domain, snap)
        if args.follow:
            print("watching for membership changes (ctrl-c to stop)...")
            r.poll_events()
            while True:
                events = r.poll_events()
                for ev in events:
                    print("-- %s %s" % (ev["type"], ev["name"] or ev["domain"]))
                if events:
                    show(args.domain, r.snapshot(args.domain, local_first=True))
                time.sleep(0.2)
    except KeyboardInterrupt:
        pass
    finally:
        r.stop()
    return 0


if __name__ == "__main__":
    sys.exit(main())
