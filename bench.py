#!/usr/bin/env python3
"""bench.py — flagship benchmark: ephemeral registrations/sec + p50 ZK
heartbeat RTT at 1k znodes per registrar process (BASELINE.json metric).

One registrar process per GPU (rank), all sharing a single synthetic
in-process ZooKeeper ensemble hosted by rank 0 (shared-nothing
except the ensemble). Each timed step is one full re-registration cycle of
1000 znodes through the real engine pipeline — cleanupPreviousEntries (1000
pipelined unlinks) → setupDirectories (mkdirp) → registerEntries (1000
pipelined ephemeral creates) → one app-level heartbeat (1000 pipelined
exists) — i.e. the reference's hot paths (lib/register.js:132-171,
lib/zk.js:21-44) exercised end-to-end over the real jute wire protocol on
localhost TCP.

The reference publishes no numbers, so vs_baseline is null and
the envelope check is behavioral: the 1k-node heartbeat must fit well inside
the reference's 3000 ms cadence.

Launch (driver contract):
  python bench.py --gpus 1 --steps 30 --warmup 5
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the result line.
--dump-outputs DIR also writes what the last timed step returned (see
dump_outputs); --full is reserved for secondary measurements that need runs
of their own (none today: every reported figure comes from the timed steps).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ZNODES_PER_PROC = 1000


def log(msg):
    print("[bench] %s" % msg, file=sys.stderr, flush=True)


def percentile(values, p):
    if not values:
        return 0.0
    vs = sorted(values)
    idx = min(len(vs) - 1, max(0, int(round(p / 100.0 * (len(vs) - 1)))))
    return vs[idx]


def read_cpu_quota():
    """Effective CPU quota (fractional CPUs) from cgroup v2 or v1; None = unlimited."""
    try:  # v2
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            return float(q) / float(p)
    except (OSError, ValueError):
        pass
    try:  # v1
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            return q / p
    except (OSError, ValueError):
        pass
    return None


def read_cpu_stat():
    """CFS throttle counters (v2 usec / v1 ns, normalized to usec); None if absent."""
    for path in ("/sys/fs/cgroup/cpu.stat", "/sys/fs/cgroup/cpu/cpu.stat"):
        try:
            d = {}
            for line in open(path):
                parts = line.split()
                if len(parts) == 2:
                    d[parts[0]] = int(parts[1])
        except OSError:
            continue
        if "throttled_usec" in d:  # v2
            return {"nr_throttled": d.get("nr_throttled", 0),
                    "throttled_usec": d["throttled_usec"],
                    "usage_usec": d.get("usage_usec")}
        if "throttled_time" in d:  # v1 (ns)
            return {"nr_throttled": d.get("nr_throttled", 0),
                    "throttled_usec": d["throttled_time"] // 1000,
                    "usage_usec": None}
    return None


def partition_cpus(world, rank):
    """Partition the allowed CPUs into per-rank client slices plus an
    ensemble slice (rank 0 hosts the ensemble's IO pool). Returns
    (my_cpus, ensemble_cpus, effective_cpu_count) — my_cpus/ensemble_cpus are
    None when partitioning is pointless (single proc or too few CPUs).
    BENCH_RANK_CPUS=k forces k CPUs per rank (remainder to the ensemble);
    BENCH_AFFINITY=0 disables pinning entirely."""
    cpus = sorted(os.sched_getaffinity(0))
    quota = read_cpu_quota()
    effective = len(cpus) if quota is None else max(1, min(len(cpus), int(quota)))
    if os.environ.get("BENCH_AFFINITY", "1") == "0":
        return None, None, effective
    usable = cpus[:effective]
    k = int(os.environ.get("BENCH_RANK_CPUS", "0"))
    if k > 0:
        if len(usable) < world * k + 1:
            return None, None, effective
        my = set(usable[rank * k:(rank + 1) * k])
        ens = set(usable[world * k:])
        return my, ens, effective
    # default: a registrar client is essentially one busy thread + the python
    # driver — 2 CPUs per rank is plenty; everything left feeds the ensemble
    # IO pool, which serves ALL ranks' traffic and is the scaling bottleneck
    if world <= 1 or len(usable) < world + 2:
        return None, None, effective
    k = max(1, min(2, (len(usable) - 2) // world))
    my = set(usable[rank * k:(rank + 1) * k])
    ens = set(usable[world * k:])
    return my, ens, effective


def dump_outputs(out_dir, last, rank, world):
    """Write what the last timed step handed back to its caller as
    out_dir/<name>.npy, so two builds can be compared output for output.

    The step's inputs (the registration config) are a pure function of the
    command-line arguments and the rank, so with the same arguments these
    arrays are identical from run to run:
      register_rc   float64 [1]     register_()'s return code
      znodes        float32 [n, w]  the znode paths register_() returned, in
                                    the order returned: row i holds the UTF-8
                                    bytes of path i, zero-padded to width w
      heartbeat_rc  float64 [1]     heartbeat()'s return code
    The heartbeat's measured RTT is a timing, not a computed value, and is
    reported in the result line instead. With several ranks each rank writes
    its own files, suffixed _rank<r>."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    paths = [p.encode("utf-8") for p in last["znodes"]]
    width = max([len(p) for p in paths] + [1])
    max_rows = (60 << 20) // (4 * width)  # keep the dump under 64 MB
    if len(paths) > max_rows:  # a fixed, seeded sample of the rows, in order
        keep = np.sort(np.random.default_rng(0).choice(len(paths), max_rows, replace=False))
        paths = [paths[i] for i in keep]
    table = np.zeros((len(paths), width), dtype=np.float32)
    for i, p in enumerate(paths):
        table[i, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    arrays = {
        "register_rc": np.array([last["register_rc"]], dtype=np.float64),
        "znodes": table,
        "heartbeat_rc": np.array([last["heartbeat_rc"]], dtype=np.float64),
    }
    suffix = "" if world == 1 else "_rank%d" % rank
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, name + suffix + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--znodes", type=int, default=ZNODES_PER_PROC)
    ap.add_argument("--servers", type=int, default=0,
                    help="ensemble server count (0 = auto: 1 for a single proc, "
                         "3 — the standard ZK quorum size — for multi-proc, "
                         "matching BASELINE configs 1 vs 2/3)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step "
                         "returned to its caller as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also run the benchmark's secondary measurements; a plain "
                         "run does only what the headline figure needs (today every "
                         "figure in the result line comes from the timed steps "
                         "themselves, so --full adds no work)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # The driver contract is ONE JSON line on stdout from rank 0 — but gloo
    # writes "[Gloo] Rank ... connected ..." banners straight to fd 1 via
    # std::cout (TORCH_CPP_LOG_LEVEL does not cover them). Route ALL
    # incidental stdout to stderr at the fd level and keep the real stdout
    # for the single result line.
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import registrar_amd as ra

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", str(max(1, args.gpus))))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    distributed = world > 1 or "RANK" in os.environ

    import torch

    use_cuda = torch.cuda.is_available()
    if use_cuda:
        torch.cuda.set_device(local_rank % max(1, torch.cuda.device_count()))

    dist = None
    if distributed:
        import torch.distributed as dist  # noqa: F811

        # Coordination barriers only (broadcast of the ensemble address, the
        # timed-region fence, elapsed/rtt gathers): gloo. The workload itself
        # is a host-side control plane — registration traffic carries no GPU
        # tensors and RCCL is deliberately NOT its transport (SURVEY.md §5.8:
        # xGMI's role here is topology metadata in the payload, not data
        # movement). BENCH_BACKEND=nccl opts into RCCL barriers instead.
        backend = os.environ.get("BENCH_BACKEND") or "gloo"
        dist.init_process_group(backend=backend, rank=rank, world_size=world)

    def barrier():
        if dist is not None:
            dist.barrier()
        if use_cuda:
            torch.cuda.synchronize()

    # ---- CPU topology: per-rank affinity + quota-sized ensemble IO pool ----
    # Under a CFS quota (the r1 lease throttled the 4-proc point into a
    # non-monotone curve) free-roaming threads over-subscribe the cgroup and
    # burn the budget on context switches. Pin each rank's client threads to
    # its own CPU slice and give the ensemble IO pool a dedicated slice; the
    # timed region is bracketed by cpu.stat reads so any residual throttling
    # self-labels in the output JSON. BENCH_AFFINITY=0 disables pinning.
    my_cpus, ens_cpus, effective_cpus = partition_cpus(world, rank)

    # ---- ensemble: hosted by rank 0, shared over localhost TCP ----
    if args.servers <= 0:
        # production ZK quorum sizes: 1 standalone / 3 / 5 (BASELINE configs
        # 1 vs 2/3; 5-node quorums are standard at 8-client scale)
        args.servers = 1 if world == 1 else (3 if world <= 4 else 5)
    ensemble = None
    if rank == 0:
        io_threads = int(os.environ.get("BENCH_IO_THREADS", "0"))
        if io_threads == 0 and ens_cpus:
            io_threads = max(2, len(ens_cpus))  # size the pool to its slice
        if ens_cpus:
            os.sched_setaffinity(0, ens_cpus)  # IO threads inherit this mask
        ensemble = ra.Ensemble(servers=args.servers, tick_ms=100, max_session_timeout_ms=60000,
                               io_threads=io_threads)
        ensemble.start()
        connect = ensemble.connect_string()
        log("rank0 hosts ensemble at %s (io_threads=%d, ens_cpus=%s)"
            % (connect, io_threads, sorted(ens_cpus) if ens_cpus else "all"))
    else:
        connect = None
    if my_cpus:
        # client/worker threads created from here on inherit the rank slice
        os.sched_setaffinity(0, my_cpus)
        log("rank %d pinned to cpus %s" % (rank, sorted(my_cpus)))
    if dist is not None:
        obj = [connect]
        dist.broadcast_object_list(obj, src=0)
        connect = obj[0]

    servers = []
    for hp in connect.split(","):
        host, port = hp.rsplit(":", 1)
        servers.append((host, int(port)))
    # deterministic load balance: rank r starts at server r % len(servers)
    rot = rank % len(servers)
    servers = servers[rot:] + servers[:rot]

    client = ra.ZkClient(servers=servers, session_timeout_ms=40000, randomize_start=False)
    client.start()
    if not client.wait_connected(30000):
        raise RuntimeError("rank %d: could not connect to ensemble" % rank)

    # ---- per-rank registration config: 1k znodes via hostname + aliases ----
    registration = {
        "domain": "rank%d.bench.mi355x" % rank,
        "type": "host",
        "adminIp": "127.0.0.1",
        "hostname": "bench-r%d" % rank,
        "settleMs": 0,  # the 1 s post-cleanup settle is watcher politeness,
                        # not work; configurable in the engine, off here
        "aliases": ["a%04d.rank%d.bench.mi355x" % (i, rank) for i in range(args.znodes - 1)],
    }
    if use_cuda:
        # per-GPU identity in the payload (BASELINE config 3 shape); also
        # touch the device so the job really runs one rank per GPU
        gpus = ra.discover_gpus("")
        gi = local_rank % max(1, len(gpus)) if gpus else 0
        registration["gpu"] = {
            "index": gi,
            "xgmiRank": gpus[gi]["xgmi_rank"] if gpus else -1,
            "uuid": gpus[gi]["uuid"] if gpus else "",
        }
        t = torch.ones(1024, device="cuda")
        assert float(t.sum().item()) == 1024.0
    # parsed once — each timed step is pure wire work through the native
    # pipeline, exactly like the daemon's re-register path
    prep = ra.PreparedRegistration(json.dumps(registration))

    phase_time = {"reg": 0.0, "hb": 0.0}
    last = {}  # what the most recent step returned (for --dump-outputs)

    def step():
        """One full re-register of all znodes + one 1k-node heartbeat."""
        t0 = time.perf_counter()
        rc, err, znodes = prep.register_(client)
        t1 = time.perf_counter()
        if rc != 0:
            raise RuntimeError("rank %d register failed: %s" % (rank, err))
        reg_rc = rc
        rc, rtt_us = prep.heartbeat(client)
        phase_time["reg"] += t1 - t0
        phase_time["hb"] += time.perf_counter() - t1
        if rc != 0:
            raise RuntimeError("rank %d heartbeat failed: %s" % (rank, ra.error_name(rc)))
        last.update(register_rc=reg_rc, znodes=znodes, heartbeat_rc=rc)
        return rtt_us

    # ---- warmup ----
    for _ in range(args.warmup):
        step()
    log("rank %d warmup done" % rank)

    # ---- timed region ----
    barrier()
    stat_before = read_cpu_stat() if rank == 0 else None
    t0 = time.perf_counter()
    rtts_us = [step() for _ in range(args.steps)]
    elapsed = time.perf_counter() - t0
    stat_after = read_cpu_stat() if rank == 0 else None
    barrier()

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last, rank, world)

    # max elapsed over ranks is THE job time; p50 over all ranks' heartbeats
    if dist is not None:
        el = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        elapsed_max = float(el.item())
        gathered = [None] * world
        dist.all_gather_object(gathered, rtts_us)
        all_rtts = [r for lst in gathered for r in lst]
        if os.environ.get("BENCH_DEBUG"):
            per = [None] * world
            dist.all_gather_object(per, (elapsed, phase_time["reg"], phase_time["hb"]))
            if rank == 0:
                log("per-rank (elapsed, reg, hb): %s"
                    % ", ".join("(%.3f, %.3f, %.3f)" % e for e in per))
    else:
        elapsed_max = elapsed
        all_rtts = rtts_us

    if rank == 0:
        total_regs = world * args.znodes * args.steps
        value = total_regs / elapsed_max
        p50_ms = percentile(all_rtts, 50) / 1000.0
        p99_ms = percentile(all_rtts, 99) / 1000.0
        result = {
            "metric": "ephemeral registrations/sec",
            "baseline_metric": "ephemeral registrations/sec + p50 ZK heartbeat RTT, "
                               "1k znodes, 1/2/4/8 procs",  # BASELINE.json's name
            "value": round(value, 1),
            "unit": "registrations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed_max / args.steps * 1000.0, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # reference publishes no numbers
            "dtype": "n/a",  # host-side control-plane daemon: no tensor math
            "data": "synthetic",
            "p50_heartbeat_rtt_ms": round(p50_ms, 3),
            "p99_heartbeat_rtt_ms": round(p99_ms, 3),
            # CFS-throttle evidence for the timed region (cgroup is shared by
            # all ranks, so rank 0's delta covers the whole job): a throttled
            # scaling point self-labels instead of silently bending the curve
            "cpu_stat": {
                "cpu_quota": read_cpu_quota(),
                "cpus_allowed": effective_cpus,
                "affinity": "per-rank slices + dedicated ensemble slice" if my_cpus else "none",
                "nr_throttled_delta": (stat_after["nr_throttled"] - stat_before["nr_throttled"])
                if stat_before and stat_after else None,
                "throttled_usec_delta": (stat_after["throttled_usec"] - stat_before["throttled_usec"])
                if stat_before and stat_after else None,
            },
            "config": {
                "model": "registrar re-register cycle, 1k ephemeral znodes/proc",
                "global_batch": world * args.znodes,
                "seq_len": None,
                "parallelism": "%d registrar procs (1/GPU), shared synthetic ZK ensemble (%d server%s) on rank 0"
                % (world, args.servers, "s" if args.servers != 1 else ""),
                "znodes_per_proc": args.znodes,
                "step": "cleanup(1k unlink) + mkdirp + 1k ephemeral create + 1k-node heartbeat",
                "envelope_check_heartbeat_under_ms": 3000,
            },
        }
        os.write(real_stdout, (json.dumps(result) + "\n").encode())

    client.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if ensemble is not None:
        ensemble.stop()


if __name__ == "__main__":
    main()
