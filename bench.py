"""Benchmark: perturbation-samples/s of the XP-GNN hot path on MI355X (BASELINE.json metric).

Headline (`value`), configs[1] ("c2"): synthetic homogeneous graph, 100k nodes / 1M edges,
64-dim fp32 features, 2-layer GCN 64->64->64 + Linear(64->1) + sigmoid (random init),
interpret_samples=256, epochs=50 -> 12,800 mask rows per repeat, query node 7 (node_prediction:
its 3-hop computational subgraph, as the reference extracts it).

One step = one repeat per rank through the north-star split of Explainer.run (explainer.py:490-532,
SURVEY.md §8e), inputs resident in HBM:
  device mask sampling (Philox Shapley rows of this rank's row shard, keyed by global row) ->
  masked receptive-field forward of the shard -> KernelSHAP of the shard ->
  RCCL all-gather of the per-row fp32 logits and fp64 kernel weights ->
  surrogate Adam loops of this rank's repeats (ceil(R / (R // epochs)) steps each) ->
  all-gather of the fitted weights -> mean / std over repeats (weight_stacking).
With N ranks a step covers N repeats (weak scaling: one repeat's rows and one fit per rank).

`regimes` (every N unless noted):
  c3_full_graph   configs[2]: 1M nodes / 10M edges, 2-layer SAGE 128, 512 mask rows sharded over
                  the ranks (strong scaling), every node a target (SURVEY.md §8d regime (ii): the
                  >= 40 % HBM roofline target), + the all-gather of the rows' query logits
  c5_hetero       configs[4]: 1M-node 3-type graph, 256-dim features, 20 communities, device
                  community sampler, interpret_samples=1024, repeats=10, community scoring
  hetero_c4       configs[3]: 500k-node 3-type graph, 5 relations, a job of 4 repeats sharded
                  over the ranks (rows, then fits by repeat)
  node_c3         configs[2] in node_prediction (regime (i))
  graph_prediction_c3, communities_c2, graph_queries, explainer_api   (N = 1 only; at N > 1
                  they are listed in the line's `sections_skipped`)

A plain run (`python bench.py --gpus N --steps K --warmup W`) sets up, warms up, times the K
steps of the headline and prints the result line.  `--full` adds everything else: the headline's
phase breakdown (eager steps), its graph / exchange checks against an eager step, its roofline
and CPU baseline, and the `regimes` sections (`--sections` picks among them).
`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR]
    python bench.py --full [--gpus N] [--steps K] [--warmup W] [--sections a,b] [--no-cpu-baseline]
    torchrun --nproc-per-node N bench.py --gpus N ...
"""
import argparse
import gc
import json
import math
import os
import platform
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "perturbation-samples/sec (masked GNN fwd) per query node; 1/2/4/8 GPU"
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_MFMA_PEAK_TF = 157.3    # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
SECTIONS = ("headline", "c3", "node_c3", "c5", "gp", "c4", "comm", "queries", "api")
MULTI_GPU_SECTIONS = ("headline", "c3", "node_c3", "c5", "c4")


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--nodes", type=int, default=100_000)
    p.add_argument("--edges", type=int, default=1_000_000)
    p.add_argument("--feat", type=int, default=64)
    p.add_argument("--interpret-samples", type=int, default=256)
    p.add_argument("--epochs", type=int, default=50)
    p.add_argument("--query", type=int, default=7)
    p.add_argument("--repeats", type=int, default=1,
                   help="repeats per rank per step (Explainer.run(times=...) / world)")
    p.add_argument("--full", action="store_true",
                   help="beside the timed headline steps: its phase breakdown, graph / exchange "
                        "checks, roofline and CPU baseline, and the regime sections (--sections)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last timed step's outputs (mean / std "
                        "of the fitted weights; the last fit's weights, logits and kernel weights "
                        "where the launch form keeps them) as DIR/<name>.npy")
    p.add_argument("--sections", default="all",
                   help="with --full: comma list of " + ",".join(SECTIONS) +
                        " (PMC passes run one each)")
    p.add_argument("--no-cpu-baseline", action="store_true",
                   help="with --full: leave the CPU baselines out")
    p.add_argument("--no-graph", action="store_true",
                   help="headline at world 1: eager launches instead of replaying one captured "
                        "HIP graph per step")
    p.add_argument("--cpu-rows", type=int, default=12800)
    p.add_argument("--cpu-procs", type=int, default=0,
                   help="CPU baseline worker processes (0: every usable host core)")
    p.add_argument("--c3-rows", type=int, default=512,
                   help="regime (ii): mask rows of the c3 full-graph forward (all ranks)")
    p.add_argument("--c5-times", type=int, default=10)
    p.add_argument("--c5-samples", type=int, default=1024)
    p.add_argument("--c4-times", type=int, default=4,
                   help="c4 repeats per job (the job is sharded over the ranks)")
    args = p.parse_args()
    if not args.full and args.sections not in ("all", "headline"):
        p.error("--sections other than headline needs --full")
    return args


# ----------------------------------------------------------------------------- plumbing
def launch_ranks(args):
    """`--gpus N > 1` without a torch.distributed environment: start N ranks (one process per GPU,
    RCCL) with torch.distributed.run as a CHILD process and return its exit code.  Called before
    anything touches the GPU; rank 0 of the child prints the JSON line."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1",
           "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print(f"[bench] launching {args.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.call(cmd)


# XPG_BENCH_RCCL1=1 at one rank: a process group of ONE rank over RCCL, with every N-rank code
# path (exchange staging, async all-gathers and their stream waits, uneven gathers, max over
# ranks) taken as at N > 1 -- the RCCL path executed on a one-GPU box (a rehearsal, not a bench)
RCCL1 = os.environ.get("XPG_BENCH_RCCL1") == "1"


def multi(world):
    """True when the run takes the N-rank code paths (N > 1, or the one-rank RCCL rehearsal)."""
    return world > 1 or RCCL1


def setup_dist(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench: --gpus {args.gpus} but WORLD_SIZE {world}: launch one rank per "
                         "GPU (python bench.py --gpus N starts them itself)")
    if world == 1 and RCCL1:
        import torch.distributed as dist
        torch.cuda.set_device(0)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 1000))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        return world, rank, 0
    if world > 1:
        import torch.distributed as dist
        # XPG_BENCH_BACKEND=gloo + XPG_BENCH_ONE_GPU=1: a rehearsal of the N-rank path with
        # every rank on cuda:0 (one-GPU box); the driver's runs use RCCL, one GPU per rank
        if os.environ.get("XPG_BENCH_ONE_GPU") == "1":
            local = 0
        elif local >= torch.cuda.device_count():
            raise SystemExit(f"bench: rank {rank} has local rank {local} but only "
                             f"{torch.cuda.device_count()} GPU(s) are visible")
        torch.cuda.set_device(local)
        backend = os.environ.get("XPG_BENCH_BACKEND", "nccl")
        dist.init_process_group(backend, **({"device_id": torch.device("cuda", local)}
                                            if backend == "nccl" else {}))
        assert dist.get_world_size() == args.gpus
    else:
        torch.cuda.set_device(0)
    return world, rank, local


def rank_layout(world, local):
    """Backend, world size and every rank's device (index + PCI bus) — gathered once, untimed."""
    props = torch.cuda.get_device_properties(local)
    me = {"local_rank": local, "device": local, "name": props.name,
          "pci_bus_id": getattr(props, "pci_bus_id", None), "host": platform.node()}
    if not multi(world):
        return {"backend": None, "world": 1, "ranks": [me]}
    import torch.distributed as dist
    ranks = [None] * world
    dist.all_gather_object(ranks, me)
    backend = dist.get_backend()
    return {"backend": "nccl (RCCL)" if backend == "nccl" else backend, "world": world,
            "ranks": ranks, "distinct_devices": len({(r["host"], r["pci_bus_id"], r["device"])
                                                     for r in ranks})}


def barrier(world):
    torch.cuda.synchronize()
    if multi(world):
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()


def max_over_ranks(x, world, dev):
    if not multi(world):
        return x
    import torch.distributed as dist
    t = torch.tensor([x], device=dev, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def log(rank, msg):
    """Progress on stderr (rank 0): the JSON line stays the only stdout output."""
    if rank == 0:
        print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


DUMP_BYTES = 64 << 20  # --dump-outputs: the files' data together stay within this


def dump_outputs(out_dir, tensors):
    """--dump-outputs: each tensor as out_dir/<name>.npy (fp32 as float32, everything else as
    float64).  An array over its share of DUMP_BYTES is written as a fixed sample: the elements
    at sorted flat indices drawn once from numpy's default_rng(0)."""
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BYTES // max(1, len(tensors))
    for name, t in tensors.items():
        a = t.detach().cpu().numpy()
        a = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def host_info():
    model = platform.processor() or "?"
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for line in out.splitlines():
            if line.startswith("Model name:"):
                model = line.split(":", 1)[1].strip()
    except Exception:  # pragma: no cover
        pass
    return model, os.cpu_count()


def host_cores():
    """(usable, detail): the CPUs this job may run on — the affinity mask, capped by the cgroup
    CPU quota (a GPU box shows every CPU of the machine in os.cpu_count(), but schedules this
    job on its share)."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = int(q) / int(per)
    except (OSError, ValueError):
        pass
    n = max(1, min(aff, int(quota)) if quota else aff)
    return n, {"os_cpu_count": os.cpu_count(), "affinity_cpus": aff, "cgroup_cpu_quota": quota}


def cpu_procs(args, cap=None):
    """CPU baseline worker processes: every usable host core (--cpu-procs overrides); `cap`
    bounds memory-heavy workers."""
    n = args.cpu_procs or host_cores()[0]
    return max(1, min(n, cap) if cap else n)


def _pool(n):
    import multiprocessing as mp
    return mp.get_context("spawn").Pool(n)


def pmc_file(section):
    """{exact kernel instantiation: per-dispatch record} and the op count of a section's PMC file
    (profiles/pmc_<section>.json, tools/pmc_traffic.py: 2 x FETCH_SIZE + WRITE_SIZE per dispatch,
    MI355X_MICROARCH.md HBM section), or (None, None)."""
    fn = os.path.join(ROOT, "profiles", f"pmc_{section}.json")
    if not os.path.exists(fn):
        return None, None
    data = json.load(open(fn))
    ops = data.pop("_ops", None)
    return data, ops


def pmc_chain(section, kernels):
    """Counter-measured HBM bytes of ONE operation of a section's launch chain.  `kernels` are
    exact kernel instantiations as rocprofv3 names them (template arguments included: another
    instantiation of the same template, e.g. a comparison run's, is a different kernel); the
    file's bytes of those kernels over all their dispatches are divided by `ops`, the number of
    operations the profiled run made (`_ops`, written by the profiling script).  Returns
    (bytes per op, {kernel: bytes per op}) or (None, None) when a kernel is missing."""
    data, ops = pmc_file(section)
    if data is None or ops is None:
        return None, None
    per = {}
    for name in kernels:
        d = data.get(name)
        if d is None or d.get("traffic_bytes") is None:
            return None, None
        per[name] = d["traffic_bytes"] * d["dispatches"] / ops
    return sum(per.values()), per


def roofline(alg_bytes, seconds, section=None, kernels=(), alg_per_kernel=None):
    """The roofline object of one launch chain: algorithmic bytes per op over the measured time,
    plus the counter-measured bytes (traffic) of the same op when the section's PMC file exists."""
    achieved = alg_bytes / seconds / 1e9
    out = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "frac": achieved / HBM_PEAK_GBS, "bytes_per_launch": alg_bytes, "traffic": None}
    if section is not None:
        traffic, per = pmc_chain(section, set(kernels))
        if traffic is not None:
            out["traffic"] = traffic
            out["traffic_source"] = f"profiles/pmc_{section}.json"
            out["achieved_counter"] = traffic / seconds / 1e9
            out["frac_counter"] = traffic / seconds / 1e9 / HBM_PEAK_GBS
            out["counter_over_alg"] = traffic / alg_bytes
            out["per_kernel_counter_bytes"] = per
            if alg_per_kernel:
                out["per_kernel_counter_over_alg"] = {
                    k: per[k] / v for k, v in alg_per_kernel.items() if k in per and v}
    return out


# ----------------------------------------------------------------------------- c2 (headline)
def build_c2(args, dev):
    """configs[1]: the c2 graph, its 2-layer GCN and the 3-hop computational subgraph of the
    query (Data.comp_graph with L + 1 hops, data.py:325-333)."""
    from bikg_graph_explainability_public_amd import pipeline
    from bikg_graph_explainability_public_amd.data import Data
    from bikg_graph_explainability_public_amd.nn import ConvStack

    g = torch.Generator().manual_seed(0)
    feat = torch.randn((args.nodes, args.feat), generator=g)
    ei = torch.randint(0, args.nodes, (2, args.edges), generator=g)
    torch.manual_seed(0)
    arch = ConvStack("gcn", [args.feat, 64, 64], [64, 1]).eval().to(dev)
    data = Data(feat.to(dev), ei.to(dev))
    names = [str(i) for i in range(args.nodes)]
    sub_feat, sub_ei, _, sub_ind, _, _ = data.comp_graph(args.query, 2, "node", names)
    q = int(sub_ind.reshape(-1)[0])
    plan = pipeline.build_plan(arch, sub_feat, sub_ei, [q])
    return arch, sub_feat, sub_ei, q, plan


def build_c3node(args, dev):
    """configs[2] in the reference's node_prediction semantics (SURVEY.md §8d regime (i)): the
    c3 graph (1M nodes / 10M edges, 128 feats), 2-layer SAGEConv(mean) 128 + Linear(128, 1) +
    sigmoid, the 3-hop computational subgraph of the query."""
    from bikg_graph_explainability_public_amd import pipeline
    from bikg_graph_explainability_public_amd.data import Data
    x, ei, arch = c3_graph(dev)
    arch = arch.to(dev)
    data = Data(x.to(dev), ei.to(dev))
    names = [str(i) for i in range(x.shape[0])]
    sub_feat, sub_ei, _, sub_ind, _, _ = data.comp_graph(args.query, 2, "node", names)
    q = int(sub_ind.reshape(-1)[0])
    plan = pipeline.build_plan(arch, sub_feat, sub_ei, [q])
    return arch, sub_feat, sub_ei, q, plan


WORKLOADS = {
    "c2": dict(build=build_c2, kind="gcn", samples=lambda a: a.interpret_samples,
               text="c2 (BASELINE configs[1]): synthetic homogeneous 100k nodes / 1M edges, 64-dim "
                    "feats, 2-layer GCN, interpret_samples=256, node_prediction (3-hop "
                    "computational subgraph of node 7)"),
    "c3node": dict(build=build_c3node, kind="sage", samples=lambda a: 512,
                   text="c3 (BASELINE configs[2]) in node_prediction (SURVEY.md §8d regime (i)): "
                        "synthetic homogeneous 1M nodes / 10M edges, 128-dim feats, 2-layer "
                        "SAGEConv(mean) 128 + Linear(128, 1) + sigmoid, interpret_samples=512 "
                        "(25,600 rows per repeat), 3-hop computational subgraph of node 7"),
}


def oracle_spec_of(arch, kind):
    """The numpy oracle's model spec of a ConvStack (conv Linear weights + the dense head)."""
    convs = []
    for i in range(0, len(arch.conv), 2):
        c = arch.conv[i]
        if kind == "gcn":
            prm = {"W": c.lin.weight.detach().cpu().numpy(), "b": c.bias.detach().cpu().numpy()}
        else:
            prm = {"Wl": c.lin_l.weight.detach().cpu().numpy(),
                   "bl": c.lin_l.bias.detach().cpu().numpy(),
                   "Wr": c.lin_r.weight.detach().cpu().numpy()}
        convs.append({"kind": kind, "rels": [None], "act": "relu", "params": {None: prm}})
    nfc = len(arch.fc) // 2
    fc = [{"W": arch.fc[2 * i].weight.detach().cpu().numpy(),
           "b": arch.fc[2 * i].bias.detach().cpu().numpy(),
           "act": "sigmoid" if i == nfc - 1 else "relu"} for i in range(nfc)]
    return {"convs": convs, "fc": fc}


def wlm_bytes(rows, cols, batch):
    """Algorithmic bytes of one surrogate fit: the mask bits once, y + kernel, the Adam state
    (w, m, v read + written), one loss per step."""
    W = (cols + 31) // 32
    return rows * W * 4 + rows * (4 + 8) + cols * 4 * 6 + 8 * math.ceil(rows / batch)


WLM_KERNELS = ("k_wlm_prep", "k_wlm_fit_mc<1, 1>", "k_wlm_loss_best")


def headline(args, dev, world, rank, workload="c2"):
    """The repeat pipeline of a node_prediction workload (c2: the headline; c3node: regime (i)
    of configs[2]), sharded as Explainer.run shards it (module docstring).

    A step is one repeat per rank (its own masks, forward, KernelSHAP and surrogate fit).  The
    pipelined graphs take each rank's steps in groups of G (XPG_BENCH_GROUP, default 2; 1 = the
    round-5 form): the G repeats' masks -> forward -> KernelSHAP run as one production and
    their G fits as ONE k_wlm_fit_mc launch, which places each fit on its own XCD, so the G
    latency-bound fits run side by side (as Explainer.run(times) batches its repeats).  The
    round-5 pipeline kept two fits in flight on two replay streams instead, and the hardware
    queues mostly ran them one after the other (profiles/r6_headline_group_ab.log: 2 lanes
    78-80 M samples/s, groups of 2 135 M, of 4 181 M).  Every one of the K steps is still
    processed in full inside the timed region; the line reports K steps of one repeat each."""
    group = 1
    if args.repeats == 1 and not args.no_graph and os.environ.get("XPG_BENCH_PIPE", "1") == "1":
        g = max(1, int(os.environ.get("XPG_BENCH_GROUP", "2")))
        if g > 1 and args.steps % g == 0:
            group = g
    if group == 1:
        return _headline_core(args, dev, world, rank, workload)
    a2 = argparse.Namespace(**vars(args))
    a2.repeats, a2.steps, a2.warmup = group, args.steps // group, -(-args.warmup // group)
    line = _headline_core(a2, dev, world, rank, workload, lanes_ok=False)
    line["steps"], line["warmup"] = args.steps, args.warmup
    line["ms_per_step"] = line["ms_per_step"] / group
    cfg = line["config"]
    cfg["repeats_per_step"] = world  # one repeat per rank per step
    cfg["steps_per_group"] = group
    cfg["fits_in_flight"] = group
    cfg["launch"] = (f"pipelined captured HIP graphs over groups of {group} consecutive steps "
                     "(XPG_BENCH_GROUP): a group's repeats are produced together (masks -> "
                     "forward + KernelSHAP, one launch each) and fitted by ONE k_wlm_fit_mc launch "
                     "(one fit per XCD, side by side), beside the next group's production; the "
                     "fit's prologue runs with the production, its losses / best epoch and the "
                     "mean / std after its Adam steps on the side stream; prologue untimed; every "
                     "step is one repeat of its own rows, masks and fit; "
                     f"{a2.steps} group(s) = {args.steps} steps timed (device-resident sampler "
                     "seed advanced inside the graph)" +
                     ("; phases_ms from eager steps of one group" if args.full else ""))
    if args.full:
        line["phases_ms_per"] = f"group of {group} repeats"
    return line


def _headline_core(args, dev, world, rank, workload="c2", lanes_ok=True):
    from bikg_graph_explainability_public_amd import engine, sharding
    wdef = WORKLOADS[workload]
    arch, sub_feat, sub_ei, q, plan = wdef["build"](args, dev)
    S = plan.cols
    n_samples = wdef["samples"](args)
    R = n_samples * args.epochs
    batch = R // args.epochs
    times = args.repeats * world
    n_rows = times * R
    r0, r1 = sharding.shard_range(n_rows, world, rank)
    f0, f1 = sharding.shard_range(times, world, rank)
    params = {"lr": 0.01, "l1_lambda": 1e-4}
    stream = torch.cuda.current_stream()
    side = torch.cuda.Stream(device=dev)
    use_side = True  # KernelSHAP beside the forward, as sharding.gather_map_beside runs it
    w0 = torch.zeros((times, S), device=dev)
    statuses = []
    phases = ("sample", "forward", "shap", "gather", "wlm")
    ev = {k: [] for k in phases}
    # The step is host-launch-bound in eager mode (~55 us of GPU idle per 0.3 ms step in the
    # kernel trace), so it is replayed from captured HIP graphs: the sampler reads its seed from
    # device memory and the graph advances it, so every replay draws new mask rows.  Default:
    # the pipelined graphs (below).  XPG_BENCH_PIPE=0: ONE graph per step (one process), or the
    # split form with eager RCCL all-gathers between two graphs (several ranks, or
    # XPG_BENCH_SPLIT_GRAPH=1).
    use_graph = not args.no_graph
    split = multi(world) or os.environ.get("XPG_BENCH_SPLIT_GRAPH") == "1"
    # the pipelined graphs need each rank's fits to read only its own rows ((f0, f1) repeats
    # == rows [r0, r1), e.g. times = world): the fit must not regenerate rows from seed_t
    unroll, depth = 1, 1
    pipe = use_graph and (f0 * R, f1 * R) == (r0, r1) and \
        os.environ.get("XPG_BENCH_PIPE", "1") == "1"
    split = split and not pipe
    seed_t = torch.full((1,), 1000 + args.warmup, dtype=torch.int64, device=dev)
    k_buf = torch.empty(r1 - r0, dtype=torch.float64, device=dev)
    stash = {}
    cnt_buf = torch.empty(r1 - r0, dtype=torch.int32, device=dev)
    exchange = None

    def part_a(seed, dev_seed, mk=lambda j: None):
        """masks -> forward (+ KernelSHAP on the side stream): this rank's rows"""
        # the CURRENT stream: inside a capture that is the capture stream, not `stream`
        cur = torch.cuda.current_stream()
        mk(0)
        if dev_seed:
            bits = engine.sample_shapley_dev(seed_t, r1 - r0, S, row_offset=r0)
        else:
            bits = engine.sample_shapley(seed, r1 - r0, S, dev, row_offset=r0)
        mk(1)
        # KernelSHAP on a side stream beside the forward (as Explainer.run does,
        # sharding.gather_map_beside); "shap" = the wait for it after the forward
        side.wait_stream(cur)
        y_loc = plan.forward(bits)[:, 0]
        with torch.cuda.stream(side if use_side else cur):
            # (graph capture: the side stream must not allocate; its buffers are static)
            k_loc = engine.shap_kernel(bits, S, out=k_buf, scratch=cnt_buf) if dev_seed else \
                engine.shap_kernel(bits, S)
        mk(2)
        cur.wait_stream(side)
        if not dev_seed:  # (a captured graph's memory is private until the graph is freed)
            k_loc.record_stream(cur)
        mk(3)
        if dev_seed:
            stash.update(bits=bits, y=y_loc, k=k_loc)
        return bits, y_loc, k_loc

    def part_b(seed, dev_seed, bits, y, k):
        """this rank's repeats' surrogate fits"""
        if (f0 * R, f1 * R) == (r0, r1):
            fbits = bits
        elif dev_seed:  # this rank's repeats straddle other shards: regenerate their rows
            fbits = engine.sample_shapley_dev(seed_t, (f1 - f0) * R, S, row_offset=f0 * R)
        else:
            fbits = engine.sample_shapley(seed, (f1 - f0) * R, S, dev, row_offset=f0 * R)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        w, _, _, _, _ = engine.wlm_fit(fbits.view(f1 - f0, R, -1), S, batch,
                                       y[f0 * R:f1 * R].view(f1 - f0, R),
                                       k[f0 * R:f1 * R].view(f1 - f0, R), w0[f0:f1], params,
                                       check=False, status=st)
        statuses.append(st)
        if dev_seed:
            stash.update(w=w, st=st)
        return w

    def part_c(w):
        w_all = sharding.gather_rows(w.reshape(f1 - f0, S), times)
        std, mean = torch.std_mean(w_all, 0, unbiased=False)  # Explainer.weight_stacking
        return mean, std

    def step(i, record, dev_seed=False):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)]
        mk = (lambda j: marks[j].record(stream)) if record else (lambda j: None)
        seed = 1000 + i
        bits, y_loc, k_loc = part_a(seed, dev_seed, mk)
        y = sharding.gather_rows(y_loc, n_rows)           # RCCL all-gather of the logits
        k = sharding.gather_rows(k_loc, n_rows)
        mk(4)
        w = part_b(seed, dev_seed, bits, y, k)
        mk(5)
        if record:
            for j, name in enumerate(phases):
                ev[name].append((marks[j], marks[j + 1]))
        out = part_c(w)
        if dev_seed:
            seed_t.add_(1)  # the next replay's masks
        return out

    for i in range(args.warmup):
        step(i, False)
    results = []
    if use_graph:
        # --full: the phase breakdown comes from 3 eager steps outside the timed region (events
        # cannot split a graph replay); then one eager dev-seed step and the capture
        for i in range(3 if args.full else 0):
            step(args.warmup + i, True)
        step(0, False, dev_seed=True)
        seed_t.fill_(1000 + args.warmup)
        torch.cuda.synchronize()
        if pipe:
            # Pipelined graphs over two static buffer sets (bits, y, k and a PreparedFit each):
            # global step i fits the repeat in set i & 1 on the capture stream while the next
            # repeat's masks -> forward -> KernelSHAP -> fit prologue fill set 1 - (i & 1) on a
            # side stream (allocation-free).  The fit is latency-bound on a few workgroups, the
            # production fills the rest of the chip beside it.  Every rank fits its own repeats
            # (rows [r0, r1) are repeats [f0, f1)), which it produced itself, so no fit waits
            # for a collective.  Several ranks: each step's logits, kernel weights (copied on
            # the side stream) and fitted weights (after the fit) go to a staging row; ONE RCCL
            # all-gather per graph replay, issued asynchronously right after it, exchanges the
            # replay's rows.  The host never waits: the stream waits for that exchange only
            # before the replay that rewrites its staging buffer (two replays later), and the
            # mean / std over all ranks' repeats (weight_stacking) of those steps runs then.
            # A graph holds U consecutive steps (XPG_BENCH_UNROLL, default 4: one launch and one
            # exchange per U steps; U = 1 or even, dividing --steps).  Prologue (untimed): the
            # first repeat's production; the K timed steps do K fits + K productions.
            # Two lanes (default with one rank; XPG_BENCH_FIT_DEPTH=1: one lane): the repeats
            # alternate between two such pipelines, each with its own buffer sets, side stream
            # and seed (lane l draws the seeds of steps l, l + 2, ...), whose graphs are replayed
            # on two streams, so fit i + 1 runs beside fit i (the fits are independent; each is
            # a latency-bound chain on ~13 workgroups) and a step costs the production rather
            # than the fit.  (One graph holding both lanes' streams, with event waits between its
            # side streams, ended in a segfault of hipStreamEndCapture on this stack:
            # tools/capture_probe.py p2:*.)
            want = max(1, int(os.environ.get("XPG_BENCH_UNROLL", "4")))

            def pick_unroll(n):
                return next((u for u in range(want, 1, -1) if u % 2 == 0 and n % u == 0), 1)
            n_lanes = 2 if (lanes_ok and os.environ.get("XPG_BENCH_FIT_DEPTH", "2") == "2" and
                            not multi(world) and args.steps % 2 == 0) else 1
            depth = n_lanes
            per_lane = args.steps // n_lanes
            unroll = pick_unroll(per_lane)
            W_, nl, nf = (S + 31) // 32, r1 - r0, f1 - f0

            def make_lane(lane):
                sets_ = []
                for _ in range(2):
                    d = dict(bits=torch.empty((nl, W_), dtype=torch.int32, device=dev),
                             y=torch.empty((nl, plan.n_out), dtype=torch.float32, device=dev),
                             k=torch.empty(nl, dtype=torch.float64, device=dev),
                             cnt=torch.empty(nl, dtype=torch.int32, device=dev),
                             fit=engine.PreparedFit(nf, R, S, batch, params, dev))
                    statuses.append(d["fit"].status)
                    sets_.append(d)
                seed_l = torch.full((1,), 1000 + args.warmup + lane, dtype=torch.int64, device=dev)
                return dict(sets=sets_, s1=torch.cuda.Stream(device=dev), ev=torch.cuda.Event(),
                            seed=seed_l, graphs=[], stream=torch.cuda.Stream(device=dev),
                            ws=torch.empty(plan.workspace_bytes(nl), dtype=torch.uint8, device=dev))
            lanes = [make_lane(lane) for lane in range(n_lanes)]
            sets = lanes[0]["sets"]
            ex = multi(world)
            if ex:  # staging row: y fp32 [nl] | k fp64 [nl] | w fp32 [nf, S]
                oy, ok_ = 0, -(-nl * 4 // 8) * 8
                ow = ok_ + nl * 8
                sb = -(-(ow + nf * S * 4) // 16) * 16
                stage = [torch.zeros((unroll, sb), dtype=torch.uint8, device=dev) for _ in range(2)]
                gath = [torch.zeros((world, unroll, sb), dtype=torch.uint8, device=dev)
                        for _ in range(2)]

            def produce(L, d):  # (in order on its stream: it is off the fit's critical path)
                engine.sample_shapley_dev(L["seed"], nl, S, row_offset=r0, out=d["bits"])
                L["seed"].add_(n_lanes)
                plan.forward(d["bits"], out=d["y"], workspace=L["ws"])  # the lane's own workspace
                engine.shap_kernel(d["bits"], S, out=d["k"], scratch=d["cnt"])
                d["fit"].prepare(d["bits"], d["y"][:, 0], d["k"], w0[f0:f1])

            def pipe_step(L, i_set, row):
                # the fit's Adam steps alone are the chain: the next repeat's production, and
                # this fit's losses / best epoch / status and its mean / std (or staging copy)
                # run on s1; the next fit waits only for its production (the lane's event)
                cur = torch.cuda.current_stream()
                s1 = L["s1"]
                s1.wait_stream(cur)  # the production rewrites the set the previous fit used
                d = L["sets"][i_set]
                w = d["fit"].fit_steps(d["bits"], d["k"])
                out = None
                with torch.cuda.stream(s1):
                    if row is not None:  # this step's repeat: logits + kernel weights
                        row[oy:oy + nl * 4].view(torch.float32).copy_(d["y"][:, 0])
                        row[ok_:ok_ + nl * 8].view(torch.float64).copy_(d["k"])
                    produce(L, L["sets"][1 - i_set])
                    L["ev"].record(s1)
                    s1.wait_stream(cur)  # after this fit's steps
                    d["fit"].finish(d["k"])
                    if row is None:
                        out = part_c(w)
                    else:
                        row[ow:ow + nf * S * 4].view(torch.float32).copy_(w.reshape(-1))
                cur.wait_event(L["ev"])
                return out

            def stacked(b):  # mean / std over all ranks' repeats of replay buffer b's U steps
                w_all = gath[b][:, :, ow:ow + nf * S * 4].contiguous().view(torch.float32)
                w_all = w_all.view(world, unroll, nf, S).transpose(0, 1).reshape(unroll, world * nf, S)
                std, mean = torch.std_mean(w_all, 1, unbiased=False)
                return [(mean[j], std[j]) for j in range(unroll)]

            for L in lanes:  # prologue: each lane's first timed repeat
                produce(L, L["sets"][0])
            torch.cuda.synchronize()
            for L in lanes:
                for b in range(2):
                    gph, outs = torch.cuda.CUDAGraph(), []
                    with engine.capture_guard(), torch.cuda.graph(gph):
                        for j in range(unroll):
                            outs.append(pipe_step(L, (b * unroll + j) & 1, stage[b][j] if ex else None))
                        torch.cuda.current_stream().wait_stream(L["s1"])  # join the side stream
                    L["graphs"].append((gph, outs))
            graphs = lanes[0]["graphs"]
            def exchange(b):
                return sharding.all_gather_async(gath[b].view(-1), stage[b].view(-1))
        elif not split:
            graph = torch.cuda.CUDAGraph()
            with engine.capture_guard(), torch.cuda.graph(graph):
                g_out = step(0, False, dev_seed=True)
        else:
            y_s = torch.empty(n_rows, dtype=torch.float32, device=dev)
            k_s = torch.empty(n_rows, dtype=torch.float64, device=dev)
            graph_a, graph_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with engine.capture_guard(), torch.cuda.graph(graph_a):
                g_bits, g_y, g_k = part_a(0, True)
            with engine.capture_guard(), torch.cuda.graph(graph_b, pool=graph_a.pool()):
                g_w = part_b(0, True, g_bits, y_s, k_s)
                seed_t.add_(1)

            def split_step():
                graph_a.replay()
                y_s.copy_(sharding.gather_rows(g_y, n_rows))  # eager RCCL all-gathers
                k_s.copy_(sharding.gather_rows(g_k, n_rows))
                graph_b.replay()
                return part_c(g_w)
        torch.cuda.synchronize()
    barrier(world)
    t0 = time.perf_counter()
    if pipe:
        pending = [None, None]
        for m in range(per_lane // unroll):
            b = m & 1
            if pending[b] is not None:  # replay m - 2's exchange: before its buffer is rewritten
                pending[b].wait()
                results += stacked(b)
            if n_lanes == 1:
                graphs[b][0].replay()
            else:  # the lanes' graphs on their own streams: the two replays run side by side
                for L in lanes:
                    with torch.cuda.stream(L["stream"]):
                        L["graphs"][b][0].replay()
            if ex:
                pending[b] = exchange(b)
        for m in range(max(0, args.steps // unroll - 2), args.steps // unroll):
            if pending[m & 1] is not None:
                pending[m & 1].wait()
                results += stacked(m & 1)
    else:
        for i in range(args.steps):
            if use_graph and not split:
                graph.replay()
            elif use_graph:
                results.append(split_step())
            else:
                eager_out = step(args.warmup + i, True)
    torch.cuda.synchronize()
    barrier(world)
    elapsed = max_over_ranks(time.perf_counter() - t0, world, dev)
    graph_check = exchange_check = None
    # the last timed step's result: (mean, std) of the fitted weights over the step's repeats
    if not use_graph:
        last = eager_out
    elif pipe:
        # the last step (index K - 1) is the last lane's last step
        last = results[-1] if ex else lanes[-1]["graphs"][(per_lane // unroll - 1) & 1][1][-1]
    else:
        last = results[-1] if split else g_out
    if args.dump_outputs and rank == 0:
        arrays = {"weights_mean": last[0], "weights_std": last[1]}
        if pipe:  # the buffer set of this rank's last fit (the other set holds the next repeat)
            d = lanes[-1]["sets"][(per_lane - 1) & 1]
            arrays.update(fit_weights=d["fit"].w, logits=d["y"][:, 0], kernel_weights=d["k"])
        elif use_graph:  # the static buffers of the last replay
            arrays.update(fit_weights=stash["w"], logits=stash["y"], kernel_weights=stash["k"])
        dump_outputs(args.dump_outputs, arrays)
    if use_graph and args.full:
        # outside the timed region: the last step == an eager step on the same seed
        ref = step(args.warmup + args.steps - 1, False)
        graph_check = max(float((last[0] - ref[0]).abs().max()), float((last[1] - ref[1]).abs().max()))
        if pipe and ex:
            # this rank's staged slot of the last exchange == its last fitted repeat's
            # logits / kernel weights (every rank checks its own slot; max over ranks)
            bl, d = (args.steps // unroll - 1) & 1, sets[(args.steps - 1) & 1]
            mine = gath[bl][rank, unroll - 1]
            exchange_check = max_over_ranks(max(
                float((mine[oy:oy + nl * 4].view(torch.float32) - d["y"][:, 0]).abs().max()),
                float((mine[ok_:ok_ + nl * 8].view(torch.float64) - d["k"]).abs().max())), world, dev)
        if os.environ.get("XPG_BENCH_DEBUG") and not pipe:
            sd = 1000 + args.warmup + args.steps - 1
            b_e = engine.sample_shapley(sd, r1 - r0, S, dev, row_offset=r0)
            y_e = plan.forward(b_e)[:, 0]
            k_e = engine.shap_kernel(b_e, S)
            w_e = engine.wlm_fit(b_e.view(1, R, -1), S, batch, y_e.view(1, R), k_e.view(1, R), w0, params)[0]
            for nm, e in (("bits", b_e), ("y", y_e), ("k", k_e), ("w", w_e)):
                g = stash[nm]
                log(rank, f"stage {nm}: max|diff| {float((g.double() - e.double()).abs().max()):.3e} "
                          f"nan {int(torch.isnan(g.double()).sum())} shape {tuple(g.shape)} vs {tuple(e.shape)}")
    for st in statuses:  # outside the timed region: every fit's (sticky) exchange status
        engine.check_fit_status(st)
    phase_ms = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in ev.items()} \
        if ev["wlm"] else None  # (a plain run of the captured graphs records no eager phases)
    total_rows = n_rows * args.steps
    wl = wlm_bytes(R, S, batch) * (f1 - f0)
    line = {
        "metric": METRIC,
        "value": total_rows / elapsed,
        "unit": "samples/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp32",
        "data": "synthetic",
        "config": {"workload": wdef["text"],
                   "nodes": args.nodes if workload == "c2" else 1_000_000,
                   "edges": args.edges if workload == "c2" else 10_000_000,
                   "feat": args.feat if workload == "c2" else 128,
                   "subgraph_nodes": S, "subgraph_edges": int(sub_ei.shape[1]),
                   "interpret_samples": n_samples, "epochs": args.epochs,
                   "rows_per_repeat": R, "repeats_per_step": times,
                   "parallelism": f"dp{world}: one repeat per rank per step (its rows and its "
                                  "fit); per graph replay one async RCCL all-gather of the "
                                  "replay's logits, kernel weights and fitted weights, then "
                                  "mean / std over all ranks' repeats" if pipe and world > 1 else
                                  f"dp{world}: rows of the step's {times} repeat(s) sharded over "
                                  "ranks, RCCL all-gather of logits + kernel weights, fits "
                                  "sharded by repeat",
                   "mask_sampler": "device (Philox Shapley)",
                   "surrogate_fit": "%s (%d workgroup(s) per fit)" % engine.wlm_plan(f1 - f0, R, S, batch),
                   "fits_in_flight": depth if pipe else 1,
                   "launch": ("eager" if not use_graph else
                              ("two captured HIP graphs per step (masks -> forward + KernelSHAP; "
                               "surrogate fit) with eager RCCL all-gathers between them"
                               if split else
                              f"pipelined captured HIP graphs ({unroll} step(s) per graph "
                              "replay, XPG_BENCH_UNROLL): step i's surrogate "
                              "fit runs beside step i+1's masks -> forward + KernelSHAP "
                              + ("and beside fit i+1: the repeats alternate between two such "
                                 "pipelines (lanes: own buffer sets, side stream and seeds), "
                                 "whose graphs are replayed on two streams (the fit's prologue "
                                 "kernel runs with the production, its losses / best epoch and "
                                 "the mean / std after its Adam steps on the lane's side stream; "
                                 if depth == 2 else
                                 "(double-buffered; the fit's prologue kernel runs with the "
                                 "production, its losses / best epoch and the mean / std after "
                                 "its Adam steps on the side stream, so consecutive fits' steps "
                                 "run back to back; ") +
                              "prologue untimed, K fits + K productions timed; every step is "
                              "one repeat of its own rows, masks and fit)"
                              if pipe else "one captured HIP graph replayed per step") +
                              " (device-resident sampler seed advanced inside the graph)" +
                              ("; phases_ms from eager steps" if args.full else ""))},
        "fit_status": "clean (sticky status words of every fit checked after the timed region)",
    }
    if args.dump_outputs:
        line["outputs_dumped"] = args.dump_outputs
    if not args.full:  # a plain run: the timed steps alone
        del plan
        return line
    line.update({
        "phases_ms": phase_ms,
        "graph_check_max_abs_diff": graph_check,
        "exchange_check_max_abs_diff": exchange_check,
        "roofline": dict(roofline(wl, phase_ms["wlm"] * 1e-3, "headline", WLM_KERNELS),
                         kernel="surrogate fit chain (" + ", ".join(WLM_KERNELS) + ")",
                         note="latency-bound (51 sequential Adam steps, SURVEY.md §8d regime "
                              "(i)); the HBM fraction is reported, not the bound"),
    })
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline_subgraph(args, arch, wdef["kind"], sub_feat, sub_ei,
                                                     q, n_samples)
    del plan
    return line


def _c2_cpu_worker(task):
    """Worker (spawned process, numpy only, 1 BLAS thread): oracle forward of a row chunk."""
    import oracle
    from threadpoolctl import threadpool_limits
    spec, x, ei, m, q = task
    with threadpool_limits(limits=1):
        return oracle.masked_query_outputs(spec, x, {None: ei}, m, q, dtype=np.float32)


def cpu_baseline_subgraph(args, arch, kind, sub_feat, sub_ei, q, n_samples):
    """The numpy oracle (CPU restatement of the reference path) on the host cores: cpu_rows mask
    rows of the same workload, the union-graph forward split over worker processes, then
    KernelSHAP and the (sequential) surrogate fit."""
    import oracle
    S = sub_feat.shape[0]
    rows = args.cpu_rows
    rng = np.random.default_rng(0)
    m = rng.random((rows, S)) < 0.5
    spec = oracle_spec_of(arch, kind)
    x, e = sub_feat.cpu().numpy(), sub_ei.cpu().numpy()
    procs = cpu_procs(args)
    chunks = [(spec, x, e, m[c], q) for c in np.array_split(np.arange(rows), procs * 4)]
    with _pool(procs) as pool:
        pool.map(_c2_cpu_worker, chunks[:procs])  # start-up (imports) outside the timing
        t0 = time.perf_counter()
        y = np.concatenate(pool.map(_c2_cpu_worker, chunks))
        k = oracle.shap_kernel(m)
        oracle.train_wlm(m, n_samples, y, k, np.zeros(S, np.float32),
                         {"lr": 0.01, "l1_lambda": 1e-4}, dtype=np.float32)
        dt = time.perf_counter() - t0
    model, ncpu = host_info()
    return {"value": rows / dt, "unit": "samples/s", "cores": procs, "kind": "port",
            "host_cpu": model, "host_logical_cpus": ncpu, "host_cores": host_cores()[1],
            "sample": f"{rows} mask rows of the same workload (S={S}) through the numpy oracle: "
                      f"union-graph forward over {procs} worker processes (1 thread each), "
                      f"KernelSHAP, surrogate fit ({n_samples} rows per Adam step); "
                      f"{dt:.1f} s"}


# ----------------------------------------------------------------------------- c3 (north star)
def c3_graph(dev, nodes=1_000_000, edges=10_000_000, feat=128, seed=0):
    """configs[2] graph: synthetic homogeneous, 2-layer SAGEConv(mean) 128-128-128, head
    Linear(128, 1) + sigmoid (random init, ConvStack layout of the reference tests)."""
    from bikg_graph_explainability_public_amd.nn import ConvStack
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((nodes, feat), generator=g)
    ei = torch.randint(0, nodes, (2, edges), generator=g)
    torch.manual_seed(seed)
    arch = ConvStack("sage", [feat, feat, feat], [feat, 1]).eval()
    return x, ei, arch


def full_graph_alg_bytes(n, e_kept_per_row, e, f_in, f_out, rows, layers=2):
    """SURVEY.md §8d algorithmic bytes per sample of the full-graph masked forward, summed over
    the rows; per layer 4(N+1) + 4E (CSR) + N/8 (mask bits) + 4 F_g E_kept (gathered rows,
    F_g = min(F_in, F_out)) + 4 F_root N (SAGE self rows) + 4 F_out N (layer output).
    Returns (total, per layer)."""
    per_layer = 4 * (n + 1) * rows + 4 * e * rows + n / 8 * rows + \
        4 * min(f_in, f_out) * float(np.sum(e_kept_per_row)) + 4 * f_in * n * rows + \
        4 * f_out * n * rows
    return layers * per_layer, per_layer


def wide_kernel_bytes(n, e, f, rows, e_kept_rows, active_rows, gcn=False):
    """Algorithmic HBM bytes of the implemented wide kernels over `rows` mask rows (32-row passes),
    per kernel:
      k_wide_l1s (layer 1): per pass the CSR (ptr, source positions, target positions, self
        counts), the keep words of every in-edge and target, every in-edge's table row ONCE
        (features are never masked: one read serves all 32 samples), the target's own table rows
        (term + ROOT), the h1 rows of the samples that keep the target and one inactive row
        (ctab) per target;
      k_wide_last_ws (layer 2 + head): per pass the CSR (ptr, edge sources, source positions,
        target positions, self counts), the keep words, per sample the h1 row of every kept
        in-edge and the target's own row (h1 when the sample keeps it, else the shared ctab row,
        one read per target), and the logits.
    e_kept_rows / active_rows: per mask row, the kept-edge count and the active-node count."""
    passes = -(-rows // 32)
    fb = 4 * f
    l1 = passes * (4 * (n + 1) + 4 * e + 8 * n + 4 * e + 4 * n + fb * e + 2 * fb * n + fb * n) + \
        fb * float(np.sum(active_rows))
    l2 = passes * (4 * (n + 1) + 8 * e + 12 * n + 4 * e + 4 * n + fb * n) + \
        fb * float(np.sum(e_kept_rows)) + fb * float(np.sum(active_rows)) + 4 * rows * n
    return {"k_wide_l1s": l1, "k_wide_last_ws": l2}


C3_KERNELS = ("k_wide_bits", "k_wide_f0", "k_wide_degree", "k_wide_l1s", "k_wide_last_ws")
# the instantiations the c3 plan runs with no XPG_WIDE_* switch set (run_wide_forward's
# defaults), as rocprofv3 names them: the counter bytes of the line are these kernels' own
# dispatches (the exact-f32 comparison pass is another instantiation and is not mixed in)
C3_DEFAULT_INSTANCES = {"k_wide_l1s": "k_wide_l1s<2, false>",
                        "k_wide_last_ws": "k_wide_last_ws<8, 32, 8, true, 1, true, 8, true, true>"}
C3_EXACT_F32_INSTANCE = "k_wide_last_ws<8, 32, 8, false, 1, false, 4, false, false>"


def c3_section(args, dev, world, rank):
    """Regime (ii) on configs[2]: every node a target of the masked forward,
    c3_rows mask rows sharded over the ranks in 32-row passes (strong scaling), then the RCCL
    all-gather of 64 query columns' logits of every row (what the surrogate fits consume).
    Per-kernel device times come from HIP events the library records around each launch on its
    stream (engine.profile_*), so every kernel's roofline fraction is its own bytes over its
    own time; the line's roofline is the dominant kernel (layer 2)."""
    from bikg_graph_explainability_public_amd import engine, pipeline, sharding
    x, ei, arch = c3_graph(dev)
    N, E = x.shape[0], ei.shape[1]
    eid = ei.to(dev)
    plan = pipeline.build_plan(arch.to(dev), x.to(dev), eid, list(range(N)))
    total = args.c3_rows
    # shard in whole 32-sample passes where possible
    passes = -(-total // 32)
    p0, p1 = sharding.shard_range(passes, world, rank)
    r0, r1 = min(total, 32 * p0), min(total, 32 * p1)
    bits = engine.sample_shapley(77, r1 - r0, N, dev, row_offset=r0)
    qcols = torch.arange(7, N, N // 64, device=dev)[:64]
    stream = torch.cuda.current_stream()
    plan.forward(bits)  # warm-up (workspace, code objects); counted in the PMC ops
    reps = 3
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    barrier(world)
    t0 = time.perf_counter()
    a.record(stream)
    for _ in range(reps):
        y = plan.forward(bits)
    b.record(stream)
    logits = y[:, qcols] if not multi(world) else _gather_uneven(y[:, qcols].contiguous(), world)
    torch.cuda.synchronize()
    barrier(world)
    wall = max_over_ranks((time.perf_counter() - t0) / reps, world, dev)
    fwd_ms = a.elapsed_time(b) / reps
    # per-kernel device times (HIP events around each launch): one forward with the passes
    # serialised (XPG_WIDE_OVERLAP=0) — with layer 1 of pass p+1 queued beside layer 2 of pass p,
    # a side-stream launch's events also count its wait for the CUs layer 2 holds
    os.environ["XPG_WIDE_OVERLAP"] = "0"
    try:
        engine.profile_enable(True)
        plan.forward(bits)
        kt = engine.profile_read()
        engine.profile_enable(False)
    finally:
        os.environ.pop("XPG_WIDE_OVERLAP", None)
    assert logits.shape == (total, qcols.numel())
    # bitwise fingerprint of the gathered query-column logits (the 2-rank rehearsal compares it
    # with a 1-rank run: sharding + all-gather must not change a bit)
    import hashlib
    checksum = hashlib.sha256(logits.float().cpu().numpy().tobytes()).hexdigest()[:16]
    # per row: kept edges (both endpoints active) and active nodes, for the byte counts
    kept, act = [], []
    for c0 in range(0, r1 - r0, 32):
        m = engine.unpack_masks(bits[c0:c0 + 32], N)
        kept.append((m[:, eid[0]] & m[:, eid[1]]).sum(1).double().cpu().numpy())
        act.append(m.sum(1).double().cpu().numpy())
        del m
    kept = np.concatenate(kept) if kept else np.zeros(0)
    act = np.concatenate(act) if act else np.zeros(0)
    rows_rank = r1 - r0
    alg_survey, per_layer = full_graph_alg_bytes(N, kept, E, 128, 128, rows_rank)
    kb = wide_kernel_bytes(N, E, 128, rows_rank, kept, act)
    npass = -(-rows_rank // 32)
    slot = {"k_wide_l1s": "wide_l1", "k_wide_last_ws": "wide_l2"}
    # counter bytes per launch (= per 32-row pass) of the exact default instantiations, from the
    # section's PMC file (per-dispatch averages: no op count involved)
    pm, _ = pmc_file("c3")
    kernels = {}
    for k, sl in slot.items():
        ms_tot, launches = kt[sl]
        ms = ms_tot / max(1, launches)  # per launch = per 32-row pass
        alg = kb[k] / npass
        d = {"launch_ms": ms, "launches": launches, "alg_bytes_per_launch": alg,
             "achieved_GBps": alg / (ms * 1e-3) / 1e9, "frac": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
        rec = (pm or {}).get(C3_DEFAULT_INSTANCES[k])
        if rec is not None and rec.get("traffic_bytes") is not None:
            cb = rec["traffic_bytes"]
            d.update(counter_instance=C3_DEFAULT_INSTANCES[k], counter_dispatches=rec["dispatches"],
                     counter_bytes_per_launch=cb, counter_GBps=cb / (ms * 1e-3) / 1e9,
                     frac_counter=cb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, counter_over_alg=cb / alg)
        kernels[k] = d
    dom = max(kernels, key=lambda k: kernels[k]["launch_ms"])
    kd = kernels[dom]
    other_ms = {k: kt[k][0] / max(1, kt[k][1]) for k in ("wide_bits", "wide_f0", "wide_degree")}
    # the exact-f32 layer 2 (XPG_WIDE_B3=0) beside the default three-piece bf16 products: one pass
    os.environ["XPG_WIDE_B3"] = "0"
    try:
        b32 = bits[:32]
        y_b3 = plan.forward(b32)
        engine.profile_enable(True)
        y_ex = plan.forward(b32)
        kt_ex = engine.profile_read()
        engine.profile_enable(False)
    finally:
        os.environ.pop("XPG_WIDE_B3", None)
    y_b3 = plan.forward(b32)
    ex_ms = kt_ex["wide_l2"][0] / max(1, kt_ex["wide_l2"][1])
    alg2 = kb["k_wide_last_ws"] / npass
    exact = {"kernel": C3_EXACT_F32_INSTANCE, "layer2_ms": ex_ms,
             "achieved_GBps": alg2 / (ex_ms * 1e-3) / 1e9,
             "frac": alg2 / (ex_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
             "note": "the same algorithmic bytes per pass over the exact-f32 MFMA kernel's time "
                     "(one pass of the first 32 rows)",
             "max_abs_diff_vs_bf16x3": float((y_ex - y_b3).abs().max())}
    rec = (pm or {}).get(C3_EXACT_F32_INSTANCE)
    if rec is not None and rec.get("traffic_bytes") is not None:
        exact.update(counter_bytes_per_launch=rec["traffic_bytes"],
                     frac_counter=rec["traffic_bytes"] / (ex_ms * 1e-3) / 1e9 / HBM_PEAK_GBS)
    flops = rows_rank * N * 2.0 * (2 * 128 * 128 + 128)  # layer-2 dense (l and r) + head
    out = {
        "workload": "c3 (BASELINE configs[2]) full-graph masked forward (SURVEY.md §8d regime "
                    "(ii)): 1M nodes / 10M edges, 128 feats, 2-layer SAGEConv(mean) + "
                    "Linear(128,1) + sigmoid, every node a target (all 1M outputs per mask row), "
                    f"{total} mask rows sharded over {world} rank(s) in 32-row passes, then an "
                    "all-gather of 64 query columns of every row",
        "rows": total, "rows_per_rank": rows_rank, "logits_checksum": checksum,
        "ms": wall * 1e3,
        "forward_ms_rank0": fwd_ms, "pass_ms_rank0": fwd_ms / max(1, npass),
        "samples_per_s": total / wall,
        "samples_per_s_per_rank": rows_rank / (fwd_ms * 1e-3),
        "node_outputs_per_s": total * N / wall,
        "scaling": "strong",
        "kernels": kernels, "small_kernels_launch_ms": other_ms,
        "kernel_time_source": "one forward with the passes serialised (XPG_WIDE_OVERLAP=0), HIP "
                              "events around each launch; the timed forwards overlap layer 1 of "
                              "pass p+1 with layer 2 of pass p",
        "roofline": {"bound": "hbm", "kernel": dom, "achieved": kd["achieved_GBps"],
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": kd["frac"],
                     "bytes_per_launch": kd["alg_bytes_per_launch"],
                     "traffic": kd.get("counter_bytes_per_launch"),
                     "traffic_source": "profiles/pmc_c3.json" if kd.get("counter_instance") else None,
                     "traffic_kernel": kd.get("counter_instance"),
                     "frac_counter": kd.get("frac_counter"),
                     "counter_over_alg": kd.get("counter_over_alg"),
                     "time_source": "HIP events around each launch on its stream (xpg_profile_*)",
                     "bytes_formula": "wide_kernel_bytes (implemented algorithm, per 32-row pass)"},
        "survey_formula": {"alg_bytes": alg_survey, "alg_bytes_per_layer": per_layer,
                           "achieved_GBps": alg_survey / (fwd_ms * 1e-3) / 1e9,
                           "note": "SURVEY.md §8d B_alg per sample: counts layer 1's table-row "
                                   "gather per sample (the kernel reads each row once per 32 "
                                   "samples) and a 128-wide layer-2 output per node (the head "
                                   "is fused: 4 B per node) — an upper bound on useful bytes, "
                                   "not a fraction of peak"},
        "layer2_exact_f32": exact,
        "mfma": {"tflops": flops / (fwd_ms * 1e-3) / 1e12, "peak_fp32_tflops": FP32_MFMA_PEAK_TF,
                 "note": "fp32-equivalent layer-2 + head flops over the whole chain time (the "
                         "products run as three bf16 MFMAs): a rate, not MFMA-pipe utilisation"},
    }
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_c3(args)
    del plan, y
    torch.cuda.empty_cache()
    return out


def _gather_uneven(t, world):
    """All-gather of per-rank row blocks of different sizes (pads to the largest)."""
    import torch.distributed as dist
    n = torch.tensor([t.shape[0]], device=t.device)
    sizes = [torch.empty_like(n) for _ in range(world)]
    dist.all_gather(sizes, n)
    sizes = [int(s.item()) for s in sizes]
    cap = max(sizes)
    buf = t.new_zeros((cap,) + tuple(t.shape[1:]))
    buf[:t.shape[0]] = t
    outs = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(outs, buf)
    return torch.cat([o[:s] for o, s in zip(outs, sizes)])


def _c3_cpu_worker(seed):
    """Worker (spawned, numpy oracle, 1 BLAS thread): ONE full-size c3 mask row — the graph and
    the model are regenerated from their seeds (same as the GPU run), every node an output."""
    import oracle
    from threadpoolctl import threadpool_limits
    x, ei, arch = c3_graph("cpu")
    sd = {k: v.detach().numpy() for k, v in arch.state_dict().items()}
    spec = {"convs": [{"kind": "sage", "rels": [None], "act": "relu",
                       "params": {None: {"Wl": sd[f"conv.{2 * i}.lin_l.weight"],
                                         "bl": sd[f"conv.{2 * i}.lin_l.bias"],
                                         "Wr": sd[f"conv.{2 * i}.lin_r.weight"]}}}
                      for i in range(2)],
            "fc": [{"W": sd["fc.0.weight"], "b": sd["fc.0.bias"], "act": "sigmoid"}]}
    xn, e = x.numpy(), ei.numpy()
    m = np.random.default_rng(seed).random(xn.shape[0]) < 0.5
    keep = m[e[0]] & m[e[1]]
    with threadpool_limits(limits=1):
        t0 = time.perf_counter()
        oracle.forward_union(spec, xn, {None: (e[0][keep], e[1][keep])}, dtype=np.float32)
        return time.perf_counter() - t0


def cpu_baseline_c3(args):
    """The numpy oracle on the host cores: one full-size c3 mask row (1M nodes / 10M edges, every
    node an output) per worker process, all workers at once."""
    procs = cpu_procs(args, cap=48)  # each worker regenerates the 1M / 10M graph (~2 GB)
    with _pool(procs) as pool:
        t0 = time.perf_counter()
        per = pool.map(_c3_cpu_worker, list(range(procs)))
        dt = time.perf_counter() - t0
    model, ncpu = host_info()
    return {"value": procs / max(per), "unit": "samples/s", "cores": procs, "kind": "port",
            "host_cpu": model, "host_logical_cpus": ncpu, "host_cores": host_cores()[1],
            "sample": f"{procs} full-size mask rows, one per worker process (1 thread each, all "
                      f"concurrent), through the numpy oracle's union-graph forward: "
                      f"{np.mean(per):.1f} s mean / {max(per):.1f} s max forward per row "
                      f"(value = rows / max); {dt:.1f} s wall incl. graph generation"}


# ----------------------------------------------------------------------------- c5
C5_RELS = [("gene", "interacts", "gene"), ("gene", "encodes", "protein"),
           ("protein", "binds", "protein"), ("drug", "targets", "protein"),
           ("protein", "regulates", "gene")]


def c5_section(args, dev, world, rank):
    """configs[4]: 1M-node heterogeneous graph (500k gene / 300k protein / 200k drug, 256-dim
    features each), 5 relations (3 bipartite), 10M edges, 2-layer HeteroConv(SAGE) 256 -> 64 ->
    64 + head 64 -> 16 -> 1 + sigmoid, node_prediction of gene 7 (the L+1-hop subgraph by the HIP
    k-hop kernel), 20 random communities over the subgraph, device community sampler,
    interpret_samples=1024 x epochs=50, repeats=10, the reference's Q4 targets, community scores.
    One step = the whole 10-repeat job, sharded as Explainer.run shards it: each rank forwards +
    KernelSHAPs its shard of the 10 x R rows, all-gathers the logits and kernel weights, fits its
    share of the repeats in one batched launch, all-gathers the weights, then mean / std and the
    community means.  The community sampler addresses rows directly, so a rank draws only the
    rows it forwards and the repeats it fits (every repeat's seed is the same on every rank;
    Explainer.run still draws every repeat's rows on every rank and checks them replicated)."""
    from bikg_graph_explainability_public_amd import engine, pipeline, sharding
    from bikg_graph_explainability_public_amd.data import Data
    from bikg_graph_explainability_public_amd.masks import Mask
    from bikg_graph_explainability_public_amd.nn import HeteroSageStack
    from bikg_graph_explainability_public_amd.pathways import Pathways
    sizes = {"gene": 500_000, "protein": 300_000, "drug": 200_000}
    F = 256
    g = torch.Generator(device=dev).manual_seed(5)
    feat = {t: torch.randn((n, F), generator=g, device=dev) for t, n in sizes.items()}
    ei = {r: torch.stack([torch.randint(0, sizes[r[0]], (2_000_000,), generator=g, device=dev),
                          torch.randint(0, sizes[r[-1]], (2_000_000,), generator=g, device=dev)])
          for r in C5_RELS}
    torch.manual_seed(0)
    arch = HeteroSageStack(C5_RELS, {t: F for t in sizes}, 64, 2, [64, 16, 1]).to(dev).eval()
    fh, eh, nt, et, _, _, pads = Data(feat, ei).hetero2homo()
    ntn, etn = list(feat), list(ei)
    del feat, ei
    sub_x, sub_ei, _, sub_ind, sub_nt, sub_et = Data(fh, eh).comp_graph(
        7, 2, "node", [str(i) for i in range(fh.shape[0])], nt, et)
    del fh, eh, nt, et
    sub_nt = sub_nt.long()
    q = int(sub_ind)
    plan = pipeline.build_plan(arch, sub_x, sub_ei, [q], sub_nt, sub_et, ntn, etn, pads)
    assert plan is not None and plan.multi_type
    S = sub_x.shape[0]
    rng = np.random.default_rng(20)
    cuts = np.sort(rng.choice(np.arange(1, S), 19, replace=False))
    pathways = [sorted(c.tolist()) for c in np.split(rng.permutation(S), cuts)]
    epochs, times = 50, args.c5_times
    params = {"interpret_samples": args.c5_samples, "epochs": epochs, "lr": 0.01,
              "l1_lambda": 1e-4}
    cplan = Mask(sub_x, sub_ei, pathways, params, "node_prediction").community_plan()
    tabs = engine.community_tables(cplan, pathways, S, dev)
    R = cplan[2]
    batch = R // epochs
    n_rows = times * R
    r0, r1 = sharding.shard_range(n_rows, world, rank)
    f0, f1 = sharding.shard_range(times, world, rank)
    w0 = torch.zeros((times, S), device=dev)
    fit = {"lr": 0.01, "l1_lambda": 1e-4}
    pw = Pathways(pathways, [f"community_{i}" for i in range(20)])
    stream = torch.cuda.current_stream()
    statuses = []
    phases = ("sample", "forward", "shap", "gather", "wlm", "scores")
    ev = {k: [] for k in phases}

    def rows_of(step_seed, lo, hi):
        """global mask rows [lo, hi) of the job (repeat i = seed step_seed * 100 + i)"""
        buf = torch.empty((hi - lo, (S + 31) // 32), dtype=torch.int32, device=dev)
        for i in range(lo // R, (hi - 1) // R + 1 if hi > lo else lo // R):
            a_, b_ = max(lo, i * R) - i * R, min(hi, (i + 1) * R) - i * R
            engine.sample_communities(step_seed * 100 + i, cplan, pathways, S, dev, tables=tabs,
                                      row_offset=a_, rows=b_ - a_,
                                      out=buf[i * R + a_ - lo:i * R + b_ - lo])
        return buf

    def job(step_seed, record):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)]
        mk = (lambda j: marks[j].record(stream)) if record else (lambda j: None)
        mk(0)
        # this rank's forward rows [r0, r1) and fit repeats' rows [f0 R, f1 R): one draw over
        # their union when they overlap or touch (one rank: the same range), else two
        g0, g1 = f0 * R, f1 * R
        if f1 == f0:
            shard = rows_of(step_seed, r0, r1)
            fbits = shard[:0]
        elif g0 <= r1 and r0 <= g1:
            lo, hi = min(r0, g0), max(r1, g1)
            u = rows_of(step_seed, lo, hi)
            shard, fbits = u[r0 - lo:r1 - lo], u[g0 - lo:g1 - lo]
        else:
            shard, fbits = rows_of(step_seed, r0, r1), rows_of(step_seed, g0, g1)
        fbits = fbits.reshape(f1 - f0, R, (S + 31) // 32)
        mk(1)
        y_loc = plan.forward(shard)[:, 0]
        empty = pipeline.empty_copy_rows(shard, S, sub_ei)
        mk(2)
        k_loc = engine.shap_kernel(shard, S)
        mk(3)
        y = sharding.gather_rows(y_loc, n_rows).view(times, R)
        empty = sharding.gather_rows(empty, n_rows).view(times, R)
        k = sharding.gather_rows(k_loc, n_rows).view(times, R)
        y = torch.stack([pipeline.multi_type_targets(y[i], empty[i], batch, q, S, q4=True)
                         for i in range(f0, f1)]) if f1 > f0 else y[:0]
        mk(4)
        st = torch.zeros(1, dtype=torch.int32, device=dev)  # sticky status word: starts at 0
        if f1 > f0:
            w, _, _, _, _ = engine.wlm_fit(fbits, S, batch, y, k[f0:f1], w0[f0:f1], fit,
                                           check=False, status=st)
            statuses.append(st)
        else:
            w = torch.empty((0, S), device=dev)
        w_all = sharding.gather_rows(w, times)
        mean, std = w_all.mean(0), w_all.std(0, unbiased=False)
        mk(5)
        pdf = pw.aggregate(mean, pathways)  # device segmented mean + DataFrame (host sync)
        mk(6)
        if record:
            for j, name in enumerate(phases):
                ev[name].append((marks[j], marks[j + 1]))
        return mean, std, pdf

    job(0, False)
    reps = 2
    barrier(world)
    t0 = time.perf_counter()
    for i in range(reps):
        res = job(1 + i, True)
    torch.cuda.synchronize()
    barrier(world)
    wall = max_over_ranks((time.perf_counter() - t0) / reps, world, dev)
    for st in statuses:
        engine.check_fit_status(st)
    ph = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in ev.items()}
    out = {"workload": "c5 (BASELINE configs[4]): 1M-node hetero graph (3 node types, 256-dim "
                       "feats, 5 relations / 10M edges), 2-layer HeteroConv(SAGE) 256->64->64 + "
                       "head 64->16->1, node_prediction of gene 7, 20 random communities, device "
                       f"community sampler, interpret_samples={args.c5_samples} x epochs=50, "
                       f"repeats={times}, reference Q4 targets, community scores",
           "subgraph_nodes": S, "subgraph_edges": int(sub_ei.shape[1]),
           "rows_per_repeat": R, "repeats": times, "rows_per_job": n_rows,
           "ms_per_job": wall * 1e3, "samples_per_s": n_rows / wall,
           "phases_ms_rank0": ph, "scaling": "strong",
           # the last job's mean / std weights: bitwise the same at every world size (rows are
           # independent, each repeat's fit is the same computation on one rank)
           "result_checksum": float(res[0].double().abs().sum() + res[1].double().abs().sum()),
           "parallelism": f"{world} rank(s): each rank draws, forwards and KernelSHAPs its shard of "
                          f"the {times} x R rows, RCCL all-gather of logits / kernel weights, "
                          "fits sharded by repeat (batched launch per rank, masks of its repeats "
                          "drawn by the rank)"}
    del plan
    torch.cuda.empty_cache()
    return out


# ----------------------------------------------------------------------------- N = 1 sections
GP_KERNELS = ("k_wlm_stats", "k_gw_p", "k_gw_g", "k_gw_grad", "k_gw_loss", "k_argmin_first")
GP_FUSED_KERNELS = ("k_wlm_stats", "k_gw_fused", "k_gw_loss", "k_argmin_first")


def graph_prediction_section(args, dev):
    """The reference's graph_prediction semantics on the c3 graph (explainer.py:427-447: no
    subgraph, S = N = 1M mask columns) for one query node, one repeat of interpret_samples=512,
    epochs=50 (25,600 rows): device sampler with fused row counts -> receptive-field forward ->
    KernelSHAP -> many-column surrogate fit (k_gw_fused: one persistent launch, each step's mask
    bits read once; XPG_WLM=grid3: the three-launch k_gw_p / k_gw_g / k_gw_grad steps, which
    stream them twice)."""
    from bikg_graph_explainability_public_amd import engine, pipeline
    x, ei, arch = c3_graph(dev)
    N = x.shape[0]
    plan = pipeline.build_plan(arch.to(dev), x.to(dev), ei.to(dev), [7])
    R, epochs = 512 * 50, 50
    batch = R // epochs
    w0 = torch.zeros(N, device=dev)
    params = {"lr": 0.01, "l1_lambda": 1e-4}
    stream = torch.cuda.current_stream()
    status = torch.zeros(1, dtype=torch.int32, device=dev)  # sticky fit status, read after timing

    def rep(i, ev=None):
        mk = (lambda j: ev[j].record(stream)) if ev else (lambda j: None)
        mk(0)
        bits, cnt = engine.sample_shapley(500 + i, R, N, dev, with_counts=True)
        mk(1)
        y = plan.forward(bits)[:, 0]
        mk(2)
        k = engine.shap_kernel(bits, N, counts=cnt)
        mk(3)
        engine.wlm_fit(bits, N, batch, y, k, w0, params, check=False, status=status)
        mk(4)

    rep(0)
    torch.cuda.synchronize()
    reps = 3
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(reps)]
    for i in range(reps):
        rep(1 + i, evs[i])
    torch.cuda.synchronize()
    ph = {name: float(np.mean([e[j].elapsed_time(e[j + 1]) for e in evs]))
          for j, name in enumerate(("sample", "forward", "shap", "wlm"))}
    engine.check_fit_status(status)  # a fit whose exchange timed out raises (after the timing)
    total = sum(ph.values())
    W = (N + 31) // 32
    kind, parts = engine.wlm_plan(1, R, N, batch)
    if kind == "grid_fused":  # bits once per step; w / m / v read and written once per fit
        wbytes, kernels = R * W * 4 + 6 * N * 4, GP_FUSED_KERNELS
        formula = "R x ceil(S/32) x 4 (bits, read once) + 24 S (w, m, v read + write, once per fit)"
    else:
        wbytes, kernels = 2 * R * W * 4 + epochs * 6 * N * 4, GP_KERNELS
        formula = "2 x R x ceil(S/32) x 4 (bits, p and grad passes) + steps x 24 S (w, m, v read + write)"
    return {"workload": "c3 graph_prediction, one query (node 7), S = 1M mask columns, "
                        "interpret_samples=512 x epochs=50 = 25,600 rows, one repeat",
            "ms_per_repeat": total, "samples_per_s": R / (total * 1e-3), "phases_ms": ph,
            "surrogate_fit": "%s (%d workgroup(s) per fit)" % (kind, parts),
            "fit_status": "clean (sticky status word of every fit checked after the timed repeats)",
            "roofline": dict(roofline(wbytes, ph["wlm"] * 1e-3, "gp", kernels),
                             kernel="many-column surrogate fit (" + ", ".join(kernels) + ")",
                             bytes_formula=formula),
            "sampler_GBps": R * W * 4 / (ph["sample"] * 1e-3) / 1e9}


def hetero_c4_section(args, dev, world=1, rank=0):
    """c4 (BASELINE.json configs[3], "4 x MI355X"): 3 node types (200k gene / 200k protein /
    100k drug, 84 / 64 / 32 features), 5 relations (3 bipartite), 5M edges, one HeteroConv(SAGE)
    layer (gcn_hetero_1hop shape: 84 -> 16, head 16 -> 16 -> 32 -> 1; GCNConv cannot take
    bipartite relations), node_prediction of gene 7 through Explainer's host steps (hetero2homo,
    k-hop subgraph on the GPU).  One step = a job of `c4_times` repeats of interpret_samples=256
    x epochs=50 rows: device Shapley masks -> node-type-gated forward -> empty-copy targets ->
    KernelSHAP -> surrogate fits, sharded as Explainer.run shards it (each rank draws, forwards
    and KernelSHAPs its contiguous shard of the times x R rows -- the Philox sampler addresses
    rows directly --, RCCL all-gather of logits / empty flags / kernel weights, fits split by
    repeat, weights all-gathered, mean / std).  Targets are per-copy (hetero_q4=False): the
    reference's Q4 extraction cannot run at this shape (see q4_true).  Regime (i): the subgraph
    is cache-resident, so samples/s is the figure (no HBM fraction).  `reference_loop` (one rank)
    times the reference's own per-copy multi-type loop (model.py:196-249, one arch call + host
    sync per row) on the same GPU for one batch."""
    from bikg_graph_explainability_public_amd import engine, pipeline, sharding
    from bikg_graph_explainability_public_amd.data import Data
    from bikg_graph_explainability_public_amd.model import Model
    from bikg_graph_explainability_public_amd.nn import HeteroSageStack
    sizes = {"gene": 200_000, "protein": 200_000, "drug": 100_000}
    dims = {"gene": 84, "protein": 64, "drug": 32}
    g = torch.Generator(device=dev).manual_seed(4)
    feat = {t: torch.randn((n, dims[t]), generator=g, device=dev) for t, n in sizes.items()}
    ei = {r: torch.stack([torch.randint(0, sizes[r[0]], (1_000_000,), generator=g, device=dev),
                          torch.randint(0, sizes[r[-1]], (1_000_000,), generator=g, device=dev)])
          for r in C5_RELS}
    torch.manual_seed(0)
    arch = HeteroSageStack(C5_RELS, dims, 16, 1, [16, 16, 32, 1]).to(dev).eval()
    d = Data(feat, ei)
    fh, eh, nt, et, _, _, pads = d.hetero2homo()
    ntn, etn = list(feat), list(ei)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sub_x, sub_ei, _, sub_ind, sub_nt, sub_et = Data(fh, eh).comp_graph(
        7, 1, "node", [str(i) for i in range(fh.shape[0])], nt, et)
    torch.cuda.synchronize()
    t_khop = time.perf_counter() - t0
    sub_nt = sub_nt.long()
    q = int(sub_ind)  # gene = type 0 comes first in the sorted subset: position among genes
    plan = pipeline.build_plan(arch, sub_x, sub_ei, [q], sub_nt, sub_et, ntn, etn, pads)
    assert plan is not None and plan.multi_type
    S = sub_x.shape[0]
    R, epochs = 256 * 50, 50
    batch = R // epochs
    times = args.c4_times
    n_rows = times * R
    r0, r1 = sharding.shard_range(n_rows, world, rank)
    f0, f1 = sharding.shard_range(times, world, rank)
    params = {"lr": 0.01, "l1_lambda": 1e-4}
    w0 = torch.zeros((times, S), device=dev)
    stream = torch.cuda.current_stream()
    phases = ("sample", "forward", "shap", "gather", "wlm")
    ev = {k: [] for k in phases}
    statuses = []

    def rows_of(step_seed, lo, hi, counts=False):
        """global rows [lo, hi) of the job (repeat i = Philox seed step_seed * 100 + i)"""
        parts, cparts = [], []
        for i in range(lo // R, (hi - 1) // R + 1 if hi > lo else lo // R):
            a_, b_ = max(lo, i * R) - i * R, min(hi, (i + 1) * R) - i * R
            bits, cnt = engine.sample_shapley(step_seed * 100 + i, b_ - a_, S, dev,
                                              row_offset=a_, with_counts=True)
            parts.append(bits)
            cparts.append(cnt)
        if not parts:
            e = torch.empty((0, (S + 31) // 32), dtype=torch.int32, device=dev)
            return (e, torch.empty(0, dtype=torch.int32, device=dev)) if counts else e
        bits = parts[0] if len(parts) == 1 else torch.cat(parts)
        cnt = cparts[0] if len(cparts) == 1 else torch.cat(cparts)
        return (bits, cnt) if counts else bits

    def job(step_seed, record):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)]
        mk = (lambda j: marks[j].record(stream)) if record else (lambda j: None)
        mk(0)
        shard, cnt = rows_of(step_seed, r0, r1, counts=True)
        fbits = rows_of(step_seed, f0 * R, f1 * R).reshape(f1 - f0, R, (S + 31) // 32)
        mk(1)
        y_loc = plan.forward(shard)[:, 0]
        empty = pipeline.empty_copy_rows(shard, S, sub_ei)
        mk(2)
        k_loc = engine.shap_kernel(shard, S, counts=cnt)
        mk(3)
        y = sharding.gather_rows(y_loc, n_rows).view(times, R)
        empty = sharding.gather_rows(empty, n_rows).view(times, R)
        k = sharding.gather_rows(k_loc, n_rows).view(times, R)
        y = torch.stack([pipeline.multi_type_targets(y[i], empty[i], batch, q, S, q4=False)
                         for i in range(f0, f1)]) if f1 > f0 else y[:0]
        mk(4)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        if f1 > f0:
            w, _, _, _, _ = engine.wlm_fit(fbits, S, batch, y, k[f0:f1], w0[f0:f1], params,
                                           check=False, status=st)
            statuses.append(st)
        else:
            w = torch.empty((0, S), device=dev)
        w_all = sharding.gather_rows(w, times)
        mean, std = w_all.mean(0), w_all.std(0, unbiased=False)
        mk(5)
        if record:
            for j, name in enumerate(phases):
                ev[name].append((marks[j], marks[j + 1]))
        return mean, std

    job(0, False)
    torch.cuda.synchronize()
    reps = 5
    barrier(world)
    t0 = time.perf_counter()
    for i in range(reps):
        res = job(1 + i, True)
    torch.cuda.synchronize()
    barrier(world)
    wall = max_over_ranks((time.perf_counter() - t0) / reps, world, dev)
    for st in statuses:
        engine.check_fit_status(st)
    ph = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in ev.items()}
    ncut = len(range(q, batch, S))
    out = {"workload": "c4 (BASELINE configs[3]): 3 node types (200k/200k/100k, 84/64/32 "
                       "feats), 5 relations (3 bipartite), 5M edges, HeteroConv(SAGE) 1 layer "
                       "84->16 + head 16->16->32->1, node_prediction of gene 7, "
                       f"interpret_samples=256 x epochs=50 = {R} rows per repeat, {times} repeats "
                       "per job, per-copy targets",
           "subgraph_nodes": S, "subgraph_edges": int(sub_ei.shape[1]), "khop_ms": t_khop * 1e3,
           "rows_per_repeat": R, "repeats": times, "rows_per_job": n_rows,
           "ms_per_job": wall * 1e3, "samples_per_s": n_rows / wall, "phases_ms_rank0": ph,
           "scaling": "strong", "world": world,
           # the last job's mean / std weights: bitwise the same at every world size
           "result_checksum": float(res[0].double().abs().sum() + res[1].double().abs().sum()),
           "parallelism": f"{world} rank(s): each rank draws, forwards and KernelSHAPs its shard "
                          f"of the {times} x R rows, RCCL all-gather of logits / empty flags / "
                          "kernel weights, fits sharded by repeat, weights all-gathered",
           "q4_false": {"semantics": "per-copy targets (hetero_q4=False)",
                        "ms_per_repeat": wall * 1e3 / times, "samples_per_s": n_rows / wall}}
    if ncut not in (1, batch):
        # the reference's Q4 extraction keeps out[sub_ind::S] of each batch of copies: with batch
        # > S it keeps several values, which weighted_mse_loss cannot broadcast against the
        # [batch] prediction -- the reference fails on this configuration
        out["q4_true"] = {
            "semantics": "reference (quirk Q4)",
            "result": f"not runnable in the reference: batch {batch} > subgraph {S} nodes, so "
                      f"each batch's extraction out[{q}::{S}] keeps {ncut} values and "
                      "weighted_mse_loss (wlm.py:517) cannot broadcast them against the "
                      f"{batch} predictions; the engine raises the same error "
                      "(pipeline.multi_type_targets)"}
    if world == 1:
        # the reference's per-copy loop on the same GPU, one batch of rows
        mask = engine.unpack_masks(engine.sample_shapley(77, batch, S, dev), S)
        cf, cnt_t, pei, pet = Data(sub_x, sub_ei).perturbator(mask, "node", sub_nt, sub_et)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Model(arch).predict_hetero_output(cf, pei.long(), cnt_t, pet, ntn, etn, batch, S, q,
                                          pads, "node")
        torch.cuda.synchronize()
        out["reference_loop_gpu_samples_per_s"] = batch / (time.perf_counter() - t0)
    del plan
    torch.cuda.empty_cache()
    return out


def communities_section(args, dev, reps=10):
    """c2 with 20 random communities over the subgraph (SURVEY.md §8d c5-style communities):
    the device community sampler (k_communities) inside the full repeat pipeline, and the
    compat CPU sampler (the reference's masks.py:262-397 algorithm and RNG order) beside it."""
    from bikg_graph_explainability_public_amd import engine
    from bikg_graph_explainability_public_amd.masks import Mask
    arch, sub_feat, sub_ei, q, plan = build_c2(args, dev)
    S = plan.cols
    rng = np.random.default_rng(20)
    cuts = np.sort(rng.choice(np.arange(1, S), 19, replace=False))
    pathways = [c.tolist() for c in np.split(rng.permutation(S), cuts)]
    params = {"interpret_samples": args.interpret_samples, "epochs": args.epochs}
    m = Mask(sub_feat, sub_ei, pathways, params, "node_prediction")
    cplan = m.community_plan()
    tabs = engine.community_tables(cplan, pathways, S, dev)
    R = cplan[2]
    batch = R // args.epochs
    w0 = torch.zeros((1, S), device=dev)
    fit = {"lr": 0.01, "l1_lambda": 1e-4}
    stream = torch.cuda.current_stream()

    def rep(i):
        bits, _ = engine.sample_communities(4000 + i, cplan, pathways, S, dev, tables=tabs)
        y = plan.forward(bits)[:, 0]
        k = engine.shap_kernel(bits, S)
        return engine.wlm_fit(bits.view(1, R, -1), S, batch, y.view(1, R), k.view(1, R), w0,
                              fit, check=False)

    rep(0)
    torch.cuda.synchronize()
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record(stream)
    for i in range(reps):
        engine.sample_communities(5000 + i, cplan, pathways, S, dev, tables=tabs)
    b.record(stream)
    for i in range(reps):
        rep(i)
    c.record(stream)
    torch.cuda.synchronize()
    samp_ms = a.elapsed_time(b) / reps
    rep_ms = b.elapsed_time(c) / reps
    # the compat (bit-identical) community sampler as Explainer.run uses it: the reference's
    # torch CPU draws replayed natively, rows uploaded (Mask.generate_bits); median of 5
    compat = []
    for i in range(5):
        torch.manual_seed(i)
        m = Mask(sub_feat.cpu(), sub_ei.cpu(), [list(p) for p in pathways], params,
                 "node_prediction")
        t0 = time.perf_counter()
        m.generate_bits(dev)
        torch.cuda.synchronize()
        compat.append((time.perf_counter() - t0) * 1e3)
    cpu_ms = float(np.median(compat))
    torch.manual_seed(0)
    m = Mask(sub_feat.cpu(), sub_ei.cpu(), [list(p) for p in pathways], params, "node_prediction")
    t0 = time.perf_counter()
    m._generate_torch()
    torch_loop_ms = (time.perf_counter() - t0) * 1e3
    return {"workload": f"c2 subgraph ({S} cols), 20 random communities, {R} rows per repeat",
            "samples_per_s": R / (rep_ms * 1e-3), "ms_per_repeat": rep_ms,
            "sampler_ms": samp_ms,
            "sampler_write_GBps": R * ((S + 31) // 32) * 4 / (samp_ms * 1e-3) / 1e9,
            "cpu_compat_sampler_ms": cpu_ms, "cpu_compat_sampler_torch_loop_ms": torch_loop_ms,
            "cpu_sampler_cores": torch.get_num_threads()}


def graph_queries_section(args, dev, n=10_000, e=100_000, f=64, queries=8):
    """graph_prediction with several queries: `Explainer.run_queries` (one mask
    set per repeat shared by all queries) against the reference's usage, one `Explainer.run` per
    query, both through the public API end to end (host orchestration included), device
    sampler, synthetic graph, random-init 2-layer GCN + Linear head + sigmoid."""
    from bikg_graph_explainability_public_amd.explainer import Explainer
    from bikg_graph_explainability_public_amd.nn import ConvStack
    g = torch.Generator().manual_seed(3)
    feat = torch.randn((n, f), generator=g)
    ei = torch.randint(0, n, (2, e), generator=g)
    torch.manual_seed(3)
    arch = ConvStack("gcn", [f, f, f], [f, 1]).eval()
    params = {"seed": 1, "interpret_samples": args.interpret_samples, "epochs": args.epochs,
              "optimizer": "adam", "lr": 0.01, "lr_patience": 10, "l1_lambda": 1e-4,
              "mask_sampler": "device"}
    names = [str(i) for i in range(n)]
    exp = Explainer(feat.to(dev), ei.to(dev), arch, params, names,
                    problem="graph_prediction")
    els = [str(7 + 97 * i) for i in range(queries)]
    exp.run_queries(els[:2], 1)
    exp.run(els[0], 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    exp.run_queries(els, 1)
    torch.cuda.synchronize()
    t_shared = time.perf_counter() - t0
    t0 = time.perf_counter()
    for el in els:
        exp.run(el, 1)
    torch.cuda.synchronize()
    t_loop = time.perf_counter() - t0
    R = args.interpret_samples * args.epochs
    return {"workload": f"graph_prediction, {n} nodes / {e} edges, {f} feats, 2-layer GCN, "
                        f"{queries} queries x {R} rows, one repeat, device sampler",
            "run_queries_ms": t_shared * 1e3, "run_per_query_ms": t_loop * 1e3,
            "samples_per_s_shared": queries * R / t_shared,
            "samples_per_s_per_query_runs": queries * R / t_loop,
            "speedup": t_loop / t_shared}


# ----------------------------------------------------------------------------- regime (i) c3, API
def node_c3_section(args, dev, world, rank):
    """configs[2] in node_prediction semantics (regime (i)): the headline's repeat pipeline on the
    c3 graph's computational subgraph of node 7 (SAGE 128, interpret_samples=512), one repeat
    per rank per step (weak scaling), with its own graph check and CPU baseline."""
    args = argparse.Namespace(**dict(vars(args), dump_outputs=None))  # (the headline's dump stays)
    line = headline(args, dev, world, rank, workload="c3node")
    keep = ("value", "ms_per_step", "graph_check_max_abs_diff", "exchange_check_max_abs_diff",
            "phases_ms", "cpu_baseline", "scaling")
    out = {k: line[k] for k in keep if k in line}
    out["samples_per_s"] = out.pop("value")
    out["workload"] = line["config"]["workload"]
    out["config"] = {k: v for k, v in line["config"].items() if k != "workload"}
    out["roofline"] = dict(line["roofline"], traffic=None,
                           note="latency-bound (cache-resident subgraph, regime (i)); HBM "
                                "fraction reported, not the bound; no PMC pass for this section")
    out["roofline"].pop("traffic_source", None)
    for k in ("achieved_counter", "frac_counter", "counter_over_alg", "per_kernel_counter_bytes"):
        out["roofline"].pop(k, None)
    return out


def explainer_section(args, dev):
    """The public API end to end (Explainer(...).run(element, times), explainer.py:316-546):
    host orchestration (hetero flattening, k-hop subgraph, plan, arch check), masks, forward,
    KernelSHAP, surrogate fits, DataFrames — what a user calling run() gets, per phase
    (Explainer.last_run["phases"]: host ms and device ms between phase marks).  c2 with the
    device sampler (times=10) and the compat sampler (the reference's torch-CPU RNG order,
    times=1); c3 node_prediction with the device sampler (times=10).  After set-up the caller's
    objects are frozen out of the cyclic collector (gc.freeze(), as a long-running caller's are
    after start-up).  The timed call explains node 7 after a warm-up call on node 8 (code objects,
    allocator; nothing of node 8's query is reused); `same_query_again` then times a second call
    on node 7, which reuses the query's subgraph, plan and arch check (Explainer's per-query
    cache), and `same_query_after_gc_collect` a third one right after a forced gc.collect()."""
    from bikg_graph_explainability_public_amd.explainer import Explainer
    from bikg_graph_explainability_public_amd.nn import ConvStack
    out = {}
    g = torch.Generator().manual_seed(0)
    feat = torch.randn((args.nodes, args.feat), generator=g)
    ei = torch.randint(0, args.nodes, (2, args.edges), generator=g)
    torch.manual_seed(0)
    arch = ConvStack("gcn", [args.feat, 64, 64], [64, 1]).eval()
    x3, ei3, arch3 = c3_graph(dev)
    cases = [("c2_device_times10", feat, ei, arch, args.interpret_samples, "device", 10),
             ("c2_compat_times1", feat, ei, arch, args.interpret_samples, "compat", 1),
             ("c3node_device_times10", x3, ei3, arch3, 512, "device", 10)]
    for name, f, e, a, ns, sampler, times in cases:
        params = {"seed": 1, "interpret_samples": ns, "epochs": args.epochs, "optimizer": "adam",
                  "lr": 0.01, "lr_patience": 10, "l1_lambda": 1e-4, "mask_sampler": sampler}
        names = [str(i) for i in range(f.shape[0])]
        exp = Explainer(f.to(dev), e.to(dev), a, params, names)
        # the setup's objects (inputs, the 100k / 1M names list, the module) leave the cyclic
        # collector's generations, as a long-running caller's do after start-up; no collection is
        # forced right before a timed call: a full gc.collect() over the unfrozen heap walks every
        # tracked object and leaves the host caches cold for the call after it
        gc.collect()
        gc.freeze()
        exp.run(str(args.query + 1), times)  # warm (another query: nothing of it is reused)
        torch.cuda.synchronize()

        def timed_run():
            t0 = time.perf_counter()
            res = exp.run(str(args.query), times)
            torch.cuda.synchronize()
            return res, time.perf_counter() - t0
        (df, _), wall = timed_run()
        R = exp.last_run["repeats"][0]["rows"]
        out[name] = {"samples_per_s": times * R / wall, "wall_ms": wall * 1e3, "rows": times * R,
                     "times": times, "mask_sampler": sampler, "subgraph_nodes": exp.last_run["S"],
                     "engine": bool(exp.last_run["engine"]),
                     "phases": exp.last_run["phases"].times(), "top_element": str(df.index[0])}
        # the same query explained again (new masks: the RNG stream moved on): Explainer.run
        # reuses the query's subgraph, plan and arch check (its per-query cache)
        _, wall2 = timed_run()
        out[name]["same_query_again"] = {"samples_per_s": times * R / wall2, "wall_ms": wall2 * 1e3,
                                         "phases": exp.last_run["phases"].times()}
        # and once more right after a forced collection (of what the calls left unfrozen)
        gc.collect()
        _, wall3 = timed_run()
        out[name]["same_query_after_gc_collect"] = {"samples_per_s": times * R / wall3,
                                                    "wall_ms": wall3 * 1e3}
        gc.unfreeze()
        del exp
        torch.cuda.empty_cache()
    out["workload"] = ("Explainer(feat, edge_index, arch, params, names).run('7', times) end to "
                       "end (node_prediction), inputs on the GPU; c2 = configs[1], c3node = "
                       "configs[2] graph in node_prediction")
    return out


# ----------------------------------------------------------------------------- north star
BF16_MFMA_PEAK_TF = 2500.0   # MI355X_MICROARCH.md: ~2.5 PF dense BF16 MFMA


def sq_file(section):
    """profiles/sq_<section>.json (tools/sq_json.py: SQ / GRBM counters per exact kernel
    instantiation from one rocprofv3 PMC pass), or {}."""
    fn = os.path.join(ROOT, "profiles", f"sq_{section}.json")
    return json.load(open(fn)) if os.path.exists(fn) else {}


def north_star_block(c3):
    """The north-star evidence (BASELINE.json: >= 40 % HBM roofline on the masked message-passing
    gather at 1 GPU, MFMA utilisation against chip peak) as a compact block for the headline's
    `roofline`: the c3 full-graph pass (configs[2], SURVEY.md §8d regime (ii)) per kernel —
    live ms and algorithmic-byte fraction, the counter-byte fraction (profiles/pmc_c3.json), the
    exact-f32 layer 2 beside the default three-piece bf16 one, and the MFMA pipe: busy fraction
    from SQ_VALU_MFMA_BUSY_CYCLES / (SIMDs x GRBM_GUI_ACTIVE / 8) (profiles/sq_c3.json) and the
    live bf16 MFMA rate of the layer-2 products against the dense bf16 peak."""
    ks = c3["kernels"]
    l1, l2 = ks["k_wide_l1s"], ks["k_wide_last_ws"]
    sq = sq_file("c3")
    ex = c3.get("layer2_exact_f32", {})

    def kern(d, inst):
        out = {"kernel": inst, "ms": d["launch_ms"], "alg_bytes": d["alg_bytes_per_launch"],
               "achieved_GBps": d["achieved_GBps"], "frac": d["frac"],
               "frac_counter": d.get("frac_counter")}
        s = sq.get(inst)
        if s:
            out["mfma_busy"] = s.get("mfma_busy")
            out["wave_wait_frac"] = s.get("wait_frac")
        return out

    blk = {
        "workload": f"c3 full graph (configs[2]): 1M nodes / 10M edges, 2-layer SAGE 128 + "
                    f"Linear(128,1), every node a target, {c3['rows']} rows in 32-row passes",
        "kernel": C3_DEFAULT_INSTANCES["k_wide_last_ws"],
        "frac": l2["frac"], "achieved": l2["achieved_GBps"], "peak": HBM_PEAK_GBS,
        "unit": "GB/s", "frac_counter": l2.get("frac_counter"),
        "pass_ms": c3["pass_ms_rank0"],
        "pass_frac": (l1["alg_bytes_per_launch"] + l2["alg_bytes_per_launch"]) /
                     (c3["pass_ms_rank0"] * 1e-3) / 1e9 / HBM_PEAK_GBS,
        "samples_per_s": c3["samples_per_s"],
        "layer1": kern(l1, C3_DEFAULT_INSTANCES["k_wide_l1s"]),
        "layer2": kern(l2, C3_DEFAULT_INSTANCES["k_wide_last_ws"]),
    }
    if ex:
        blk["layer2_exact_f32"] = {"kernel": ex["kernel"], "ms": ex["layer2_ms"], "frac": ex["frac"],
                                   "frac_counter": ex.get("frac_counter"),
                                   "max_abs_diff_vs_bf16x3": ex.get("max_abs_diff_vs_bf16x3")}
        s = sq.get(ex["kernel"])
        if s:
            blk["layer2_exact_f32"]["mfma_busy"] = s.get("mfma_busy")
    # live MFMA rate of layer 2: per pass 32 samples x N targets x (K = 256) x (F_out = 128)
    # products, each as three bf16 MFMA products (a_hi w_hi + a_hi w_lo + a_lo w_hi)
    flops = 3 * 2.0 * 32 * 1_000_000 * 256 * 128
    blk["mfma"] = {
        "layer2_bf16_tflops": flops / (l2["launch_ms"] * 1e-3) / 1e12,
        "peak_bf16_tflops": BF16_MFMA_PEAK_TF,
        "rate_frac": flops / (l2["launch_ms"] * 1e-3) / 1e12 / BF16_MFMA_PEAK_TF,
        "busy": blk["layer2"].get("mfma_busy"),
        "busy_clock_ghz": (sq.get(C3_DEFAULT_INSTANCES["k_wide_last_ws"]) or {}).get("clock_ghz"),
        "busy_source": "profiles/sq_c3.json" if sq else None,
        "note": "busy = SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8) of a "
                "profiled run; rate_frac = the live layer-2 bf16 MFMA flops / 2.5 PF dense: the "
                "kernel is HBM-gather-bound, MFMA is not its bound"}
    return blk


def compact_api(api):
    """explainer_api with each phase as [host_ms, device_ms] (the bulky per-phase dicts kept the
    driver's stdout tail from reaching the c3 section)."""
    def ph(p):
        if not isinstance(p, dict):
            return p
        return {k: [round(v.get("host_ms", 0.0), 3), round(v.get("device_ms") or 0.0, 3)]
                if isinstance(v, dict) else round(v, 3) for k, v in p.items()}
    out = {}
    for k, v in api.items():
        if isinstance(v, dict):
            v = dict(v)
            if "phases" in v:
                v["phases_host_device_ms"] = ph(v.pop("phases"))
            if isinstance(v.get("same_query_again"), dict):
                a = dict(v["same_query_again"])
                if "phases" in a:
                    a["phases_host_device_ms"] = ph(a.pop("phases"))
                v["same_query_again"] = a
        out[k] = v
    return out


# ----------------------------------------------------------------------------- main
def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    world, rank, local = setup_dist(args)
    dev = torch.device("cuda", torch.cuda.current_device())
    from bikg_graph_explainability_public_amd import _lib
    _lib.load()
    layout = rank_layout(world, local)
    if not args.full:  # a plain run: the headline's timed steps and nothing else
        want = ("headline",)
    else:
        want = SECTIONS if args.sections == "all" else tuple(args.sections.split(","))
    skipped = ()
    if world > 1:
        skipped = tuple(s for s in want if s not in MULTI_GPU_SECTIONS)
        want = tuple(s for s in want if s in MULTI_GPU_SECTIONS)
    log(rank, f"bench: world {world}, sections {','.join(want)}" +
        (f" (single-GPU sections skipped at world {world}: {','.join(skipped)})" if skipped else ""))
    line = headline(args, dev, world, rank) if "headline" in want else \
        {"metric": METRIC, "value": None, "unit": "samples/s", "n_gpus": world,
         "note": "headline skipped (--sections)"}
    torch.cuda.empty_cache()
    regimes = {}
    runners = [("c3", "c3_full_graph", lambda: c3_section(args, dev, world, rank)),
               ("node_c3", "node_c3", lambda: node_c3_section(args, dev, world, rank)),
               ("c5", "c5_hetero", lambda: c5_section(args, dev, world, rank)),
               ("gp", "graph_prediction_c3", lambda: graph_prediction_section(args, dev)),
               ("c4", "hetero_c4", lambda: hetero_c4_section(args, dev, world, rank)),
               ("comm", "communities_c2", lambda: communities_section(args, dev)),
               ("queries", "graph_queries", lambda: graph_queries_section(args, dev)),
               ("api", "explainer_api", lambda: explainer_section(args, dev))]
    for key, name, fn in runners:
        if key in want:
            t0 = time.perf_counter()
            regimes[name] = fn()
            torch.cuda.empty_cache()
            log(rank, f"section {name}: {time.perf_counter() - t0:.1f} s")
    if "explainer_api" in regimes:
        regimes["explainer_api"] = compact_api(regimes["explainer_api"])
    if "c3_full_graph" in regimes and isinstance(line.get("roofline"), dict):
        line["roofline"]["north_star"] = north_star_block(regimes["c3_full_graph"])
    line["rank_layout"] = layout
    if skipped:
        line["sections_skipped"] = {"sections": list(skipped),
                                    "reason": f"single-GPU workloads (N = 1 only), not run at world {world}"}
    if regimes:
        # the north-star section last: the end of the line is what a stdout tail keeps
        order = [n for n in regimes if n != "c3_full_graph"] + \
            (["c3_full_graph"] if "c3_full_graph" in regimes else [])
        line["regimes"] = {n: regimes[n] for n in order}
    if RCCL1 and world == 1:
        line["rccl1_rehearsal"] = True
    if rank == 0:
        print(json.dumps(line), flush=True)
    if multi(world):
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
