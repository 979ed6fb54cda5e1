"""Benchmark of the GP-transportation hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W          (N > 1: starts its own N ranks, see `launch_ranks`)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Metric (BASELINE.json): posterior (mean + var + Jacobian) predictions/sec, N=8192 source points,
3-D, fp64.  A step = one fused predict pass (mean (M,3), variance (M,), Jacobian (M,3,3)) over one
batch of M = 500 000 synthetic queries already resident in HBM (configs[2]); with N GPUs every rank
runs the same per-GPU batch on its own query shard (configs[3]: 8 x 500k = 4M, weak scaling) after ONE
RCCL broadcast of the model fitted on rank 0.  Prints one JSON line on rank 0.

A plain run does only what the headline needs: set up (fit, resident queries), W warm-up steps, K timed steps, the
outputs of the last step if --dump-outputs DIR is given, the JSON line.  --full adds what takes measurements of its
own: the repeat fits behind fit_ms, the CPU baseline (--cpu-sample) and, on one GPU, the `secondary` records (mode J+Jvar,
configs[1], configs[4]; --no-secondary drops them).

--dump-outputs DIR writes, after the timed steps, the arrays the timed path returned in its last step as DIR/<name>.npy
(exact: mean, var, J, and Jvar with --jvar, fp64; --config svgp: the same four, fp32), rank 0's queries only.  The inputs
are seeded, so two builds run with the same arguments compare output for output; above DUMP_LIMIT_BYTES every array keeps
the same seeded sample of query rows (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP64_MFMA_TFLOPS = 78.6      # MI355X datasheet fp64 matrix peak (not in MI355X_MICROARCH.md)
PEAK_FP32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md "Peak FP32 (matrix)": v_mfma_f32_16x16x4_f32, 64 FLOP/clk/SIMD
DUMP_LIMIT_BYTES = 60_000_000     # --dump-outputs: array data written at most (under 64 MB in all with the .npy headers)


def flops_per_query(N, D, O, jvar):
    """Algorithmic work model of SURVEY §8d / BASELINE.md (exp = 1 flop)."""
    lin = N * (3 * D + 1 + 2 * O + 2 * D * O + D + 2)
    return (1 + D) * N * N + lin if jvar else N * N + lin


def var_kernel_flops_per_query(N, D, jvar):
    """Algorithmic flops of the dominant (variance) kernel alone: N^2 triangular multiply-add + 2N
    reduction + its k* row (3D N + N exp); x(1+D) columns with the Jacobian variance."""
    per_col = N * N + 2 * N
    return (1 + D) * per_col + N * (3 * D + 1) if jvar else per_col + N * (3 * D + 1)


def synthetic_sources(N, D=3, seed=0):
    """SURVEY §8d synthetic inputs: X ~ U[0,1]^D, Y = 0.05 sin(4X) + 0.01 N(0,1)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (N, D))
    Y = 0.05 * np.sin(4 * X) + 0.01 * rng.standard_normal((N, D))
    return X, Y


def dump_outputs(dirname, arrays, limit=DUMP_LIMIT_BYTES, seed=0):
    """--dump-outputs: the arrays a step returned to its caller (torch tensors or numpy, row i = query i), copied to the
    host after the timed region and written as DIR/<name>.npy in their own dtype.  When they hold more than `limit` bytes
    together, every array keeps the same fixed sample of rows (seeded, ascending).  Returns {name: shape written}."""
    host = {k: np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in arrays.items() if v is not None}
    M = next(iter(host.values())).shape[0]
    total = sum(a.nbytes for a in host.values())
    if total > limit:
        rows = np.sort(np.random.default_rng(seed).choice(M, M * limit // total, replace=False))
        host = {k: a[rows] for k, a in host.items()}
    os.makedirs(dirname, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(dirname, k + ".npy"), a)
    return {k: list(a.shape) for k, a in host.items()}


def cpu_baseline(N, D, O, sample, jvar):
    """Times the CPU oracle (numpy/scipy restatement of the reference's algorithm, all host cores
    through BLAS) on a bounded sample of the same workload.  kind = "port"."""
    from oracle import gp_oracle as orc
    X, Y, Xq = orc.synthetic_problem(N, sample)
    c, ls, noise, jit = 0.1, np.array([0.1] * D), 1e-4, 1e-10
    t0 = time.perf_counter()
    L, a = orc.gpr_fit(X, Y, c, ls, noise, jit)
    t_fit = time.perf_counter() - t0
    t0 = time.perf_counter()
    orc.posterior_all_fast(Xq, X, L, a, c, ls, noise, want_jvar=jvar)
    t_pred = time.perf_counter() - t0
    out = {"value": sample / t_pred, "unit": "predictions/s", "cores": os.cpu_count(), "kind": "port",
           "sample": f"oracle.posterior_all_fast on {sample} of the queries at N={N} (mean+var+J"
                     f"{'+Jvar' if jvar else ''}), numpy/scipy BLAS threads; CPU fit (Gram+potrf+potrs) took {t_fit:.1f} s",
           "fit_s": t_fit}
    # The library the reference itself calls for fit / mean / std (gaussian_process.py:19-21, 37, 48): scikit-learn's
    # GaussianProcessRegressor with the reference's kernel and optimizer=None, same inputs, mean + std only (the
    # reference's Jacobian code is its own and does not exist on this box).  Reported beside the port, never as `value`.
    try:
        from sklearn.gaussian_process import GaussianProcessRegressor
        from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
        gpr = GaussianProcessRegressor(kernel=ConstantKernel(c) * RBF(ls) + WhiteKernel(noise), alpha=jit, optimizer=None)
        t0 = time.perf_counter()
        gpr.fit(X, Y)
        t_sk_fit = time.perf_counter() - t0
        t0 = time.perf_counter()
        gpr.predict(Xq, return_std=True)
        t_sk = time.perf_counter() - t0
        out["sklearn"] = {"fit_s": t_sk_fit, "mean_std_predictions_per_s": sample / t_sk,
                          "what": f"GaussianProcessRegressor(optimizer=None).fit + predict(return_std=True) on {sample} queries"}
    except ImportError:
        out["sklearn"] = None
    return out


def visible_device_shortfall(gpus):
    """A device restriction already in the environment (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES,
    which the ROCm runtime also honours) is kept: rank r uses device r OF THE VISIBLE SET (the children inherit the
    variables unchanged and select `LOCAL_RANK` inside them).  Returns a message when a variable lists fewer devices than
    --gpus — known from the strings alone, before any process is started or any GPU is touched — else None."""
    for name in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        val = os.environ.get(name)
        if val is None:
            continue
        ids = [t for t in val.replace(" ", "").split(",") if t != ""]
        if "-1" in ids:                                   # the runtimes stop reading the list at -1
            ids = ids[:ids.index("-1")]
        if len(ids) < gpus:
            return f"--gpus {gpus} but {name}={val!r} leaves {len(ids)} device(s) visible"
    return None


def launch_ranks(args, argv):
    """`python bench.py --gpus N` with N > 1 and no torch.distributed environment: this process becomes a pure
    launcher.  It has not imported torch, loaded libgpt_hip.so or made any HIP call (and never does): it starts
    one fresh child process per GPU with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, relays what the ranks
    print (rank 0's JSON line on stdout, everything else on stderr) and exits with the worst return code."""
    import socket
    import subprocess
    # (a --dry-run uses no device: the check is rehearsed there only on request, GPT_BENCH_DRY_CHECK_DEVICES=1)
    short = visible_device_shortfall(args.gpus) if (not args.dry_run or os.environ.get("GPT_BENCH_DRY_CHECK_DEVICES") == "1") else None
    if short:
        print(f"bench launcher: {short}", file=sys.stderr)
        return 2
    with socket.socket() as sk:                      # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GPT_BENCH_CHILD="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, text=(r == 0)))
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    rcs = [None] * len(procs)
    while any(rc is None for rc in rcs):
        for r, pr in enumerate(procs):
            if rcs[r] is None:
                rcs[r] = pr.poll()
        if any(rc not in (None, 0) for rc in rcs):   # a failed rank leaves the others inside a collective: stop them
            for r, pr in enumerate(procs):
                if rcs[r] is None:
                    pr.terminate()                   # exactly the PIDs started above
                    rcs[r] = pr.wait()
            break
        time.sleep(0.05)
    reader.join(timeout=30)
    out0 = "".join(c or "" for c in chunks)
    lines = [ln for ln in (out0 or "").splitlines() if ln.strip()]
    for ln in lines:
        print(ln, flush=True)
    worst = max((abs(rc) for rc in rcs), default=0)
    if worst == 0 and not any(ln.lstrip().startswith("{") for ln in lines):
        print("bench launcher: rank 0 printed no JSON line", file=sys.stderr)
        worst = 1
    return worst


def dry_run(args):
    """--dry-run: the multi-rank skeleton of the benchmark (rendezvous, barriers, rank count check, max-reduce of the
    elapsed time, one JSON line from rank 0) over gloo on the CPU — no GPU, no library; what the CPU test of the
    launcher runs."""
    import datetime
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    if os.environ.get("GPT_BENCH_DRY_FAIL_RANK") == str(rank):      # test hook: this rank dies before the rendezvous
        raise SystemExit(3)
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
    ones = torch.ones(1, dtype=torch.float64)
    dist.all_reduce(ones)
    if int(ones.item()) != args.gpus or dist.get_world_size() != args.gpus:
        raise SystemExit(f"dry run: {int(ones.item())} ranks answered, --gpus {args.gpus}")
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.001 * (1 + rank))
    dist.barrier()
    tt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "ranks_seen": int(ones.item()), "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": float(tt.item()) / max(args.steps, 1) * 1e3,
                          "backend": "gloo"}), flush=True)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n-source", type=int, default=8192)
    ap.add_argument("--queries", type=int, default=500_000, help="queries per GPU per step")
    ap.add_argument("--jvar", action="store_true", help="also compute the Jacobian variance (mode J+Jvar)")
    ap.add_argument("--cpu-sample", type=int, default=2000, help="queries of the CPU baseline of --full (0 = skip)")
    ap.add_argument("--config", choices=["exact", "svgp"], default="exact",
                    help="exact: the headline metric (BASELINE configs[2]/[3]); svgp: configs[4], fp32 SVGP-MIMO path")
    ap.add_argument("--inducing", type=int, default=2048, help="inducing points of --config svgp")
    ap.add_argument("--dry-run", action="store_true", help="multi-rank skeleton over gloo on the CPU, no GPU work")
    ap.add_argument("--full", action="store_true",
                    help="also the measurements beside the headline: repeat fits (fit_ms), CPU baseline, `secondary` records")
    ap.add_argument("--no-secondary", dest="secondary", action="store_false",
                    help="with --full: skip the `secondary` records (mode J+Jvar, configs[1], configs[4]) measured after the headline on one GPU")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (rank 0; see dump_outputs)")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")

    # ---- launcher: before torch / the library / any HIP call
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args, sys.argv[1:]))
    if args.dry_run:
        return dry_run(args)

    if args.config == "svgp":
        return run_svgp(args)
    return run_exact(args)


def init_ranks(args):
    """torch + library + (for more than one rank, or GPT_BENCH_FORCE_DIST=1) the RCCL process group."""
    import torch
    from gaussian_process_transportation_amd import _lib
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    short = visible_device_shortfall(args.gpus)
    if short:
        raise SystemExit(f"rank {rank}: {short}")
    n_visible = torch.cuda.device_count()                  # (no exec follows in this process, so it does not matter whether counting initialises HIP)
    if local_rank >= n_visible or args.gpus > n_visible:
        raise SystemExit(f"rank {rank}: --gpus {args.gpus}, LOCAL_RANK {local_rank}, but only {n_visible} HIP device(s) are visible "
                         "(HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES?)")
    _lib.require_gpu()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    ranks_seen = 1
    # GPT_BENCH_FORCE_DIST=1 runs the multi-rank code path (RCCL init, model broadcast, barriers, max-reduce) with
    # however many ranks there are, also one: the rehearsal available on a one-GPU box
    use_dist = world > 1 or os.environ.get("GPT_BENCH_FORCE_DIST") == "1"
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=dev)
        seen = torch.ones(1, dtype=torch.float64, device=dev)
        dist.all_reduce(seen)                                  # every rank checks that RCCL sees --gpus ranks
        ranks_seen = int(seen.item())
        if ranks_seen != args.gpus or dist.get_world_size() != args.gpus:
            raise SystemExit(f"rank {rank}: RCCL sees {ranks_seen} ranks (world size {dist.get_world_size()}), --gpus {args.gpus}")
    h = _lib.Handle(local_rank)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    return torch, dist, h, rank, world, dev, use_dist, ranks_seen


def broadcast_fitted(torch, dist, h, rank, dev, use_dist):
    """One RCCL broadcast of the model blob from rank 0 (outside the timed region: once per fit, not per batch)."""
    from gaussian_process_transportation_amd.distributed import broadcast_model
    if not use_dist:
        return None, 0
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nbytes = broadcast_model(h, fitted=(rank == 0), src=0, device=dev)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, nbytes


def timed_steps(torch, dist, h, step, args, dev, use_dist, steps=None, warmup=None):
    """W warm-up steps, then exactly K steps between barrier + synchronize on both sides; MAX over ranks.  The
    dominant kernel's duration is read per step from the library's hipEvents on the launch stream."""
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    def sync_all():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(warmup):
        step()
    sync_all()
    h.set_profiling(True)
    var_ms, mj_ms = [], []
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
        t = h.predict_timings()          # waits for this step's events only (the next launch follows at once)
        var_ms.append(t["var_ms"]); mj_ms.append(t["mean_jac_ms"])
    sync_all()
    elapsed = time.perf_counter() - t0
    h.set_profiling(False)
    if use_dist:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    return elapsed, float(np.mean(var_ms)), float(np.mean(mj_ms))


# k_var goes out as several launches per prediction call (csrc/gpt_predict.hip launch_var_t); the library's hipEvents
# bracket all of them, and achieved / traffic are per call as well
KERNEL_MS_IS = ("all k_var launches of one step (the rounds of 256 column blocks go out 16 per launch at the N = 8192 shape, "
                "proportionally more for smaller models) + k_var_combine + k_var_finalize")


def pmc_traffic(key, n_source, queries):
    """HBM-side traffic of the dominant kernel comes from a SEPARATE rocprofv3 --pmc run (profiles/pmc_traffic.json,
    written by tools/pmc_traffic.py with the workload and commit it was measured on); it is quoted only when this run's
    workload is the one measured there and the library is the in-tree build."""
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(tpath) or os.environ.get("GPT_HIP_LIB"):
        return None, None
    try:
        rec = json.load(open(tpath)).get(key, {})
        if (rec.get("n_source"), rec.get("queries")) == (n_source, queries):
            return rec.get("hbm_bytes_per_launch"), (f"profiles/pmc_traffic.json (rocprofv3 --pmc, separate run, "
                                                     f"commit {rec.get('commit', '?')})")
    except Exception:
        pass
    return None, None


def exact_queries(M, D, seed):
    return np.random.default_rng(seed).uniform(-0.1, 1.1, (M, D))


def exact_buffers(torch, dev, M, D, O, jvar, seed):
    xq = torch.from_numpy(exact_queries(M, D, seed)).to(dev)
    mean = torch.empty((M, O), dtype=torch.float64, device=dev)
    var = torch.empty((M,), dtype=torch.float64, device=dev)
    J = torch.empty((M, O, D), dtype=torch.float64, device=dev)
    Jvar = torch.empty((M, D), dtype=torch.float64, device=dev) if jvar else None
    return xq, mean, var, J, Jvar


def measure_exact(ctx, args, N, M, jvar, steps, warmup, c=0.1, noise=1e-4, dump=None):
    """K timed steps of the fused predict pass of a fitted exact-GP handle over M resident queries; returns the record of
    this mode (value over all ranks, dominant-kernel duration from the library's hipEvents, roofline fields).  dump: the
    --dump-outputs directory (rank 0 writes the last step's outputs there)."""
    torch, dist, h, rank, world, dev, use_dist = ctx
    D = O = 3
    xq, mean, var, J, Jvar = exact_buffers(torch, dev, M, D, O, jvar, 1 + rank)
    h.reserve(M, jvar)               # library scratch of the timed calls: allocated here, not inside the first step

    def step():
        h.predict_all_dev(xq.data_ptr(), M, mean.data_ptr(), var.data_ptr(), J.data_ptr(),
                          Jvar.data_ptr() if Jvar is not None else 0, 0)

    elapsed, kern_ms, mj_ms = timed_steps(torch, dist, h, step, args, dev, use_dist, steps, warmup)
    # ---- sanity of the timed outputs (finite, variance within [0, c+noise])
    ok = bool(torch.isfinite(mean).all() and torch.isfinite(J).all() and torch.isfinite(var).all()
              and float(var.min()) >= 0.0 and float(var.max()) <= c + noise + 1e-12
              and (Jvar is None or bool(torch.isfinite(Jvar).all())))
    if not ok and not os.environ.get("GPT_BENCH_ABLATE"):     # timing-only ablation builds compute wrong values
        raise SystemExit("bench: non-finite or out-of-range outputs")
    dumped = dump_outputs(dump, {"mean": mean, "var": var, "J": J, "Jvar": Jvar}) if dump and rank == 0 else None
    kflops = var_kernel_flops_per_query(N, D, jvar) * M
    achieved = kflops / (kern_ms * 1e-3) / 1e12
    traffic, traffic_source = pmc_traffic("jvar" if jvar else "j", N, M)
    return {"value": world * M * steps / elapsed, "elapsed_s": elapsed, "ms_per_step": elapsed / steps * 1e3, "steps": steps,
            "dumped": dumped,
            "warmup": warmup, "flops_per_query": flops_per_query(N, D, O, jvar),
            "roofline": {"bound": "mfma", "kernel": "k_var (variance / Jacobian-variance triangular MFMA GEMM)",
                         "achieved": achieved, "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_FP64_MFMA_TFLOPS, "traffic": traffic, "traffic_source": traffic_source,
                         "kernel_ms": kern_ms, "mean_jac_kernel_ms": mj_ms, "kernel_ms_is": KERNEL_MS_IS}}


def measure_config1(_lib, steps=5):
    """BASELINE configs[1]: N = 1024 sources, M = 50 000 queries, fit + predict(mean, std), no Jacobian, fp64 — as a caller
    of the drop-in sees it: numpy in, numpy out through the host-pointer entry points (PCIe inclusive)."""
    N, M, D = 1024, 50_000, 3
    X, Y = synthetic_sources(N, D)
    Xq = np.random.default_rng(1).uniform(-0.1, 1.1, (M, D))
    ls = np.array([0.1] * D)
    h = _lib.Handle(0)
    h.fit(X, Y, ls, 0.1, 1e-4, 1e-10)
    h.predict_all(Xq, mean=True, var=True)
    fit_s, pred_s, kern = [], [], []
    h.set_profiling(True)
    for _ in range(steps):
        t0 = time.perf_counter(); h.fit(X, Y, ls, 0.1, 1e-4, 1e-10); fit_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); out = h.predict_all(Xq, mean=True, var=True); pred_s.append(time.perf_counter() - t0)
        kern.append(h.predict_timings()["var_ms"])
    h.set_profiling(False)
    fit_phases = h.fit_timings()
    ok = bool(np.isfinite(out["mean"]).all() and out["var"].min() >= 0.0 and out["var"].max() <= 0.1 + 1e-4 + 1e-12)
    h.close()
    if not ok:
        raise SystemExit("bench (configs[1]): non-finite or out-of-range outputs")
    fit_ms, pred_ms, kern_ms = float(np.median(fit_s)) * 1e3, float(np.median(pred_s)) * 1e3, float(np.median(kern))
    kflops = (N * N + 2 * N + N * (3 * D + 1)) * M
    achieved = kflops / (kern_ms * 1e-3) / 1e12
    return {"workload": "BASELINE configs[1]: N=1024 source pts, M=50000 queries, fit + predict(mean, std), no Jacobian, fp64, "
                        "numpy in -> numpy out (host-pointer API, PCIe inclusive)",
            "value": M / (pred_ms * 1e-3), "unit": "predictions/s (predict mean+std, host to host)", "ms_per_step": pred_ms,
            "fit_ms": fit_ms, "fit_plus_predict_ms": fit_ms + pred_ms, "fit_phases_ms": fit_phases, "steps": steps, "dtype": "f64",
            "roofline": {"bound": "mfma", "kernel": "k_var<double,1>", "kernel_ms": kern_ms, "achieved": achieved,
                         "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": achieved / PEAK_FP64_MFMA_TFLOPS}}


def run_exact(args):
    torch, dist, h, rank, world, dev, use_dist, ranks_seen = init_ranks(args)
    N, D, O, M = args.n_source, 3, 3, args.queries

    # ---- fit on rank 0, broadcast the factor (outside the timed region; the fit's time is reported with --full)
    fit_ms = fit_timings = fit_ms_median = fit_total_median = None
    if rank == 0:
        X, Y = synthetic_sources(N, D)
        ls = np.array([0.1] * D)
        h.fit(X, Y, ls, 0.1, 1e-4, 1e-10)                  # first call: allocations + code load
        walls, totals = [], []
        for _ in range(3 if args.full else 0):             # three repeat fits: the fastest is reported as fit_ms / fit_phases_ms (the
            t0 = time.perf_counter()                       # second call is still 4 % slow: tools/fit_stream_probe.py 9.83-9.91 ms, then
            h.fit(X, Y, ls, 0.1, 1e-4, 1e-10)              # 9.45-9.55), the median beside it (rounds 1 and 2 reported the second call)
            ms = (time.perf_counter() - t0) * 1e3
            walls.append(ms); totals.append(h.fit_timings()["total"])
            if fit_ms is None or ms < fit_ms:
                fit_ms, fit_timings = ms, h.fit_timings()
        if walls:
            fit_ms_median, fit_total_median = float(np.median(walls)), float(np.median(totals))
    bcast_ms, bcast_bytes = broadcast_fitted(torch, dist, h, rank, dev, use_dist)

    ctx = (torch, dist, h, rank, world, dev, use_dist)
    rec = measure_exact(ctx, args, N, M, args.jvar, args.steps, args.warmup, dump=args.dump_outputs)

    # ---- --full: the other single-GPU configurations, after the headline's timed region, same process (N = 1 only)
    secondary = None
    if args.full and world == 1 and not use_dist and args.secondary:
        from gaussian_process_transportation_amd import _lib
        secondary = {}
        if not args.jvar:
            r = measure_exact(ctx, args, N, M, True, 5, 1)
            secondary["mode_J+Jvar"] = {"workload": f"N={N}, M={M}, mean+var+Jacobian+Jacobian variance (4 columns per query), fp64, resident",
                                        "value": r["value"], "unit": "predictions/s", "ms_per_step": r["ms_per_step"], "steps": 5,
                                        "dtype": "f64", "roofline": r["roofline"]}
        torch.cuda.synchronize()
        secondary["configs[1]"] = measure_config1(_lib)
        sv = measure_svgp((torch, dist, None, rank, world, dev, use_dist), args, args.inducing, 1_000_000, 10, 1)
        secondary["configs[4]"] = {"workload": sv["workload"], "value": sv["value"], "unit": "predictions/s",
                                   "ms_per_step": sv["ms_per_step"], "steps": 10, "dtype": "f32", "fit_ms": sv["fit_ms"],
                                   "roofline": sv["roofline"]}

    if rank == 0:
        out = {
            "metric": "posterior (mean+var+Jacobian) preds/sec, N=8192 source pts, 3-D fp64",
            "value": rec["value"], "unit": "predictions/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": rec["ms_per_step"], "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic", "full": args.full,
            "config": {"workload": f"N={N} source pts, M={M} queries per GPU per step, D=O=3, "
                                   f"mean+var+Jacobian{'+Jacobian variance' if args.jvar else ''}, RBF GP, fp64"
                                   + (f"; {world}x{M} queries sharded, one RCCL broadcast of the factor" if world > 1 else ""),
                       "n_source": N, "queries_per_gpu": M, "mode": "J+Jvar" if args.jvar else "J"},
            "flops_per_query": rec["flops_per_query"],
            "achieved_tflops_whole_path": rec["value"] * rec["flops_per_query"] / 1e12 / world,
            "roofline": rec["roofline"],
            "fit_ms": fit_ms, "fit_phases_ms": fit_timings, "fit_ms_is": "min of 3 repeat fits (host wall; fit_phases_ms: that fit's device events)",
            "fit_ms_median": fit_ms_median, "fit_device_total_ms_median": fit_total_median,
            "bcast_ms": bcast_ms, "bcast_bytes": bcast_bytes, "ranks_seen": ranks_seen,
        }
        if fit_timings:
            # factorisation + explicit inverse: N^3/3 flop each (sklearn/_gpr.py:346-364, gaussian_process.py:42-43)
            fi_ms = fit_timings["cholesky"] + fit_timings["inverse"]
            fi_tf = (2.0 * N ** 3 / 3.0) / (fi_ms * 1e-3) / 1e12
            out["fit_roofline"] = {"bound": "mfma", "what": "Cholesky + triangular inverse, 2 N^3 / 3 flop, device events of the fastest repeat fit",
                                   "kernel_ms": fi_ms, "achieved": fi_tf, "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s",
                                   "frac": fi_tf / PEAK_FP64_MFMA_TFLOPS}
        if use_dist and bcast_ms is not None:
            # "include broadcast time in cfg4's number" — `value` times the K steps only (a model is broadcast
            # once per fit, not per batch); value_incl_bcast charges the one broadcast to these K steps
            out["value_incl_bcast"] = world * M * args.steps / (rec["elapsed_s"] + bcast_ms * 1e-3)
            out["value_note"] = ("value = queries of all ranks / time of the K timed steps (max over ranks), the model broadcast "
                                 "excluded; value_incl_bcast = the same queries / (that time + bcast_ms)")
        if args.full and world == 1 and args.cpu_sample > 0:
            out["cpu_baseline"] = cpu_baseline(N, D, O, args.cpu_sample, args.jvar)
        else:
            out["cpu_baseline"] = None
        if secondary is not None:
            out["secondary"] = secondary
        if rec["dumped"] is not None:
            out["dumped_outputs"] = rec["dumped"]
        print(json.dumps(out), flush=True)
    h.close()
    if use_dist:
        dist.destroy_process_group()


def svgp_flops_per_query(Z, D, T):
    """SURVEY §8d work model applied to the multi-task model: per task and column Z^2 (+2Z), (1+D) columns; the kernel
    row (3DZ flop + Z exp) is shared by the tasks; mean + Jacobian contraction 2ZT + 2ZDT + DZ."""
    var = T * (1 + D) * (Z * Z + 2 * Z) + Z * (3 * D + 1)
    return var + Z * (2 * T + 2 * D * T + D + 2), var


def svgp_synthetic_model(Zn, T=3, D=3, seed=0):
    """SURVEY §8d cfg5 inputs: inducing points U[0,1]^D, Sigma_pseudo = A A^T / Z + 1e-3 I (A ~ N(0,1)), y_pseudo ~
    N(0,1), outputscale 1, length-scale 0.2 (the same draws as oracle.svgp_synthetic_problem)."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(0, 1, (Zn, D))
    Sigma = np.empty((T, Zn, Zn))
    for t in range(T):
        A = rng.standard_normal((Zn, Zn))
        Sigma[t] = A @ A.T / Zn + 1e-3 * np.eye(Zn)
    y = rng.standard_normal((T, Zn))
    return Z, Sigma, y, np.ones(T), np.full(D, 0.2)


def svgp_cpu_baseline(Z, sample):
    """The SVGP exact-conversion algebra restated in the reference's arithmetic (numpy float32: it casts with .float()
    and inverts K_uu + Sigma in fp32; BLAS on all host cores) on a bounded sample of the queries.  kind = "port"."""
    from oracle import gp_oracle as orc
    Zp, Sigma, y, osc, ls, Xq = orc.svgp_synthetic_problem(Z, sample)
    t0 = time.perf_counter()
    orc.svgp_exact_oracle_fast(Xq[:8], Zp, Sigma, y, osc, ls, dtype=np.float32)      # the T inverses (the "fit")
    t_fit = time.perf_counter() - t0
    t0 = time.perf_counter()
    orc.svgp_exact_oracle_fast(Xq, Zp, Sigma, y, osc, ls, dtype=np.float32)
    t_all = time.perf_counter() - t0
    t_pred = max(t_all - t_fit, 1e-9)
    return {"value": sample / t_pred, "unit": "predictions/s", "cores": os.cpu_count(), "kind": "port",
            "sample": f"oracle.svgp_exact_oracle_fast(float32) on {sample} of the queries at Z={Z}, T=D=3 (mean+std+J+J std), "
                      f"numpy BLAS threads; conversion (3 fp32 inverses) took {t_fit:.2f} s", "fit_s": t_fit}


def measure_svgp(ctx, args, Z, M, steps, warmup, h=None, bcast=None, dump=None):
    """BASELINE configs[4]: SVGP-MIMO derivative path, Z inducing points, T = D = 3, M resident queries, fp32.
    A step = mean (M,T), variance (M,T), Jacobian (M,T,D) and Jacobian variance (M,T,D) of one batch.  Fits the model
    on a handle of its own unless one is passed in (already fitted / broadcast).  dump: as in measure_exact."""
    from gaussian_process_transportation_amd import _lib
    torch, dist, _, rank, world, dev, use_dist = ctx
    T, D = 3, 3
    fit_ms = None
    own = h is None
    if own:
        h = _lib.Handle(dev.index or 0)
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        Zp, Sigma, y, osc, ls = svgp_synthetic_model(Z, T, D)
        h.fit_svgp(Zp, y, Sigma, ls, osc, dtype=_lib.GPT_F32)
        t0 = time.perf_counter()
        h.fit_svgp(Zp, y, Sigma, ls, osc, dtype=_lib.GPT_F32)
        fit_ms = (time.perf_counter() - t0) * 1e3
    xq = torch.from_numpy(np.random.default_rng(1 + rank).uniform(-0.1, 1.1, (M, D)).astype(np.float32)).to(dev)
    f32 = torch.float32
    mean = torch.empty((M, T), dtype=f32, device=dev); var = torch.empty((M, T), dtype=f32, device=dev)
    J = torch.empty((M, T, D), dtype=f32, device=dev); Jvar = torch.empty((M, T, D), dtype=f32, device=dev)
    h.reserve(M, True)

    def step():
        h.predict_all_dev(xq.data_ptr(), M, mean.data_ptr(), var.data_ptr(), J.data_ptr(), Jvar.data_ptr(), 0)

    elapsed, kern_ms, mj_ms = timed_steps(torch, dist, h, step, args, dev, use_dist, steps, warmup)
    ok = bool(torch.isfinite(mean).all() and torch.isfinite(J).all() and torch.isfinite(var).all() and torch.isfinite(Jvar).all()
              and float(var.min()) >= 0.0 and float(var.max()) <= 1.0 + 1e-5)
    if not ok and not os.environ.get("GPT_BENCH_ABLATE"):     # timing-only ablation builds compute wrong values
        raise SystemExit("bench (svgp): non-finite or out-of-range outputs")
    dumped = dump_outputs(dump, {"mean": mean, "var": var, "J": J, "Jvar": Jvar}) if dump and rank == 0 else None
    if own:
        h.close()
    fq, fq_var = svgp_flops_per_query(Z, D, T)
    achieved = fq_var * M / (kern_ms * 1e-3) / 1e12
    traffic, traffic_source = pmc_traffic("svgp", Z, M)
    return {"workload": f"BASELINE configs[4]: SVGP exact conversion, Z={Z} inducing pts, T=D=3, M={M} queries per GPU "
                        "per step, mean+std+Jacobian+Jacobian std, fp32 prediction (fp64 factorisation)",
            "value": world * M * steps / elapsed, "elapsed_s": elapsed, "ms_per_step": elapsed / steps * 1e3, "fit_ms": fit_ms,
            "dumped": dumped,
            "flops_per_query": fq,
            "roofline": {"bound": "mfma", "kernel": "k_var<float> (stacked per-task triangular MFMA GEMM, v_mfma_f32_16x16x4_f32)",
                         "achieved": achieved, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_FP32_MFMA_TFLOPS, "traffic": traffic, "traffic_source": traffic_source,
                         "kernel_ms": kern_ms, "mean_jac_kernel_ms": mj_ms, "kernel_ms_is": KERNEL_MS_IS}}


def run_svgp(args):
    """`--config svgp`: BASELINE configs[4] as the headline of the JSON line (one rank, or sharded like the exact path)."""
    from gaussian_process_transportation_amd import _lib
    torch, dist, h, rank, world, dev, use_dist, ranks_seen = init_ranks(args)
    Z, T, D = args.inducing, 3, 3
    M = args.queries if args.queries != 500_000 else 1_000_000
    fit_ms = None
    if rank == 0:
        Zp, Sigma, y, osc, ls = svgp_synthetic_model(Z, T, D)
        h.fit_svgp(Zp, y, Sigma, ls, osc, dtype=_lib.GPT_F32)
        if args.full:                                      # fit_ms: a repeat fit
            t0 = time.perf_counter()
            h.fit_svgp(Zp, y, Sigma, ls, osc, dtype=_lib.GPT_F32)
            fit_ms = (time.perf_counter() - t0) * 1e3
    bcast_ms, bcast_bytes = broadcast_fitted(torch, dist, h, rank, dev, use_dist)
    rec = measure_svgp((torch, dist, None, rank, world, dev, use_dist), args, Z, M, args.steps, args.warmup, h=h,
                       dump=args.dump_outputs)
    if rank == 0:
        out = {
            "metric": "SVGP-MIMO posterior (mean+std+Jacobian+Jacobian std) preds/sec, 2048 inducing pts, 3 tasks, 3-D fp32",
            "value": rec["value"], "unit": "predictions/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": rec["ms_per_step"], "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic", "full": args.full,
            "config": {"workload": rec["workload"], "inducing": Z, "tasks": T, "queries_per_gpu": M},
            "flops_per_query": rec["flops_per_query"], "achieved_tflops_whole_path": rec["value"] * rec["flops_per_query"] / 1e12 / world,
            "roofline": rec["roofline"],
            "fit_ms": fit_ms, "bcast_ms": bcast_ms, "bcast_bytes": bcast_bytes, "ranks_seen": ranks_seen,
        }
        if use_dist and bcast_ms is not None:
            out["value_incl_bcast"] = world * M * args.steps / (rec["elapsed_s"] + bcast_ms * 1e-3)
        out["cpu_baseline"] = svgp_cpu_baseline(Z, args.cpu_sample * 5) if args.full and world == 1 and args.cpu_sample > 0 else None
        if rec["dumped"] is not None:
            out["dumped_outputs"] = rec["dumped"]
        print(json.dumps(out), flush=True)
    h.close()
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
