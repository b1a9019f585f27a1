#!/usr/bin/env python
"""Time the V x V similarity sweep (K1) on synthetic domains.

    python scripts/sim_sweep_bench.py [--v 20000] [--repeats 5]
                                      [--parent-ext /path/to/parent/_C*.so]
                                      [--metric {levenshtein,osa,jaro}]

Three seeded domains of V values, each built as clusters of mutated copies so
that the index is not empty:

  short  ASCII, lengths 4..64       sim_pairs_gpu, this build (and, with
                                    --parent-ext, the parent commit's build,
                                    alternating, with an output digest to show
                                    both computed the same index)
  long   ASCII, lengths 65..256     sim_pairs_gpu at V, and sim_pairs_gpu vs
                                    sim_pairs_cpu at --long-cpu-v values
  wide   16-bit ids, lengths 4..64  sim_pairs_gpu vs sim_pairs_cpu

Every timed step runs in a child process of its own under ``timeout``; the
driver stops at the first child that fails. The CPU pass uses the OpenMP
thread count of the environment (OMP_NUM_THREADS). ``--metric osa`` times the
transposition-aware sweeps instead (both the GPU and the CPU pass); a
``--parent-ext`` build older than that metric can only be compared under the
default, ``levenshtein``. ``--metric jaro`` times ``jaro_pairs_gpu`` and
``jaro_pairs_cpu`` (Jaro similarity with the Winkler prefix boost,
``prefixScale`` 0.1) at the same threshold. Prints one JSON document.
"""

import argparse
import glob
import hashlib
import importlib.machinery
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR, MSIM = 5.0, 10.0
PREFIX_SCALE = 0.1  # --metric jaro


def make_domain(case, V, seed=1234):
    """[V, stride] symbol buffer and int32 lengths for one synthetic domain."""
    rng = np.random.default_rng(seed)
    if case == "long":
        lo, hi, stride, dtype, nsym = 65, 256, 256, np.uint8, 26
    elif case == "wide":
        lo, hi, stride, dtype, nsym = 4, 64, 64, np.uint16, 6000
    else:
        lo, hi, stride, dtype, nsym = 4, 64, 64, np.uint8, 26
    first = 97 if dtype == np.uint8 else 1
    buf = np.zeros((V, stride), dtype=dtype)
    lens = np.zeros(V, dtype=np.int32)
    copies = 4
    for c in range(0, V, copies):
        n = int(rng.integers(lo, hi + 1))
        base = rng.integers(first, first + nsym, size=n).astype(dtype)
        for k in range(c, min(c + copies, V)):
            s = base.copy()
            if k > c:  # a few substitutions and one cut keep copies near the base
                idx = rng.integers(0, n, size=max(1, n // 16))
                s[idx] = rng.integers(first, first + nsym, size=idx.size).astype(dtype)
                cut = int(rng.integers(0, min(3, n - lo) + 1))
                s = s[cut:]
            buf[k, : s.size] = s
            lens[k] = s.size
    perm = rng.permutation(V)  # value ids carry no length order
    return buf[perm], lens[perm]


def load_ext(path):
    import torch  # noqa: F401  (the extension links against it)

    loader = importlib.machinery.ExtensionFileLoader("_C", path)
    spec = importlib.util.spec_from_loader("_C", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def digest(row_ptr, col, expsim):
    """Order-independent digest of an index (rows are filled atomically)."""
    import torch

    V = row_ptr.numel() - 1
    counts = row_ptr[1:] - row_ptr[:-1]
    row_of = torch.repeat_interleave(torch.arange(V, device=col.device), counts)
    order = torch.argsort(row_of * V + col.to(torch.int64))
    h = hashlib.sha256()
    h.update(row_ptr.cpu().numpy().tobytes())
    h.update(col[order].cpu().numpy().tobytes())
    h.update(expsim[order].cpu().numpy().tobytes())
    return h.hexdigest()


def worker(args):
    import torch

    C = load_ext(args.ext)
    buf, lens = make_domain(args.case, args.v)
    if buf.dtype == np.uint16:
        buf = buf.view(np.int16)
    tb, tl = torch.from_numpy(buf), torch.from_numpy(lens)
    out = {"case": args.case, "kind": args.kind, "V": args.v, "ext": args.ext,
           "metric": args.metric}
    # the default keeps the four-argument call an older extension understands
    extra = (True,) if args.metric == "osa" else ()
    sweep = "sim_pairs"
    if args.metric == "jaro":
        sweep, extra = "jaro_pairs", (PREFIX_SCALE,)
    if args.kind == "gpu":
        assert torch.cuda.is_available(), "the GPU timing needs a GPU"
        tb, tl = tb.cuda(), tl.cuda()
        sweep_gpu = getattr(C, sweep + "_gpu")
        run = lambda: sweep_gpu(tb, tl, THR, MSIM, *extra)  # noqa: E731
        sync = torch.cuda.synchronize
    else:
        out["threads"] = torch.get_num_threads()
        sweep_cpu = getattr(C, sweep + "_cpu")
        run = lambda: sweep_cpu(tb, tl, THR, MSIM, *extra)  # noqa: E731
        sync = lambda: None  # noqa: E731
    for _ in range(args.warmup):
        run()
    times = []
    for _ in range(args.repeats):
        sync()
        t0 = time.perf_counter()
        res = run()
        sync()
        times.append(time.perf_counter() - t0)
    out["seconds"] = times
    out["nnz"] = int(res[1].numel())
    if args.kind == "gpu":
        out["digest"] = digest(*res)
    print("RESULT " + json.dumps(out), flush=True)


def spawn(ext, case, kind, v, repeats, warmup, limit, metric="levenshtein"):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
           "--worker", "--ext", ext, "--case", case, "--kind", kind, "--v", str(v),
           "--repeats", str(repeats), "--warmup", str(warmup), "--metric", metric]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"step {case}/{kind} failed with exit status {p.returncode}; stopping")
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def stats(times):
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times),
            "repeats": len(times)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--v", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-repeats", type=int, default=1,
                    help="repeats of each CPU pass (minutes each at V = 20000)")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of parent and new (short)")
    ap.add_argument("--cases", default="short,long,wide")
    ap.add_argument("--long-cpu-v", type=int, default=4000,
                    help="V of the long-domain CPU-vs-GPU pair (the CPU pass takes "
                         "tens of minutes on the long domain at V = 20000)")
    ap.add_argument("--timeout", type=int, default=390, help="seconds per child step")
    ap.add_argument("--ext", default=None, help="extension to time (default: this tree's)")
    ap.add_argument("--parent-ext", default=None, help="parent commit's built extension")
    ap.add_argument("--metric", choices=["levenshtein", "osa", "jaro"], default="levenshtein",
                    help="metric of both sweeps (osa: adjacent swaps cost 1; jaro: "
                         "Jaro similarity with the Winkler prefix boost)")
    ap.add_argument("--short-cpu", action="store_true",
                    help="also run the CPU pass on the short domain and compare nnz")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--case", default="short", help=argparse.SUPPRESS)
    ap.add_argument("--kind", default="gpu", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    ext = args.ext or sorted(glob.glob(os.path.join(ROOT, "dblink_amd", "_C*.so")))[0]
    cases = args.cases.split(",")
    report = {"V": args.v, "threshold": THR, "max_similarity": MSIM, "metric": args.metric}
    if "short" in cases:
        new, parent, digests = [], [], set()
        for _ in range(args.rounds if args.parent_ext else 1):
            if args.parent_ext:
                r = spawn(args.parent_ext, "short", "gpu", args.v, args.repeats, args.warmup,
                          args.timeout, args.metric)
                parent += r["seconds"]
                digests.add(r["digest"])
            r = spawn(ext, "short", "gpu", args.v, args.repeats, args.warmup, args.timeout,
                      args.metric)
            new += r["seconds"]
            digests.add(r["digest"])
        report["short"] = {"gpu": stats(new), "nnz": r["nnz"]}
        if parent:
            sp = stats(parent)
            report["short"]["gpu_parent"] = sp
            report["short"]["same_index_as_parent"] = len(digests) == 1
            report["short"]["median_over_parent"] = report["short"]["gpu"]["median_s"] / sp["median_s"]
            report["short"]["within_parent_spread"] = (
                report["short"]["gpu"]["median_s"] - sp["median_s"] <= sp["max_s"] - sp["min_s"])
        if args.short_cpu:
            c = spawn(ext, "short", "cpu", args.v, args.cpu_repeats, 0, args.timeout, args.metric)
            report["short"]["vs_cpu"] = {
                "V": args.v, "cpu": stats(c["seconds"]), "cpu_threads": c["threads"],
                "same_nnz": r["nnz"] == c["nnz"]}
        print(json.dumps({"short": report["short"]}), flush=True)
    for case in ("long", "wide"):
        if case not in cases:
            continue
        g = spawn(ext, case, "gpu", args.v, args.repeats, args.warmup, args.timeout,
                  args.metric)
        report[case] = {"gpu": stats(g["seconds"]), "nnz": g["nnz"]}
        # the CPU pass is quadratic in V and, on long values, in the length:
        # the pair is timed on identical buffers at a V the CPU finishes
        v = min(args.v, args.long_cpu_v) if case == "long" else args.v
        if v != args.v:
            g = spawn(ext, case, "gpu", v, args.repeats, args.warmup, args.timeout,
                      args.metric)
        c = spawn(ext, case, "cpu", v, args.cpu_repeats, 0, args.timeout, args.metric)
        report[case]["vs_cpu"] = {
            "V": v, "gpu": stats(g["seconds"]), "cpu": stats(c["seconds"]),
            "cpu_threads": c["threads"], "same_nnz": g["nnz"] == c["nnz"],
            "cpu_over_gpu": statistics.median(c["seconds"]) / statistics.median(g["seconds"])}
        print(json.dumps({case: report[case]}), flush=True)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
