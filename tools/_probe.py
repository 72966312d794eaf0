"""What the serving probes share (recommend_probe, rank_eval_probe, rerank_probe, explain_probe,
foldin_probe, negatives_probe, calibrate_probe): the package on sys.path, the common options, "needs a ROCm device", the clock, warm-up
plus alternating arms, the timings' record fields, and the JSON line with --out. Importing it (the
probes run as `python tools/<name>.py`, so it is found next to them) puts the package on the path."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "movie-recommender-system-with-gnns_amd"))


def parser(reps: int) -> argparse.ArgumentParser:
    """--reps (the probe's default), --scale, --dim, --out; the probe adds its own."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--out", default=None)
    return ap


def device(probe: str) -> torch.device:
    if not torch.cuda.is_available():
        raise SystemExit(f"{probe} needs a ROCm device (a CPU timing says nothing here)")
    return torch.device("cuda")


def timed(fn, n: int = 1):
    """(fn's last result, ms per call) of n calls: host clock around a device synchronise."""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3 / n


def median(ts):
    return sorted(ts)[len(ts) // 2]


def run_arms(arms: dict, reps: int, digits: int, inner: int = 1, label: str = ""):
    """(results, times) of the arms {name: fn}: one warm-up call of each (code objects, allocator
    pools), its result kept, then ``reps`` rounds over the arms in turn, each timing the mean of
    ``inner`` calls, printed as it comes with ``digits`` decimals."""
    results, times = {}, {name: [] for name in arms}
    for name, fn in arms.items():
        results[name], _ = timed(fn)
    for _ in range(reps):
        for name, fn in arms.items():
            _, ms = timed(fn, inner)
            times[name].append(ms)
            print(f"{label}{name}: {ms:.{digits}f} ms", flush=True)
    return results, times


def put_times(rec: dict, times: dict, digits: int, spread: bool = False) -> None:
    """<name>_ms (the median), with ``spread`` <name>_ms_range (fastest, slowest), and <name>_ms_all."""
    for name, ts in times.items():
        rec[f"{name}_ms"] = round(median(ts), digits)
        if spread:
            rec[f"{name}_ms_range"] = [round(min(ts), digits), round(max(ts), digits)]
        rec[f"{name}_ms_all"] = [round(t, digits) for t in ts]


def emit(rec: dict, out) -> None:
    """The record as one JSON line on stdout and, with --out, in that file."""
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
