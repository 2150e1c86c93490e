#!/usr/bin/env python3
"""The per-probe visibility fit through nerftex_envmap_vis_fit against its op-by-op counterpart on the same GPU: the reference's
default -- 64 probes, 800 rounds of 1024 points -- through envmap_probe_tables on a GPU tensor, and envmap_probe_tables(fused=False), the
reference's loop of framework ops (about sixty launches a round).  The op-by-op side costs about a second per probe, so --loop-probes limits it to
the first N probes and the result is scaled to 64 (it is the same work per probe); --loop-probes 64 runs it whole.  Also timed: the entry at
smaller batches and round counts, from which the time of one round and the launch's fixed cost follow.

Host clock around work that ends in a synchronise; everything warmed up first; the median and the spread of the repeats are written.
Writes profiles/probe_table_timing.json and prints it; needs a GPU and fails without one."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "nerf-texture_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def main():
    import numpy as np
    import torch

    from ngp_harness import light

    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--loop-probes", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_table_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_table_timing: no GPU")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(4242)
    env = np.zeros((16, 3), np.float32)
    env[0] = (1.8, 1.5, 1.1)
    env[1:9] = rng.normal(0, 0.12, (8, 3)).astype(np.float32)
    env = torch.from_numpy(env).to(dev)
    grid = light.probe_grid()
    out = {"device": torch.cuda.get_device_name(0), "probes": 64, "rounds": 800, "batch": 1024}

    entry = lambda **kw: light.envmap_probe_tables(env, **kw)  # noqa: E731
    tables, _ = entry()  # (warm-up)
    out["entry"] = _summary([_timed(entry, sync) for _ in range(args.repeats)])
    out["entry"]["us_per_round"] = round(out["entry"]["median_ms"] * 1e3 / 800, 3)
    out["entry_given_points"] = {}
    pts = light.envmap_probe_tables(env, points_out=True)[2]
    out["entry_with_points_out"] = _summary([_timed(lambda: entry(points_out=True), sync) for _ in range(3)])
    out["entry_given_points"] = _summary([_timed(lambda: entry(points=pts), sync) for _ in range(args.repeats)])
    del pts
    # what a round costs as its batch grows, and the launch's fixed cost (rounds -> 1)
    out["entry_by_shape"] = {}
    for rounds, batch in ((1, 1024), (800, 64), (800, 256), (800, 1024), (800, 4096), (1600, 1024)):
        entry(rounds=rounds, batch=batch)
        s = _summary([_timed(lambda: entry(rounds=rounds, batch=batch), sync) for _ in range(args.repeats)])
        s["us_per_round"] = round(s["median_ms"] * 1e3 / rounds, 3)
        out["entry_by_shape"][f"{rounds}x{batch}"] = s
    one = _summary([_timed(lambda: entry(probes=grid[:1]), sync) for _ in range(args.repeats)])
    out["entry_one_probe"] = one

    n = max(1, min(64, args.loop_probes))
    light.envmap_probe_tables(env, grid[:1], fused=False, rounds=20)  # (warm-up of every framework op of the loop)
    t_loop = [_timed(lambda: light.envmap_probe_tables(env, grid[:n], fused=False), sync) for _ in range(1 if n > 8 else 3)]
    out["op_by_op"] = dict(_summary(t_loop), probes_run=n, scaled_to_64_probes_ms=round(statistics.median(t_loop) * 64 / n, 1))
    out["speedup_at_64_probes"] = round(out["op_by_op"]["scaled_to_64_probes_ms"] / out["entry"]["median_ms"], 1)
    loop, _ = light.envmap_probe_tables(env, grid[:n], fused=False)
    # (the two sides draw different points: they agree statistically only -- tests/test_gpu_probe_table.py holds the entry on given points)
    out["max_abs_difference_on_their_own_points"] = float((loop - tables[:n]).abs().max())
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
