#!/usr/bin/env python3
"""Time of the RDS receiver (fmd_rds_run_device, csrc/rds.inc): 256 streams x 16 blocks x Bz = 1024 complex samples of z at 18750 Hz (what the
subcarrier receiver makes of the bench's default shape at D = 16; 32 MiB resident on the device), Tg = 64, avg_blocks 8.

HIP events (torch.cuda.Event) on the launch stream around all four launches of one run - matched filter, tracker, slicer, state kernel; warm-up
launches, then the median of --reps launches with p10 / p90.  Beside it, from the same session, a device-to-device copy of the same z bytes
(which reads AND writes them).  One JSON line per measurement; --out also writes them to a file.  The tool ends itself after --timeout seconds;
run it on an idle device, and under a timeout of the caller's too:

    timeout -k 10 300 python3 tools/rds_time.py --out profiles/<name>.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--block-z", type=int, default=1024)
    ap.add_argument("--rate-z", type=int, default=18750)
    ap.add_argument("--taps", default="64", help="comma-separated matched-filter lengths to time")
    ap.add_argument("--reps", type=int, default=30, help="timed launches per measurement (>= 20)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds after which the tool ends itself (SIGALRM), whatever it is waiting for")
    args = ap.parse_args()
    import signal
    signal.alarm(args.timeout)
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    import torch
    import rtl_fm_player_amd as R
    dev = torch.device("cuda:0")
    S, B, Bz = args.streams, args.blocks, args.block_z
    n = S * B * Bz
    g = torch.Generator(device=dev).manual_seed(1)
    z = torch.rand((2 * n,), dtype=torch.float32, device=dev, generator=g) * 0.1 - 0.05
    st = torch.cuda.Stream()
    lines = []

    def timed(fn):
        with torch.cuda.stream(st):
            for _ in range(args.warmup):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
            for e0, e1 in ev:
                e0.record(st)
                fn()
                e1.record(st)
        st.synchronize()
        t = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
        return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), p10_ms=float(np.percentile(t, 10)),
                    p90_ms=float(np.percentile(t, 90)), max_ms=float(t.max()), reps=args.reps)

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    copy_dst = torch.empty_like(z)
    torch.cuda.synchronize()
    t = timed(lambda: copy_dst.copy_(z, non_blocking=True))
    copy_ms = t["median_ms"]
    emit(dict(what="d2d_copy", bytes=8 * n, traffic_bytes=16 * n, bytes_per_s=8 * n / (copy_ms * 1e-3),
              traffic_share_of_8TBps=16 * n / (copy_ms * 1e-3) / HBM_PEAK, **t))
    del copy_dst
    for T in [int(x) for x in args.taps.split(",")]:
        rds = R.Rds(R.FmdRdsConfig(args.rate_z, Bz, T, 8, B), S, device=0)
        slot = rds.bits_per_block
        soft = torch.zeros((S, B, slot), dtype=torch.float32, device=dev)
        lens = torch.zeros((S, B), dtype=torch.int32, device=dev)
        est = torch.zeros((S, B, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        t = timed(lambda: rds.run_device(z, B, soft, lens, None, est, hip_stream=st.cuda_stream))
        # z read by the matched filter, y written, y read by the slicer's bits (at most all of it), soft bits and lens written
        traffic = 8 * n + 8 * n + 4 * S * B * slot + 4 * S * B
        emit(dict(what="rds", rate_z=args.rate_z, n_taps=T, streams=S, blocks=B, block_z=Bz, bits_per_block=slot, z_bytes=8 * n, traffic_bytes=traffic,
                  traffic_share_of_8TBps=traffic / (t["median_ms"] * 1e-3) / HBM_PEAK, samples_per_s=n / (t["median_ms"] * 1e-3),
                  ratio_to_copy=t["median_ms"] / copy_ms, **t))
        assert bool(torch.isfinite(soft).all()) and float(soft.abs().max()) > 0 and int(lens.min()) > 0
        rds.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
