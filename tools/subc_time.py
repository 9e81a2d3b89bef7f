#!/usr/bin/env python3
"""Time of the MPX subcarrier receiver (fmd_subc_run_device, csrc/subcarrier.inc): 256 streams x 16 blocks x M = 16384 discriminator samples
(the `v` tap of the bench's default shape, 256 MiB resident on the device), T = 128, D = 16, fc = 57000 at 300 k - the RDS recipe.

HIP events (torch.cuda.Event) on the launch stream around every launch - the receiver kernel and the state kernel behind it; warm-up launches,
then the median of --reps launches with p10 / p90.  The bound the kernel is compared with is the read of v: 4 bytes per sample, plus 8 / D bytes
written; beside it, from the same session, a device-to-device copy of the same v bytes (which reads AND writes them).  One JSON line per
measurement; --out also writes them to a file.  The tool ends itself after --timeout seconds; run it on an idle device, and under a timeout of
the caller's too:

    timeout -k 10 300 python3 tools/subc_time.py --out profiles/<name>.json"""
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
    ap.add_argument("--block-samples", type=int, default=16384)
    ap.add_argument("--rate", type=int, default=300000)
    ap.add_argument("--fc", type=int, default=57000)
    ap.add_argument("--bw", type=int, default=2400)
    ap.add_argument("--taps", type=int, default=128)
    ap.add_argument("--decim", default="16", help="comma-separated decimations to time")
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
    S, B, M = args.streams, args.blocks, args.block_samples
    n = S * B * M
    g = torch.Generator(device=dev).manual_seed(1)
    v = (torch.rand((n,), dtype=torch.float32, device=dev, generator=g) * 2 - 1) * float(np.pi)
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

    copy_dst = torch.empty_like(v)
    torch.cuda.synchronize()
    t = timed(lambda: copy_dst.copy_(v, non_blocking=True))
    copy_ms = t["median_ms"]
    emit(dict(what="d2d_copy", bytes=4 * n, traffic_bytes=8 * n, bytes_per_s=4 * n / (copy_ms * 1e-3),
              traffic_share_of_8TBps=8 * n / (copy_ms * 1e-3) / HBM_PEAK, **t))
    del copy_dst
    for D in [int(x) for x in args.decim.split(",")]:
        sub = R.Subcarrier(R.FmdSubcConfig(args.rate, args.fc, args.bw, args.taps, D, M), S, device=0)
        z = torch.zeros((S, B, M // D, 2), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        t = timed(lambda: sub.run_device(v, B, z, hip_stream=st.cuda_stream))
        traffic = 4 * n + 8 * n // D
        emit(dict(what="subcarrier", rate=args.rate, fc=args.fc, bw=args.bw, n_taps=args.taps, decim=D, streams=S, blocks=B, block_samples=M,
                  v_bytes=4 * n, traffic_bytes=traffic, traffic_share_of_8TBps=traffic / (t["median_ms"] * 1e-3) / HBM_PEAK,
                  samples_per_s=n / (t["median_ms"] * 1e-3), ratio_to_copy=t["median_ms"] / copy_ms, **t))
        assert bool(torch.isfinite(z).all()) and float(z.abs().max()) > 0
        sub.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
